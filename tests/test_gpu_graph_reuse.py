"""The captured decode graphs across a history of requests on ONE context (csrc/wm_internal.h DecGraphKey / DecGraphSlot): a decode
replays the graph of an earlier decode exactly when its key is that decode's, the plain slot survives a beam call and the beam slot a plain one, and
whatever ran on the context before, the ids are those of the same request on a fresh context.  The other suites pin every mode's fresh-context run
against its own reference; this one adds only that history does not matter.

Capture or reuse is read off wm_get_stats (wm_decode_run): a decode that finds its graph launches it from its second iteration on
(graph_replays == iterations_launched - 1), one that has to capture does so at its third (graph_replays == iterations_launched - 2)."""
import dataclasses
import os

import numpy as np
import pytest

import sample_ref as S
import seq_bias_ref as B
from helpers import clip_for
from whisper_medusa import WhisperMedusaModel
from whisper_medusa.engine import Engine

pytestmark = pytest.mark.gpu

CLIPS = (0, 1)
MAX_BATCH = 4
CAPTURES, REUSES = 2, 1         # iterations_launched - graph_replays


def _requests(cfg):
    V = S.dec_gp(cfg, False, False)                               # vanilla greedy, 24 new tokens, no length penalty
    T, _, _, seed = S.DEC_CASES["T1.0"]
    keys = list(S.DEC_KEYS[: len(CLIPS)])
    return {
        "M": dataclasses.replace(V, vanilla=False),               # exact-match Medusa
        "V": V,
        "Bm": dataclasses.replace(V, num_beams=2),
        "S1": dataclasses.replace(V, sampling_temperature=T, sampling_seed=seed, sampling_keys=keys),
        "S2": dataclasses.replace(V, sampling_temperature=T, sampling_seed=S.DEC_SECOND_SEED, sampling_keys=keys),
        "Vb": dataclasses.replace(V, sequence_bias=B.DEC_ENTRIES["plain"][:2]),
        "Vb'": dataclasses.replace(V, sequence_bias=B.DEC_ENTRIES["plain2"][:2]),
        "Vts": S.dec_gp(cfg, True, False),
    }


# (step, request or call, what the decode does with the slot's graph)
SEQUENCE = [
    (1, "M", CAPTURES), (2, "M", REUSES), (3, "V", CAPTURES), (4, "V", REUSES), (5, "Bm", CAPTURES),
    (6, "V", REUSES),               # the plain slot survived the beam call
    (7, "Bm", REUSES),              # ... and the beam slot the plain one
    (8, "S1", CAPTURES), (9, "S1", REUSES),
    (10, "S2", CAPTURES),           # the launches carry the seed by value
    (11, "Vb", CAPTURES),
    (12, "Vb'", REUSES),            # as many groups: the captured launches read the new tables
    (13, "Vts", CAPTURES), (14, "V", CAPTURES),
    (15, "taps", None),             # score_tokens + a sampling tap: calls with scalars of their own, the graphs stay
    (16, "V", REUSES),
    (17, "forward", None),          # wm_forward_logits drops every graph
    (18, "V", CAPTURES),
]


def _run(eng, gp):
    ids = eng.decode(gp, len(CLIPS))
    st = eng.stats()
    return ids, (st["iterations_launched"], st["graph_replays"])


def test_history_on_the_context_does_not_matter(gpu):
    cfg, sd = S.dec_checkpoint()
    assert cfg.vocab_size - cfg.timestamp_begin >= 2              # the vocabulary has the timestamp block: step 13 runs
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=MAX_BATCH, act_fp16=False)
    other = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=MAX_BATCH, act_fp16=False)
    graphs = not os.environ.get("WM_NO_GRAPH")
    try:
        feats = m.extract_features([clip_for(cfg, c) for c in CLIPS])
        req = _requests(cfg)
        assert [len(B.groups_of(req[k].sequence_bias)) for k in ("Vb", "Vb'")] == [2, 2] and req["Vb"].sequence_bias != req["Vb'"].sequence_bias
        # every request on a context of its own (the second model instance's weights)
        fresh = {}
        for name, gp in req.items():
            eng = Engine(cfg, other._blob, other._offsets, max_batch=MAX_BATCH, device=gpu, act_fp16=False)
            try:
                eng.encode(feats)
                fresh[name] = _run(eng, gp)
            finally:
                eng.close()
        print("graph reuse, fresh contexts (iterations_launched, graph_replays):", {k: v[1] for k, v in fresh.items()})
        # what keeps the sequence below from passing vacuously: every decode runs long enough to capture and replay, and the requests that
        # share a graph or differ in one scalar give different ids
        for name, (ids, (launched, replays)) in fresh.items():
            assert launched >= 4, (name, launched)
            if graphs:
                assert launched - replays == CAPTURES, (name, launched, replays)
        assert fresh["S1"][0] != fresh["S2"][0] and fresh["Vb"][0] != fresh["Vb'"][0] and fresh["Vb'"][0] != fresh["V"][0]
        assert fresh["S1"][0] != fresh["V"][0] and fresh["Bm"][0] != fresh["V"][0]

        eng = m.engine
        eng.encode(feats)                                         # two clips, encoded once
        record, last = [], None
        for step, what, expect in SEQUENCE:
            if what == "taps":
                P, eos = len(req["V"].prompt), req["V"].eos_token_id
                eng.score_tokens([S.own_end(s, P, eos) for s in last], P, req["V"])
                rows = np.random.default_rng(5).standard_normal((2, cfg.vocab_size)).astype(np.float32)
                eng.sample_rows(req["V"], rows, [list(req["V"].prompt), list(req["V"].prompt) + [9]], [0, 1], 1.0, 3)
                continue
            if what == "forward":
                eng.forward_logits([[req["V"].prompt[0]]], 0, True)
                continue
            ids, (launched, replays) = _run(eng, req[what])
            last = ids
            record.append((step, what, launched, replays))
            assert ids == fresh[what][0], (step, what, ids, fresh[what][0])
            assert launched == fresh[what][1][0], (step, what, launched, fresh[what][1][0])
            if graphs:
                assert launched - replays == expect, (step, what, launched, replays, "captures" if expect == CAPTURES else "reuses")
        print("graph reuse, one context (step, request, iterations_launched, graph_replays):", record)
    finally:
        m.engine.close()
        other.engine.close()
