"""Per-clip languages in one batch on the GPU (include/wm.h wm_set_stream_prompts / wm_detect_language / wm_lang_pick_rows).  The
references and the cases are tests/lang_ref.py's: HF's mask + argmax for the pick, the one-clip call with a scalar language for every row of a
list call (the batch-invariance contract the suite holds makes that comparison exact), the default grouped call for group_by_language=False.  The
clips and language ids were chosen on the CPU (lang_ref.mix_guard holds their conditions and is asserted before anything is compared)."""
import contextlib
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lang_ref as L
from helpers import MedusaConfig, GenParams, ACCEPT_GREEDY, synth, clip_for
from oracle.whisper_medusa_oracle import Oracle
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu
NEW = 10


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=L.TAP_V)
def tap_model(gpu, request):
    V = request.param
    cfg = MedusaConfig.micro(vocab=V)
    m = WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=3), device=gpu, max_batch=1)
    yield V, m
    m.engine.close()


@pytest.mark.parametrize("n", L.TAP_N)
def test_tap_equals_hf(tap_model, n):
    V, m = tap_model
    ids = L.tap_lang_ids(V, n)
    for R_ in L.TAP_R:
        rows = L.tap_rows(V, R_, ids)
        want = L.hf_pick(rows, ids)
        got = m.engine.lang_pick_rows(rows, ids)
        assert np.array_equal(got, want), (R_, got, want)
        assert np.array_equal(m.engine.lang_pick_rows(rows, ids[::-1]), want)           # the order of lang_ids does not matter
        assert np.array_equal(m.engine.lang_pick_rows(rows, sorted(ids)), want)
    rows = L.tap_rows(V, 33, ids)
    back = m.engine.lang_pick_rows(rows[::-1], ids)
    assert np.array_equal(back[::-1], L.hf_pick(rows, ids))                              # nor the row's slot
    twice = m.engine.lang_pick_rows(np.concatenate([rows[4:5]] * 17), ids)               # one row in 17 slots, over two row groups
    assert len(set(twice.tolist())) == 1 and twice[0] == L.hf_pick(rows[4:5], ids)[0]


def test_tap_bad_arguments_come_back_with_their_reason(tap_model):
    V, m = tap_model
    eng = m.engine
    rows = np.zeros((2, V), dtype=np.float32)
    for bad, word in (([], "n must be"), (list(range(257)), "n must be"), ([3, V], "outside the vocabulary"), ([3, -1], "outside the vocabulary"),
                      ([3, 4, 3], "given twice")):
        with pytest.raises(ValueError, match=word):
            eng.lang_pick_rows(rows, bad)
    with pytest.raises(ValueError, match=r"\[R, vocab\]"):
        eng.lang_pick_rows(rows[:, :-1], [3])
    assert eng.lang_pick_rows(rows, [5, 3]).tolist() == [3, 3]                           # still usable: an all-equal row gives the smallest id


# ---- the decode rig ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(gpu):
    cfg, sd = L.mix_checkpoint()
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=8)
    feats = m.extract_features([clip_for(cfg, c) for c in L.MIX_CLIPS])
    orc = Oracle(cfg, sd, sim="bf16")
    detected = L.mix_guard(orc, cfg, L.oracle_encs(orc, cfg, L.MIX_CLIPS))      # the guard, on the reference alone, before anything is compared
    yield dict(cfg=cfg, sd=sd, m=m, feats=feats, detected=detected, gpu=gpu)
    m.engine.close()


@contextlib.contextmanager
def _encodes(m):
    seen, real = [], m.engine.encode
    m.engine.encode = lambda f: (seen.append(f.shape[0]), real(f))[1]
    try:
        yield seen
    finally:
        m.engine.encode = real


def _seq(out):
    return out["sequences"] if isinstance(out, dict) else out


def _alone(rig, langs, one_kw=None, **kw):
    """The one-clip call with the scalar language of every clip."""
    m, feats = rig["m"], rig["feats"]
    return [m.generate(feats[b: b + 1], language=langs[b], **kw, **(one_kw(b) if one_kw else {})) for b in range(len(langs))]


def _check_rows(rig, out, alone, langs):
    cfg = rig["cfg"]
    t = _seq(out)
    for b, a in enumerate(alone):
        a = _seq(a)[0].tolist()
        assert t[b, : len(a)].tolist() == a, (b, t[b].tolist(), a)
        assert all(v == cfg.pad_token_id for v in t[b, len(a):].tolist())
        assert cfg.lang_to_id[langs[b]] in a[:4]


# ---- 2. detection on the device --------------------------------------------------------------------------------------------------------------
def test_detect_language_equals_the_host_path(rig):
    cfg, m, feats = rig["cfg"], rig["m"], rig["feats"]
    eng = m.engine
    toks = sorted(cfg.lang_to_id, key=lambda k: cfg.lang_to_id[k])
    ids = [cfg.lang_to_id[t] for t in toks]
    eng.encode(feats)
    z = eng.forward_logits([[cfg.decoder_start_token_id]] * 4, 0, True)[0, :, 0].numpy()
    want = L.hf_pick(z, ids).tolist()
    assert [next(k for k, v in cfg.lang_to_id.items() if v == t) for t in want] == rig["detected"]     # (the chosen clips: the reference's languages)
    eng.encode(feats)
    got4 = eng.detect_language(ids, cfg.decoder_start_token_id)
    assert got4 == want and got4 == eng.detect_language(ids[::-1], cfg.decoder_start_token_id)
    for b in range(4):                                                                   # every clip's answer at B = 4 is its answer at B = 1
        eng.encode(feats[b: b + 1])
        z1 = eng.forward_logits([[cfg.decoder_start_token_id]], 0, True)[0, :, 0].numpy()
        eng.encode(feats[b: b + 1])
        assert eng.detect_language(ids, cfg.decoder_start_token_id) == L.hf_pick(z1, ids).tolist() == [got4[b]]
    assert m.detect_language(feats) == rig["detected"]                                   # the public host path
    eng.encode(feats)
    with pytest.raises(ValueError, match="start_token"):
        eng.detect_language(ids, cfg.vocab_size)
    with pytest.raises(ValueError, match="given twice"):
        eng.detect_language(ids + ids[:1], cfg.decoder_start_token_id)


# ---- 3. a mixed list on the three paths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["medusa", "vanilla", "timestamps"])
def test_mixed_list_equals_the_one_clip_calls(rig, path):
    m, feats, langs = rig["m"], rig["feats"], list(L.MIX_LIST)
    kw = dict(max_new_tokens=NEW, **{"medusa": {}, "vanilla": {"vanilla": True}, "timestamps": {"return_timestamps": True}}[path])
    with _encodes(m) as seen:
        out = m.generate(feats, language=langs, **kw)
    assert seen == [4]                                                                   # exactly one encoder pass
    assert out[:, 1].tolist() == [rig["cfg"].lang_to_id[l] for l in langs]
    _check_rows(rig, out, _alone(rig, langs, **kw), langs)
    same = m.generate(feats, language=["de"] * 4, **kw)                                  # a list of equal entries: the scalar call
    assert same.tolist() == m.generate(feats, language="de", **kw).tolist()


# ---- 4. the same equality, one short case per feature ----------------------------------------------------------------------------------------
def test_with_prompt_ids(rig):
    langs, pid = list(L.MIX_LIST), torch.tensor([rig["cfg"].prev_sot_token_id, 41, 42, 43])
    kw = dict(max_new_tokens=NEW, prompt_ids=pid)
    out = rig["m"].generate(rig["feats"], language=langs, **kw)
    assert out[:, 5].tolist() == [rig["cfg"].lang_to_id[l] for l in langs]
    t = _seq(out)
    for b, a in enumerate(_alone(rig, langs, **kw)):
        a = a[0].tolist()
        assert t[b, : len(a)].tolist() == a


def test_with_sampling_seed(rig):
    langs = list(L.MIX_LIST)
    kw = dict(max_new_tokens=NEW, sampling_seed=11, temperature=0.7)
    out = rig["m"].generate(rig["feats"], language=langs, **kw)
    alone = _alone(rig, langs, one_kw=lambda b: dict(sampling_stream_ids=[b]), **kw)    # the same stream keys
    _check_rows(rig, out, alone, langs)
    assert out.tolist() != rig["m"].generate(rig["feats"], language=langs, max_new_tokens=NEW, vanilla=True).tolist()


def test_with_beams(rig):
    langs = list(L.MIX_LIST)
    kw = dict(max_new_tokens=NEW, num_beams=2, vanilla=True, return_dict_in_generate=True)
    out = rig["m"].generate(rig["feats"], language=langs, **kw)
    alone = _alone(rig, langs, **kw)
    _check_rows(rig, out, alone, langs)
    assert out["sequences_scores"].tolist() == [a["sequences_scores"][0].item() for a in alone]


def test_with_a_sequence_bias_table(rig):
    langs = list(L.MIX_LIST)
    plain = rig["m"].generate(rig["feats"], language=langs, max_new_tokens=NEW, vanilla=True)
    P = 4
    banned = {int(plain[b, P]) for b in range(4)}                                        # every clip's first token: banned, so every row changes
    kw = dict(max_new_tokens=NEW, vanilla=True, sequence_bias={**{(t,): float("-inf") for t in banned}, (101, 102): 3.0})
    out = rig["m"].generate(rig["feats"], language=langs, **kw)
    assert all(int(out[b, P]) not in banned for b in range(4))
    _check_rows(rig, out, _alone(rig, langs, **kw), langs)


def test_with_scores_and_a_skipped_clip(rig):
    cfg, m, feats, langs = rig["cfg"], rig["m"], rig["feats"], list(L.MIX_LIST)
    first = m.generate(feats, language=langs, max_new_tokens=NEW, return_token_logprobs=True)
    ns = sorted(first["no_speech_prob"].tolist())
    assert ns[0] < ns[-1]
    thr = 0.5 * (ns[0] + ns[-1])                                                          # at least one clip is skipped, at least one is not
    kw = dict(max_new_tokens=NEW, return_token_logprobs=True, no_speech_threshold=thr)
    out = m.generate(feats, language=langs, **kw)
    alone = _alone(rig, langs, **kw)
    _check_rows(rig, out, alone, langs)
    skipped = out["skipped"].tolist()
    assert any(skipped) and not all(skipped)
    rows = L.init_token_rows(cfg, langs)
    for b, a in enumerate(alone):
        n = int(a["lengths"][0])
        assert out["token_logprobs"][b, :n].tolist() == a["token_logprobs"][0, :n].tolist()
        for k in ("avg_logprob", "no_speech_prob", "skipped", "lengths"):
            assert out[k][b].item() == a[k][0].item(), (k, b)
        if skipped[b]:                                                                   # a skipped clip is ITS OWN prompt + EOS
            assert out["sequences"][b, : len(rows[b]) + 1].tolist() == rows[b] + [cfg.eos_token_id]


def test_with_token_timestamps(rig):
    langs = list(L.MIX_LIST)
    kw = dict(max_new_tokens=NEW, return_token_timestamps=True, alignment_heads=synth.synth_alignment_heads(rig["cfg"]))
    out = rig["m"].generate(rig["feats"], language=langs, **kw)
    alone = _alone(rig, langs, **kw)
    _check_rows(rig, out, alone, langs)
    for b, a in enumerate(alone):
        n = a["sequences"].shape[1]
        assert out["token_timestamps"][b, :n].tolist() == a["token_timestamps"][0].tolist()


def test_with_the_pool_at_two_contexts(rig):
    m, langs = rig["m"], list(L.MIX_LIST)
    want = m.generate(rig["feats"], language=langs, max_new_tokens=NEW)
    before = m._micro_batches
    m.set_micro_batches(2)
    try:
        out = m.generate(rig["feats"], language=langs, max_new_tokens=NEW)
        assert m.last_stats.get("micro_batches") == 2
    finally:
        m.set_micro_batches(before)
    assert out.tolist() == want.tolist()


def test_with_a_candidate_tree(gpu):
    """The Medusa loop over a candidate tree (medusa_choices with top-k > 1) reads its ids per stream as the chain does."""
    cfg = MedusaConfig.micro(K=4, medusa_choices=[1, 2, 2, 1, 1])
    cfg.is_multilingual, cfg.lang_to_id, cfg.task_to_id = True, dict(L.LANGS), dict(L.TASKS)
    m = WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=L.MIX_SEED), device=gpu, max_batch=4)
    feats = m.extract_features([clip_for(cfg, c) for c in L.MIX_CLIPS])
    langs = list(L.MIX_LIST)
    out = m.generate(feats, language=langs, max_new_tokens=NEW)
    for b in range(4):
        a = m.generate(feats[b: b + 1], language=langs[b], max_new_tokens=NEW)[0].tolist()
        assert out[b, : len(a)].tolist() == a and a[1] == cfg.lang_to_id[langs[b]]
    m.engine.close()


# ---- 5. group_by_language=False --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(return_dict_in_generate=True, return_token_logprobs=True, return_timestamps=True)], ids=["ids", "dict"])
def test_detection_on_the_device_equals_the_grouped_call(rig, kw):
    m, feats = rig["m"], rig["feats"]
    with _encodes(m) as grouped_enc:
        want = m.generate(feats, max_new_tokens=NEW, **kw)
    langs = list(m.detected_languages)
    assert langs == rig["detected"] and len(set(langs)) >= 2
    with _encodes(m) as seen:
        out = m.generate(feats, max_new_tokens=NEW, group_by_language=False, **kw)
    assert seen == [4] and len(grouped_enc) > 1 and m.detected_languages == langs        # one encoder pass against the grouped call's several
    assert _seq(out).tolist() == _seq(want).tolist()
    if kw:
        assert set(out.keys()) == set(want.keys()) and {"token_logprobs", "avg_logprob", "lengths"} <= set(out.keys())
        for k in want.keys():
            if torch.is_tensor(want[k]):
                assert out[k].tolist() == want[k].tolist(), k


# ---- 6. the sticky table is cleared ----------------------------------------------------------------------------------------------------------
def _gp(cfg, lang="<|de|>", rows=None):
    prompt = synth.default_prompt(cfg, lang)
    return GenParams(prompt=list(rows[0]) if rows else prompt, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id, suppress_tokens=[3, 5],
                     begin_suppress_tokens=list(cfg.begin_suppress_tokens), max_length=len(prompt) + NEW, hard_max_length=cfg.max_length,
                     accept_mode=ACCEPT_GREEDY, temperature=0.0, vanilla=True, prompts=rows)


def test_a_scalar_decode_after_a_list_decode_is_the_scalar_call(rig):
    cfg, eng, feats = rig["cfg"], rig["m"].engine, rig["feats"]
    rows = L.init_token_rows(cfg, L.MIX_LIST)
    eng.encode(feats)
    scalar = eng.decode(_gp(cfg), 4)
    mixed = eng.decode(_gp(cfg, rows=rows), 4)
    assert [s[:4] for s in mixed] == rows and mixed[0] == scalar[0] and mixed[1] != scalar[1]
    assert eng.decode(_gp(cfg), 4) == scalar                                             # cleared: a pooled context never inherits a table
    # what only a decode can check comes back with its reason
    for bad, word in ((rows[:3], "rows for a decode of 4 clips"), ([r + [7] for r in rows], "one common length"),
                      ([rows[0], rows[1], rows[2], rows[3][:3] + [cfg.vocab_size]], "outside the vocabulary")):
        with pytest.raises(ValueError, match=word):
            eng.decode(dataclasses.replace(_gp(cfg), prompts=bad), 4)                    # (wm_gen_params.prompt stays the four-token scalar prompt)
    ts_rows = [r[:3] for r in rows]
    ts_rows[2] = [cfg.timestamp_begin + 1] + ts_rows[2][1:]
    gts = dataclasses.replace(_gp(cfg, rows=ts_rows), timestamps=True, no_timestamps_token_id=cfg.no_timestamps_token_id)
    with pytest.raises(ValueError, match="row 2.*timestamp_begin"):
        eng.decode(gts, 4)
    assert eng.decode(_gp(cfg), 4) == scalar


# ---- 7. eager launches, graph replay, two tables ---------------------------------------------------------------------------------------------
LIST2 = ("<|fr|>", "<|fr|>", "<|en|>", "<|de|>")
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch
import lang_ref as L
from helpers import clip_for
from test_gpu_language_list import _gp, LIST2
from whisper_medusa import WhisperMedusaModel
cfg, sd = L.mix_checkpoint()
m = WhisperMedusaModel(cfg, sd, device=torch.device("cuda", 0), max_batch=8)
m.engine.encode(m.extract_features([clip_for(cfg, c) for c in L.MIX_CLIPS]))
out = []
for lst in (L.MIX_LIST, LIST2):
    out.append(dict(seqs=m.engine.decode(_gp(cfg, rows=L.init_token_rows(cfg, lst)), 4), graph_replays=m.engine.stats()["graph_replays"]))
print("RESULT " + json.dumps(out))
"""


def test_eager_launches_equal_graph_replay_over_two_tables(rig, tmp_path):
    cfg, eng, feats = rig["cfg"], rig["m"].engine, rig["feats"]
    eng.encode(feats)
    here, stats = [], []
    for lst in (L.MIX_LIST, LIST2):
        here.append(eng.decode(_gp(cfg, rows=L.init_token_rows(cfg, lst)), 4))
        stats.append(eng.stats())
    assert here[0] != here[1] and [s[:4] for s in here[1]] == L.init_token_rows(cfg, LIST2)
    # the key of the captured graphs does not see the ids: the second table replays the graph the first one left, from its second step on
    assert stats[1]["graph_replays"] == stats[1]["iterations_launched"] - 1 and stats[1]["graph_replays"] > 0
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, WM_NO_GRAPH="1")
    r = subprocess.run([sys.executable, str(script), os.path.dirname(os.path.abspath(__file__))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    assert [o["graph_replays"] for o in out] == [0, 0] and [o["seqs"] for o in out] == here
