"""Constrained decoding on the plain decode path on the GPU (include/wm.h wm_set_constraint / wm_constraint_rows).  The reference is
tests/constraint_ref.py: transformers' PrefixConstrainedLogitsProcessor in front of the existing references (sample_ref's processed row, filter_ref's
draw, the oracle's plain step, beam_ref's ClipBeams); tests/test_constraint_cpu.py holds, from that reference alone, the conditions these inputs
were chosen under."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import constraint_ref as C
import sample_ref as S
import beam_ref as R
from helpers import MedusaConfig, synth, clip_for
from whisper_medusa import WhisperMedusaModel
from whisper_medusa.engine import Engine

pytestmark = pytest.mark.gpu


def _model(cfg, sd, gpu, Bmax, act_fp16=False):
    return WhisperMedusaModel(cfg, sd, device=gpu, max_batch=Bmax, act_fp16=act_fp16)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=C.TAP_V)
def tap_model(gpu, request):
    V = request.param
    cfg = MedusaConfig.micro(vocab=V)
    m = _model(cfg, synth.synth_state_dict(cfg, seed=3), gpu, 1)
    yield V, cfg, m
    m.engine.close()


def _tap(eng, seqs, eos, P, rows, pre):
    """The tap against HF by value, and its count of allowed ids against the reference's."""
    got, n = eng.constraint_rows(seqs, eos, P, rows, pre)
    want = C.hf_rows(rows, pre, seqs, eos, P)
    assert np.array_equal(got, want), (len(seqs), P, np.argwhere(got != want)[:5])
    assert n.tolist() == [len(C.allowed(seqs, eos, p[P:])) for p in pre]
    return got


@pytest.mark.parametrize("R_", C.TAP_R)
def test_tap_equals_hf(tap_model, R_):
    V, cfg, m = tap_model
    eos, table = C.tap_eos(V), C.tap_table(V)
    for P in C.TAP_P:
        rows, pre = C.tap_rows(V, R_), C.tap_prefixes(V, R_, P)
        got = _tap(m.engine, table, eos, P, rows, pre)
        kept = np.isfinite(got)
        assert np.array_equal(got[kept], rows[kept])            # allowed elements come back as they went in
    one = [(10, 11, 12)]                                        # the one-sequence table
    _tap(m.engine, one, eos, 1, C.tap_rows(V, R_), C.tap_prefixes(V, R_, 1))


def test_tap_big_table_row_position_and_caller_order(tap_model):
    V, cfg, m = tap_model
    eng, eos = m.engine, C.tap_eos(V)
    big = C.big_table(V)
    assert len(big) == C.MAX_SEQS
    rows, pre = C.tap_rows(V, 33), C.big_prefixes(big, 33, 4)
    fwd = _tap(eng, big, eos, 4, rows, pre)
    assert len({int(np.isfinite(r).sum()) for r in fwd}) >= 3  # the root's five ids, inner nodes, rows that left the trie
    rev, _ = eng.constraint_rows(big, eos, 4, rows[::-1], pre[::-1])
    assert np.array_equal(rev[::-1], fwd)                       # the same row gives the same output wherever it stands in the call
    back, _ = eng.constraint_rows(big[::-1], eos, 4, rows, pre)
    assert np.array_equal(back, fwd)                            # the same set in another caller order gives the same rows
    table = C.tap_table(V)
    rows, pre = C.tap_rows(V, 33), C.tap_prefixes(V, 33, 4)
    a, na = eng.constraint_rows(table, eos, 4, rows, pre)
    b, nb = eng.constraint_rows(table[::-1], eos, 4, rows[::-1], pre[::-1])
    assert np.array_equal(b[::-1], a) and nb[::-1].tolist() == na.tolist()


# ---- 2. bad arguments ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_come_back_with_their_reason(gpu):
    cfg, sd = C.dec_checkpoint()
    m = _model(cfg, sd, gpu, 2)
    eng, V, eos = m.engine, cfg.vocab_size, cfg.eos_token_id
    gp = C.dec_gp(cfg)
    feats = m.extract_features([clip_for(cfg, 0), clip_for(cfg, 1)])
    eng.encode(feats)
    base = eng.decode(gp, 2)                                    # before any table was set
    many = [(a, b) for a in range(100, 230) for b in range(100, 230)][: C.MAX_SEQS + 1]
    for bad, word in (([], "n must be"), (many, "n must be"), ([tuple(range(100, 133))], "length"), ([()], "length"),
                      ([(V,)], "outside the vocabulary"), ([(101, -1)], "outside the vocabulary"), ([(101, 102), (103,), (101, 102)], "identical")):
        with pytest.raises(ValueError, match=word):
            eng.set_constraint(bad)
        with pytest.raises(ValueError, match=word):
            eng.constraint_rows(bad, eos, 1, np.zeros((1, V), np.float32), [[1, 2]])
    with pytest.raises(ValueError, match="prompt_len"):
        eng.constraint_rows([(101,)], eos, 3, np.zeros((1, V), np.float32), [[1, 2]])
    with pytest.raises(ValueError, match="eos"):
        eng.constraint_rows([(101, eos)], eos, 1, np.zeros((1, V), np.float32), [[1, 2]])
    ok = [(101, 102), (103,)]
    sup, bsup = gp.suppress_tokens[0], [t for t in gp.begin_suppress_tokens if t != eos][0]
    for bad_gp, word in ((dataclasses.replace(gp, vanilla=False, accept_mode=S.ACCEPT_TYPICAL, temperature=1.0, allowed_sequences=ok), "plain decode path"),
                         (dataclasses.replace(S.dec_gp(cfg, True, False), allowed_sequences=ok), "timestamp rules"),
                         (dataclasses.replace(gp, exp_decay=(2, 1.1), allowed_sequences=ok), "exponential decay"),
                         (dataclasses.replace(gp, allowed_sequences=[(101, eos, 102)]), "eos"),
                         (dataclasses.replace(gp, allowed_sequences=[(101, sup)]), "suppress list"),
                         (dataclasses.replace(gp, allowed_sequences=[(bsup, 101)]), "begin-suppress list")):
        eng.encode(feats)
        with pytest.raises(ValueError, match=word):
            eng.decode(bad_gp, 2)
        eng.encode(feats)
        assert eng.decode(gp, 2) == base                        # the context is usable afterwards, nothing left of the refused table
    eng.decode(dataclasses.replace(gp, allowed_sequences=[(bsup + 1, bsup)]), 2)       # (a begin-suppressed id behind the first place is fine)
    eng.close()
    tree = dataclasses.replace(cfg, medusa_choices=[1, 2, 1, 1, 1])
    mt = _model(tree, S._sr.ts_state_dict(tree, 21), gpu, 1)
    mt.engine.encode(mt.extract_features([clip_for(tree, 0)]))
    with pytest.raises(ValueError, match="candidate tree"):
        mt.engine.decode(dataclasses.replace(gp, allowed_sequences=ok), 1)
    mt.engine.close()


# ---- 3. / 4. the greedy and the sampled plain decode -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dec_rig(gpu):
    cfg, sd = C.dec_checkpoint()
    m = _model(cfg, sd, gpu, 4)
    ref = C.ConsRef(cfg, sd)
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in C.DEC_CLIPS]))
    enc = m.engine.encoder_output(4)
    encs = {c: enc[C.DEC_CLIPS.index(c)] for c in set(C.DEC_CLIPS)}
    yield dict(cfg=cfg, sd=sd, m=m, ref=ref, encs=encs)
    m.engine.close()


def _decode(rig, gp, clips=C.DEC_CLIPS):
    cfg, m = rig["cfg"], rig["m"]
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in clips]))
    return m.engine.decode(gp, len(clips))


@pytest.mark.parametrize("name", sorted(C.DEC_CASES))
def test_greedy_decode_equals_the_reference(dec_rig, name):
    cfg = dec_rig["cfg"]
    gp = C.dec_gp(cfg, C.DEC_CASES[name][0])
    ents = C.case_entries(name)
    runs = C.dec_guards(dec_rig["ref"], gp, dec_rig["encs"], C.DEC_TABLE, ents)       # the guards, on the engine's own encoder output
    gpc = dataclasses.replace(gp, allowed_sequences=C.DEC_TABLE, sequence_bias=ents)
    seqs = _decode(dec_rig, gpc)
    P, eos = len(gp.prompt), gp.eos_token_id
    for b, c in enumerate(C.DEC_CLIPS):                         # all four streams, strictly: every reference decision clears 10 x TIE
        assert seqs[b] == runs[c][0], (name, b, seqs[b], runs[c][0])
        assert C.is_member(seqs[b], P, eos, C.DEC_TABLE)
    assert dec_rig["m"].engine.stats()["graph_replays"] > 0
    assert _decode(dec_rig, gpc, C.DEC_CLIPS[::-1])[::-1] == seqs          # the batch reversed: every clip gives the ids it had


def test_sampled_decode_equals_the_reference(dec_rig):
    cfg, m, ref = dec_rig["cfg"], dec_rig["m"], dec_rig["ref"]
    gp = C.dec_gp(cfg)
    T, seed, k = C.SAMPLE_CASE["T"], C.SAMPLE_CASE["seed"], C.SAMPLE_CASE["top_k"]
    runs = C.sample_guards(ref, gp, dec_rig["encs"], C.DEC_TABLE, T, seed, (k, 1.0, 0.0))
    gps = dataclasses.replace(gp, allowed_sequences=C.DEC_TABLE, sampling_temperature=T, sampling_seed=seed, sampling_keys=list(C.DEC_KEYS),
                              sampling_top_k=k)
    seqs = _decode(dec_rig, gps)
    for b, (c, key) in enumerate(zip(C.DEC_CLIPS, C.DEC_KEYS)):
        assert seqs[b] == runs[(c, key)][0], (b, seqs[b], runs[(c, key)][0])
        assert C.is_member(seqs[b], len(gp.prompt), gp.eos_token_id, C.DEC_TABLE)
    # the same stream key gives the same text at batch 1
    b = 3
    alone = _decode(dec_rig, dataclasses.replace(gps, sampling_keys=[C.DEC_KEYS[b]]), (C.DEC_CLIPS[b],))
    assert alone == [seqs[b]]


# ---- 5. beam decode --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.BEAM_CASES))
def test_beam_decode_equals_the_reference(gpu, name):
    case = C.BEAM_CASES[name]
    cfg, sd, gp = R.e2e_setup(case)
    n, lp, es, nret = case[2], case[3], case[4], case[7]
    m = _model(cfg, sd, gpu, case[8])
    try:
        eng = m.engine
        feats = m.extract_features([clip_for(cfg, c) for c in case[1]])
        eng.encode(feats)
        enc = eng.encoder_output(len(case[1]))
        runs, seqs = C.beam_reference(name, {c: enc[i] for i, c in enumerate(case[1])})[4:6]
        C.beam_guards(runs, gp, nret)                           # the CPU guard holds on the engine's own encoder output too
        G = max(1, case[8] // n)                                # clips per decode: max_batch // n
        for g0 in range(0, len(case[1]), G):
            eng.encode(feats[g0: g0 + G])
            gpb = dataclasses.replace(gp, num_beams=n, length_penalty=lp, early_stopping=es, allowed_sequences=seqs)
            best = eng.decode(gpb, len(feats[g0: g0 + G]))
            for c, (plain, cb) in enumerate(runs[g0: g0 + G]):
                last = len(cb.steps) - 1
                for r in range(nret):
                    ids, score = eng.beam_result(c, r)
                    assert ids == cb.fin_ids[r], (name, g0 + c, r, ids, cb.fin_ids[r])
                    assert abs(score - float(cb.fin_score[r])) <= R.e2e_bound(last), (name, g0 + c, r, score, float(cb.fin_score[r]))
                assert best[c] == cb.fin_ids[0] != plain.fin_ids[0]
        # generate(): num_return_sequences rows per clip and their scores
        out = m.generate(feats[:G], vanilla=True, num_beams=n, num_return_sequences=nret, length_penalty=lp, early_stopping=es, max_new_tokens=case[9],
                         language="en", allowed_sequences=[list(s) for s in seqs], return_dict_in_generate=True)
        for c, (plain, cb) in enumerate(runs[:G]):
            for r in range(nret):
                row = out["sequences"][c * nret + r].tolist()
                assert row[: len(cb.fin_ids[r])] == cb.fin_ids[r] and all(t == gp.pad_token_id for t in row[len(cb.fin_ids[r]):])
                assert abs(float(out["sequences_scores"][c * nret + r]) - float(cb.fin_score[r])) <= R.e2e_bound(len(cb.steps) - 1)
    finally:
        m.engine.close()


def test_under_populated_beams(gpu):
    """Three sequences under four beams: fewer finite candidates than 2n, where HF's top-k order among -inf candidates is undefined — no HF
    comparison; what must hold whatever that order is.  A score that HF's fp32 -1e9 arithmetic has shifted stands for -inf (an entry never set:
    -1e9; a beam kept alive only because fewer than n candidates were left: (-1e9 + w) / length >= -1e9 / 8 at 8 new tokens): a hypothesis counts
    as found when its score lies above REAL = -1e6, which no sum of at most 8 log-probabilities of a 1031-id vocabulary comes near."""
    REAL = -1.0e6
    case = C.FEW_CASE
    cfg, sd, gp = R.e2e_setup(case)
    m = _model(cfg, sd, gpu, case[8])
    try:
        eng = m.engine
        feats = m.extract_features([clip_for(cfg, c) for c in case[1]])
        P, eos = len(gp.prompt), gp.eos_token_id
        members = [list(gp.prompt) + list(s) + [eos] for s in C.FEW_TABLE]
        res = {}
        for n in (4, 2):
            eng.encode(feats)
            eng.decode(dataclasses.replace(gp, num_beams=n, allowed_sequences=C.FEW_TABLE), 1)
            res[n] = [eng.beam_result(0, r) for r in range(n)]
            real = [(ids, s) for ids, s in res[n] if s > REAL]
            assert not any(np.isnan(s) for _, s in res[n]) and len(real) >= 1
            assert all(ids in members for ids, _ in real), real
            assert len({tuple(ids) for ids, _ in real}) == len(real)                                   # distinct
            assert all(a[1] >= b[1] for a, b in zip(real[:-1], real[1:])) and all(np.isfinite(s) for _, s in real)
            assert res[n][: len(real)] == real                 # the real hypotheses come first
        assert len([1 for _, s in res[4] if s > REAL]) == 3  # four beams find all three members
        # rank 0 of the four-beam run against the two-beam run, where that run satisfies the CPU guard (2n finite candidates at every step)
        eng.encode(feats)
        enc = eng.encoder_output(1)[0]
        from oracle.whisper_medusa_oracle import Oracle
        orc = Oracle(cfg, sd, sim="bf16", act="hilo")
        cb = C.beam_run(R.OracleBeams(orc, enc, 2), gp, 2, cfg.vocab_size, 1.0, False, C.FEW_TABLE)
        if all(np.isfinite(rec["cand_val"]).all() and not rec["planted"] for rec in cb.steps):
            assert res[4][0][0] == res[2][0][0]
    finally:
        m.engine.close()


# ---- 6. graph reuse --------------------------------------------------------------------------------------------------------------------------
def test_two_tables_of_one_size_replay_one_graph(gpu):
    cfg, sd = C.dec_checkpoint()
    m = _model(cfg, sd, gpu, 4)
    graphs = not os.environ.get("WM_NO_GRAPH")
    try:
        gp = C.dec_gp(cfg)
        t1, t2 = C.DEC_TABLE, C.dec_table(seed=2)[: len(C.DEC_TABLE)]
        assert len(t1) == len(t2) and set(t1) != set(t2)
        feats = m.extract_features([clip_for(cfg, c) for c in C.DEC_CLIPS])
        req = {"plain": gp, "t1": dataclasses.replace(gp, allowed_sequences=t1), "t2": dataclasses.replace(gp, allowed_sequences=t2)}
        fresh = {}
        for name, g in req.items():                             # every request on a context of its own
            eng = Engine(cfg, m._blob, m._offsets, max_batch=4, device=gpu, act_fp16=False)
            try:
                eng.encode(feats)
                fresh[name] = eng.decode(g, 4)
                st = eng.stats()
                assert st["iterations_launched"] >= 4, (name, st)
                if graphs:
                    assert st["iterations_launched"] - st["graph_replays"] == 2, (name, st)    # a fresh context captures at its third iteration
            finally:
                eng.close()
        assert fresh["t1"] != fresh["t2"] != fresh["plain"]
        eng = m.engine
        eng.encode(feats)
        for name, reuse in (("t1", False), ("t2", True), ("t1", True), ("plain", False), ("t2", False)):
            ids = eng.decode(req[name], 4)
            st = eng.stats()
            assert ids == fresh[name], (name, ids, fresh[name])
            if graphs:                                          # equal sizes: replayed from the second iteration on, no capture
                assert st["iterations_launched"] - st["graph_replays"] == (1 if reuse else 2), (name, reuse, st)
    finally:
        m.engine.close()
