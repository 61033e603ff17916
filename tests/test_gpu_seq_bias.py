"""Sequence bias, bad words and hotwords on the plain decode path on the GPU (include/wm.h wm_set_sequence_bias / wm_seq_bias_rows, DESIGN.md
§2j).  The reference is tests/seq_bias_ref.py: transformers' SequenceBiasLogitsProcessor in front of the existing references (sample_ref's
processed row and draw, the oracle's plain step, beam_ref's ClipBeams); tests/test_seq_bias_cpu.py holds, from that reference alone, the
conditions these inputs were chosen under."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq_bias_ref as B
import sample_ref as S
import beam_ref as R
from helpers import MedusaConfig, synth, clip_for
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu
NEG = float("-inf")


def _model(cfg, sd, gpu, Bmax, act_fp16=False):
    return WhisperMedusaModel(cfg, sd, device=gpu, max_batch=Bmax, act_fp16=act_fp16)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=B.TAP_V)
def tap_model(gpu, request):
    V = request.param
    cfg = MedusaConfig.micro(vocab=V)
    m = _model(cfg, synth.synth_state_dict(cfg, seed=3), gpu, 1)
    yield V, cfg, m
    m.engine.close()


@pytest.mark.parametrize("R_", B.TAP_R)
def test_tap_equals_hf(tap_model, R_):
    V, cfg, m = tap_model
    ents = B.tap_entries(V)
    rows, pre = B.tap_rows(V, R_), B.tap_prefixes(V, R_)
    got = m.engine.seq_bias_rows(ents, rows, pre)
    assert np.array_equal(got, B.hf_rows(rows, pre, ents))
    # without one-token entries a row with no match comes back unchanged
    multi = B.tap_entries(V, singles=False)
    got = m.engine.seq_bias_rows(multi, rows, pre)
    want = B.hf_rows(rows, pre, multi)
    assert np.array_equal(got, want)
    same = ~(want != rows).any(axis=1)
    assert np.array_equal(got[same], rows[same]) and (R_ == 1 or (same.any() and not same.all()))


def test_tap_row_position_order_and_table_sizes(tap_model):
    V, cfg, m = tap_model
    eng = m.engine
    ents = B.tap_entries(V)
    rows, pre = B.tap_rows(V, 33), B.tap_prefixes(V, 33)
    fwd = eng.seq_bias_rows(ents, rows, pre)
    rev = eng.seq_bias_rows(ents, rows[::-1], pre[::-1])
    assert np.array_equal(rev[::-1], fwd)                       # the same row gives the same output wherever it stands in the call
    # the caller's order is the order of the sum: the table reversed follows HF on the reversed table
    back = ents[::-1]
    got = eng.seq_bias_rows(back, rows, pre)
    assert np.array_equal(got, B.hf_rows(rows, pre, back)) and not np.array_equal(got, fwd)
    # n = 1 and n = 1024 (more than one block of groups)
    one = [((21, 7), 1.5)]
    assert np.array_equal(eng.seq_bias_rows(one, rows, pre), B.hf_rows(rows, pre, one))
    big = B.big_table(V)
    assert np.array_equal(eng.seq_bias_rows(big, rows, pre), B.hf_rows(rows, pre, big))


def test_bad_arguments_come_back_with_their_reason(gpu):
    cfg, sd = B.dec_checkpoint()
    m = _model(cfg, sd, gpu, 2)
    eng, V, eos = m.engine, cfg.vocab_size, cfg.eos_token_id
    for bad, word in (([], "n must be"), ([((t,), 1.0) for t in range(1025)], "n must be"), ([(tuple(range(1, 18)), 1.0)], "length"),
                      ([((), 1.0)], "length"), ([((V,), 1.0)], "outside the vocabulary"), ([((3, -1), 1.0)], "outside the vocabulary"),
                      ([((3,), float("nan"))], "NaN"), ([((3,), float("inf"))], r"\+inf"), ([((3, 4), 1.0), ((5,), 2.0), ((3, 4), -1.0)], "identical")):
        with pytest.raises(ValueError, match=word):
            eng.set_sequence_bias(bad)
        with pytest.raises(ValueError, match=word):
            eng.seq_bias_rows(bad, np.zeros((1, V), np.float32), [[1, 2]])
    gp = B.dec_gp(cfg, "plain")
    eng.encode(m.extract_features([clip_for(cfg, 0), clip_for(cfg, 1)]))
    with pytest.raises(ValueError, match="eos"):
        eng.decode(dataclasses.replace(gp, sequence_bias=[((5, eos), NEG)]), 2)
    with pytest.raises(ValueError, match="plain decode path"):
        eng.decode(dataclasses.replace(gp, vanilla=False, accept_mode=S.ACCEPT_TYPICAL, temperature=1.0, sequence_bias=[((5,), 1.0)]), 2)
    plain = eng.decode(gp, 2)                                   # the context is usable afterwards, nothing left of the refused tables
    assert plain == eng.decode(dataclasses.replace(gp, sequence_bias=None), 2)
    eng.close()
    tree = dataclasses.replace(cfg, medusa_choices=[1, 2, 1, 1, 1])
    mt = _model(tree, S._sr.ts_state_dict(tree, 21), gpu, 1)
    mt.engine.encode(mt.extract_features([clip_for(tree, 0)]))
    with pytest.raises(ValueError, match="candidate tree"):
        mt.engine.decode(dataclasses.replace(gp, sequence_bias=[((5,), 1.0)]), 1)
    mt.engine.close()


# ---- 2. / 3. the greedy and the sampled plain decode -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dec_rig(gpu):
    cfg, sd = B.dec_checkpoint()
    m = _model(cfg, sd, gpu, 4)
    ref = B.BiasRef(cfg, sd)
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in B.DEC_CLIPS]))
    enc = m.engine.encoder_output(4)
    encs = {c: enc[B.DEC_CLIPS.index(c)] for c in set(B.DEC_CLIPS)}
    rig = dict(cfg=cfg, sd=sd, m=m, ref=ref, encs=encs, cache={})
    yield rig
    m.engine.close()


def _case(rig, name):
    """(gp, entries, {clip: (ids, gaps)}): the entries chosen on the CPU reference, the reference runs and their guards on the engine's own
    encoder output."""
    if name not in rig["cache"]:
        gp = B.dec_gp(rig["cfg"], "plain" if name == "plain2" else name)
        ents = B.DEC_ENTRIES[name]
        rig["cache"][name] = (gp, ents, B.dec_guards(rig["ref"], gp, rig["encs"], ents))
    return rig["cache"][name]


def _decode(rig, gp, ents, clips=B.DEC_CLIPS):
    cfg, m = rig["cfg"], rig["m"]
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in clips]))
    return m.engine.decode(dataclasses.replace(gp, sequence_bias=ents), len(clips))


@pytest.mark.parametrize("name", ["plain", "ts", "ts_rep"])
def test_greedy_decode_equals_the_reference(dec_rig, name):
    gp, ents, runs = _case(dec_rig, name)
    seqs = _decode(dec_rig, gp, ents)
    for b, c in enumerate(B.DEC_CLIPS):                         # all four streams, strictly: every reference decision clears 10 x TIE
        assert seqs[b] == runs[c][0], (name, b, seqs[b], runs[c][0])
    assert dec_rig["m"].engine.stats()["graph_replays"] > 0
    rev = _decode(dec_rig, gp, ents, B.DEC_CLIPS[::-1])
    assert rev[::-1] == seqs                                    # the batch reversed: every clip gives the ids it had


def test_second_table_and_clearing_on_one_context(dec_rig):
    gp, ents, runs = _case(dec_rig, "plain")
    gp2, ents2, runs2 = _case(dec_rig, "plain2")
    eng = dec_rig["m"].engine
    base = _decode(dec_rig, gp, None)                           # the engine's unbiased ids, before this test sets a table
    first = _decode(dec_rig, gp, ents)
    second = _decode(dec_rig, gp2, ents2)                       # another number of groups: the launch carries it, the graph is captured anew
    assert [len(B.groups_of(e)) for e in (ents, ents2, ents[:2])] == [3, 2, 2] and ents != ents2
    for b, c in enumerate(B.DEC_CLIPS):
        assert first[b] == runs[c][0] and second[b] == runs2[c][0] and first[b] != second[b]
    two = _decode(dec_rig, gp, ents[:2])                        # as many groups as the last: the captured graph replays over the new table
    want2 = {c: dec_rig["ref"].decode(dec_rig["encs"][c], gp, ents[:2]) for c in set(B.DEC_CLIPS)}
    for b, c in enumerate(B.DEC_CLIPS):
        if min(want2[c][1]) >= 10 * S.TIE:
            assert two[b] == want2[c][0]
    off = _decode(dec_rig, gp, None)                            # cleared: the unbiased ids — the captured graph does not keep the bias
    plain = {c: dec_rig["ref"].decode(dec_rig["encs"][c], gp, None) for c in set(B.DEC_CLIPS)}
    assert off == base
    for b, c in enumerate(B.DEC_CLIPS):
        assert off[b] != first[b]
        if min(plain[c][1]) >= 10 * S.TIE:                      # (the unbiased run is no chosen case: compared where the reference itself is decisive)
            assert off[b] == plain[c][0], b
    eng.set_sequence_bias(ents)                                 # set directly, then cleared directly: decode() follows its parameters
    eng.set_sequence_bias(None)
    assert _decode(dec_rig, gp, None) == off


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dataclasses, torch
import seq_bias_ref as B
import sample_ref as S
from helpers import clip_for
from whisper_medusa import WhisperMedusaModel
cfg, sd = B.dec_checkpoint()
m = WhisperMedusaModel(cfg, sd, device=torch.device("cuda", 0), max_batch=4, act_fp16=False)
gp = B.dec_gp(cfg, "ts")
ents = B.DEC_ENTRIES["ts"]
m.engine.encode(m.extract_features([clip_for(cfg, c) for c in B.DEC_CLIPS]))
seqs = m.engine.decode(dataclasses.replace(gp, sequence_bias=ents), 4)
print("RESULT " + json.dumps(dict(seqs=seqs, graph_replays=m.engine.stats()["graph_replays"])))
"""


def test_eager_launches_equal_graph_replay(dec_rig, tmp_path):
    """WM_NO_GRAPH=1 in a fresh child process: the same ids as the graph replay of this process."""
    gp, ents, runs = _case(dec_rig, "ts")
    here = _decode(dec_rig, gp, ents)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, WM_NO_GRAPH="1")
    r = subprocess.run([sys.executable, str(script), os.path.dirname(os.path.abspath(__file__))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    assert out["graph_replays"] == 0 and out["seqs"] == here


def test_sampled_decode_equals_the_reference(dec_rig):
    cfg, m, ref = dec_rig["cfg"], dec_rig["m"], dec_rig["ref"]
    gp = B.dec_gp(cfg, "plain")
    T, seed = B.SAMPLE_CASE["T"], B.SAMPLE_CASE["seed"]
    ents = B.SAMPLE_ENTRIES                                     # a boost and a ban
    runs = B.sample_guards(ref, gp, dec_rig["encs"], ents, T, seed)
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in B.DEC_CLIPS]))
    gps = dataclasses.replace(gp, sequence_bias=ents, sampling_temperature=T, sampling_seed=seed, sampling_keys=list(S.DEC_KEYS))
    seqs = m.engine.decode(gps, 4)
    for b, (c, k) in enumerate(zip(B.DEC_CLIPS, S.DEC_KEYS)):
        assert seqs[b] == runs[(c, k)][0], (b, seqs[b], runs[(c, k)][0])


# ---- 4. beam decode --------------------------------------------------------------------------------------------------------------------------
_BEAM = {}


def _beam(gpu, name):
    """(model, feats, gp, case, reference runs on the engine's own encoder output, entries chosen on the CPU reference)."""
    if name not in _BEAM:
        case, pick = B.beam_case(name)
        cfg, sd, gp = R.e2e_setup(case)
        ents = B.BEAM_ENTRIES[name]                             # chosen on the CPU reference (tests/test_seq_bias_cpu.py holds their conditions)
        m = _model(cfg, sd, gpu, case[8])
        feats = m.extract_features([clip_for(cfg, c) for c in case[1]])
        m.engine.encode(feats)
        enc = m.engine.encoder_output(len(case[1]))
        runs = B.beam_reference(name, {c: enc[i] for i, c in enumerate(case[1])}, ents)[4]
        _BEAM[name] = (m, feats, gp, case, runs, ents)
    return _BEAM[name]


@pytest.fixture(scope="module", autouse=True)
def _close_beam_models():
    yield
    for v in _BEAM.values():
        v[0].engine.close()
    _BEAM.clear()


@pytest.mark.parametrize("name", sorted(B.BEAM_CASES))
def test_beam_decode_equals_the_reference(gpu, name):
    m, feats, gp, case, runs, ents = _beam(gpu, name)
    n, lp, es = case[2], case[3], case[4]
    B.beam_guards(runs)                                         # no indecisive step on the engine's own encoder output either
    eng = m.engine
    eng.encode(feats)
    gpb = dataclasses.replace(gp, num_beams=n, length_penalty=lp, early_stopping=es, sequence_bias=ents)
    best = eng.decode(gpb, len(case[1]))
    for c, (plain, cb, widen) in enumerate(runs):
        last = len(cb.steps) - 1
        for r in range(n):
            ids, score = eng.beam_result(c, r)
            if r == 0 or not B.beam_indecisive(cb, widen, r):   # (rank 0 is guarded; a deeper rank where its order is decided too)
                assert ids == cb.fin_ids[r], (name, c, r, ids, cb.fin_ids[r])
                assert abs(score - float(cb.fin_score[r])) <= R.e2e_bound(last), (name, c, r, score, float(cb.fin_score[r]))
        assert best[c] == cb.fin_ids[0]
    assert best[0] != runs[0][0].fin_ids[0]                    # the winning hypothesis of clip 0 changed
    # the same call without the table: the unbiased winner again
    eng.encode(feats)
    off = eng.decode(dataclasses.replace(gpb, sequence_bias=None), len(case[1]))
    assert off[0] == runs[0][0].fin_ids[0]


# ---- 5. generate() ---------------------------------------------------------------------------------------------------------------------------
def _own(row, P, eos):
    s = [int(t) for t in row]
    return s[: s.index(eos, P) + 1] if eos in s[P:] else s


def test_generate_runs_the_engine_level_cases(dec_rig):
    cfg, m = dec_rig["cfg"], dec_rig["m"]
    gp, ents, runs = _case(dec_rig, "plain")
    P, eos = len(gp.prompt), gp.eos_token_id
    feats = m.extract_features([clip_for(cfg, c) for c in B.DEC_CLIPS])
    kw = dict(vanilla=True, max_new_tokens=B.DEC_MAX_NEW, language="en", suppress_tokens=list(gp.suppress_tokens))
    want = [_own(runs[c][0], P, eos) for c in B.DEC_CLIPS]
    before = m.generate(feats, **kw)
    # sequence_bias: HF's dict form, the whole table
    out = m.generate(feats, sequence_bias={i: b for i, b in ents}, **kw)
    assert [_own(r, P, eos) for r in out.tolist()] == want
    # the bans as bad_words_ids, the boost as sequence_bias (list form)
    out = m.generate(feats, sequence_bias=[[list(ents[0][0]), ents[0][1]]], bad_words_ids=[list(i) for i, b in ents if b == NEG], **kw)
    assert [_own(r, P, eos) for r in out.tolist()] == want
    # hotwords on a fake tokenizer: the expansion is a table of its own; the engine follows the reference under that table
    word = list(ents[0][0])
    tok = B.FakeTokenizer({"w": word, " w": word[1:]})
    from whisper_medusa import api
    hw = api.hotword_entries(["w"], ents[0][1], tok)
    ref_hw = {c: dec_rig["ref"].decode(dec_rig["encs"][c], gp, hw) for c in set(B.DEC_CLIPS)}
    out = m.generate(feats, hotwords=["w"], hotword_boost=ents[0][1], tokenizer=tok, **kw)
    for b, c in enumerate(B.DEC_CLIPS):
        if min(ref_hw[c][1]) >= 10 * S.TIE:
            assert _own(out[b].tolist(), P, eos) == _own(ref_hw[c][0], P, eos), b
    # without the new arguments: the ids of the call before any table was set, id for id
    assert torch.equal(m.generate(feats, **kw), before)
    assert before.tolist() != out.tolist()


def test_generate_with_beams_and_a_table(gpu):
    m, feats, gp, case, runs, ents = _beam(gpu, "n2")
    kw = dict(vanilla=True, num_beams=case[2], length_penalty=case[3], early_stopping=case[4], max_new_tokens=case[9], language="en",
              return_dict_in_generate=True)
    before = m.generate(feats, **kw)
    out = m.generate(feats, sequence_bias={ents[0][0]: ents[0][1]}, bad_words_ids=[list(ents[1][0])], **kw)
    cb = runs[0][1]
    row = out["sequences"][0].tolist()
    assert row[: len(cb.fin_ids[0])] == cb.fin_ids[0] and all(t == gp.pad_token_id for t in row[len(cb.fin_ids[0]):])
    last = len(cb.steps) - 1
    assert abs(float(out["sequences_scores"][0]) - float(cb.fin_score[0])) <= R.e2e_bound(last)
    after = m.generate(feats, **kw)
    assert torch.equal(after["sequences"], before["sequences"]) and torch.equal(after["sequences_scores"], before["sequences_scores"])
    assert before["sequences"][0].tolist()[: len(runs[0][0].fin_ids[0])] == runs[0][0].fin_ids[0]


# ---- 6. the other numerics contract ------------------------------------------------------------------------------------------------------------
def test_default_contract_library_has_the_same_kernel(gpu):
    """libwm_f16.so (the fp16 single-plane decode contract): the tap equals HF bit for bit there too; a biased decode does not depend on the
    batch slot and the cleared context gives the unbiased ids again."""
    cfg, sd = B.dec_checkpoint()
    m = _model(cfg, sd, gpu, 4, act_fp16=True)
    V = cfg.vocab_size
    ents = B.tap_entries(V)
    rows, pre = B.tap_rows(V, 33), B.tap_prefixes(V, 33)
    assert np.array_equal(m.engine.seq_bias_rows(ents, rows, pre), B.hf_rows(rows, pre, ents))
    gp = B.dec_gp(cfg, "ts")
    feats = m.extract_features([clip_for(cfg, c) for c in B.DEC_CLIPS])
    m.engine.encode(feats)
    plain = m.engine.decode(gp, 4)
    table = [((int(plain[0][len(gp.prompt) + 1]),), NEG), ((int(plain[1][len(gp.prompt)]), int(plain[1][len(gp.prompt) + 1])), NEG)]
    fwd = m.engine.decode(dataclasses.replace(gp, sequence_bias=table), 4)
    assert fwd[0] == fwd[2] and fwd[1] == fwd[3] and fwd[0] != plain[0] and fwd[1] != plain[1]
    assert all(table[0][0][0] not in s[len(gp.prompt):] for s in fwd)
    m.engine.encode(feats.flip(0))
    assert m.engine.decode(dataclasses.replace(gp, sequence_bias=table), 4)[::-1] == fwd
    m.engine.encode(feats)
    assert m.engine.decode(gp, 4) == plain
    m.engine.close()
