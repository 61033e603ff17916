"""Seeded sampling on the plain decode path and the temperature fallback on the GPU (include/wm.h wm_set_sampling / wm_sample_rows, DESIGN.md
§2h).  The reference is tests/sample_ref.py: the contract's noise (Philox4x32-10 in numpy, fp64 Gumbel), transformers' processors per row, the
oracle's plain step function; tests/test_sampling_cpu.py holds, from that reference alone, the conditions these inputs were chosen under."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sample_ref as S
from helpers import MedusaConfig, synth, clip_for, check_tokens, ACCEPT_TYPICAL
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu


def _model(cfg, sd, gpu, B):
    return WhisperMedusaModel(cfg, sd, device=gpu, max_batch=B, act_fp16=False)       # the oracle's contract (bf16 hi / lo)


# ---- 1. the tap against fp64 -----------------------------------------------------------------------------------------------------------------
def _check_tap(got, ref, label):
    """value within the arithmetic tolerance (sample_ref.tolerance: fp32 rounding of v / T and of the two logf calls); forced exact where the
    decision margin exceeds it; token equal where the reference's top-2 perturbed gap exceeds 10 x it."""
    worst, skipped = 0.0, 0
    for r, d in enumerate(ref):
        err = abs(float(got["value"][r]) - d["value"])
        if d["margin"] > d["tol"]:
            assert int(got["ts_forced"][r]) == d["forced"], (label, r, d)
        else:
            skipped += 1
            continue                                    # (a row on the decision: either side is right, the other checks follow the side)
        assert err <= d["tol"], (label, r, err, d)
        worst = max(worst, err / d["tol"])
        if d["gap"] > 10 * d["tol"]:
            assert int(got["token"][r]) == d["token"], (label, r, int(got["token"][r]), d)
        else:
            skipped += 1
    print(f"sampling tap[{label}]: {len(ref)} rows, {skipped} indecisive, largest |value - fp64| = {worst:.3f} of the tolerance")
    return worst


@pytest.fixture(scope="module")
def tap_model(gpu):
    cfg = S.tap_cfg()
    m = _model(cfg, S._sr.ts_state_dict(cfg, 21), gpu, 1)
    yield cfg, m
    m.engine.close()


@pytest.mark.parametrize("setting", S.TAP_SETTINGS)
def test_tap_matches_fp64(tap_model, setting):
    cfg, m = tap_model
    assert cfg.vocab_size == 1031
    gp = S.tap_gp(cfg, setting)
    rows, pre = S.tap_cases(cfg, setting)
    keys = S.tap_keys(len(pre))
    for T in S.TAP_T:
        for seed in S.TAP_SEEDS:
            got = m.engine.sample_rows(gp, rows, pre, keys, T, seed)
            _check_tap(got, S.tap_reference(setting, T, seed), f"{setting} T={T} seed={seed:#x}")
    with pytest.raises(ValueError, match="temperature"):
        m.engine.sample_rows(gp, rows[:1], pre[:1], keys[:1], 0.0, 1)
    with pytest.raises(ValueError, match="lens"):
        m.engine.sample_rows(gp, rows[:1], [[1] * (cfg.max_target_positions + 1)], keys[:1], 1.0, 1)


@pytest.mark.parametrize("V", [516, 51864])
def test_tap_other_vocabularies(gpu, V):
    """V = 516: slices of 33 ids, the last one partial; V = 51864: every thread sweeps several Philox blocks."""
    cfg = MedusaConfig.micro(vocab=V)
    m = _model(cfg, synth.synth_state_dict(cfg, seed=3), gpu, 1)
    for T in S.TAP_T:
        rows, pre, keys, ref = S.plain_reference(V, T, S.TAP_SEEDS[0])
        got = m.engine.sample_rows(S.plain_gp(cfg), rows, pre, keys, T, S.TAP_SEEDS[0])
        _check_tap(got, ref, f"V={V} T={T}")
        assert not got["ts_forced"].any()
    m.engine.close()


# ---- 2. the distribution ---------------------------------------------------------------------------------------------------------------------
def test_distribution_is_the_references(tap_model):
    cfg, m = tap_model
    V = cfg.vocab_size
    gp = S.plain_gp(cfg)
    pre = list(gp.prompt) + [9] * 7
    want = S.dist_reference(V, len(pre))
    rows = np.repeat(S.dist_row(V)[None], S.DIST_N, axis=0)
    keys = list(range(S.DIST_N))
    got = m.engine.sample_rows(gp, rows, [pre] * S.DIST_N, keys, 1.0, S.DIST_SEED)["token"]
    assert np.array_equal(got, want), int((got != want).sum())          # (the four live values are far apart in every one of the 4096 draws' noise:
    #                                                                      test_sampling_cpu.py holds the counts to the binomial expectation)
    assert np.bincount(got, minlength=V)[list(S.DIST_TOKENS)].tolist() == np.bincount(want, minlength=V)[list(S.DIST_TOKENS)].tolist()
    # the same key gives the same token twice, wherever the row stands in the call
    again = m.engine.sample_rows(gp, rows[:64], [pre] * 64, keys[:64][::-1], 1.0, S.DIST_SEED)["token"]
    assert np.array_equal(again[::-1], got[:64])
    other = m.engine.sample_rows(gp, rows[:64], [pre] * 64, keys[:64], 1.0, S.DIST_SEED + 1)["token"]
    assert not np.array_equal(other, got[:64])


# ---- 3. / 4. the decode loop equals the reference loop ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dec_rig(gpu):
    cfg, sd = S.dec_checkpoint()
    m = _model(cfg, sd, gpu, 4)
    ref = S.SampleRef(cfg, sd)
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in S.DEC_CLIPS]))
    enc = m.engine.encoder_output(4)
    encs = {c: enc[S.DEC_CLIPS.index(c)] for c in set(S.DEC_CLIPS)}
    rig = dict(cfg=cfg, sd=sd, m=m, ref=ref, encs=encs, runs={})
    yield rig
    m.engine.close()


def _ref_runs(rig, name, seed=None):
    """The reference runs of one case on the engine's own encoder output (one decode per (clip, key), shared by the tests), with their guards."""
    T, ts, rep, s0 = S.DEC_CASES[name]
    seed = s0 if seed is None else seed
    if (name, seed) not in rig["runs"]:
        rig["runs"][(name, seed)] = S.dec_guards(rig["ref"], S.dec_gp(rig["cfg"], ts, rep), T, seed, rig["encs"])
    return rig["runs"][(name, seed)]


def _sampled(gp, T, seed, keys):
    return dataclasses.replace(gp, sampling_temperature=T, sampling_seed=seed, sampling_keys=list(keys))


def _decode_and_check(rig, name, seed=None, reverse=False):
    cfg, m = rig["cfg"], rig["m"]
    T, ts, rep, s0 = S.DEC_CASES[name]
    seed = s0 if seed is None else seed
    runs = _ref_runs(rig, name, seed)
    gp = S.dec_gp(cfg, ts, rep)
    clips, keys = list(S.DEC_CLIPS), list(S.DEC_KEYS)
    if reverse:
        clips, keys = clips[::-1], keys[::-1]
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in clips]))
    seqs = m.engine.decode(_sampled(gp, T, seed, keys), 4)
    ties = sum(S.check_run(seqs[b], runs[(clips[b], keys[b])], T, f"{name} seed {seed} slot {b}", len(gp.prompt)) for b in range(4))
    assert ties <= 1
    return seqs


@pytest.mark.parametrize("name", list(S.DEC_CASES))
def test_decode_matches_reference(dec_rig, name):
    _decode_and_check(dec_rig, name)
    assert dec_rig["m"].engine.stats()["graph_replays"] > 0


def test_permutation_and_second_seed(dec_rig):
    """The batch reversed, with its keys: every (clip, key) gives the ids it gave in the other slot.  A second decode on the same context under
    another seed follows the reference of THAT seed (the captured graph does not replay the first seed's noise)."""
    fwd = _decode_and_check(dec_rig, "T1.0")
    rev = _decode_and_check(dec_rig, "T1.0", reverse=True)
    assert rev[::-1] == fwd
    other = _decode_and_check(dec_rig, "T1.0", seed=S.DEC_SECOND_SEED)
    assert other != fwd
    # other keys under one seed: the keys live in device memory the captured launches read
    m, cfg = dec_rig["m"], dec_rig["cfg"]
    T, ts, rep, seed = S.DEC_CASES["T1.0"]
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in S.DEC_CLIPS]))
    moved = m.engine.decode(_sampled(S.dec_gp(cfg, ts, rep), T, seed, [2, 3, 0, 1]), 4)
    assert moved == [fwd[2], fwd[3], fwd[0], fwd[1]]
    # and sampling off again: the greedy plain decode, nothing left of the request on the context
    greedy = m.engine.decode(S.dec_gp(cfg, ts, rep), 4)
    assert greedy[0] == greedy[2] and greedy[0] != fwd[0]


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dataclasses, torch
import sample_ref as S
from helpers import clip_for
from whisper_medusa import WhisperMedusaModel
cfg, sd = S.dec_checkpoint()
m = WhisperMedusaModel(cfg, sd, device=torch.device("cuda", 0), max_batch=4, act_fp16=False)
T, ts, rep, seed = S.DEC_CASES["T0.4_ts"]
m.engine.encode(m.extract_features([clip_for(cfg, c) for c in S.DEC_CLIPS]))
gp = dataclasses.replace(S.dec_gp(cfg, ts, rep), sampling_temperature=T, sampling_seed=seed, sampling_keys=list(S.DEC_KEYS))
seqs = m.engine.decode(gp, 4)
print("RESULT " + json.dumps(dict(seqs=seqs, graph_replays=m.engine.stats()["graph_replays"])))
"""


def test_eager_launches_equal_graph_replay(dec_rig, tmp_path):
    """WM_NO_GRAPH=1 in a fresh child process: the same ids as the graph replay of this process."""
    here = _decode_and_check(dec_rig, "T0.4_ts")
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, WM_NO_GRAPH="1")
    r = subprocess.run([sys.executable, str(script), os.path.dirname(os.path.abspath(__file__))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    assert out["graph_replays"] == 0 and out["seqs"] == here


def test_engine_refusals(dec_rig):
    m, cfg = dec_rig["m"], dec_rig["cfg"]
    gp = S.dec_gp(cfg, False, False)
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in S.DEC_CLIPS]))
    for T in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            m.engine.decode(_sampled(gp, T, 1, S.DEC_KEYS), 4)
    with pytest.raises(ValueError, match="n_keys"):
        m.engine.decode(_sampled(gp, 1.0, 1, [0, 1]), 4)
    with pytest.raises(ValueError, match="plain decode path"):
        m.engine.decode(dataclasses.replace(_sampled(gp, 1.0, 1, S.DEC_KEYS), vanilla=False, accept_mode=ACCEPT_TYPICAL, temperature=1.0), 4)
    m.engine.decode(gp, 4)                                  # the context is usable afterwards


# ---- 5. generate() with a fallback schedule --------------------------------------------------------------------------------------------------
def _own(row, P, eos):
    s = [int(t) for t in row]
    return s[: s.index(eos, P) + 1] if eos in s[P:] else s


def _rows(out):
    """The streams' own ids of a dict output (pad == eos: a padded row alone cannot tell a stream's end from its padding; `lengths` can)."""
    seq = out["sequences"].cpu().tolist()
    return [seq[b][: int(out["lengths"][b])] for b in range(len(seq))]


def test_generate_fallback_end_to_end(gpu):
    cfg, sd = S.fb_checkpoint()
    m = _model(cfg, sd, gpu, 2)
    ref = S.SampleRef(cfg, sd)
    gp = S.fb_gp(cfg, sd)
    P, eos = len(gp.prompt), gp.eos_token_id
    feats = m.extract_features([clip_for(cfg, c) for c in S.FB_CLIPS])
    m.engine.encode(feats)
    enc = m.engine.encoder_output(2)
    runs = S.fb_reference(ref, cfg, gp, {c: enc[b] for b, c in enumerate(S.FB_CLIPS)})
    thr, low, high = S.fb_threshold(runs)
    assert low < thr < high, (low, thr, high)               # (the guard of test_sampling_cpu.py, on the engine's encoder output)
    for r in runs:
        assert min(r["greedy_gaps"]) >= 10 * S.TIE and min(r["sampled_gaps"]) >= 10 * S.TIE / S.t32(S.FB_TEMPS[1])
    kw = dict(max_new_tokens=S.FB_MAX_NEW, compression_ratio_threshold=thr, return_dict_in_generate=True)
    out = m.generate(feats, temperature=S.FB_TEMPS, sampling_seed=S.FB_SEED, **kw)
    seq = _rows(out)
    assert out["fallback_attempts"].tolist() == [2, 1]
    assert out["fallback_temperature"].tolist() == pytest.approx([S.FB_TEMPS[1], S.FB_TEMPS[0]])
    assert m.last_stats["fallback_decodes"] == 1
    assert seq[0] == S.own_end(runs[0]["sampled"], P, eos)
    assert out["needs_fallback"].tolist() == [False, False]
    # the stream that passed at once: the ids of today's call without the tuple
    today = m.generate(feats, temperature=0.0, **kw)
    assert today["needs_fallback"].tolist() == [True, False]
    assert seq[1] == _rows(today)[1] == S.own_end(runs[1]["greedy"], P, eos)
    # the tuple without a seed: today's behaviour (attempt 0 only), id for id
    noseed = m.generate(feats, temperature=S.FB_TEMPS, **kw)
    assert torch.equal(noseed["sequences"], today["sequences"]) and "fallback_attempts" not in noseed
    # a threshold nothing passes: the last temperature's result is kept
    out = m.generate(feats, temperature=S.FB_TEMPS, sampling_seed=S.FB_SEED, **dict(kw, compression_ratio_threshold=0.5))
    assert out["fallback_attempts"].tolist() == [2, 2] and out["needs_fallback"].tolist() == [True, True]
    assert _rows(out) == [S.own_end(runs[b]["sampled"], P, eos) for b in range(2)]
    # a scalar temperature: one sampled plain decode under attempt index 0
    one = m.generate(feats[0:1], temperature=S.FB_TEMPS[1], sampling_seed=S.FB_SEED, max_new_tokens=S.FB_MAX_NEW)
    want = ref.decode(enc[0], S.plain_of(gp), S.FB_TEMPS[1], S.FB_SEED, S.stream_key(0, 0, 0))
    S.check_run(_own(one[0].tolist(), P, eos), (S.own_end(want[0], P, eos), want[1]), S.FB_TEMPS[1], "scalar", P)
    # calls without sampling_seed are unchanged: the suite's typical-acceptance parity on this checkpoint (the engine's own ids, as
    # tests/test_gpu_parity.py compares them, are what generate() returns up to the stream's end)
    plain = m.generate(feats[0:1], max_new_tokens=S.FB_MAX_NEW)
    gp_t = m._gen_params(None, None, None, S.FB_MAX_NEW, None, None, False, None, None, None, None, None)
    m.engine.encode(feats[0:1])
    raw = m.engine.decode(gp_t, 1)[0]
    check_tokens(ref.orc, enc[0], gp_t, raw, label="no seed")
    assert _own(plain[0].tolist(), P, eos) == _own(raw, P, eos)
    m.engine.close()


# ---- 6. sequential long-form with a fallback schedule ----------------------------------------------------------------------------------------
def test_sequential_longform_falls_back_per_window(gpu):
    """One recording of about 2.3 windows under temperature=(0.0, 0.4) and a threshold that flags exactly one window of the reference: that window
    is decoded again under the key (clip, its seek, attempt 1); segments and seeks are the reference loop's; next to another recording in one
    batch the recording gives the same ids (the keys come from clip and seek, not from the round)."""
    import longform_seek as LS
    cfg, sd, gp = S.lf_setup()
    ref = S.SampleRef(cfg, sd)
    wavs = S.lf_inputs()
    thr, hi, lo, plain, rec = S.lf_run(ref, cfg, gp, wavs)
    assert lo < thr < hi and [w["attempts"] for w in rec] == [2, 1, 1]           # (tests/test_sampling_cpu.py: the conditions of this recording)
    m = _model(cfg, sd, gpu, 2)
    kw = dict(sequential_longform=True, return_timestamps=True, return_segments=True, max_new_tokens=S.LF_MAX_NEW, temperature=S.LF_TEMPS,
              sampling_seed=S.LF_SEED, compression_ratio_threshold=thr)
    # the recording alone, padded as in the batch below (the log-mel of a recording does not depend on the padding; its length does not change)
    n = LS.padded_len([len(w) for w in wavs])
    alone = np.zeros((1, n), dtype=np.float32)
    alone[0, : len(wavs[0])] = wavs[0]
    feats = m.extract_features([alone[0]], truncation=False)
    frames = torch.tensor([len(wavs[0]) // 160])
    out = m.generate(feats, num_frames=frames, **kw)
    want_seq = LS.sequence_of(gp, rec)
    got = out["sequences"][0].tolist()
    assert got[: len(want_seq)] == want_seq and all(t == cfg.pad_token_id for t in got[len(want_seq):]), (got, want_seq)
    assert out["window_attempts"][0].tolist() == [w["attempts"] for w in rec]
    assert out["window_temperature"][0].tolist() == pytest.approx([w["temperature"] for w in rec])
    assert out["window_seek"][0].tolist() == [w["seek"] for w in rec]
    assert m.last_stats["fallback_decodes"] == 1 and m.last_stats["longform_windows"] == [3]
    segs = [sg for w in rec for sg in w["segments"]]
    assert len(out["segments"][0]) == len(segs)
    for g, w in zip(out["segments"][0], segs):
        assert g["tokens"].tolist() == w["tokens"].tolist() and float(g["start"]) == float(w["start"]) and float(g["end"]) == float(w["end"])
    # in a batch next to another recording
    both = m.generate_from_wav(wavs, **kw)
    assert both["sequences"][0].tolist()[: len(want_seq)] == want_seq
    assert both["window_attempts"][0].tolist() == [w["attempts"] for w in rec] and both["window_seek"][0].tolist() == [w["seek"] for w in rec]
    # without the tuple and the seed: the greedy pass, whose flagged window stays flagged
    greedy = m.generate(feats, num_frames=frames, **dict(kw, temperature=0.0, sampling_seed=None))
    assert greedy["sequences"][0].tolist()[: len(LS.sequence_of(gp, plain))] == LS.sequence_of(gp, plain)
    assert greedy["needs_fallback"][0].tolist() == [True, False, False] and "window_attempts" not in greedy
    m.engine.close()
