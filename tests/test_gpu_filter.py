"""Top-k, top-p and min-p filters of the seeded draw on the GPU (include/wm.h wm_set_sampling_filter / wm_filter_rows).  The
reference is tests/filter_ref.py: the threshold in fp64 from the fp32 row, sample_ref's noise, draw and decode loop; tests/test_filter_cpu.py holds,
from that reference alone, the conditions these inputs were chosen under."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import filter_ref as F
import sample_ref as S
from helpers import clip_for
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu


def _model(cfg, sd, gpu, B):
    return WhisperMedusaModel(cfg, sd, device=gpu, max_batch=B, act_fp16=False)       # the oracle's contract (bf16 hi / lo)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ---- 1. the kernels alone, through filter_rows -----------------------------------------------------------------------------------------------
_MODELS = {}


@pytest.fixture(scope="module")
def tap_models(gpu):
    def get(name):
        cfg, gp, _ = F.shape(name)
        key = cfg.vocab_size
        if key not in _MODELS:
            sd = S._sr.ts_state_dict(cfg, 21) if name in F.SETTINGS else S.synth.synth_state_dict(cfg, seed=3)
            _MODELS[key] = _model(cfg, sd, gpu, 1)
        return cfg, gp, _MODELS[key]
    yield get
    for m in _MODELS.values():
        m.engine.close()
    _MODELS.clear()


def _check(got, ref, flt, label):
    """forced exact (off the decision's own margin); thr bit-equal and kept equal on every top-k-only row and on every decided row; there the
    token equal and val within the draw's tolerance.  (tests/test_filter_cpu.py asserts that EVERY row's top-2 perturbed gap exceeds 10 x that
    tolerance — tests/test_gpu_sampling.py's condition for comparing a token — so no token goes unchecked.)"""
    topk_only = flt[1] == 1.0 and flt[2] == 0.0
    undecided, worst = 0, 0.0
    for r, d in enumerate(ref):
        assert d["margin"] > d["tol"], (label, r, "a crafted row on the timestamp decision")
        assert int(got["ts_forced"][r]) == d["forced"], (label, r, d)
        if not (topk_only or F.decided(d)):
            undecided += 1
            continue
        assert _bits(got["thr"][r]) == _bits(d["thr"]), (label, r, float(got["thr"][r]), d)
        assert int(got["kept"][r]) == d["kept"], (label, r, int(got["kept"][r]), d)
        if d["kept"] == 0:
            assert int(got["token"][r]) == 0 and float(got["value"][r]) == -np.inf
            continue
        err = abs(float(got["value"][r]) - d["value"])
        assert err <= d["tol"], (label, r, err, d)
        worst = max(worst, err / d["tol"])
        assert d["gap"] > 10 * d["tol"], (label, r, "a row on a tie of the draw")
        assert int(got["token"][r]) == d["token"], (label, r, int(got["token"][r]), d)
    print(f"filter tap[{label}]: {len(ref)} rows, {undecided} undecided, largest |value - fp64| = {worst:.3f} of the tolerance")
    return undecided


@pytest.mark.parametrize("name", F.SHAPES)
def test_tap_matches_fp64(tap_models, name):
    cfg, gp, m = tap_models(name)
    rows, pre, lab = F.cases(name)
    keys = F.keys_of(len(pre))
    V, eng = cfg.vocab_size, m.engine
    for T in F.TAP_T:
        for flt in F.FILTERS:
            got = eng.filter_rows(gp, rows, pre, keys, T, F.TAP_SEED, *flt)
            n_und = _check(got, F.reference(name, T, flt), flt, f"{name} T={T} {flt}")
            assert n_und <= F.UNDECIDED_CAP * len(pre), (name, T, flt, n_und)           # the cap of every case list, as tests/test_filter_cpu.py
        # the keep-everything filter: wm_sample_rows' token and perturbed value, bit for bit
        plain = eng.sample_rows(gp, rows, pre, keys, T, F.TAP_SEED)
        allk = eng.filter_rows(gp, rows, pre, keys, T, F.TAP_SEED, top_k=V)
        assert np.array_equal(allk["token"], plain["token"]) and np.array_equal(_bits(allk["value"]), _bits(plain["value"]))
        assert np.array_equal(allk["ts_forced"], plain["ts_forced"])
        assert np.all(np.isneginf(allk["thr"])) and allk["kept"].tolist() == [F.region_count(name, r) for r in range(len(pre))]
        off = eng.filter_rows(gp, rows, pre, keys, T, F.TAP_SEED)              # all three off: wm_sample_rows' own kernels
        assert np.array_equal(off["token"], plain["token"]) and np.array_equal(_bits(off["value"]), _bits(plain["value"]))
        # top_k = 1: the arg-max of v wherever it is unique
        one = eng.filter_rows(gp, rows, pre, keys, T, F.TAP_SEED, top_k=1)
        ref1 = F.reference(name, T, (1, 1.0, 0.0))
        proc = S._sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
        for r, d in enumerate(ref1):
            if d["kept"] == 1:
                v = F.processed_cached(rows[r], pre[r], gp, cfg, proc)[0]
                assert int(one["token"][r]) == int(np.argmax(v)) == d["token"], (name, T, r)
    # k at |R|, |R| - 1, |R| + 1 and V, on the rows whose region is small, whole or tied
    T = F.TAP_T[1]
    for r in [lab.index(x) for x in ("dup17", "forced_few", "one_finite", "all_equal", "random1") if x in lab]:
        n = F.region_count(name, r)
        for k in sorted({max(n - 1, 1), n, n + 1, V}):
            got = eng.filter_rows(gp, rows[r: r + 1], pre[r: r + 1], keys[r: r + 1], T, F.TAP_SEED, top_k=k)
            d = F.filter_row(rows[r], pre[r], gp, cfg, T, F.TAP_SEED, keys[r], (k, 1.0, 0.0), proc)
            assert _bits(got["thr"][0]) == _bits(d["thr"]) and int(got["kept"][0]) == d["kept"], (name, lab[r], n, k, got, d)
            if k >= n:
                assert np.isneginf(got["thr"][0]) and int(got["kept"][0]) == n
            if d["gap"] > 10 * d["tol"]:
                assert int(got["token"][0]) == d["token"]
    # the same row and key: the same outputs wherever the row stands in the call and whatever R is (17 rows: two chunks of the tap)
    flt = F.FILTERS[-1]
    fwd = eng.filter_rows(gp, rows, pre, keys, T, F.TAP_SEED, *flt)
    rev = eng.filter_rows(gp, rows[::-1], pre[::-1], keys[::-1], T, F.TAP_SEED, *flt)
    for f in ("thr", "value"):
        assert np.array_equal(_bits(rev[f][::-1]), _bits(fwd[f])), f
    for f in ("kept", "token", "ts_forced"):
        assert np.array_equal(rev[f][::-1], fwd[f]), f
    for r in (0, len(pre) - 1):
        solo = eng.filter_rows(gp, rows[r: r + 1], pre[r: r + 1], keys[r: r + 1], T, F.TAP_SEED, *flt)
        assert _bits(solo["thr"][0]) == _bits(fwd["thr"][r]) and _bits(solo["value"][0]) == _bits(fwd["value"][r])
        assert (int(solo["kept"][0]), int(solo["token"][0])) == (int(fwd["kept"][r]), int(fwd["token"][r]))
    for bad in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(min_p=-0.1), dict(min_p=1.5)):
        with pytest.raises(ValueError, match="top_k|top_p|min_p"):
            eng.filter_rows(gp, rows[:1], pre[:1], keys[:1], 1.0, 1, **bad)


# ---- 2. the distribution ---------------------------------------------------------------------------------------------------------------------
def test_distribution_under_top_k(tap_models):
    cfg, _, m = tap_models("plain")
    V = cfg.vocab_size
    gp = S.plain_gp(cfg)
    pre = list(gp.prompt) + [9] * 7
    want = F.dist_reference(V, len(pre))
    rows = np.repeat(S.dist_row(V)[None], S.DIST_N, axis=0)
    got = m.engine.filter_rows(gp, rows, [pre] * S.DIST_N, list(range(S.DIST_N)), 1.0, S.DIST_SEED, top_k=2)
    assert np.array_equal(got["token"], want), int((got["token"] != want).sum())
    assert set(got["token"].tolist()) == set(S.DIST_TOKENS[:2]) and np.all(got["kept"] == 2)
    n0 = int((got["token"] == S.DIST_TOKENS[0]).sum())
    sigma = (S.DIST_N * (2 / 3) * (1 / 3)) ** 0.5
    assert abs(n0 - S.DIST_N * 2 / 3) <= 4 * sigma, n0                  # 2/3 : 1/3 within 4 sigma


# ---- 3. the decode loop equals the reference loop --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dec_rig(gpu):
    cfg, sd = S.dec_checkpoint()
    m = _model(cfg, sd, gpu, 4)
    ref = F.FilterRef(cfg, sd)
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in S.DEC_CLIPS]))
    enc = m.engine.encoder_output(4)
    encs = {c: enc[S.DEC_CLIPS.index(c)] for c in set(S.DEC_CLIPS)}
    rig = dict(cfg=cfg, sd=sd, m=m, ref=ref, encs=encs, runs={})
    yield rig
    m.engine.close()


def _ref_runs(rig, name, flt=None):
    T, ts, rep, f0, seed = F.DEC_CASES[name]
    flt = f0 if flt is None else flt
    if (name, flt) not in rig["runs"]:
        gp = S.dec_gp(rig["cfg"], ts, rep)
        if tuple(flt) == F.OFF:
            rig["runs"][(name, flt)] = {(c, k): rig["ref"].decode(rig["encs"][c], gp, T, seed, k) for c, k in zip(S.DEC_CLIPS, S.DEC_KEYS)}
        else:
            rig["runs"][(name, flt)] = F.dec_guards(rig["ref"], gp, T, seed, flt, rig["encs"])
    return rig["runs"][(name, flt)]


def _sampled(gp, T, seed, keys, flt):
    return dataclasses.replace(gp, sampling_temperature=T, sampling_seed=seed, sampling_keys=list(keys), sampling_top_k=flt[0],
                               sampling_top_p=flt[1], sampling_min_p=flt[2])


def _decode_and_check(rig, name, flt=None, reverse=False):
    cfg, m = rig["cfg"], rig["m"]
    T, ts, rep, f0, seed = F.DEC_CASES[name]
    flt = f0 if flt is None else flt
    runs = _ref_runs(rig, name, flt)
    gp = S.dec_gp(cfg, ts, rep)
    clips, keys = list(S.DEC_CLIPS), list(S.DEC_KEYS)
    if reverse:
        clips, keys = clips[::-1], keys[::-1]
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in clips]))
    seqs = m.engine.decode(_sampled(gp, T, seed, keys, flt), 4)
    ties = sum(S.check_run(seqs[b], runs[(clips[b], keys[b])][:2], T, f"{name} {flt} slot {b}", len(gp.prompt)) for b in range(4))
    assert ties <= 1
    return seqs


@pytest.mark.parametrize("name", list(F.DEC_CASES))
def test_decode_matches_reference(dec_rig, name):
    _decode_and_check(dec_rig, name)
    assert dec_rig["m"].engine.stats()["graph_replays"] > 0


def test_permutation_second_filter_and_filter_off(dec_rig):
    """The batch reversed, with its keys: every (clip, key) keeps its ids.  A second decode on the same context with another top_k follows THAT
    setting's reference (the graph key holds the filter: the graphs are captured anew).  The filter cleared: the ids of sample_ref.decode."""
    name = F.DEC_DIFFERS
    fwd = _decode_and_check(dec_rig, name)
    rev = _decode_and_check(dec_rig, name, reverse=True)
    assert rev[::-1] == fwd
    other = _decode_and_check(dec_rig, name, flt=(F.DEC_SECOND_K, 1.0, 0.0))
    assert other != fwd
    plain = _decode_and_check(dec_rig, name, flt=F.OFF)
    assert plain != fwd                                     # the filter changed the ids of this case
    unfiltered = _ref_runs(dec_rig, name, F.OFF)
    filtered = _ref_runs(dec_rig, name)
    assert any(unfiltered[ck][0] != filtered[ck][0] for ck in filtered)
    # a set filter on a decode that does not sample is refused, never ignored
    m, cfg = dec_rig["m"], dec_rig["cfg"]
    T, ts, rep, f0, seed = F.DEC_CASES[name]
    m.engine.encode(m.extract_features([clip_for(cfg, c) for c in S.DEC_CLIPS]))
    with pytest.raises(ValueError, match="does not sample"):
        m.engine.decode(dataclasses.replace(S.dec_gp(cfg, ts, rep), sampling_top_k=5), 4)
    greedy = m.engine.decode(S.dec_gp(cfg, ts, rep), 4)     # and the context is usable afterwards, the filter gone with gp
    assert greedy[0] == greedy[2]


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dataclasses, torch
import filter_ref as F
import sample_ref as S
from helpers import clip_for
from whisper_medusa import WhisperMedusaModel
cfg, sd = S.dec_checkpoint()
m = WhisperMedusaModel(cfg, sd, device=torch.device("cuda", 0), max_batch=4, act_fp16=False)
T, ts, rep, flt, seed = F.DEC_CASES[sys.argv[2]]
m.engine.encode(m.extract_features([clip_for(cfg, c) for c in S.DEC_CLIPS]))
gp = dataclasses.replace(S.dec_gp(cfg, ts, rep), sampling_temperature=T, sampling_seed=seed, sampling_keys=list(S.DEC_KEYS),
                         sampling_top_k=flt[0], sampling_top_p=flt[1], sampling_min_p=flt[2])
seqs = m.engine.decode(gp, 4)
print("RESULT " + json.dumps(dict(seqs=seqs, graph_replays=m.engine.stats()["graph_replays"])))
"""


def test_eager_launches_equal_graph_replay(dec_rig, tmp_path):
    """WM_NO_GRAPH=1 in a fresh child process: the same ids as the graph replay of this process."""
    name = "p0.8_T0.4_ts"
    here = _decode_and_check(dec_rig, name)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, WM_NO_GRAPH="1")
    r = subprocess.run([sys.executable, str(script), os.path.dirname(os.path.abspath(__file__)), name], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    assert out["graph_replays"] == 0 and out["seqs"] == here


# ---- 4. generate() ---------------------------------------------------------------------------------------------------------------------------
def _rows(out):
    seq = out["sequences"].cpu().tolist()
    return [seq[b][: int(out["lengths"][b])] for b in range(len(seq))]


def test_generate_fallback_with_top_k(gpu):
    """The fallback fixture of sample_ref under sampling_top_k=50: attempts and ids are those of the reference loop run with the filtered draw."""
    cfg, sd = S.fb_checkpoint()
    m = _model(cfg, sd, gpu, 2)
    ref = F.FilterRef(cfg, sd)
    gp = S.fb_gp(cfg, sd)
    P, eos = len(gp.prompt), gp.eos_token_id
    feats = m.extract_features([clip_for(cfg, c) for c in S.FB_CLIPS])
    m.engine.encode(feats)
    enc = m.engine.encoder_output(2)
    runs = F.fb_reference(ref, cfg, gp, {c: enc[b] for b, c in enumerate(S.FB_CLIPS)})
    thr, low, high = S.fb_threshold(runs)
    assert low < thr < high, (low, thr, high)               # (the guards of test_filter_cpu.py, on the engine's encoder output)
    for r in runs:
        assert min(r["greedy_gaps"]) >= 10 * S.TIE and min(r["sampled_gaps"]) >= 10 * S.TIE / S.t32(S.FB_TEMPS[1]) and min(r["ratios"]) > F.GUARD
    # the reference loop: a stream is flagged while its compression ratio exceeds the threshold
    res, temp, att, log = S.fallback_loop(S.FB_TEMPS, 2, lambda idx, T, i: [runs[b]["greedy" if T == 0.0 else "sampled"] for b in idx],
                                          lambda ids, T: (S._sr.hf_compression_ratio(S.own_end(ids, P, eos)[P:], cfg.vocab_size) > thr, False))
    kw = dict(max_new_tokens=S.FB_MAX_NEW, compression_ratio_threshold=thr, return_dict_in_generate=True)
    out = m.generate(feats, temperature=S.FB_TEMPS, sampling_seed=S.FB_SEED, sampling_top_k=F.GEN_FILTER[0], **kw)
    assert out["fallback_attempts"].tolist() == att == [2, 1]
    assert _rows(out) == [S.own_end(r, P, eos) for r in res]
    # the keywords are refused by name on a call that does not sample
    with pytest.raises(ValueError, match="sampling_top_k"):
        m.generate(feats, temperature=0.0, sampling_top_k=50, **kw)
    m.engine.close()


def test_sequential_longform_with_top_k(gpu):
    """The 2.3-window recording of sample_ref under temperature=(0.0, 0.4) with sampling_top_k=5: window attempts, ids and seeks are the
    filtered reference loop's, and the retried window is not the unfiltered draw's (tests/test_filter_cpu.py: top_k = 50 would leave it so)."""
    import longform_seek as LS
    cfg, sd, gp = S.lf_setup()
    ref = F.Filtered(F.FilterRef(cfg, sd), F.LF_FILTER)
    wavs = S.lf_inputs()
    thr, hi, lo, plain, rec = S.lf_run(ref, cfg, gp, wavs)
    assert lo < thr < hi and [w["attempts"] for w in rec] == [2, 1, 1]           # (tests/test_filter_cpu.py: the conditions of this recording)
    rec0 = S.lf_run(S.SampleRef(cfg, sd), cfg, gp, wavs)[4]
    assert rec[0]["ids"] != rec0[0]["ids"]                                        # the filter shows in the retried window
    m = _model(cfg, sd, gpu, 2)
    kw = dict(sequential_longform=True, return_timestamps=True, return_segments=True, max_new_tokens=S.LF_MAX_NEW, temperature=S.LF_TEMPS,
              sampling_seed=S.LF_SEED, sampling_top_k=F.LF_FILTER[0], compression_ratio_threshold=thr)
    n = LS.padded_len([len(w) for w in wavs])
    alone = np.zeros((1, n), dtype=np.float32)
    alone[0, : len(wavs[0])] = wavs[0]
    feats = m.extract_features([alone[0]], truncation=False)
    out = m.generate(feats, num_frames=torch.tensor([len(wavs[0]) // 160]), **kw)
    want_seq = LS.sequence_of(gp, rec)
    got = out["sequences"][0].tolist()
    assert got[: len(want_seq)] == want_seq and all(t == cfg.pad_token_id for t in got[len(want_seq):]), (got, want_seq)
    assert out["window_attempts"][0].tolist() == [w["attempts"] for w in rec]
    assert out["window_seek"][0].tolist() == [w["seek"] for w in rec]
    m.engine.close()
