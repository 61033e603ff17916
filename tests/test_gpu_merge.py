"""Overlapping long-form windows on the GPU (include/wm.h wm_merge_windows).  The kernel against the two references of
tests/merge_ref.py — the restated contract slice for slice, transformers' own function on the reassembled ids —, the entry's independence of
the decode state and its argument errors, then generate(chunk_longform=True, stride_length_s=..) end to end on the micro checkpoint against
the same windows decoded one by one and merged on the host by transformers' function."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import merge_ref as M
from helpers import synth
from test_gpu_token_timestamps import checkpoint
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu
STRIDE, NEW = 32, 12                    # frames each side of the micro window (192); max_new_tokens


@pytest.fixture(scope="module")
def rig(gpu):
    cfg, sd = checkpoint("micro")       # micro shape with alignment heads (they do not touch the decode)
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=8)
    yield cfg, m
    m.engine.close()


# ---- 1. the kernel: slices ------------------------------------------------------------------------------------------------------------------------
def _check(eng, cases):
    """One call for all the cases that have no times and one for those that have: every clip's slices are the contract's, and reassemble
    to what transformers returns."""
    for timed in (False, True):
        sel = [c for c in cases if (c["times"] is not None) == timed]
        if not sel:
            continue
        got = eng.merge_windows([c["windows"] for c in sel], [c["times"] for c in sel] if timed else None)
        assert len(got) == len(sel)
        for n, (c, keep) in enumerate(zip(sel, got)):
            ws, ts = c["windows"], c["times"]
            assert keep == M.keep_slices(ws, ts), (timed, n, [len(w) for w in ws], keep)
            want = M.hf_merge(ws, ts)
            assert M.assemble(ws, keep) == (want[0] if timed else want), (timed, n)
            if timed:
                assert M.assemble(ws, keep, ts) == want[1]
                alone = eng.merge_windows([ws], None)[0]           # the same windows without times: the other branch
                assert alone == M.keep_slices(ws), (n, "ids alone")


def test_kernel_equals_the_references_on_the_cpu_case_list(rig):
    _, m = rig
    _check(m.engine, M.cpu_cases())
    assert m.engine.last_merge_ms > 0


def test_kernel_on_lane_wave_and_thread_count_edges(rig):
    _, m = rig
    cases = M.gpu_length_cases()
    shifts = {len(c["windows"][0]) + len(c["windows"][1]) - 1 for c in cases if len(c["windows"]) == 2}
    assert {255, 256, 257, 511, 512, 513, 767, 768, 1022, 1023} <= shifts
    assert {len(c["windows"]) for c in cases} == {1, 2, 3, 9}
    _check(m.engine, cases)
    for c in cases[:6]:                 # and every clip in a call of its own
        assert m.engine.merge_windows([c["windows"]], None if c["times"] is None else [c["times"]]) == [M.keep_slices(c["windows"], c["times"])]


def test_five_clips_in_one_call_and_in_reversed_order(rig):
    _, m = rig
    clips = M.five_clips()
    assert sorted(len(ws) for ws in clips) == [1, 2, 3, 4, 9]
    want = [M.keep_slices(ws) for ws in clips]
    got = m.engine.merge_windows(clips)
    assert got == want
    assert m.engine.merge_windows(clips[::-1]) == want[::-1]
    assert m.engine.merge_windows([[]] + clips[:2] + [[], []] + clips[2:]) == [[]] + want[:2] + [[], []] + want[2:]      # clips that own no window


# ---- 2. the kernel: state and errors ----------------------------------------------------------------------------------------------------------------
def test_a_merge_inside_a_decode_leaves_the_decode_alone(rig):
    cfg, m = rig
    eng = m.engine
    feats = m.extract_features([synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160) for i in (0, 1)])
    gp = m._gen_params(None, None, None, 20, None, None, False, None, None, None, None, None)
    eng.encode(feats)
    want = eng.decode(gp, 2)
    clips = M.five_clips()
    keep = [M.keep_slices(ws) for ws in clips]
    # between wm_decode_begin and wm_decode_run
    eng.encode(feats)
    g, _alive = eng._gen_struct(gp)
    eng._check(eng.lib.wm_decode_begin(eng.h, C.byref(g), 2), "wm_decode_begin")
    assert eng.merge_windows(clips) == keep
    left = C.c_int32(0)
    eng._check(eng.lib.wm_decode_run(eng.h, 1 << 30, C.byref(left)), "wm_decode_run")
    assert [eng.tokens(b) for b in range(2)] == want
    # and between the iterations of a run
    eng.encode(feats)
    seen = []
    got = eng.decode(gp, 2, on_iteration=lambda new: seen.append(eng.merge_windows(clips) == keep))
    assert got == want and seen and all(seen)
    assert eng.decode(gp, 2) == want            # the captured graphs still replay


def _raw(eng, C_, first, tokens, Tmax, lens, times=None, keep=True):
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    arr = lambda v, t: None if v is None else np.ascontiguousarray(v, dtype=t)          # noqa: E731
    f, t, l, tm = arr(first, np.int32), arr(tokens, np.int32), arr(lens, np.int32), arr(times, np.float32)
    out = np.zeros((max(len(lens) if lens is not None else 1, 1), 2), np.int32) if keep else None
    p = lambda a, ty: None if a is None else a.ctypes.data_as(ty)                        # noqa: E731
    rc = eng.lib.wm_merge_windows(eng.h, C_, p(f, i32p), p(t, i32p), Tmax, p(l, i32p), p(tm, f32p), p(out, i32p), None)
    return rc, eng.lib.wm_last_error(eng.h).decode(), out


def test_argument_errors_come_back_with_their_reason(rig):
    _, m = rig
    eng = m.engine
    tok = np.zeros((2, 4), np.int32)
    ok = dict(C_=1, first=[0, 2], tokens=tok, Tmax=4, lens=[3, 4])
    for change, word in ((dict(first=None), "null pointer"), (dict(tokens=None), "null pointer"), (dict(lens=None), "null pointer"),
                         (dict(keep=False), "null pointer"), (dict(C_=0), "C must be"), (dict(first=[1, 2]), r"first\[0\] must be 0"),
                         (dict(C_=2, first=[0, 2, 1]), "first must ascend"), (dict(lens=[3, 5]), r"lens\[1\] = 5 outside"),
                         (dict(lens=[-1, 2]), r"lens\[0\] = -1 outside"), (dict(Tmax=0), "Tmax must be")):
        rc, err, _ = _raw(eng, **dict(ok, **change))
        assert rc == -1, (change, rc)
        assert re.search(word, err), (change, err)
        assert eng.merge_windows([[[1, 2, 3, 4], [3, 4, 5]]]) == [[(0, 3), (1, 3)]]          # still usable
    W = M.WINDOWS_MAX + 1
    rc, err, _ = _raw(eng, 1, [0, W], np.zeros((W, 1), np.int32), 1, [1] * W)
    assert rc == -1 and "exceed WM_MERGE_WINDOWS_MAX" in err
    with pytest.raises(ValueError, match=r"lens\[0\] = 513 outside"):
        eng.merge_windows([[list(range(M.LEN_MAX + 1))]])
    with pytest.raises(ValueError, match="shape of windows_per_clip"):
        eng.merge_windows([[[1, 2]]], [[[0.0]]])
    # the limits themselves are fine: LEN_MAX ids, WINDOWS_MAX windows
    assert eng.merge_windows([[list(range(M.LEN_MAX))]]) == [[(0, M.LEN_MAX)]]
    many = eng.merge_windows([[[7]] * M.WINDOWS_MAX])
    assert many == [[(0, 1)] * M.WINDOWS_MAX]


# ---- 3. end to end on the micro checkpoint ----------------------------------------------------------------------------------------------------------------
def _strip(row, P, cfg):
    gen = row[P:]
    return gen[: next((q for q, t in enumerate(gen) if t in (cfg.eos_token_id, cfg.pad_token_id)), len(gen))]


def _own(row, cfg, P):
    """The row up to and including its first EOS behind the prompt."""
    return row[: P + len(_strip(row, P, cfg)) + 1]


def _cut_features(feats, F, step):
    """The plan's windows of [B, n_mels, T], cut here: frames behind T hold the clip's own minimum."""
    B, _, T = feats.shape
    starts = [0]
    while starts[-1] + F < T:
        starts.append(starts[-1] + step)
    wins = []
    for b in range(B):
        row = []
        for s in starts:
            w = torch.full((1, feats.shape[1], F), float(feats[b].min()), dtype=torch.float32, device=feats.device)
            n = min(F, T - s)
            w[0, :, :n] = feats[b, :, s: s + n]
            row.append(w)
        wins.append(row)
    return wins


def _reference(m, cfg, wins, **kw):
    """Every window decoded by a one-window generate, stripped, merged per clip by transformers' function, re-assembled."""
    P = len(synth.default_prompt(cfg))
    rows, cut, per_window = [], 0, []
    for clip in wins:
        outs = [m.generate(w, max_new_tokens=NEW, **kw) for w in clip]
        seqs = [(o["sequences"] if isinstance(o, dict) else o)[0].tolist() for o in outs]
        text = [_strip(s, P, cfg) for s in seqs]
        rows.append(seqs[0][:P] + M.hf_merge(text) + [cfg.eos_token_id])
        cut += sum(1 for b in M.boundary_info(text) if b["win"] is not None)
        per_window.append((outs, text))
    return rows, cut, per_window


@pytest.fixture(scope="module")
def long_feats(rig):
    cfg, m = rig
    T = 2 * cfg.n_mel_frames + 37
    return m.extract_features([synth.synth_clip(i, n_samples=T * 160) for i in (3, 4)], truncation=False)


@pytest.mark.parametrize("vanilla", [False, True], ids=["medusa", "vanilla"])
def test_strided_features_equal_the_windows_decoded_alone(rig, long_feats, vanilla):
    cfg, m = rig
    F, P = cfg.n_mel_frames, len(synth.default_prompt(cfg))
    assert F == 192 and long_feats.shape == (2, cfg.num_mel_bins, 2 * F + 37)
    kw = dict(vanilla=True) if vanilla else {}
    out = m.generate(long_feats, chunk_longform=True, stride_length_s=STRIDE * 0.01, max_new_tokens=NEW, return_dict_in_generate=True, **kw)
    assert m.last_stats["ms_merge"] > 0 and m.last_stats["longform_windows"] == [3, 3]
    wins = _cut_features(long_feats, F, F - 2 * STRIDE)
    assert [len(r) for r in wins] == [3, 3]
    want, cut, per_window = _reference(m, cfg, wins, **kw)
    print(f"strided end to end ({'vanilla' if vanilla else 'medusa'}): {cut} of 4 boundaries were cut inside an overlap")
    for b in range(2):
        assert _own(out["sequences"][b].tolist(), cfg, P) == want[b], b
        text = per_window[b][1]
        assert out["window_keep"][b].tolist() == [list(k) for k in M.keep_slices(text)]
    # stride_length_s=None: the route as it was — the windows cut at multiples of F, concatenated
    a = m.generate(long_feats, chunk_longform=True, max_new_tokens=NEW, **kw)
    b_ = m.generate(long_feats, chunk_longform=True, stride_length_s=None, max_new_tokens=NEW, return_dict_in_generate=True, **kw)
    assert isinstance(b_, torch.Tensor) and torch.equal(a, b_) and "ms_merge" not in m.last_stats
    plain = _cut_features(long_feats, F, F)
    for c in range(2):
        ids = synth.default_prompt(cfg) + [t for w in plain[c] for t in _strip(m.generate(w, max_new_tokens=NEW, **kw)[0].tolist(), P, cfg)]
        assert _own(a[c].tolist(), cfg, P) == ids + [cfg.eos_token_id]


def test_strided_wav_door_with_two_lengths(rig):
    cfg, m = rig
    F, P = cfg.n_mel_frames, len(synth.default_prompt(cfg))
    n, step = F * 160, (F - 2 * STRIDE) * 160
    wavs = [synth.synth_clip(5, n_samples=(2 * F + 37) * 160), synth.synth_clip(6, n_samples=300 * 160 + 77)]
    out = m.generate_from_wav(wavs, chunk_longform=True, stride_length_s=(STRIDE * 0.01, STRIDE * 0.01), max_new_tokens=NEW, return_dict_in_generate=True)
    assert m.last_stats["longform_windows"] == [3, 2]
    wins = []
    for wav in wavs:
        starts = [0]
        while starts[-1] + n < len(wav):
            starts.append(starts[-1] + step)
        wins.append([m.extract_features([wav[s: s + n]]) for s in starts])      # (the front end zero-pads a short chunk to the window)
    assert [len(r) for r in wins] == [3, 2]
    want, cut, per_window = _reference(m, cfg, wins)
    print(f"strided wav door: {cut} of 3 boundaries were cut inside an overlap")
    for b in range(2):
        assert _own(out["sequences"][b].tolist(), cfg, P) == want[b], b
    assert out["window_keep"][1, 2].tolist() == [-1, -1] and out["window_keep"][1, :2].min() >= 0


def test_strided_token_logprobs_follow_the_slices(rig, long_feats):
    cfg, m = rig
    F, P = cfg.n_mel_frames, len(synth.default_prompt(cfg))
    out = m.generate(long_feats, chunk_longform=True, stride_length_s=STRIDE * 0.01, max_new_tokens=NEW, return_token_logprobs=True)
    want, cut, per_window = _reference(m, cfg, _cut_features(long_feats, F, F - 2 * STRIDE), return_token_logprobs=True)
    for b in range(2):
        outs, text = per_window[b]
        assert _own(out["sequences"][b].tolist(), cfg, P) == want[b], b
        keep = M.keep_slices(text)
        lp = [0.0] * P + [float(v) for w, (lo, hi) in enumerate(keep) for v in outs[w]["token_logprobs"][0, P + lo: P + hi]]
        eos_lp = 0.0                     # the clip's one EOS: the score of the last window that emitted one
        for w, o in enumerate(outs):
            if P + len(text[w]) < int(o["lengths"][0]):
                eos_lp = float(o["token_logprobs"][0, P + len(text[w])])
        lp.append(eos_lp)
        n = len(want[b])
        assert int(out["lengths"][b]) == n
        # the tolerance tests/test_gpu_scores.py holds between a batch's scoring pass and the one-clip call's
        assert torch.allclose(out["token_logprobs"][b, :n].cpu(), torch.tensor(lp, dtype=torch.float32), atol=1e-4), b
    assert out["window_avg_logprob"].shape == (2, 3) and out["window_keep"].shape == (2, 3, 2)


def test_strided_token_timestamps_follow_the_slices(rig, long_feats):
    cfg, m = rig
    assert cfg.alignment_heads
    F, P = cfg.n_mel_frames, len(synth.default_prompt(cfg))
    step = F - 2 * STRIDE
    out = m.generate(long_feats, chunk_longform=True, stride_length_s=STRIDE * 0.01, max_new_tokens=NEW, return_token_timestamps=True)
    assert m.last_stats["ms_token_timestamps"] > 0 and m.last_stats["ms_merge"] > 0
    wins = _cut_features(long_feats, F, step)
    cuts = 0
    for b in range(2):
        outs = [m.generate(w, max_new_tokens=NEW, return_token_timestamps=True) for w in wins[b]]
        text = [_strip(o["sequences"][0].tolist(), P, cfg) for o in outs]
        times = [(o["token_timestamps"][0, P: P + len(t)].cpu() + torch.tensor(j * step * 0.01, dtype=torch.float32)).tolist()
                 for j, (o, t) in enumerate(zip(outs, text))]
        ids, tt = M.hf_merge(text, times)
        cuts += sum(1 for x in M.boundary_info(text, times) if x["win"] is not None)
        n = P + len(ids) + 1
        assert out["sequences"][b, :n].tolist() == synth.default_prompt(cfg) + ids + [cfg.eos_token_id], b
        want_tt = [0.0] * P + tt
        want_tt.append(want_tt[-1])
        assert out["token_timestamps"][b, :n].tolist() == [float(np.float32(v)) for v in want_tt], b
    print(f"strided token timestamps: {cuts} of 4 boundaries were cut inside an overlap")
