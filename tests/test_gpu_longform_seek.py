"""Sequential long-form decoding on the GPU (generate(sequential_longform=True)): the whole-recording log-mel (wm_logmel_long), the
window gather (wm_gather_windows) and the seek loop end to end, at the micro shape of tests/test_gpu_timestamps.py (window: 192 frames, 30 720
samples).  The end-to-end reference is the loop of tests/longform_seek.py: torch slicing plus zero pad on the oracle's log-mel, `Ref.decode`
(oracle + transformers' timestamp processor) and transformers' `_retrieve_segment`; its recordings clear 10 x the tie tolerances at every decision
(tests/test_longform_seek_cpu.py asserts it), so no tie is followed and no window left out."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import longform_seek as LS
from helpers import synth
from oracle.whisper_medusa_oracle import log_mel
from whisper_medusa import WhisperMedusaModel
from whisper_medusa.timestamps import row_segments

pytestmark = pytest.mark.gpu

W = LS.WINDOW                   # 30 720 samples
FW = 192


@pytest.fixture(scope="module")
def rig(gpu):
    cfg, sd, gp, wavs, recs = LS.reference_run()
    # the bf16 hi / lo operand contract, as tests/test_gpu_timestamps.py (the oracle of Ref runs it too)
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=4, act_fp16=False)
    return dict(cfg=cfg, gp=gp, wavs=wavs, recs=recs, m=m)


def _pad_batch(wavs, n):
    buf = np.zeros((len(wavs), n), dtype=np.float32)
    for i, w in enumerate(wavs):
        buf[i, : len(w)] = w
    return buf


# ---- 1. wm_logmel_long -------------------------------------------------------------------------------------------------------------------------
def test_logmel_long_matches_the_oracle(gpu, rig):
    m, cfg = rig["m"], rig["cfg"]
    lens = (160, W + 160 * 7, 3 * W + 160)
    wavs = [synth.synth_clip(i, n_samples=n) for i, n in enumerate(lens)]
    n = max(lens)
    got = m.engine.logmel_long(torch.from_numpy(_pad_batch(wavs, n)).to(gpu)).cpu().numpy()
    assert got.shape == (3, cfg.num_mel_bins, n // 160)
    for i, w in enumerate(wavs):
        d = np.abs(got[i] - log_mel(w, cfg.num_mel_bins, n))
        print(f"logmel_long clip {i} ({lens[i]} samples in {n}): max |d| {d.max():.3g}")
        assert d.max() <= 2e-3, (i, d.max())
    # the public route: a list of ragged clips -> the same features, every clip's own frame count kept
    f = m.extract_features(wavs, truncation=False)
    assert m.last_num_frames.tolist() == [1, 199, 577] and m.last_num_frames.dtype == torch.long
    assert np.array_equal(f.cpu().numpy(), got)
    # 160 samples alone: one frame, both reflections inside the clip
    one = m.engine.logmel_long(torch.from_numpy(wavs[0][None]).to(gpu)).cpu().numpy()
    assert one.shape == (1, cfg.num_mel_bins, 1) and np.abs(one[0] - log_mel(wavs[0], cfg.num_mel_bins, 160)).max() <= 2e-3
    with pytest.raises(ValueError, match="wm_logmel_long"):
        m.engine.logmel_long(torch.zeros(1, 200, device=gpu))


def test_logmel_long_clamps_at_the_whole_recordings_maximum(gpu, rig):
    """The loudest burst of the recording sits in its LAST window; the first window is digital silence, i.e. clamped: its level is the
    recording's maximum - 8 (in log10 units; - 2 after (x + 4) / 4) and moves with the burst."""
    m, cfg = rig["m"], rig["cfg"]
    n = 3 * W
    base = 0.1 * synth.synth_clip(4, n_samples=n)
    base[:W] = 0.0
    loud = base.copy()
    loud[2 * W + 5000: 2 * W + 9000] = synth.synth_clip(5, n_samples=4000)
    f = m.engine.logmel_long(torch.from_numpy(np.stack([base, loud])).to(gpu)).cpu()
    for i, w in enumerate((base, loud)):
        assert float((f[i] - torch.from_numpy(log_mel(w, cfg.num_mel_bins, n))).abs().max()) <= 2e-3
    first = f[:, :, 2: FW - 2]                                   # (the frames next to the second window see its samples)
    floor = first.amin(dim=(1, 2))
    assert torch.equal(first.amax(dim=(1, 2)), floor)            # silence: every value is the clamp
    assert torch.allclose(floor, f.amax(dim=(1, 2)) - 2.0, atol=1e-6)
    assert int(f[1].flatten().argmax()) % f.shape[-1] >= 2 * FW  # the maximum is in the last window
    assert float(floor[1] - floor[0]) > 0.25                     # a burst 10 x the level: about 2 in log10 power, / 4


def test_logmel_long_at_one_window_is_wm_logmel(gpu, rig):
    m = rig["m"]
    wav = torch.from_numpy(np.stack([synth.synth_clip(6, n_samples=W), synth.synth_clip(7, n_samples=W)])).to(gpu)
    assert torch.equal(m.engine.logmel_long(wav), m.engine.logmel(wav))


# ---- 2. wm_gather_windows ----------------------------------------------------------------------------------------------------------------------
def test_gather_windows_is_slice_then_zero_pad(gpu, rig):
    m, cfg = rig["m"], rig["cfg"]
    frames = 578
    feats = torch.randn(3, cfg.num_mel_bins, frames, generator=torch.Generator().manual_seed(3)).to(gpu)
    #        clip seek n_valid: seek 0; an odd multiple of 2; the last full window; n_valid 1 and F - 1; two windows of clip 0; 7 windows of 3 clips
    wins = [(0, 0, FW), (1, 38, FW), (2, frames - FW, FW), (0, 100, 1), (0, 200, FW - 1), (1, frames - 50, 50), (2, frames - 1, 1)]
    got = m.engine.gather_windows(feats, [w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    assert got.shape == (len(wins), cfg.num_mel_bins, FW)
    for q, (c, s, n) in enumerate(wins):
        want = F.pad(feats[c, :, s: s + n], (0, FW - n))
        assert torch.equal(got[q], want), (q, c, s, n)
    # an odd frame count (rows of the source are then not even 8-byte aligned)
    odd = feats[:, :, :577].contiguous()
    got = m.engine.gather_windows(odd, [1, 2], [2, 386], [FW, 191])
    assert torch.equal(got[0], odd[1, :, 2: 2 + FW]) and torch.equal(got[1], F.pad(odd[2, :, 386: 577], (0, 1)))


@pytest.mark.parametrize("clip,seek,n_valid,word", [([0, 3], [0, 0], [FW, FW], "clip index"), ([0, 1], [0, -2], [FW, FW], "seek"),
                                                    ([0, 1], [0, 0], [FW, FW + 1], "n_valid"), ([0, 1], [0, 578 - FW + 2], [FW, FW], "exceeds frames")])
def test_gather_windows_refuses_bad_windows(gpu, rig, clip, seek, n_valid, word):
    m, cfg = rig["m"], rig["cfg"]
    feats = torch.ones(3, cfg.num_mel_bins, 578, device=gpu)
    out = torch.full((2, cfg.num_mel_bins, FW), 7.0, device=gpu)
    with pytest.raises(ValueError, match=word):                    # WM_ERR_ARG
        m.engine.gather_windows(feats, clip, seek, n_valid, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- 3. the loop, end to end -------------------------------------------------------------------------------------------------------------------
def _check_against_reference(out, stats, cfg, gp, recs):
    pad = cfg.pad_token_id
    assert stats["longform_windows"] == [len(r) for r in recs]
    T = out["sequences"].shape[1]
    for b, rec in enumerate(recs):
        want = LS.sequence_of(gp, rec)
        assert out["sequences"][b].tolist() == want + [pad] * (T - len(want)), (b, out["sequences"][b].tolist(), want)
        segs = [sg for w in rec for sg in w["segments"]]
        assert len(out["segments"][b]) == len(segs)
        for g, w in zip(out["segments"][b], segs):
            assert g["tokens"].tolist() == w["tokens"].tolist()
            for k in ("start", "end"):
                assert g[k].dtype == torch.float64 and float(g[k]) == float(w[k]), (b, k, g[k], w[k])


def test_sequential_longform_matches_the_reference_loop(gpu, rig):
    m, cfg, gp, recs = rig["m"], rig["cfg"], rig["gp"], rig["recs"]
    out = m.generate_from_wav(rig["wavs"], sequential_longform=True, return_timestamps=True, return_segments=True, max_new_tokens=LS.MAX_NEW)
    print("windows", m.last_stats["longform_windows"], "seeks", [[(w["seek"], w["segment_offset"]) for w in r] for r in recs])
    assert m.last_num_frames.tolist() == [len(w) // 160 for w in rig["wavs"]]
    _check_against_reference(out, m.last_stats, cfg, gp, recs)
    assert max(len(r) for r in recs) >= 4 and sum(len(r) for r in recs) == 8
    # one recording alone (the longest: padded to the same length, so the same features): the batch does not matter
    one = m.generate_from_wav(rig["wavs"][2:], sequential_longform=True, return_timestamps=True, return_segments=True, max_new_tokens=LS.MAX_NEW)
    _check_against_reference(one, m.last_stats, cfg, gp, recs[2:])
    # plain tensor without return_segments; features + attention_mask is the same call
    feats = m.extract_features(rig["wavs"], truncation=False)
    mask = (torch.arange(feats.shape[-1])[None] < m.last_num_frames[:, None]).long()
    t = m.generate(feats, attention_mask=mask, sequential_longform=True, return_timestamps=True, max_new_tokens=LS.MAX_NEW)
    assert isinstance(t, torch.Tensor) and torch.equal(t, out["sequences"])


# ---- 4. a window the no-speech gate skips ----------------------------------------------------------------------------------------------------------
def test_sequential_longform_skips_one_window(gpu, rig):
    m, cfg, gp, recs = rig["m"], rig["cfg"], rig["gp"], rig["recs"]
    thr, p0, p1 = LS.skip_threshold(recs)
    hit = [(b, j) for b, rec in enumerate(recs) for j, w in enumerate(rec) if w["no_speech_prob"] > thr]
    assert len(hit) == 1
    hb, hj = hit[0]
    out = m.generate_from_wav(rig["wavs"], sequential_longform=True, return_timestamps=True, return_segments=True, max_new_tokens=LS.MAX_NEW,
                              no_speech_threshold=thr)
    for b, rec in enumerate(recs):
        got = out["no_speech_prob"][b].tolist()
        print(f"no-speech, recording {b}: engine {got}, reference {[w['no_speech_prob'] for w in rec]}, threshold {thr}")
        assert len(got) == len(rec)
        for g, w in zip(got, rec):
            assert abs(math.log(g) - math.log(w["no_speech_prob"])) <= 0.12          # the bound of tests/test_gpu_scores.py
        assert out["skipped"][b].tolist() == [(b, j) == (hb, hj) for j in range(len(rec))]
    # the skipped window advanced by its seek_num_frames — what its own rule gave as well (tests/test_longform_seek_cpu.py), so the windows behind
    # it are the reference's — and left neither ids nor segments
    w = recs[hb][hj]
    nxt = w["seek"] + w["seek_num_frames"]
    assert out["window_seek"][hb].tolist() == [x["seek"] for x in recs[hb]]
    assert nxt >= len(rig["wavs"][hb]) // 160 or recs[hb][hj + 1]["seek"] == nxt
    want = [[dict(x, segments=[], ids=[]) if (b, j) == (hb, hj) else x for j, x in enumerate(rec)] for b, rec in enumerate(recs)]
    _check_against_reference(out, m.last_stats, cfg, gp, want)
    assert out["segments"][hb] == [] or all(float(g["start"]) >= nxt * 0.01 or float(g["end"]) <= w["seek"] * 0.01 for g in out["segments"][hb])
    if len(recs[hb]) == 1:
        assert out["sequences"][hb].tolist()[: len(gp.prompt) + 1] == list(gp.prompt) + [gp.eos_token_id] and out["segments"][hb] == []


# ---- 5. chunk_longform is where it was ---------------------------------------------------------------------------------------------------------
def test_chunk_longform_is_untouched(gpu, rig):
    """The fixed-window path on the same input, two ways through code this feature does not touch: `chunk_longform=True`, and the short-form
    generate() on the fixed windows (padded with the clip's minimum) assembled by that path's rule — before and after a sequential run on the
    same model."""
    m, cfg, gp = rig["m"], rig["cfg"], rig["gp"]
    feats = m.extract_features(rig["wavs"], truncation=False)
    kw = dict(return_timestamps=True, return_segments=True, max_new_tokens=LS.MAX_NEW)
    a = m.generate(feats, chunk_longform=True, **kw)
    m.generate(feats, sequential_longform=True, **kw)
    b = m.generate(feats, chunk_longform=True, **kw)
    assert torch.equal(a["sequences"], b["sequences"])
    B, _, T = feats.shape
    n = -(-T // FW)
    x = feats.amin(dim=(1, 2), keepdim=True).expand(B, cfg.num_mel_bins, n * FW).clone()
    x[..., :T] = feats
    P, eos, pad = len(gp.prompt), cfg.eos_token_id, cfg.pad_token_id
    win = x.view(B, cfg.num_mel_bins, n, FW).permute(0, 2, 1, 3).reshape(B * n, cfg.num_mel_bins, FW).contiguous()
    rows = m.generate(win, return_timestamps=True, max_new_tokens=LS.MAX_NEW)          # (one batch, as that path decodes them)
    for c in range(B):
        ids, segs = list(gp.prompt), []
        for j in range(n):
            r = rows[c * n + j].tolist()
            ids += LS.generated(r, P, eos)
            segs += row_segments(r, P, eos, cfg.timestamp_begin, FW, time_offset=j * FW * 0.01)
        ids.append(eos)
        assert a["sequences"][c].tolist()[: len(ids)] == ids and all(t == pad for t in a["sequences"][c].tolist()[len(ids):])
        assert len(a["segments"][c]) == len(segs)
        for g, w in zip(a["segments"][c], segs):
            assert torch.equal(g["start"], w["start"]) and torch.equal(g["end"], w["end"]) and torch.equal(g["tokens"], w["tokens"])
