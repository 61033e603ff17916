"""chunk_longform with overlapping windows (stride_length_s) without a GPU: the two references of tests/merge_ref.py against each
other on the shared case list, the classes that list has to hold, the window plan against transformers' chunk_iter, the route through generate()
and generate_from_wav() over an engine double whose merge_windows IS the restated contract, and the surface (refusals, header, export, ABI)."""
import os

import numpy as np
import pytest
import torch

import merge_ref as M
import scores_ref as R
from helpers import synth
from test_topk_cpu import _Eng, _model
from whisper_medusa import scores as S
from whisper_medusa.api import WhisperMedusaModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = M.cpu_cases()


# ---- the references ---------------------------------------------------------------------------------------------------------------------------
def test_keep_slices_reassemble_to_transformers_merge_on_every_case():
    for n, c in enumerate(CASES):
        ws, ts = c["windows"], c["times"]
        keep = M.keep_slices(ws, ts)
        assert all(keep[w] == (0, 0) for w in range(len(ws)) if len(ws[w]) == 0), n
        assert all(0 <= a <= b <= len(ws[w]) for w, (a, b) in enumerate(keep)), n
        if ts is None:
            assert M.assemble(ws, keep) == M.hf_merge(ws), n
        else:
            ids, times = M.hf_merge(ws, ts)
            assert M.assemble(ws, keep) == ids and M.assemble(ws, keep, ts) == times, n
            # the same windows without times: transformers' other branch (one numpy compare per shift)
            assert M.assemble(ws, M.keep_slices(ws)) == M.hf_merge(ws), n


def test_case_list_holds_every_class():
    """On the references alone: at least 5 boundaries (cases, for the two case-level classes) of every class the issue names."""
    total = {}
    for c in CASES:
        for k, v in M.case_classes(c).items():
            total[k] = total.get(k, 0) + v
    print("classes:", total)
    assert set(M.CLASSES) <= set(total), sorted(set(M.CLASSES) - set(total))
    assert all(total[k] >= 5 for k in M.CLASSES), total


def test_one_window_and_empty_windows():
    assert M.keep_slices([[5, 6, 7]]) == [(0, 3)]
    assert M.keep_slices([[], [], []]) == [(0, 0)] * 3
    # the empty window is no link: [1 2 3 4] and [3 4 5] meet directly (shift 2, cut in the middle of the overlap)
    assert M.keep_slices([[1, 2, 3, 4], [], [3, 4, 5]]) == [(0, 3), (0, 0), (1, 3)]
    assert M.assemble([[1, 2, 3, 4], [], [3, 4, 5]], [(0, 3), (0, 0), (1, 3)]) == [1, 2, 3, 4, 5]
    # one common id is no match (matches > 1): concatenation
    assert M.keep_slices([[1, 2, 3], [3, 9]]) == [(0, 3), (0, 2)]
    # times out of order: the overlap does not count
    assert M.keep_slices([[1, 2, 3, 4], [3, 4, 5]], [[0.0, 1.0, 2.0, 3.0], [1.0, 2.0, 6.0]]) == [(0, 4), (0, 3)]
    assert M.keep_slices([[1, 2, 3, 4], [3, 4, 5]], [[0.0, 1.0, 2.0, 3.0], [2.0, 3.0, 6.0]]) == [(0, 3), (1, 3)]


# ---- the window plan ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,left,right", [(192, 32, 32), (192, 10, 50), (192, 0, 7), (3000, 500, 500), (192, 95, 95)])
def test_window_plan_is_chunk_iter(F, left, right):
    step = F - left - right
    Ts = {F + 1, F + step - 1, F + step, F + step + 1, F + 3 * step - 1, F + 3 * step, F + 3 * step + 1, 4 * step - 1, 4 * step, 4 * step + 1,
          2 * F + 37}
    for T in sorted(t for t in Ts if t > F):
        starts = WhisperMedusaModel._window_plan(T, F, left, right)
        assert [(s, min(s + F, T)) for s in starts] == M.hf_chunk_plan(T, F, left, right), T
        assert starts == [j * step for j in range(len(starts))] and starts[-1] + F >= T and (len(starts) < 2 or starts[-2] + F < T)


# ---- the route: an engine double ------------------------------------------------------------------------------------------------------------------
EN, DE = "<|en|>", "<|de|>"
LANG_ID = {EN: 20, DE: 21}
# what a window whose first frame holds the code decodes to (text ids alone); 0 / 1 / 2 overlap by two ids each, 6 / 7 by three with one damaged
SCRIPT = {0: [101, 102, 103, 104, 105], 1: [104, 105, 106, 107, 108], 2: [107, 108, 109], 5: [300, 301],
          6: [201, 202, 203, 204, 205, 206], 7: [204, 299, 206, 207], 8: [207, 208], 9: [400, 401, 402]}
STRIDE_S, STEP, NFR = 0.32, 128, 2 * 192 + 37          # 32 frames each side of the micro window (192): 3 windows over 421 frames


def _cfg():
    cfg = R.micro_ts("base_head")
    cfg.is_multilingual = True
    cfg.lang_to_id = dict(LANG_ID)
    cfg.task_to_id = {"transcribe": 30, "translate": 31}
    cfg.alignment_heads = [[0, 0]]
    return cfg


def _lp(c, t):
    return float(np.float32(-(c + t / 100.0)))


def _ts(c, t):
    return 8.0 * c + 0.25 * t


class _StrideEng(_Eng):
    max_batch = 8

    def decode(self, gp, B, **kw):
        self.calls.append(("decode", B, tuple(gp.prompt)))
        return [list(gp.prompt_of(b)) + SCRIPT[c] + [gp.eos_token_id] for b, c in enumerate(self.clips[:B])]

    def stats(self):
        return dict(ms_decode=1.0, ms_encode=1.0)

    def token_timestamps(self, seqs, n_prompt, heads, width, time_precision, num_frames):
        self.calls.append(("token_timestamps", len(seqs), num_frames))
        out = np.zeros((len(seqs), max(len(s) for s in seqs)), np.float32)
        for b, s in enumerate(seqs):
            out[b, : len(s)] = [_ts(self.clips[b], t) for t in range(len(s))]
        return out, 2.0

    def logmel(self, buf):
        self.calls.append(("logmel", buf.shape[0]))
        assert buf.shape[1] == self.cfg.n_mel_frames * 160
        return buf[:, :1, None].expand(buf.shape[0], self.cfg.num_mel_bins, self.cfg.n_mel_frames).clone()

    def merge_windows(self, windows_per_clip, times_per_clip=None):
        self.calls.append(("merge_windows", [[list(w) for w in clip] for clip in windows_per_clip], times_per_clip))
        self.last_merge_ms = 0.5
        return [M.keep_slices(ws, None if times_per_clip is None else times_per_clip[c]) for c, ws in enumerate(windows_per_clip)]


def _strided(cfg, codes):
    """Features of NFR frames: the window that starts at j * STEP holds codes[b][j] (the double reads a window's first frame)."""
    f = torch.zeros(len(codes), cfg.num_mel_bins, NFR)
    for b, row in enumerate(codes):
        for j, v in enumerate(row):
            f[b, :, j * STEP: (j + 1) * STEP] = float(v)
    return f


def _prompt(cfg, lang):
    return synth.default_prompt(cfg, lang, "transcribe", timestamps=False)


def _padded(rows, fill, dtype):
    T = max(len(r) for r in rows)
    return torch.tensor([list(r) + [fill if fill is not None else r[-1]] * (T - len(r)) for r in rows], dtype=dtype)


def test_strided_ids_and_window_keep():
    cfg = _cfg()
    eng = _StrideEng(cfg)
    m = _model(cfg, eng, 8)
    feats = _strided(cfg, [[0, 1, 2], [6, 7, 8]])
    out = m.generate(feats, chunk_longform=True, stride_length_s=STRIDE_S, language="en", return_dict_in_generate=True)
    assert [c[:2] for c in eng.calls] == [("encode", 6), ("decode", 6), ("merge_windows", [[SCRIPT[0], SCRIPT[1], SCRIPT[2]], [SCRIPT[6], SCRIPT[7], SCRIPT[8]]])]
    assert eng.calls[-1][2] is None
    rows = [_prompt(cfg, EN) + [101, 102, 103, 104, 105, 106, 107, 108, 109, cfg.eos_token_id],
            # [201 .. 206] against [204 299 206 207]: shift 3 with 2 of 3 (fault tolerance), cut in the middle: 201 .. 204 | 299 206 ... then 207 twice -> one match only: concatenated
            _prompt(cfg, EN) + [201, 202, 203, 204, 299, 206, 207, 207, 208, cfg.eos_token_id]]
    assert torch.equal(out["sequences"], _padded(rows, cfg.pad_token_id, torch.long))
    assert out["window_keep"].tolist() == [[[0, 4], [1, 4], [1, 3]], [[0, 4], [1, 4], [0, 2]]]
    assert m.last_stats["ms_merge"] == 0.5 and m.last_stats["longform_windows"] == [3, 3]
    # the plain tensor without the dict form; the same rows
    eng.calls.clear()
    t = m.generate(feats, chunk_longform=True, stride_length_s=(STRIDE_S, STRIDE_S), language="en")
    assert isinstance(t, torch.Tensor) and torch.equal(t, out["sequences"])


def test_strided_padding_is_the_clips_minimum():
    cfg = _cfg()
    m = _model(cfg, _StrideEng(cfg), 8)
    f = _strided(cfg, [[0, 1, 2]])
    f[0, 3, 7] = -3.5
    win, counts = m._strided_feature_windows(f, (32, 32))
    assert counts == [3] and win.shape == (3, cfg.num_mel_bins, 192)
    assert torch.equal(win[2, :, : NFR - 2 * STEP], f[0, :, 2 * STEP:]) and torch.all(win[2, :, NFR - 2 * STEP:] == -3.5)
    assert torch.equal(win[1], f[0, :, STEP: STEP + 192])


def test_strided_token_logprobs_and_skipped_window():
    cfg = _cfg()
    eos = cfg.eos_token_id
    eng = _StrideEng(cfg, no_speech={5: 0.95})
    m = _model(cfg, eng, 8)
    out = m.generate(_strided(cfg, [[0, 1, 2], [0, 5, 2]]), chunk_longform=True, stride_length_s=STRIDE_S, language="en",
                     return_token_logprobs=True, no_speech_threshold=0.6)
    P = len(_prompt(cfg, EN))
    # clip 1: its middle window is gated, enters the merge empty, and [101 .. 105] / [107 108 109] share nothing: concatenated
    assert [c for c in eng.calls if c[0] == "merge_windows"][0][1] == [[SCRIPT[0], SCRIPT[1], SCRIPT[2]], [SCRIPT[0], [], SCRIPT[2]]]
    rows = [_prompt(cfg, EN) + list(range(101, 110)) + [eos], _prompt(cfg, EN) + [101, 102, 103, 104, 105, 107, 108, 109, eos]]
    assert torch.equal(out["sequences"], _padded(rows, cfg.pad_token_id, torch.long))
    assert out["window_keep"].tolist() == [[[0, 4], [1, 4], [1, 3]], [[0, 5], [0, 0], [0, 3]]]
    lp = [[0.0] * P + [_lp(0, P + q) for q in range(4)] + [_lp(1, P + q) for q in range(1, 4)] + [_lp(2, P + q) for q in (1, 2)] + [_lp(2, P + 3)],
          [0.0] * P + [_lp(0, P + q) for q in range(5)] + [_lp(2, P + q) for q in range(3)] + [_lp(2, P + 3)]]     # the EOS: the last kept window's
    assert torch.equal(out["token_logprobs"], _padded(lp, 0.0, torch.float32))
    assert out["avg_logprob"].tolist() == pytest.approx([S.avg_logprob(r, P, len(r)) for r in lp], abs=1e-6)
    assert out["compression_ratio"].tolist() == pytest.approx([S.compression_ratio(r[P:], cfg.vocab_size) for r in rows])
    assert out["lengths"].tolist() == [len(r) for r in rows]
    assert out["skipped"].tolist() == [[False, False, False], [False, True, False]]
    assert out["no_speech_prob"].tolist() == [pytest.approx([0.1, 0.1, 0.1]), pytest.approx([0.1, 0.95, 0.1])]
    assert out["window_avg_logprob"].shape == (2, 3)
    assert torch.equal(m.last_scores["token_logprobs"], out["token_logprobs"])


def test_strided_token_timestamps_carry_the_window_offsets():
    cfg = _cfg()
    eng = _StrideEng(cfg)
    m = _model(cfg, eng, 8)
    out = m.generate(_strided(cfg, [[0, 1, 2]]), chunk_longform=True, stride_length_s=STRIDE_S, language="en", return_token_timestamps=True)
    P = len(_prompt(cfg, EN))

    def at(j, q):      # window j's own value at text position q, offset by the window's start in float32
        return float(torch.tensor(_ts(j, P + q), dtype=torch.float32) + torch.tensor(j * STEP * 0.01, dtype=torch.float32))

    # the merge gets the same absolute times, one per text id of every window
    call = [c for c in eng.calls if c[0] == "merge_windows"][0]
    assert call[2] == [[[at(j, q) for q in range(len(SCRIPT[j]))] for j in range(3)]]
    tt = [0.0] * P + [at(0, q) for q in range(4)] + [at(1, q) for q in range(1, 4)] + [at(2, q) for q in (1, 2)]
    assert torch.equal(out["token_timestamps"], _padded([tt + [tt[-1]]], None, torch.float32))
    assert out["window_keep"].tolist() == [[[0, 4], [1, 4], [1, 3]]]
    assert out["sequences"][0].tolist() == _prompt(cfg, EN) + list(range(101, 110)) + [cfg.eos_token_id]
    assert m.last_stats["ms_token_timestamps"] == 2.0


def test_strided_language_list_and_detection():
    cfg = _cfg()
    eng = _StrideEng(cfg, lang_ids={0: 20, 6: 21})
    m = _model(cfg, eng, 8)
    feats = _strided(cfg, [[0, 1, 2], [6, 7, 8]])
    out = m.generate(feats, chunk_longform=True, stride_length_s=STRIDE_S, language=["de", "en"])
    rows = [_prompt(cfg, DE) + list(range(101, 110)) + [cfg.eos_token_id], _prompt(cfg, EN) + [201, 202, 203, 204, 299, 206, 207, 207, 208, cfg.eos_token_id]]
    assert torch.equal(out, _padded(rows, cfg.pad_token_id, torch.long))
    assert [c[2] for c in eng.calls if c[0] == "decode"] == [tuple(_prompt(cfg, DE)), tuple(_prompt(cfg, EN))]
    assert len([c for c in eng.calls if c[0] == "merge_windows"]) == 1           # one merge for the whole call
    # detection: once per clip, on its first window
    eng.calls.clear()
    out = m.generate(feats, chunk_longform=True, stride_length_s=STRIDE_S)
    assert eng.calls[0] == ("encode", 2)
    rows = [_prompt(cfg, EN) + rows[0][4:], _prompt(cfg, DE) + rows[1][4:]]
    assert torch.equal(out, _padded(rows, cfg.pad_token_id, torch.long))
    with pytest.raises(ValueError):
        m.generate(feats, chunk_longform=True, stride_length_s=STRIDE_S, language=["de", "en", "en"])


def test_strided_generate_from_wav_ragged_counts():
    cfg = _cfg()
    eng = _StrideEng(cfg)
    m = _model(cfg, eng, 2)
    long = np.zeros(NFR * 160, np.float32)
    for j, code in enumerate((0, 1, 2)):
        long[j * STEP * 160: (j + 1) * STEP * 160] = code
    short = np.full(20000, 9.0, np.float32)         # under one window: a single, zero-padded one
    win, counts = m._strided_wav_windows([long, short], 16000, (32, 32))
    assert [c[1] for c in eng.calls if c[0] == "logmel"] == [2, 2]              # groups of at most max_batch windows
    assert counts == [3, 1] and win[:, 0, 0].tolist() == [0.0, 1.0, 2.0, 9.0]
    eng.calls.clear()
    m = _model(cfg, eng, 8)
    out = m.generate_from_wav([long, short], chunk_longform=True, stride_length_s=STRIDE_S, language="en", return_dict_in_generate=True,
                              return_token_logprobs=True)
    assert [c[1] for c in eng.calls if c[0] == "logmel"] == [4]
    assert [c[1] for c in eng.calls if c[0] == "merge_windows"] == [[[SCRIPT[0], SCRIPT[1], SCRIPT[2]], [SCRIPT[9]]]]
    rows = [_prompt(cfg, EN) + list(range(101, 110)) + [cfg.eos_token_id], _prompt(cfg, EN) + [400, 401, 402, cfg.eos_token_id]]
    assert torch.equal(out["sequences"], _padded(rows, cfg.pad_token_id, torch.long))
    assert out["window_keep"].tolist() == [[[0, 4], [1, 4], [1, 3]], [[0, 3], [-1, -1], [-1, -1]]]
    assert m.last_stats["longform_windows"] == [3, 1]
    wavg = out["window_avg_logprob"]
    assert wavg.shape == (2, 3) and not torch.isnan(wavg[0]).any() and torch.isnan(wavg[1]).tolist() == [False, True, True]
    # without the keyword: what the method did before (one truncated window per recording)
    eng.calls.clear()
    t = m.generate_from_wav([short], language="en")
    assert [c[0] for c in eng.calls] == ["logmel", "encode", "decode"] and t[0].tolist() == rows[1]


def test_without_the_keyword_the_unstrided_route_runs():
    cfg = _cfg()
    eng = _StrideEng(cfg)
    m = _model(cfg, eng, 8)
    f = torch.zeros(1, cfg.num_mel_bins, 2 * 192)
    f[:, :, 192:] = 2.0
    out = m.generate(f, chunk_longform=True, language="en", stride_length_s=None, return_dict_in_generate=True)
    assert [c[0] for c in eng.calls] == ["encode", "decode"]                     # no merge
    assert isinstance(out, torch.Tensor) and out[0].tolist() == _prompt(cfg, EN) + SCRIPT[0] + SCRIPT[2] + [cfg.eos_token_id]
    assert "ms_merge" not in m.last_stats


# ---- surface and refusals ---------------------------------------------------------------------------------------------------------------------------
def test_stride_length_s_refusals():
    cfg = _cfg()
    m = _model(cfg, _StrideEng(cfg), 8)
    f = _strided(cfg, [[0, 1, 2]])
    short = f[..., :192]
    ok = dict(chunk_longform=True, language="en")
    for kw in (dict(language="en"), dict(language="en", chunk_longform=False), dict(language="en", sequential_longform=True, return_timestamps=True),
               dict(language="en", sequential_longform=True, chunk_longform=True, return_timestamps=True)):
        for x in (f, short):
            with pytest.raises(ValueError, match="only valid together with chunk_longform"):
                m.generate(x, stride_length_s=STRIDE_S, **kw)
    with pytest.raises(ValueError, match="only valid together with chunk_longform"):
        m.generate_from_wav(np.zeros(70000, np.float32), stride_length_s=STRIDE_S, language="en")
    for bad in (0.325, (0.32, 0.005), -0.32, float("nan")):
        with pytest.raises(ValueError, match="whole number of 10 ms frames"):
            m.generate(f, stride_length_s=bad, **ok)
    for bad in ("5", (0.1, 0.1, 0.1), True, (0.1, None)):
        with pytest.raises(ValueError, match="float or a pair"):
            m.generate(f, stride_length_s=bad, **ok)
    with pytest.raises(ValueError, match="has to be positive"):
        m.generate(f, stride_length_s=0.0, **ok)
    for bad in (0.96, (1.0, 0.92), 5.0):
        with pytest.raises(ValueError, match="less than the window"):
            m.generate(f, stride_length_s=bad, **ok)
    with pytest.raises(NotImplementedError, match="return_timestamps=True is not supported with stride_length_s"):
        m.generate(f, stride_length_s=STRIDE_S, return_timestamps=True, **ok)
    # what chunk_longform refuses stays refused
    with pytest.raises(NotImplementedError, match="chunk_longform"):
        m.generate(f, stride_length_s=STRIDE_S, top_logprobs=2, **ok)
    with pytest.raises(NotImplementedError, match="chunk_longform"):
        m.generate(f, stride_length_s=STRIDE_S, sampling_seed=1, temperature=0.5, **ok)
    with pytest.raises(NotImplementedError, match="chunk_longform"):
        m.generate(f, stride_length_s=STRIDE_S, vanilla=True, num_beams=2, **ok)
    with pytest.raises(NotImplementedError, match="num_frames"):
        m.generate(f, stride_length_s=STRIDE_S, return_token_timestamps=True, num_frames=[100], **ok)
    # unequal sides are a pair
    assert m._stride_frames((0.1, 0.5)) == (10, 50) and m._stride_frames(0.32) == (32, 32) and m._stride_frames((0, 0.07)) == (0, 7)


def test_header_export_and_abi(built_lib):
    import build as wm_build
    from whisper_medusa import engine
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert "int wm_merge_windows(wm_ctx* ctx, int C, const int32_t* first /* HOST [C+1] */," in hdr
    assert "#define WM_MERGE_LEN_MAX      512" in hdr and "#define WM_MERGE_WINDOWS_MAX 4096" in hdr and "#define WM_ABI_VERSION 9" in hdr
    assert "_find_longest_common_sequence" in hdr and "chunk_iter" in hdr
    assert "wm_merge.hip" in wm_build.SOURCES and "wm_merge_windows" in engine.EXPORTS
    assert (engine.MERGE_LEN_MAX, engine.MERGE_WINDOWS_MAX) == (M.LEN_MAX, M.WINDOWS_MAX) == (512, 4096)
    assert engine.WM_ABI_VERSION == 9
    for f16 in (False, True):
        lib = engine.load_library(act_fp16=f16)
        assert lib.wm_abi_version() == 9 and lib.wm_merge_windows.restype is not None
    assert callable(engine.Engine.merge_windows)
