"""The four routes of generate() — grouped language detection, chunk long-form, sequential long-form, short-form — combined with the requests
that ride on the short-form decode (scoring, token timestamps, beams, the temperature ladder), black-box: only the public generate() and an
engine double installed as ``m._engine``.  Every expectation is a literal or follows from the double's own rules below."""
import numpy as np
import pytest
import torch

import scores_ref as R
from helpers import synth
from test_topk_cpu import _Eng, _feats, _model
from whisper_medusa import scores as S
from whisper_medusa.api import WhisperMedusaModel

EN, DE, FR = "<|en|>", "<|de|>", "<|fr|>"
LANG_ID = {EN: 20, DE: 21, FR: 22}


def _cfg():
    cfg = R.micro_ts("base_head")
    cfg.is_multilingual = True
    cfg.lang_to_id = dict(LANG_ID)
    cfg.task_to_id = {"transcribe": 30, "translate": 31}
    cfg.alignment_heads = [[0, 0]]
    return cfg


# ---- the double's rules ---------------------------------------------------------------------------------------------------------------------
def _gen(cfg, c):
    """What a window whose features hold the value c decodes to (test_topk_cpu._Eng.decode), without prompt and EOS: two segments."""
    tb = cfg.timestamp_begin
    return [tb] + [100 + c] * (c + 1) + [tb + 10, tb + 10, 60 + c, tb + 15]


def _beam(cfg, prompt, c, rank):
    tb = cfg.timestamp_begin
    return list(prompt) + [tb] + [100 + c] * (c + 1) + [tb + 10, tb + 10, 70 + rank, tb + 15, cfg.eos_token_id], -(c + rank / 4.0)


def _lp(c, t):
    return float(np.float32(-(c + t / 100.0)))


def _ts(c, t):
    return 8.0 * c + 0.25 * t


class _RouteEng(_Eng):
    max_batch = 8

    def decode(self, gp, B, **kw):
        self.calls.append(("decode", B, tuple(gp.prompt), gp.num_beams, None if gp.sampling_keys is None else tuple(gp.sampling_keys)))
        self.prompts = [list(gp.prompt_of(b)) for b in range(B)]
        return [self.prompts[b] + _gen(self.cfg, c) + [gp.eos_token_id] for b, c in enumerate(self.clips[:B])]

    def beam_result(self, clip, rank):
        return _beam(self.cfg, self.prompts[clip], self.clips[clip], rank)

    def stats(self):
        return dict(ms_decode=1.0, ms_encode=1.0)

    def detect_language(self, lang_ids, start_token):
        self.calls.append(("detect_language", self._B))
        return [self.lang_ids[c] for c in self.clips]

    def token_timestamps(self, seqs, n_prompt, heads, width, time_precision, num_frames):
        self.calls.append(("token_timestamps", len(seqs), num_frames))
        out = np.zeros((len(seqs), max(len(s) for s in seqs)), np.float32)
        for b, s in enumerate(seqs):
            out[b, : len(s)] = [_ts(self.clips[b], t) for t in range(len(s))]
        return out, 2.0

    def gather_windows(self, feats, clip, seek, n_valid):
        self.calls.append(("gather_windows", tuple(clip), tuple(seek), tuple(n_valid)))
        win = torch.zeros(len(clip), feats.shape[1], self.cfg.n_mel_frames)
        for w, (c, s, n) in enumerate(zip(clip, seek, n_valid)):
            win[w, :, :n] = feats[c, :, s: s + n]
        return win


def _prompt(cfg, lang):
    return synth.default_prompt(cfg, lang, "transcribe", timestamps=True)


def _long(cfg, values):
    """Recordings of len(values[b]) windows; window j of recording b holds the value values[b][j]."""
    F = cfg.n_mel_frames
    f = torch.zeros(len(values), cfg.num_mel_bins, len(values[0]) * F)
    for b, row in enumerate(values):
        for j, v in enumerate(row):
            f[b, :, j * F: (j + 1) * F] = float(v)
    return f


def _trace(eng):
    return [c[:2] for c in eng.calls]


def _padded(rows, fill, dtype):
    T = max(len(r) for r in rows)
    return torch.tensor([list(r) + [fill if fill is not None else r[-1]] * (T - len(r)) for r in rows], dtype=dtype)


# ---- A. grouped detection x scoring x token timestamps --------------------------------------------------------------------------------------
def test_grouped_detection_with_scores_and_token_timestamps():
    cfg = _cfg()
    eos = cfg.eos_token_id
    eng = _RouteEng(cfg, lang_ids={3: 20, 0: 21, 1: 20}, no_speech={1: 0.95})
    m = _model(cfg, eng, 4)
    clips, langs = [3, 0, 1], [EN, DE, EN]
    out = m.generate(_feats(cfg, clips), return_timestamps=True, return_token_timestamps=True, return_token_logprobs=True,
                     no_speech_threshold=0.6, return_segments=True, num_frames=[100, 200, 300])
    assert eng.calls[0] == ("encode", 3)
    assert _trace(eng)[1:] == [("encode", 2), ("decode", 2), ("score_tokens", 2), ("token_timestamps", 2),
                               ("encode", 1), ("decode", 1), ("score_tokens", 1), ("token_timestamps", 1)]
    assert [c[2] for c in eng.calls if c[0] == "token_timestamps"] == [[100, 300], [200]]
    assert [c[2] for c in eng.calls if c[0] == "decode"] == [tuple(_prompt(cfg, EN)), tuple(_prompt(cfg, DE))]
    assert m.detected_languages == langs
    assert set(out.keys()) == {"sequences", "token_timestamps", "segments", "token_logprobs", "avg_logprob", "compression_ratio", "lengths",
                               "no_speech_prob", "skipped"}
    P = len(_prompt(cfg, EN))
    rows = [_prompt(cfg, EN) + _gen(cfg, 3) + [eos], _prompt(cfg, DE) + _gen(cfg, 0) + [eos], _prompt(cfg, EN) + [eos]]      # clip 1 is gated
    assert torch.equal(out["sequences"], _padded(rows, cfg.pad_token_id, torch.long))
    assert out["lengths"].tolist() == [len(r) for r in rows] and out["skipped"].tolist() == [False, False, True]
    assert out["no_speech_prob"].tolist() == pytest.approx([0.1, 0.1, 0.95])
    lp = [[0.0] * P + [_lp(c, t) for t in range(P, len(r))] for c, r in zip(clips, rows)]
    lp[2] = [0.0] * (P + 1)
    assert torch.equal(out["token_logprobs"], _padded(lp, 0.0, torch.float32))
    full1 = [0.0] * P + [_lp(1, t) for t in range(P, P + len(_gen(cfg, 1)) + 1)]       # the gated clip keeps the figures of what it decoded
    assert out["avg_logprob"].tolist() == pytest.approx([S.avg_logprob(lp[0], P, len(rows[0])), S.avg_logprob(lp[1], P, len(rows[1])),
                                                         S.avg_logprob(full1, P, len(full1))], abs=1e-6)
    assert out["compression_ratio"].tolist() == pytest.approx([S.compression_ratio(_gen(cfg, c) + [eos], cfg.vocab_size) for c in clips])
    tt = [[_ts(c, t) for t in range(len(r))] for c, r in zip(clips, rows)]
    assert torch.equal(out["token_timestamps"], _padded(tt, None, torch.float32))
    assert torch.equal(m.last_scores["token_logprobs"], out["token_logprobs"])
    tb = cfg.timestamp_begin
    for i, c in enumerate(clips):
        segs = out["segments"][i]
        if i == 2:
            assert len(segs) == 1 and segs[0]["tokens"].numel() == 0
            continue
        assert [sg["tokens"].tolist() for sg in segs] == [[tb] + [100 + c] * (c + 1) + [tb + 10], [tb + 10, 60 + c, tb + 15]]
        assert [(float(sg["start"]), float(sg["end"])) for sg in segs] == [pytest.approx((0.0, 0.2)), pytest.approx((0.2, 0.3))]
        o = P
        for sg in segs:
            n = int(sg["tokens"].numel())
            assert sg["token_timestamps"].tolist() == tt[i][o: o + n] and sg["token_logprobs"].tolist() == lp[i][o: o + n]
            o += n
    assert m.last_stats["ms_token_logprobs"] == 2.0 and m.last_stats["ms_token_timestamps"] == 4.0        # 1.0 / 2.0 per group, two groups


# ---- B. grouped detection x beams -----------------------------------------------------------------------------------------------------------
def test_grouped_detection_with_beams():
    cfg = _cfg()
    eng = _RouteEng(cfg, lang_ids={3: 20, 0: 21, 1: 20})
    m = _model(cfg, eng, 4)
    clips, langs = [3, 0, 1], [EN, DE, EN]
    out = m.generate(_feats(cfg, clips), return_timestamps=True, vanilla=True, num_beams=2, num_return_sequences=2, return_dict_in_generate=True)
    assert _trace(eng) == [("encode", 3), ("encode", 2), ("decode", 2), ("encode", 1), ("decode", 1)]
    assert [c[3] for c in eng.calls if c[0] == "decode"] == [2, 2]
    hyps = [_beam(cfg, _prompt(cfg, l), c, k) for c, l in zip(clips, langs) for k in range(2)]
    assert out["sequences"].shape[0] == 6
    assert torch.equal(out["sequences"], _padded([h[0] for h in hyps], cfg.pad_token_id, torch.long))
    assert out["sequences_scores"].tolist() == [-3.0, -3.25, -0.0, -0.25, -1.0, -1.25]
    assert torch.equal(m.last_sequences_scores, out["sequences_scores"])
    assert m.detected_languages == langs


# ---- C. chunk long-form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("detect", [False, True], ids=["one_language", "two_languages"])
def test_chunk_longform_with_scores_and_token_timestamps(detect):
    cfg = _cfg()
    eos, F = cfg.eos_token_id, cfg.n_mel_frames
    values = [[0, 2], [1, 3]]
    eng = _RouteEng(cfg, lang_ids={0: 21, 1: 20})
    m = _model(cfg, eng, 4)
    out = m.generate(_long(cfg, values), chunk_longform=True, return_timestamps=True, return_token_timestamps=True, return_token_logprobs=True,
                     return_segments=True, **({} if detect else {"language": "en"}))
    langs = [DE, EN] if detect else [EN, EN]
    if detect:      # one detection pass over the first windows, then one batch per language (by name): <|de|> = recording 0, <|en|> = recording 1
        assert _trace(eng) == [("encode", 2)] + [("encode", 2), ("decode", 2), ("score_tokens", 2), ("token_timestamps", 2)] * 2
        assert [c[2] for c in eng.calls if c[0] == "decode"] == [tuple(_prompt(cfg, DE)), tuple(_prompt(cfg, EN))]
    else:
        assert _trace(eng) == [("encode", 4), ("decode", 4), ("score_tokens", 4), ("token_timestamps", 4)]
    assert all(c[2] is None for c in eng.calls if c[0] == "token_timestamps")
    P = len(_prompt(cfg, EN))
    rows = [_prompt(cfg, l) + [t for v in vs for t in _gen(cfg, v)] + [eos] for l, vs in zip(langs, values)]
    assert torch.equal(out["sequences"], _padded(rows, cfg.pad_token_id, torch.long))
    assert out["lengths"].tolist() == [len(r) for r in rows]
    off = [torch.tensor(j * F * 0.01, dtype=torch.float32) for j in range(2)]
    tt, lp, wavg = [], [], []
    for vs in values:
        r_tt, r_lp, r_avg = [0.0] * P, [0.0] * P, []
        for j, v in enumerate(vs):
            n = len(_gen(cfg, v))
            r_tt += [float(torch.tensor(_ts(v, P + q), dtype=torch.float32) + off[j]) for q in range(n)]
            r_lp += [_lp(v, P + q) for q in range(n)]
            r_avg.append(S.avg_logprob([0.0] * P + [_lp(v, P + q) for q in range(n + 1)], P, P + n + 1))
        tt.append(r_tt + [r_tt[-1]])
        lp.append(r_lp + [_lp(vs[-1], P + len(_gen(cfg, vs[-1])))])         # the one EOS takes the last window's score
        wavg.append(r_avg)
    assert torch.equal(out["token_timestamps"], _padded(tt, None, torch.float32))
    assert torch.equal(out["token_logprobs"], _padded(lp, 0.0, torch.float32))
    assert out["window_avg_logprob"].shape == (2, 2) and out["window_avg_logprob"].flatten().tolist() == pytest.approx(wavg[0] + wavg[1], abs=1e-6)
    assert out["avg_logprob"].tolist() == pytest.approx([S.avg_logprob(r, P, len(r)) for r in lp], abs=1e-6)
    tb = cfg.timestamp_begin
    for b, vs in enumerate(values):
        segs = out["segments"][b]
        assert [sg["tokens"].tolist() for sg in segs] == [t for v in vs for t in ([tb] + [100 + v] * (v + 1) + [tb + 10], [tb + 10, 60 + v, tb + 15])]
        assert [float(sg["start"]) for sg in segs] == pytest.approx([0.0, 0.2, F * 0.01, F * 0.01 + 0.2])
        assert [float(sg["end"]) for sg in segs] == pytest.approx([0.2, 0.3, F * 0.01 + 0.2, F * 0.01 + 0.3])
        o = P
        for sg in segs:      # every segment carries the slice of the assembled rows that holds its own tokens
            n = int(sg["tokens"].numel())
            assert sg["token_timestamps"].tolist() == tt[b][o: o + n] and sg["token_logprobs"].tolist() == lp[b][o: o + n]
            o += n
    assert m.last_stats["ms_token_logprobs"] == (2.0 if detect else 1.0) and m.last_stats["ms_token_timestamps"] == (4.0 if detect else 2.0)


# ---- D. grouped detection x temperature ladder ----------------------------------------------------------------------------------------------
def test_grouped_detection_with_the_temperature_ladder():
    cfg = _cfg()
    eng = _RouteEng(cfg, lang_ids={3: 20, 0: 21, 1: 20})
    m = _model(cfg, eng, 4)
    clips = [3, 0, 1]
    # clips 3 and 1 (the <|en|> group) average below -1: flagged at temperature 0 and again at 0.4 (the double decodes the same ids); clip 0 passes
    out = m.generate(_feats(cfg, clips), return_timestamps=True, sampling_seed=5, temperature=(0.0, 0.4), logprob_threshold=-0.5,
                     sampling_stream_ids=[7, 8, 9], return_dict_in_generate=True)
    assert _trace(eng) == [("encode", 3), ("encode", 2), ("decode", 2), ("score_tokens", 2), ("decode", 2), ("score_tokens", 2),
                           ("encode", 1), ("decode", 1), ("score_tokens", 1)]
    assert [c[4] for c in eng.calls if c[0] == "decode"] == [None, ((1 << 32) + 7, (1 << 32) + 9), None]      # the keys of the GLOBAL stream ids
    assert out["fallback_attempts"].tolist() == [2, 1, 2] and out["fallback_temperature"].tolist() == pytest.approx([0.4, 0.0, 0.4])
    assert out["needs_fallback"].tolist() == [True, False, True]
    rows = [_prompt(cfg, l) + _gen(cfg, c) + [cfg.eos_token_id] for c, l in zip(clips, [EN, DE, EN])]
    assert torch.equal(out["sequences"], _padded(rows, cfg.pad_token_id, torch.long))
    assert m.last_stats["ms_token_logprobs"] == 3.0


# ---- E. sequential long-form x temperature ladder -------------------------------------------------------------------------------------------
def test_sequential_longform_with_the_temperature_ladder():
    cfg = _cfg()
    F = cfg.n_mel_frames
    values = [[0, 2], [1, 3]]
    eng = _RouteEng(cfg)
    m = _model(cfg, eng, 4)
    out = m.generate(_long(cfg, values), sequential_longform=True, return_timestamps=True, language="en", sampling_seed=5,
                     temperature=(0.0, 0.4), logprob_threshold=-0.5, return_dict_in_generate=True)
    key = WhisperMedusaModel.sampling_stream_key
    # round 1 (seek 0): the window holding 1 is flagged and re-encoded alone; round 2 (seek F): both windows are flagged, the batch stays resident
    assert _trace(eng) == [("gather_windows", (0, 1)), ("encode", 2), ("decode", 2), ("score_tokens", 2), ("encode", 1), ("decode", 1), ("score_tokens", 1),
                           ("gather_windows", (0, 1)), ("encode", 2), ("decode", 2), ("score_tokens", 2), ("decode", 2), ("score_tokens", 2)]
    assert [c[2] for c in eng.calls if c[0] == "gather_windows"] == [(0, 0), (F, F)]
    assert [c[4] for c in eng.calls if c[0] == "decode"] == [None, (key(1, 0, 1),), None, (key(0, F, 1), key(1, F, 1))]
    assert key(1, 0, 1) == (1 << 32) + 1 and key(0, F, 1) == ((16 * F + 1) << 32)
    rows = [_prompt(cfg, EN) + [t for v in vs for t in _gen(cfg, v)] + [cfg.eos_token_id] for vs in values]
    assert torch.equal(out["sequences"], _padded(rows, cfg.pad_token_id, torch.long))
    assert [w.tolist() for w in out["window_seek"]] == [[0, F], [0, F]]
    assert [w.tolist() for w in out["window_attempts"]] == [[1, 2], [2, 2]]
    assert [w.tolist() for w in out["window_temperature"]] == [pytest.approx([0.0, 0.4]), pytest.approx([0.4, 0.4])]
    assert m.last_stats["longform_windows"] == [2, 2] and m.last_stats["fallback_decodes"] == 2
    assert m.last_stats["ms_token_logprobs"] == 4.0
    assert [len(s) for s in out["segments"]] == [4, 4]


# ---- F. one language for all clips: the detection's encoder pass is the decode's --------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True], ids=["grouped", "group_by_language_false"])
def test_one_language_reuses_the_resident_encoder_pass(on_device):
    cfg = _cfg()
    eng = _RouteEng(cfg, lang_ids={3: 20, 0: 20, 1: 20})
    m = _model(cfg, eng, 4)
    clips = [3, 0, 1]
    out = m.generate(_feats(cfg, clips), return_timestamps=True, **({"group_by_language": False} if on_device else {}))
    assert _trace(eng) == [("encode", 3)] + ([("detect_language", 3)] if on_device else []) + [("decode", 3)]
    assert m.detected_languages == [EN] * 3
    rows = [_prompt(cfg, EN) + _gen(cfg, c) + [cfg.eos_token_id] for c in clips]
    assert isinstance(out, torch.Tensor) and torch.equal(out, _padded(rows, cfg.pad_token_id, torch.long))
    assert m._last_prompt == _prompt(cfg, EN)
