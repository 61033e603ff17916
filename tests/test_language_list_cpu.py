"""generate(language=[...]) and generate(language=None, group_by_language=False) on the host: how the list lowers to per-stream
prompt rows of one length, the call patterns against a recording engine (in the style of tests/test_host.py::_FakeEngine), HF's own errors, the
refusals by name, the sub-batches of the temperature ladder and of the micro-batch pool, the three new C-ABI entries, and — from the references of
tests/lang_ref.py alone — that the restated pick rule is HF's mask + argmax on the tap cases, ties included."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import lang_ref as L
from helpers import ROOT
from whisper_medusa import WhisperMedusaModel, engine


class _Eng:
    """Records the calls generate() makes.  Detection (host path and the engine's own entry) puts clip b on `lang_ids[b]`."""

    def __init__(self, cfg, lang_ids, max_batch=4):
        self.cfg, self.lang_ids, self.calls, self._B, self.max_batch = cfg, list(lang_ids), [], None, max_batch
        self._enc_stamp, self._kv_stamp = object(), object()
        self.low = set()            # language ids whose streams score badly on a greedy attempt (the ladder test)

    def encode(self, feats):
        self.calls.append(("encode", feats.shape[0])); self._B = feats.shape[0]

    def forward_logits(self, tokens, pos0, disable_medusa):
        self.calls.append(("forward_logits", len(tokens)))
        z = torch.zeros(1, len(tokens), 1, self.cfg.vocab_size)
        for b, t in enumerate(self.lang_ids[: len(tokens)]):
            z[0, b, 0, t] = 5.0
        return z

    def detect_language(self, lang_ids, start_token):
        assert start_token == self.cfg.decoder_start_token_id and sorted(lang_ids) == sorted(self.cfg.lang_to_id.values())
        self.calls.append(("detect_language", self._B))
        return list(self.lang_ids[: self._B])

    def decode(self, gp, B, **kw):
        rows = [list(gp.prompt_of(b)) for b in range(B)]
        self.calls.append(("decode", B, rows, gp))
        return [rows[b] + [7, gp.eos_token_id] for b in range(B)]

    def score_tokens(self, seqs, n_prompt, gp, ns_id, sot):
        self.calls.append(("score", len(seqs)))
        lp = np.zeros((len(seqs), max(len(s) for s in seqs)), dtype=np.float32)
        for b, s in enumerate(seqs):
            if gp.sampling_temperature == 0.0 and s[1] in self.low:
                lp[b, n_prompt:] = -5.0
        return lp, None, 0.0

    def stats(self):
        return {"ms_decode": 0.0, "ms_encode": 0.0, "ms_logmel": 0.0, "iterations": 1, "accept_hist": [0] * 5}


def _model(lang_ids=(), B=4):
    cfg = L.mix_cfg()
    m = WhisperMedusaModel(cfg, {})
    m._max_batch = B
    m._engine = eng = _Eng(cfg, lang_ids, B)
    return cfg, m, eng, torch.zeros(B, cfg.num_mel_bins, cfg.n_mel_frames)


def _decodes(eng):
    return [c for c in eng.calls if c[0] == "decode"]


def _hf_rows(cfg, language, B, timestamps=False):
    """HF's own WhisperGenerationMixin._retrieve_init_tokens on this configuration."""
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as W
    gc = NS(task="transcribe", language=language, decoder_start_token_id=cfg.decoder_start_token_id, lang_to_id=cfg.lang_to_id,
            task_to_id=cfg.task_to_id, is_multilingual=True, no_timestamps_token_id=cfg.no_timestamps_token_id, return_timestamps=timestamps)
    return W._retrieve_init_tokens(NS(device="cpu"), None, B, gc, NS(), 3000, {})


@pytest.mark.parametrize("ts", [False, True])
@pytest.mark.parametrize("pid", [None, [932, 11, 12]])
def test_a_list_lowers_to_prompt_rows_of_one_length(ts, pid):
    cfg, m, eng, feats = _model()
    names = ["de", "english", "<|de|>", "fr"]
    out = m.generate(feats, language=names, return_timestamps=ts, prompt_ids=None if pid is None else torch.tensor(pid), max_new_tokens=8)
    assert [c[:2] for c in eng.calls] == [("encode", 4), ("decode", 4)]                 # ONE encode, ONE decode
    rows, gp = eng.calls[1][2], eng.calls[1][3]
    toks = ["<|de|>", "<|en|>", "<|de|>", "<|fr|>"]
    want = L.init_token_rows(cfg, toks, timestamps=ts, prompt_ids=pid)
    assert rows == want and len({len(r) for r in rows}) == 1
    assert want == [(pid or []) + r for r in _hf_rows(cfg, ["de", "en", "de", "fr"], 4, ts).tolist()]        # the restated rows are HF's
    slot = len(pid or []) + 1
    assert [r[slot] for r in rows] == [cfg.lang_to_id[t] for t in toks]
    assert gp.prompt == rows[0] and gp.prompts == rows                                  # the representative is stream 0's row
    assert gp.begin_index == len(rows[0]) - len(pid or []) and gp.max_length == len(rows[0]) + 8
    for b in range(4):                                                                  # row b of the result carries clip b's language token
        assert out[b, : len(rows[b])].tolist() == rows[b]
    assert m._last_prompt == rows[0]


def test_equal_entries_give_the_scalar_call():
    cfg, m, eng, feats = _model()
    m.generate(feats, language=["de"] * 4, max_new_tokens=8)
    m.generate(feats, language="de", max_new_tokens=8)
    a, b = _decodes(eng)
    assert a[3] == b[3] and a[3].prompts is None and a[2] == b[2]                       # the same parameters, no table
    assert [c[0] for c in eng.calls] == ["encode", "decode"] * 2


def test_hf_errors():
    cfg, m, eng, feats = _model()
    for bad, B, exc in ((["de", None, "en", "fr"], 4, TypeError), (["de", "en"], 4, ValueError), (("de", "en", "fr", "de", "en"), 4, ValueError)):
        with pytest.raises(exc) as hf:
            _hf_rows(cfg, list(bad), B)
        with pytest.raises(exc) as own:
            m.generate(feats, language=bad)
        assert str(own.value) == str(hf.value)                                          # HF's own message
    for bad in (["de", "xx", "en", "fr"], ["de", "en", "fr", "klingon"], ["<|it|>", "en", "en", "en"]):
        with pytest.raises(ValueError, match="Unsupported language: " + re.escape([l for l in bad if l not in ("de", "en", "fr")][0])):
            m.generate(feats, language=bad)
    assert eng.calls == []


def test_the_list_is_ignored_without_a_language_slot():
    cfg, m, eng, feats = _model()
    cfg.is_multilingual = False
    m.generate(feats, language=["de", "en", "de", "fr"], max_new_tokens=4)
    m.generate(feats, language="de", max_new_tokens=4)
    a, b = _decodes(eng)
    assert a[3] == b[3] and a[3].prompts is None
    with pytest.raises(ValueError, match="must match the batch size"):
        m.generate(feats, language=["de"])


def test_refusals_by_name():
    from transformers import LogitsProcessor, StoppingCriteria

    class Proc(LogitsProcessor):
        def __call__(self, ids, scores):
            return scores

    class Crit(StoppingCriteria):
        def __call__(self, ids, scores, **kw):
            return False

    cfg, m, eng, feats = _model(B=1)
    streamer = NS(put=lambda *_: None, end=lambda: None)
    with pytest.raises(NotImplementedError, match=r"language=\[\.\.\.\].*streamer="):
        m.generate(feats, language=["de"], streamer=streamer)
    cfg, m, eng, feats = _model()
    with pytest.raises(NotImplementedError, match=r"language=\[\.\.\.\].*host processor path"):
        m.generate(feats, language=["de", "en", "de", "fr"], logits_processor=[Proc()])
    with pytest.raises(NotImplementedError, match=r"language=\[\.\.\.\].*host processor path"):
        m.generate(feats, language=["de", "en", "de", "fr"], stopping_criteria=[Crit()])
    assert _decodes(eng) == []
    # the same two with the detected list
    eng.lang_ids = [63, 60, 63, 748]
    with pytest.raises(NotImplementedError, match="group_by_language=False.*host processor path"):
        m.generate(feats, group_by_language=False, logits_processor=[Proc()])


def test_group_by_language_false_is_encode_detect_decode():
    ids = [63, 60, 63, 748]
    cfg, m, eng, feats = _model(ids)
    out = m.generate(feats, group_by_language=False, max_new_tokens=8)
    assert [c[:2] for c in eng.calls] == [("encode", 4), ("detect_language", 4), ("decode", 4)]
    assert m.detected_languages == ["<|de|>", "<|en|>", "<|de|>", "<|fr|>"]
    assert eng.calls[2][2] == L.init_token_rows(cfg, m.detected_languages) and out[:, 1].tolist() == ids
    # one language: still one encode, one decode, and the scalar call's parameters
    cfg, m, eng, feats = _model([63] * 4)
    m.generate(feats, group_by_language=False, max_new_tokens=8)
    assert [c[:2] for c in eng.calls] == [("encode", 4), ("detect_language", 4), ("decode", 4)] and eng.calls[2][3].prompts is None
    m.generate(feats, language="de", max_new_tokens=8)
    assert _decodes(eng)[0][3] == _decodes(eng)[1][3]


def test_the_default_keeps_the_grouped_pattern():
    cfg, m, eng, feats = _model([63, 60, 63, 60])
    for kw in ({}, {"group_by_language": True}):
        eng.calls.clear()
        m.generate(feats, **kw)
        assert [c[:2] for c in eng.calls] == [("encode", 4), ("forward_logits", 4), ("encode", 2), ("decode", 2), ("encode", 2), ("decode", 2)]
        assert all(c[3].prompts is None for c in _decodes(eng))
    # the public detect_language() keeps its host path
    eng.calls.clear()
    assert m.detect_language(feats) == ["<|de|>", "<|en|>", "<|de|>", "<|en|>"] and [c[0] for c in eng.calls] == ["encode", "forward_logits"]


def test_the_ladders_sub_batches_keep_their_streams_prompts():
    cfg, m, eng, feats = _model()
    eng.low = {cfg.lang_to_id["<|en|>"], cfg.lang_to_id["<|fr|>"]}          # streams 1 and 3 fail the first attempt
    names = ["de", "en", "de", "fr"]
    m.generate(feats, language=names, vanilla=True, sampling_seed=5, temperature=(0.0, 0.4), logprob_threshold=-1.0, max_new_tokens=8)
    rows = L.init_token_rows(cfg, ["<|de|>", "<|en|>", "<|de|>", "<|fr|>"])
    first, second = _decodes(eng)
    assert first[1] == 4 and first[2] == rows
    assert second[1] == 2 and second[2] == [rows[1], rows[3]] and second[3].prompt == rows[1]
    assert second[3].sampling_temperature == pytest.approx(0.4) and len(second[3].sampling_keys) == 2
    assert [c[:2] for c in eng.calls if c[0] == "encode"] == [("encode", 4), ("encode", 2)]


def test_the_pools_contexts_get_their_streams_rows(monkeypatch):
    import whisper_medusa.pool as pool_mod
    seen = []

    class Ctx(_Eng):
        def __init__(self, cfg, *a, **kw):
            super().__init__(cfg, [])
            self.device = torch.device("cpu")

        def decode(self, gp, B, **kw):
            seen.append((B, [list(gp.prompt_of(b)) for b in range(B)], gp.prompt))
            return super().decode(gp, B)

        def close(self):
            pass

    monkeypatch.setattr(pool_mod, "Engine", Ctx)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    cfg, m, eng, feats = _model()
    m._blob, m._offsets = torch.zeros(1), None
    m.set_micro_batches(2)
    out = m.generate(feats, language=["de", "en", "fr", "en"], max_new_tokens=8)
    rows = L.init_token_rows(cfg, ["<|de|>", "<|en|>", "<|fr|>", "<|en|>"])
    assert sorted(seen) == sorted([(2, rows[:2], rows[0]), (2, rows[2:], rows[2])])
    assert [out[b, : len(rows[b])].tolist() for b in range(4)] == rows


def test_generate_sharded_splits_the_list_with_the_clips(monkeypatch):
    import torch.distributed as td
    import whisper_medusa.dist as dist_mod
    cfg, m, eng, feats = _model()
    monkeypatch.setattr(td, "is_available", lambda: True)
    monkeypatch.setattr(td, "is_initialized", lambda: True)
    monkeypatch.setattr(td, "get_world_size", lambda: 2)
    monkeypatch.setattr(td, "get_rank", lambda: 1)
    monkeypatch.setattr(dist_mod, "gather_token_lists", lambda local: [s for _, s in sorted(local)])
    mine = dist_mod.shard_streams(4, 1, 2)
    names = ["de", "en", "fr", "en"]
    m.generate_sharded(feats, language=names, max_new_tokens=8)
    rows = L.init_token_rows(cfg, ["<|de|>", "<|en|>", "<|fr|>", "<|en|>"])
    assert _decodes(eng)[0][2] == [rows[s] for s in mine] and len(mine) == 2
    with pytest.raises(ValueError, match="must match the batch size"):
        m.generate_sharded(feats, language=names[:2])


def test_long_form_takes_the_list_as_one_language_per_recording():
    cfg, m, eng, _ = _model(B=2)
    F = cfg.n_mel_frames
    long = torch.zeros(2, cfg.num_mel_bins, 2 * F)
    m.generate(long, language=["de", "en"], chunk_longform=True, max_new_tokens=8)
    decs = _decodes(eng)
    assert [(c[1], c[2][0][1]) for c in decs] == [(2, cfg.lang_to_id["<|de|>"]), (2, cfg.lang_to_id["<|en|>"])]      # per-language groups, as before
    assert all(c[3].prompts is None for c in decs)


def test_the_c_abi_declares_and_exports_the_entries():
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert re.search(r"int wm_set_stream_prompts\(wm_ctx\* ctx, const int32_t\* prompts[^;]*int B, int P\);", hdr)
    assert re.search(r"int wm_detect_language\(wm_ctx\* ctx, int B, const int32_t\* lang_ids[^;]*int n, int32_t start_token, int32_t\* out[^;]*float\* ms[^;]*\);", hdr)
    assert re.search(r"int wm_lang_pick_rows\(wm_ctx\* ctx, int R, const float\* logits[^;]*const int32_t\* lang_ids[^;]*int n,\s*int32_t\* out[^;]*\);", hdr)
    assert "#define WM_ABI_VERSION 9" in hdr and "#define WM_LANG_MAX 256" in hdr and engine.LANG_MAX == 256
    for name in ("wm_set_stream_prompts", "wm_detect_language", "wm_lang_pick_rows"):
        assert name in engine.EXPORTS
    if os.path.exists(engine.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(engine.LIB_PATH)
        assert all(hasattr(lib, n) for n in ("wm_set_stream_prompts", "wm_detect_language", "wm_lang_pick_rows")) and lib.wm_abi_version() == 9


@pytest.mark.parametrize("V", L.TAP_V)
@pytest.mark.parametrize("n", L.TAP_N)
def test_the_restated_pick_is_hfs_mask_and_argmax(V, n):
    ids = L.tap_lang_ids(V, n)
    assert ids != sorted(ids) or n == 1
    rows = L.tap_rows(V, 33, ids)
    want = L.hf_pick(rows, ids)
    assert np.array_equal(L.pick_restated(rows, ids), want)
    assert np.array_equal(L.pick_restated(rows, ids[::-1]), want) and np.array_equal(L.hf_pick(rows, sorted(ids)), want)      # no order of the list
    assert set(want.tolist()) <= set(ids) and (rows.max(axis=1) > rows[np.arange(33), want]).all()       # the larger non-candidate is ignored
    if n > 1:
        # the cases hold what they say: ties whose smallest id wins, candidates at -inf
        tied = [r for r in range(33) if (rows[r, ids] == rows[r, want[r]]).sum() > 1]
        assert tied and all(want[r] == min(t for t in ids if rows[r, t] == rows[r, want[r]]) for r in tied)
        assert np.isinf(rows[:, ids]).any()
    if n > 64:
        pos = {t: i for i, t in enumerate(ids)}
        assert any(len({pos[t] // 64 for t in ids if rows[r, t] == rows[r, want[r]]}) > 1 for r in tied)        # a tie across waves
