"""Host side of the token alternatives (generate(top_logprobs=k); include/wm.h wm_score_tokens_topk / wm_topk_rows) without a
GPU: the C-ABI surface, the argument handling, the packing of the three output fields with an engine double, and the reference-only guards
for the inputs of tests/test_gpu_topk.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import scores_ref as R
import topk_ref as K
from helpers import MedusaConfig, synth, ROOT
from oracle.whisper_medusa_oracle import log_mel
from whisper_medusa.api import WhisperMedusaModel

NEG = -float("inf")


# ---- C-ABI surface --------------------------------------------------------------------------------------------------------------------------
def test_abi_surface_of_the_alternatives():
    from whisper_medusa import engine
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert "#define WM_ABI_VERSION 9" in hdr and engine.WM_ABI_VERSION == 9
    assert re.search(r"#define WM_TOPK_MAX 8\b", hdr)
    for name in ("wm_score_tokens_topk", "wm_topk_rows"):
        assert name + "(" in hdr and name in engine.EXPORTS
    for path in (engine.LIB_PATH, engine.LIB_PATH_F16):
        assert os.path.exists(path), f"{path}: build the engine first"
        lib = ctypes.CDLL(path)
        assert lib.wm_abi_version() == 9
        assert hasattr(lib, "wm_score_tokens_topk") and hasattr(lib, "wm_topk_rows")
        assert hasattr(lib, "wm_score_tokens") and hasattr(lib, "wm_score_rows")
    # no struct changed: the mirrors keep their sizes and field counts
    sizes = dict(WmAlignParams=(24, 4), WmConfig=(136, 19), WmGenParams=(96, 19), WmRepeatParams=(8, 2), WmScoreParams=(8, 2), WmStats=(176, 10),
                 WmTimestampParams=(16, 4), WmWeights=(32, 4))
    for name, (size, n) in sizes.items():
        st = getattr(engine, name)
        assert (ctypes.sizeof(st), len(st._fields_)) == (size, n), name
    assert engine.WmScoreParams._fields_ == [("no_speech_token_id", ctypes.c_int32), ("sot_index", ctypes.c_int32)]
    from whisper_medusa import scores
    assert scores.TOPK_MAX == 8


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def test_top_logprobs_arguments_without_a_gpu():
    m = WhisperMedusaModel(MedusaConfig.micro(K=4), {}, device=None)
    x = torch.zeros(1, 80, 192)
    for bad in (0, 9, -1, 2.5, "3", True):
        with pytest.raises(ValueError, match=r"top_logprobs.*1\.\.8"):
            m.generate(x, top_logprobs=bad)

    class Odd:
        def __call__(self, ids, scores):
            return scores
    with pytest.raises(NotImplementedError, match="top_logprobs.*host processor path"):
        m.generate(x, top_logprobs=3, logits_processor=[Odd()])
    with pytest.raises(NotImplementedError, match="top_logprobs"):
        m.generate(x, top_logprobs=3, chunk_longform=True)
    with pytest.raises(NotImplementedError, match="top_logprobs"):
        m.generate(torch.zeros(1, 80, 1000), top_logprobs=3, chunk_longform=True)
    with pytest.raises(NotImplementedError, match="top_logprobs"):
        m.generate(x, top_logprobs=3, sequential_longform=True, return_timestamps=True)
    with pytest.raises(RuntimeError, match="HIP device"):       # a valid request needs the engine, like the other scoring arguments
        m.generate(x, top_logprobs=3)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.generate(x, top_logprobs=np.int64(8))


# ---- packing with an engine double ------------------------------------------------------------------------------------------------------
class _Eng:
    """Decodes clip c (read from the features) to prompt + <|0.00|> + (c + 1) text ids + a timestamp pair + one text id + <|t|> + EOS; scores
    it with recognisable arrays: logprob -(c + t / 100), alternatives slot j = (emitted id + j, logprob - j), rank 1 + t % 3."""

    def __init__(self, cfg, lang_ids=(), no_speech=()):
        self.cfg, self.lang_ids, self.no_speech, self.calls, self._B = cfg, dict(lang_ids), dict(no_speech), [], None
        self._enc_stamp, self._kv_stamp = object(), object()
        self.clips = []

    def encode(self, feats):
        self.calls.append(("encode", feats.shape[0])); self._B = feats.shape[0]
        self.clips = [int(v) for v in feats[:, 0, 0].tolist()]

    def forward_logits(self, tokens, pos0, disable_medusa):
        z = torch.zeros(1, len(tokens), 1, self.cfg.vocab_size)
        for b, c in enumerate(self.clips):
            z[0, b, 0, self.lang_ids[c]] = 5.0
        return z

    def decode(self, gp, B, **kw):
        tb = self.cfg.timestamp_begin
        self.calls.append(("decode", B))
        return [list(gp.prompt) + [tb] + [100 + c] * (c + 1) + [tb + 10, tb + 10, 60 + c, tb + 15, gp.eos_token_id] for c in self.clips[:B]]

    def stats(self):
        return {}

    def _lp(self, seqs, n_prompt):
        T = max(len(s) for s in seqs)
        lp = np.zeros((len(seqs), T), np.float32)
        for b, s in enumerate(seqs):
            for t in range(n_prompt, len(s)):
                lp[b, t] = -(self.clips[b] + t / 100.0)
        nsp = np.asarray([self.no_speech.get(c, 0.1) for c in self.clips[: len(seqs)]], np.float32)
        return lp, nsp

    def score_tokens(self, seqs, n_prompt, gp, no_speech_token_id=None, sot_index=0):
        self.calls.append(("score_tokens", len(seqs)))
        lp, nsp = self._lp(seqs, n_prompt)
        return lp, nsp, 1.0

    def score_tokens_topk(self, seqs, n_prompt, gp, top_k, no_speech_token_id=None, sot_index=0):
        self.calls.append(("score_tokens_topk", len(seqs), top_k))
        lp, nsp = self._lp(seqs, n_prompt)
        B, T = lp.shape
        tid = np.full((B, T, top_k), -1, np.int32); tlp = np.full((B, T, top_k), -np.inf, np.float32); rk = np.zeros((B, T), np.int32)
        for b, s in enumerate(seqs):
            for t in range(n_prompt, len(s)):
                tid[b, t] = s[t] + np.arange(top_k)
                tlp[b, t] = lp[b, t] - np.arange(top_k, dtype=np.float32)
                rk[b, t] = 1 + t % 3
        return lp, nsp, tid, tlp, rk, 1.0


def _model(cfg, eng, B):
    m = WhisperMedusaModel(cfg, {}, device=None)
    m._engine, m._max_batch = eng, B
    m.set_micro_batches(1)          # the model's own (double) engine, not a pool of real contexts
    return m


def _feats(cfg, clips):
    f = torch.zeros(len(clips), cfg.num_mel_bins, cfg.n_mel_frames)
    for i, c in enumerate(clips):
        f[i] = float(c)
    return f


def _check_rows(out, cfg, P, clips, k, skipped=()):
    seq, n = out["sequences"], out["lengths"]
    ids, lps, rk, lp = out["top_token_ids"], out["top_token_logprobs"], out["token_ranks"], out["token_logprobs"]
    B, T = seq.shape
    assert ids.shape == (B, T, k) and ids.dtype == torch.long
    assert lps.shape == (B, T, k) and lps.dtype == torch.float32
    assert rk.shape == (B, T) and rk.dtype == torch.long
    for i, c in enumerate(clips):
        L = int(n[i])
        lo = L if c in skipped else P
        assert torch.all(ids[i, :lo] == -1) and torch.all(lps[i, :lo] == NEG) and torch.all(rk[i, :lo] == 0)
        assert torch.all(ids[i, L:] == -1) and torch.all(lps[i, L:] == NEG) and torch.all(rk[i, L:] == 0)
        if c in skipped:
            assert L == P + 1 and seq[i, P] == cfg.eos_token_id
            continue
        assert L == P + 1 + (c + 1) + 5
        for t in range(P, L):
            assert float(lp[i, t]) == pytest.approx(-(c + t / 100.0), abs=1e-6)           # clip c's own row
            assert ids[i, t].tolist() == [int(seq[i, t]) + j for j in range(k)]
            assert lps[i, t].tolist() == [float(np.float32(lp[i, t]) - np.float32(j)) for j in range(k)]
            assert int(rk[i, t]) == 1 + t % 3


def test_packing_fills_segments_and_no_new_key_without_the_argument():
    cfg = R.micro_ts("base_head")
    eng = _Eng(cfg)
    m = _model(cfg, eng, 4)
    P = len(synth.default_prompt(cfg, timestamps=True))
    clips = [2, 0, 3, 1]
    out = m.generate(_feats(cfg, clips), return_timestamps=True, top_logprobs=3, return_segments=True)
    assert [c[0] for c in eng.calls] == ["encode", "decode", "score_tokens_topk"] and eng.calls[-1] == ("score_tokens_topk", 4, 3)
    _check_rows(out, cfg, P, clips, 3)
    for name in ("top_token_ids", "top_token_logprobs", "token_ranks"):
        assert torch.equal(m.last_scores[name], out[name])
    for i in range(4):
        o = P
        assert len(out["segments"][i]) == 2
        for sg in out["segments"][i]:
            n = int(sg["tokens"].numel())
            assert torch.equal(sg["token_logprobs"], out["token_logprobs"][i, o: o + n])
            assert torch.equal(sg["top_token_ids"], out["top_token_ids"][i, o: o + n]) and sg["top_token_ids"].shape == (n, 3)
            assert torch.equal(sg["top_token_logprobs"], out["top_token_logprobs"][i, o: o + n])
            assert torch.equal(sg["token_ranks"], out["token_ranks"][i, o: o + n])
            o += n
    # top_logprobs alone implies the dict output, as return_token_logprobs does
    alone = m.generate(_feats(cfg, clips), return_timestamps=True, top_logprobs=1)
    assert isinstance(alone, dict) and alone["top_token_ids"].shape[-1] == 1 and "avg_logprob" in alone
    # without the argument: the old method, no new key
    eng.calls.clear()
    plain = m.generate(_feats(cfg, clips), return_timestamps=True, return_token_logprobs=True, return_segments=True)
    assert [c[0] for c in eng.calls] == ["encode", "decode", "score_tokens"]
    assert not any(k in plain for k in ("top_token_ids", "top_token_logprobs", "token_ranks"))
    assert not any(k in sg for sg in plain["segments"][0] for k in ("top_token_ids", "top_token_logprobs", "token_ranks"))
    assert torch.equal(plain["token_logprobs"], out["token_logprobs"]) and torch.equal(plain["sequences"], out["sequences"])
    eng.calls.clear()
    ids = m.generate(_feats(cfg, clips), return_timestamps=True)
    assert isinstance(ids, torch.Tensor) and [c[0] for c in eng.calls] == ["encode", "decode"]


def test_language_groups_return_the_alternatives_in_clip_order():
    cfg = R.micro_ts("base_head")
    cfg.is_multilingual = True
    cfg.lang_to_id = {"<|en|>": 20, "<|de|>": 21, "<|fr|>": 22}
    cfg.task_to_id = {"transcribe": 30, "translate": 31}
    eng = _Eng(cfg, lang_ids={0: 21, 1: 20, 2: 21, 3: 20})
    m = _model(cfg, eng, 4)
    clips = [3, 0, 1]              # groups: <|en|> = clips 3 and 1 (lengths differ), <|de|> = clip 0
    out = m.generate(_feats(cfg, clips), return_timestamps=True, top_logprobs=4)
    assert m.detected_languages == ["<|en|>", "<|de|>", "<|en|>"]
    assert [c for c in eng.calls if c[0].startswith("score")] == [("score_tokens_topk", 2, 4), ("score_tokens_topk", 1, 4)]
    _check_rows(out, cfg, len(m._last_prompt), clips, 4)


def test_a_gated_stream_holds_fills_only():
    cfg = R.micro_ts("base_head")
    eng = _Eng(cfg, no_speech={1: 0.95})
    m = _model(cfg, eng, 4)
    P = len(synth.default_prompt(cfg, timestamps=True))
    clips = [0, 1, 2, 3]
    out = m.generate(_feats(cfg, clips), return_timestamps=True, top_logprobs=2, no_speech_threshold=0.6, logprob_threshold=None)
    assert out["skipped"].tolist() == [False, True, False, False]
    _check_rows(out, cfg, P, clips, 2, skipped=(1,))


def test_sharded_ranks_forward_the_alternatives(monkeypatch):
    """generate_sharded over two ranks (torch.distributed stubbed: rank 1 runs first and leaves what it would have sent, then rank 0 gathers
    it): the three fields travel like the other score fields and come back in stream order, padded with the fills."""
    import torch.distributed as td
    cfg = R.micro_ts("base_head")
    P = len(synth.default_prompt(cfg, timestamps=True))
    clips = [2, 0, 3, 1]
    sent, state = [], dict(rank=1, n=0)

    def all_gather_object(parts, obj):
        if state["rank"] == 1:
            sent.append(obj); parts[0], parts[1] = [], obj
        else:
            parts[0], parts[1] = obj, sent[state["n"]]
        state["n"] += 1
    monkeypatch.setattr(td, "is_available", lambda: True)
    monkeypatch.setattr(td, "is_initialized", lambda: True)
    monkeypatch.setattr(td, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(td, "get_rank", lambda *a: state["rank"])
    monkeypatch.setattr(td, "all_gather_object", all_gather_object)
    out = None
    for rank in (1, 0):
        state.update(rank=rank, n=0)
        eng = _Eng(cfg)
        m = _model(cfg, eng, 4)
        out = m.generate_sharded(_feats(cfg, clips), return_timestamps=True, top_logprobs=3)
        assert eng.calls[-1] == ("score_tokens_topk", 2, 3)
    _check_rows(out, cfg, P, clips, 3)
    assert torch.equal(m.last_scores["top_token_ids"], out["top_token_ids"])


# ---- reference-only guards for the inputs of tests/test_gpu_topk.py ---------------------------------------------------------------------
def test_crafted_rows_have_clear_gaps_and_short_rows():
    """Adjacent gaps among the reference's top 9 of every crafted row, in every parameter set, are >= 1e-4 (200 x fp32 rounding at |x| < 8,
    below TIE): the ids of the GPU test are settled.  Rows that keep fewer than 8 finite entries occur (the fills are exercised)."""
    import test_gpu_scores as G
    assert K.GAP_KERNEL < G.TIE
    cfg = R.micro_ts("base_head")
    kept = set()
    gmin = float("inf")
    labels = []
    for label, gp, rows, pre, tgt, xs in K.crafted_reference(cfg):
        labels.append(label)
        for r, x in enumerate(xs):
            gaps = K.top_gaps(x, 9)
            n_fin = int(torch.isfinite(x).sum())
            kept.add(n_fin)
            assert n_fin >= 1, (label, r)
            if gaps:
                gmin = min(gmin, min(gaps))
                assert min(gaps) >= K.GAP_KERNEL, (label, r, min(gaps))
    print(f"crafted rows: sets {labels}, smallest gap among the top 9 {gmin:.3g}, finite entries per row (fewest) {sorted(kept)[:6]}")
    assert labels == ["ts", "ts+processors", "plain", "mit=1", "rules off"]
    assert 2 in kept and any(2 < n < 8 for n in kept), sorted(kept)[:8]


@pytest.mark.parametrize("ht", ["base_head", "medusa_block"])
def test_end_to_end_inputs_are_decisive_and_hold_a_rank_above_one(ht):
    """The end-to-end runs of tests/test_gpu_topk.py (micro timestamp rig, 4 clips, 40 new tokens), decoded by the oracle: at least 0.4 of
    the scored rows have gaps above 2 * MAX_D among the reference's top 3 — the exact check of the GPU test cannot go empty — and at least
    one emitted token is not the row's best (typical acceptance)."""
    from test_gpu_timestamps import Ref
    import test_gpu_scores as G
    cfg = R.micro_ts(ht)
    ref = Ref(cfg, R.ts_state_dict(cfg, G.SEEDS[ht]))
    m = WhisperMedusaModel(cfg, {}, device=None)
    gp = m._gen_params(None, None, G.EXP_DECAY, 40, None, None, False, None, None, None, None, None, timestamps=True)
    P, n = len(gp.prompt), cfg.n_mel_frames * 160
    total = dec = 0
    ranks = []
    for c in G.clips(cfg, 4):
        enc = ref.orc.encode(torch.from_numpy(log_mel(c, cfg.num_mel_bins, n)))
        ids, _, _ = ref.decode(enc, gp)
        ids = G._own(ids, P, gp.eos_token_id)
        for t, (x, _) in K.reference_rows(ref.orc, enc, ids, P, gp, cfg).items():
            total += 1
            dec += K.decisive(x, 2, 2 * G.MAX_D)
            ranks.append(K.rank_of(x.numpy(), ids[t]))
    print(f"guard[{ht}]: {dec} of {total} scored rows decisive at depth 2; ranks above 1: {sorted(r for r in ranks if r > 1)}")
    assert total > 0 and dec >= K.DECISIVE_SHARE * total, (dec, total)
    assert all(r >= 1 for r in ranks) and any(r > 1 for r in ranks)
