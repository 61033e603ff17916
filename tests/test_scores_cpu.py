"""Host side of the token log-probabilities (whisper_medusa/scores.py, the long-form assembly of api.py, the C-ABI surface) without a GPU, and
the reference-only guard for the inputs of tests/test_gpu_scores.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scores_ref as R
from helpers import MedusaConfig, synth, clip_for, ROOT
from oracle.whisper_medusa_oracle import Oracle, log_mel
from whisper_medusa import scores as S
from whisper_medusa.api import WhisperMedusaModel, ResolvedCall, ShortResult
from whisper_medusa.config import GenParams


# ---- scores.py against transformers' static methods ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ends_in_eos", "no_eos", "pad_is_eos"])
def test_avg_logprob_and_compression_ratio_equal_hf(case):
    rng = np.random.default_rng(3)
    V, eos = 1031, 1000
    for n in (1, 2, 7, 33):
        toks = [int(t) for t in rng.integers(0, V, n)]
        if case in ("ends_in_eos", "pad_is_eos"):
            toks[-1] = eos
        rows = [torch.from_numpy(rng.standard_normal(V).astype(np.float32) * 3) for _ in range(n)]
        for r in rows[::2]:
            r[rng.integers(0, V, 20)] = -float("inf")
        for i, t in enumerate(toks):
            rows[i][t] = min(abs(float(rows[i][t])), 9.0)   # the chosen id is never masked
        want = R.hf_avg_logprob(rows, toks)
        P = 3
        lp = [0.0] * P + [float(torch.log_softmax(rows[i].float(), -1)[toks[i]]) for i in range(n)]
        tail = [0.0] * 4 if case == "pad_is_eos" else []    # positions after the stream's end (pad == eos rows) do not count
        assert S.avg_logprob(lp + tail, P, P + n) == want
        assert S.compression_ratio(toks, V) == R.hf_compression_ratio(toks, V)
    rep = [5, 6, 7] * 40
    assert S.compression_ratio(rep, 51865) == R.hf_compression_ratio(rep, 51865) > 2.4
    assert S.avg_logprob([0.0, 0.0], 2, 2) == 0.0 and S.compression_ratio([], V) == 0.0


GATE_TABLE = [
    # no_speech_prob, avg_logprob, no_speech_thr, logprob_thr, compression_thr, ratio -> (needs_fallback, skip)
    (0.9, -2.0, 0.6, -1.0, None, 1.0, (False, True)),
    (0.9, -0.5, 0.6, -1.0, None, 1.0, (False, False)),
    (0.5, -2.0, 0.6, -1.0, None, 1.0, (True, False)),
    (0.9, -0.5, 0.6, None, None, 1.0, (False, True)),       # logprob_threshold=None: the no-speech probability alone decides
    (0.6, -2.0, 0.6, None, None, 1.0, (False, False)),      # strictly greater
    (0.9, -2.0, None, -1.0, None, 1.0, (True, False)),
    (None, -2.0, 0.6, -1.0, None, 1.0, (True, False)),
    (0.1, -0.5, 0.6, -1.0, 2.4, 3.0, (True, False)),
    (0.1, -0.5, 0.6, -1.0, 2.4, 2.4, (False, False)),
    (0.9, -2.0, 0.6, -1.0, 2.4, 3.0, (False, True)),        # HF: a skipped clip needs no fallback
    (0.1, -0.5, None, None, None, 9.0, (False, False)),
]


@pytest.mark.parametrize("row", GATE_TABLE)
def test_gating_rule(row):
    ns, avg, nst, lpt, crt, ratio, want = row
    assert S.gate(ns, avg, ratio, nst, lpt, crt) == want


# ---- long-form assembly with a stubbed inner generate ---------------------------------------------------------------------------------------
def test_longform_skipped_window_leaves_nothing():
    cfg = R.micro_ts("base_head")
    m = WhisperMedusaModel(cfg, {}, device=None)
    m.device = torch.device("cpu")
    tb, eos = cfg.timestamp_begin, cfg.eos_token_id
    prompt = synth.default_prompt(cfg, timestamps=True)
    P = len(prompt)
    wins = [prompt + [tb, 11, 12, tb + 10, eos], prompt + [tb, 21, tb + 5, eos, eos], prompt + [tb + 1, 31, 32, tb + 20, eos]]
    lps = [[0.0] * P + [-0.1 * (i + 1)] * (len(w) - P) for i, w in enumerate(wins)]

    def stub(skip):
        def inner(feats, call, language=None, **kw):
            assert feats.shape[0] == 3 and call.sc_req is req and language == "en"
            rows = [list(w) for w in wins]
            lp = [list(x) for x in lps]
            for j in skip:
                rows[j] = prompt + [eos]; lp[j] = [0.0] * (P + 1)
            T = max(len(r) for r in rows)
            sc = dict(token_logprobs=torch.tensor([x + [0.0] * (T - len(x)) for x in lp]), avg_logprob=torch.tensor([-0.1, -0.2, -0.3]),
                      compression_ratio=torch.ones(3), no_speech_prob=torch.tensor([0.1, 0.9, 0.1]),
                      skipped=torch.tensor([j in skip for j in range(3)]), _want=True)
            return ShortResult(rows, GenParams(prompt=list(prompt), eos_token_id=eos, pad_token_id=cfg.pad_token_id),
                               {"ms_token_logprobs": 1.0}, scores=sc)
        return inner

    F = cfg.n_mel_frames
    feats = torch.zeros(1, cfg.num_mel_bins, 3 * F)
    req = dict(want=True, no_speech_threshold=0.6, logprob_threshold=None, compression_ratio_threshold=None)
    outs = {}
    for name, skip in (("all", ()), ("mid", (1,))):
        m._generate_short = stub(skip)
        outs[name] = m._generate_longform(feats, ResolvedCall(sc_req=req, return_timestamps=True, return_segments=True), "en", False)
    full, mid = outs["all"], outs["mid"]
    gen = lambda w: [t for t in w[P:] if t != eos]      # noqa: E731
    assert full["sequences"][0].tolist() == prompt + gen(wins[0]) + gen(wins[1]) + gen(wins[2]) + [eos]
    assert mid["sequences"][0].tolist() == prompt + gen(wins[0]) + gen(wins[2]) + [eos]
    assert mid["skipped"].tolist() == [[False, True, False]]
    # the kept windows' segments are those of the ungated run: same tokens, same offsets (window 2 still starts at 2 windows)
    kept = [s for s in full["segments"][0] if not (F * 0.01 <= float(s["start"]) < 2 * F * 0.01)]
    assert len(mid["segments"][0]) == len(kept) == len(full["segments"][0]) - 1
    for a, b in zip(mid["segments"][0], kept):
        assert torch.equal(a["start"], b["start"]) and torch.equal(a["end"], b["end"]) and torch.equal(a["tokens"], b["tokens"])
        assert torch.equal(a["token_logprobs"], b["token_logprobs"])
    assert float(mid["segments"][0][-1]["start"]) >= 2 * F * 0.01
    n0, n2 = len(gen(wins[0])), len(gen(wins[2]))
    assert torch.allclose(mid["token_logprobs"][0, P: P + n0 + n2], torch.tensor([-0.1] * n0 + [-0.3] * n2))


# ---- C-ABI surface --------------------------------------------------------------------------------------------------------------------------
def test_abi_surface():
    from whisper_medusa import engine
    assert engine.WM_ABI_VERSION == 9
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert "#define WM_ABI_VERSION 9" in hdr and "wm_score_tokens(" in hdr and "wm_score_rows(" in hdr and "wm_score_params" in hdr
    for path in (engine.LIB_PATH, engine.LIB_PATH_F16):
        assert os.path.exists(path), f"{path}: build the engine first"
        lib = ctypes.CDLL(path)
        assert lib.wm_abi_version() == 9
        assert hasattr(lib, "wm_score_tokens") and hasattr(lib, "wm_score_rows")
    assert "wm_score_tokens" in engine.EXPORTS and "wm_score_rows" in engine.EXPORTS


def test_generate_arguments_without_a_gpu():
    m = WhisperMedusaModel(MedusaConfig.micro(K=4), {}, device=None)
    x = torch.zeros(1, 80, 192)

    class Odd:
        def __call__(self, ids, scores):
            return scores
    with pytest.raises(NotImplementedError, match="host processor path"):
        m.generate(x, return_token_logprobs=True, logits_processor=[Odd()])
    with pytest.raises(NotImplementedError, match="HIP engine's scoring pass"):      # off the device nothing can score the clip: the reference's refusal stays
        m.generate(x, no_speech_threshold=0.6)
    with pytest.raises(RuntimeError, match="HIP device"):       # the other scoring arguments are accepted and need the engine
        m.generate(x, logprob_threshold=-1.0)


# ---- reference-only guard for the inputs of the GPU test --------------------------------------------------------------------------------
MARGIN, CAP = 0.12, 0.10


@pytest.mark.parametrize("temperature", [None, 0.0])
@pytest.mark.parametrize("ht", ["base_head", "medusa_block"])
def test_gpu_inputs_stay_clear_of_the_timestamp_decision(ht, temperature):
    """The timestamp runs of test_gpu_scores.py::test_generate_token_logprobs (same configs, seeds, clips), decoded by the oracle: the share of
    scored rows whose decision margin |logsumexp(ts) - max(text)| is below the exclusion margin stays within the cap."""
    from test_gpu_timestamps import Ref
    import test_gpu_scores as G
    cfg = R.micro_ts(ht)
    sd = R.ts_state_dict(cfg, G.SEEDS[ht])
    ref = Ref(cfg, sd)
    m = WhisperMedusaModel(cfg, {}, device=None)
    gp = m._gen_params(None, None, G.EXP_DECAY, 40, None, temperature, False, None, None, None, None, None, timestamps=True)
    P = len(gp.prompt)
    n = cfg.n_mel_frames * 160
    below = total = 0
    lens = []
    for c in G.clips(cfg, 12):
        enc = ref.orc.encode(torch.from_numpy(log_mel(c, cfg.num_mel_bins, n)))
        ids, _, _ = ref.decode(enc, gp)
        ids = G._own(ids, P, gp.eos_token_id)
        lens.append(len(ids))
        s = R.reference_scores(ref.orc, enc, ids, P, gp, cfg)
        below += sum(1 for t in range(P, len(ids)) if s["margins"][t] < MARGIN)
        total += len(ids) - P
    print(f"guard[{ht}, T={temperature}]: {below} of {total} rows below {MARGIN}; lens {lens}")
    assert total > 0 and below <= CAP * total, (below, total)
    assert len(set(lens)) > 1


def test_crafted_rows_stay_clear_of_the_decision():
    import test_gpu_scores as G
    cfg = R.micro_ts("base_head")
    rows, pre, tgt = G.crafted_rows(cfg)
    gp = G._gp(cfg, True)
    proc = R.hf_processor(cfg, gp.begin_index)
    n_inf = 0
    for r in range(len(rows)):
        lp, margin = R.row_logprob(torch.from_numpy(rows[r]), pre[r], tgt[r], gp, proc)
        assert margin >= G.TIE, (r, margin)
        n_inf += lp == -float("inf")
    assert 0 < n_inf < len(rows)


SEEN_GATES = set()


# ---- the gating rule against transformers' own _need_fallback -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nst", [None, 0.6])
@pytest.mark.parametrize("crt", [None, 1.5])
@pytest.mark.parametrize("lpt", [-1.0, -6.0, -9.0])
def test_gate_equals_hf_need_fallback(lpt, crt, nst):
    """HF WhisperGenerationMixin._need_fallback driven with stubbed seek outputs (its logprob_threshold must be set: without one HF's
    no-speech branch is undefined) against scores.gate on the figures scores.py derives from the same scores and tokens."""
    import types
    from transformers.generation.logits_process import WhisperNoSpeechDetection
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as W
    rng = np.random.default_rng(11)
    V = 1031
    stub = types.SimpleNamespace(_retrieve_compression_ratio=W._retrieve_compression_ratio, _retrieve_avg_logprobs=W._retrieve_avg_logprobs)
    gc = types.SimpleNamespace(compression_ratio_threshold=crt, logprob_threshold=lpt, no_speech_threshold=nst)
    seen = set()
    for case in range(24):
        n = int(rng.integers(2, 30))
        toks = [int(t) for t in rng.integers(0, V, n)] if case % 3 else [7, 8] * (n // 2 + 1)
        rows = [torch.from_numpy(rng.standard_normal(V).astype(np.float32) * float(rng.uniform(0.5, 4.0))) for _ in toks]
        nsp = float(rng.uniform(0, 1))
        det = WhisperNoSpeechDetection(no_speech_token=V - 2, begin_index=1)
        det._no_speech_prob = torch.tensor([nsp])
        want = W._need_fallback(stub, torch.tensor(toks), [{"scores": tuple(rows)}], 0, [det], gc, V, 0.0)
        lp = [float(torch.log_softmax(r.float(), -1)[t]) for r, t in zip(rows, toks)]
        got = S.gate(nsp, S.avg_logprob(lp, 0, len(toks)), S.compression_ratio(toks, V), nst, lpt, crt)
        assert got == tuple(bool(x) for x in want), (case, got, want)
        seen.add(got)
    SEEN_GATES.update(seen)


def test_gate_cases_cover_every_outcome():
    """(runs behind the parametrised comparison above) HF's three outcomes all occurred: nothing, fallback, skip."""
    assert SEEN_GATES == {(False, False), (True, False), (False, True)}, SEEN_GATES


@pytest.mark.parametrize("temperature", [None, 0.0])
@pytest.mark.parametrize("ht", ["base_head", "medusa_block"])
def test_gpu_inputs_without_timestamps_end_at_different_lengths(ht, temperature):
    """The runs of test_generate_token_logprobs without the timestamp rules, decoded by the oracle: the 12 streams differ in length."""
    import test_gpu_scores as G
    cfg = G._cfg(ht, False)
    orc = Oracle(cfg, G._sd(cfg, ht, False), sim="bf16", act="hilo")
    m = WhisperMedusaModel(cfg, {}, device=None)
    gp = m._gen_params(None, None, G.decay_for(ht, temperature, False), 40, None, temperature, False, None, None, None, None, None)
    P, n = len(gp.prompt), cfg.n_mel_frames * 160
    lens = [len(G._own(orc.decode(orc.encode(torch.from_numpy(log_mel(c, cfg.num_mel_bins, n))), gp).ids, P, gp.eos_token_id)) for c in G.clips(cfg, 12)]
    assert len(set(lens)) > 1, lens
