"""Token alternatives on the GPU: top-k ids, log-probabilities and the rank of every scored token (generate(top_logprobs=k); include/wm.h
wm_score_tokens_topk / wm_topk_rows).

The reference is tests/topk_ref.py on top of tests/scores_ref.py: transformers' own processors per row at the row's own length, the order
`(-value, id)` over the finite entries, fp64 log-softmax.  End to end the reference scores the ENGINE's ids.  Bounds: ATOL_KERNEL for the
kernels' own arithmetic, MAX_D for everything behind the decoder's logits (both derived in tests/test_gpu_scores.py)."""
import numpy as np
import pytest
import torch

import scores_ref as R
import topk_ref as K
import test_gpu_scores as G
from helpers import MedusaConfig, synth
from oracle.whisper_medusa_oracle import Oracle
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu

NEG = -float("inf")
KS = (1, 3, 8)


# ---- 1. the tap against HF on the crafted rows ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tap_model(gpu):
    cfg = R.micro_ts("base_head")
    m = WhisperMedusaModel(cfg, R.ts_state_dict(cfg, 21), device=gpu, max_batch=1, act_fp16=False)
    yield cfg, m
    m.engine.close()


def test_topk_rows_matches_hf(tap_model):
    cfg, m = tap_model
    assert cfg.vocab_size == 1031 and cfg.vocab_size - cfg.timestamp_begin == 97
    short = 0
    for label, gp, rows, pre, tgt, xs in K.crafted_reference(cfg):
        want = [K.ref_topk(xs[r], tgt[r], 8) for r in range(len(rows))]
        n_rank0 = 0
        for k in KS:
            ids, lps, rk = m.engine.topk_rows(gp, np.stack(rows), pre, tgt, k)
            assert ids.shape == lps.shape == (len(rows), k) and rk.shape == (len(rows),)
            for r, (wi, wl, wr, order, _) in enumerate(want):
                assert ids[r].tolist() == wi[:k], (label, k, r, ids[r].tolist(), wi[:k])
                assert int(rk[r]) == wr, (label, k, r, int(rk[r]), wr)
                for j in range(k):
                    if wi[j] < 0:
                        assert lps[r, j] == -np.inf, (label, k, r, j)
                    else:
                        assert abs(float(lps[r, j]) - wl[j]) <= G.ATOL_KERNEL, (label, k, r, j, float(lps[r, j]), wl[j])
                short += k == 8 and len(order) < 8
                n_rank0 += k == 8 and wr == 0
        # the alternatives of a row agree with its scores: the target's entry is the score, bit for bit
        ids, lps, rk = m.engine.topk_rows(gp, np.stack(rows), pre, tgt, 8)
        lp = m.engine.score_rows(gp, np.stack(rows), pre, tgt)
        for r in range(len(rows)):
            assert (int(rk[r]) == 0) == (lp[r] == -np.inf), (label, r)
            if 1 <= int(rk[r]) <= 8:
                assert ids[r, int(rk[r]) - 1] == tgt[r] and lps[r, int(rk[r]) - 1] == lp[r], (label, r)
            else:
                assert tgt[r] not in ids[r].tolist()
        print(f"topk tap[{label}]: {len(rows)} rows, {n_rank0} masked targets")
    assert short >= 3       # rows that keep 2, 5 and 6 tokens: the fills
    for bad in (0, 9):
        with pytest.raises(ValueError, match="topk"):
            m.engine.topk_rows(gp, np.stack(rows[:1]), pre[:1], tgt[:1], bad)
    with pytest.raises(ValueError, match="vocabulary"):
        m.engine.topk_rows(gp, np.stack(rows[:1]), pre[:1], [cfg.vocab_size], 3)


# ---- 2. the tap on placed rows, rules off -----------------------------------------------------------------------------------------------
def _check_numpy(m, gp, rows, targets, label):
    """Every k of KS against numpy: ids in (-value, id) order, fp64 log-softmax within ATOL_KERNEL, exact ranks."""
    x = np.stack(rows).astype(np.float32)
    pre = [list(gp.prompt)] * len(rows)
    x64 = x.astype(np.float64)
    mx = x64.max(axis=1, keepdims=True)
    lp = x64 - mx - np.log(np.exp(x64 - mx).sum(axis=1, keepdims=True))
    for k in KS:
        ids, lps, rk = m.engine.topk_rows(gp, x, pre, targets, k)
        for r in range(len(rows)):
            order = K.order_of(x[r])
            assert ids[r].tolist() == [int(n) for n in order[:k]], (label, k, r, ids[r].tolist(), order[:k].tolist())
            assert np.abs(lps[r] - lp[r, order[:k]]).max() <= G.ATOL_KERNEL, (label, k, r)
            assert int(rk[r]) == K.rank_of(x[r], targets[r]), (label, k, r, int(rk[r]))
    return ids, rk


def _plain_gp(cfg):
    return G._gp(cfg, False)


def _placed_rows(V, rng):
    """The smallest shapes at which the selection can go wrong (V = 1031: 16 slices of 17 float4s, the last float4 has one lane beyond V)."""
    def base():
        return (rng.standard_normal(V) * 2.0).astype(np.float32)
    rows, tgt = [], []
    x = base(); x[0] = 20.0; x[V - 1] = 21.0; rows.append(x); tgt.append(0)                     # winners at ids 0 and V - 1
    x = base(); x[400:404] = [23.0, 25.0, 22.0, 24.0]; rows.append(x); tgt.append(402)          # the four largest in one float4
    x = base(); x[[204, 209, 217, 230, 231, 250, 263, 271]] = [30, 37, 31, 36, 32, 35, 33, 34]; rows.append(x); tgt.append(231)    # 8 largest in slice 3
    x = base(); x[[1000, 50, 500]] = 19.5; rows.append(x); tgt.append(500)                      # three bit-equal maxima in three slices
    for k in KS:                                                                                # a bit-equal pair across slots k and k + 1
        x = base()
        hi = rng.choice(V, size=k + 1, replace=False)
        x[hi[: k - 1]] = 40.0 - np.arange(k - 1)
        x[hi[k - 1:]] = 20.0
        rows.append(x); tgt.append(int(max(hi[k - 1:])))
    x = base(); x[[10, 300, 800]] = 1.25                                                        # a target tied with others: only lower ids count
    for t in (10, 300, 800):
        rows.append(x); tgt.append(t)
    return rows, tgt


def test_topk_rows_placed(tap_model):
    cfg, m = tap_model
    rng = np.random.default_rng(17)
    rows, tgt = _placed_rows(cfg.vocab_size, rng)
    ids, rk = _check_numpy(m, _plain_gp(cfg), rows, tgt, "V=1031")
    V = cfg.vocab_size
    assert ids[0, :2].tolist() == [V - 1, 0] and ids[3, :3].tolist() == [50, 500, 1000] and int(rk[3]) == 2
    assert int(rk[-2]) == int(rk[-3]) + 1 and int(rk[-1]) == int(rk[-3]) + 2


def test_topk_rows_short_vocabulary(gpu):
    """V = 516: 129 float4s in slices of 9 — the trailing slice is empty, the one before it partial."""
    cfg = MedusaConfig.micro(vocab=516)
    m = WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=3), device=gpu, max_batch=1, act_fp16=False)
    rng = np.random.default_rng(18)
    rows = [(rng.standard_normal(516) * 2.0).astype(np.float32) for _ in range(4)]
    rows[1][515] = 30.0; rows[1][504] = 29.0; rows[1][0] = 28.0
    rows[2][[503, 515]] = 17.0
    ids, _ = _check_numpy(m, _plain_gp(cfg), rows, [5, 515, 503, 200], "V=516")
    assert ids[1, :3].tolist() == [515, 504, 0]
    m.engine.close()


def test_topk_rows_full_vocabulary(gpu):
    """V = 51864: every thread sweeps up to 16 elements, more than its list of 8 holds (at V = 1031 it sees at most 4).  Random rows, a
    row whose 8 largest all belong to ONE thread (float4 positions congruent mod 256 inside one slice), in rising and in falling order."""
    V = 51864
    cfg = MedusaConfig.micro(vocab=V)
    m = WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=4), device=gpu, max_batch=1, act_fp16=False)
    rng = np.random.default_rng(19)
    rows = [(rng.standard_normal(V) * 2.0).astype(np.float32) for _ in range(4)]
    n4 = (V + 3) // 4
    per4 = (n4 + 15) // 16
    assert per4 > 3 * 256 + 5
    own = [4 * (2 * per4 + 5 + 256 * i) + j for i in range(4) for j in (0, 3)]            # thread 5 of slice 2: its four float4s, two lanes each
    rows[1][own] = 50.0 + np.arange(8)
    rows[2][own] = 50.0 - np.arange(8)
    rows[3][[0, V - 1]] = 60.0
    ids, _ = _check_numpy(m, _plain_gp(cfg), rows, [7, own[3], own[0], V - 1], "V=51864")
    assert ids[1].tolist() == own[::-1] and ids[2].tolist() == own and ids[3, :2].tolist() == [0, V - 1]
    m.engine.close()


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rigs():
    cache = {}

    def get(ht, ts=True, choices=None):
        if ht not in cache:
            cfg = R.micro_ts(ht)
            sd = R.ts_state_dict(cfg, G.SEEDS[ht])
            cache[ht] = (cfg, sd, Oracle(cfg, sd, sim="bf16", act="hilo"))
        return cache[ht]
    return get


KW = dict(return_timestamps=True, max_new_tokens=40, exponential_decay_length_penalty=G.EXP_DECAY)


def _self_consistent(out, plain, cfg, gp, k):
    P = len(gp.prompt)
    seq, lens = out["sequences"].cpu(), out["lengths"].cpu()
    lp, ids, lps, rk = out["token_logprobs"].cpu(), out["top_token_ids"].cpu(), out["top_token_logprobs"].cpu(), out["token_ranks"].cpu()
    assert torch.equal(out["sequences"], plain["sequences"]) and torch.equal(out["token_logprobs"], plain["token_logprobs"])
    assert not any(name in plain for name in ("top_token_ids", "top_token_logprobs", "token_ranks"))
    B, T = seq.shape
    assert ids.shape == (B, T, k) and ids.dtype == torch.long and lps.shape == (B, T, k) and lps.dtype == torch.float32
    assert rk.shape == (B, T) and rk.dtype == torch.long
    for b in range(B):
        L = int(lens[b])
        for t in list(range(P)) + list(range(L, T)):
            assert torch.all(ids[b, t] == -1) and torch.all(lps[b, t] == NEG) and int(rk[b, t]) == 0
        for t in range(P, L):
            row, tok, r = ids[b, t].tolist(), int(seq[b, t]), int(rk[b, t])
            real = [n for n in row if n >= 0]
            assert r >= 1 and len(real) >= 1 and row[: len(real)] == real and len(set(real)) == len(real)
            assert all(lps[b, t, j] >= lps[b, t, j + 1] for j in range(k - 1))
            assert all((lps[b, t, j] == NEG) == (row[j] < 0) for j in range(k))
            assert cfg.no_timestamps_token_id not in real and not set(real) & set(gp.suppress_tokens or [])
            if tok in row:
                assert lps[b, t, row.index(tok)] == lp[b, t]                 # bit-equal
            assert (r <= k) == (tok in row) and (r > k or row[r - 1] == tok), (b, t, r, row, tok)


@pytest.mark.parametrize("ht", ["base_head", "medusa_block"])
def test_generate_top_logprobs(gpu, rigs, ht):
    cfg, sd, orc = rigs(ht)
    B, k = 4, 4
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=B, act_fp16=False)
    feats = m.extract_features(G.clips(cfg, B))
    out = m.generate(feats, top_logprobs=k, **KW)
    assert m.last_stats["ms_token_logprobs"] > 0
    plain = m.generate(feats, return_token_logprobs=True, **KW)
    gp = m._gen_params(None, None, G.EXP_DECAY, 40, None, None, False, None, None, None, None, None, timestamps=True)
    P = len(gp.prompt)
    _self_consistent(out, plain, cfg, gp, k)
    seq, lens = out["sequences"].cpu(), out["lengths"].cpu()
    ids, lps, rk = out["top_token_ids"].cpu(), out["top_token_logprobs"].cpu(), out["token_ranks"].cpu()
    enc = m.engine.encoder_output(B)
    n_rows = n_dec = n_above = 0
    worst_lp = worst_cut = 0.0
    for b in range(B):
        own = seq[b].tolist()[: int(lens[b])]
        for t, (x, margin) in K.reference_rows(orc, enc[b], own, P, gp, cfg).items():
            n_rows += 1
            _, _, _, order, ref_lp = K.ref_topk(x, own[t], k)
            ref_sorted = ref_lp[order]
            cut = ref_sorted[k - 1] if len(order) >= k else NEG
            for r in range(k):
                n = int(ids[b, t, r])
                if n < 0:
                    continue
                worst_cut = max(worst_cut, float(cut - ref_lp[n]))
                worst_lp = max(worst_lp, abs(float(lps[b, t, r]) - float(ref_lp[n])))
                assert ref_lp[n] >= cut - 2 * G.MAX_D, (ht, b, t, r, n, float(ref_lp[n]), float(cut), margin)
                assert abs(float(lps[b, t, r]) - float(ref_lp[n])) <= G.MAX_D, (ht, b, t, r, n, float(lps[b, t, r]), float(ref_lp[n]), margin)
            ref_t = ref_lp[own[t]]
            lo, hi = 1 + int(np.sum(ref_lp > ref_t + 2 * G.MAX_D)), 1 + int(np.sum(ref_lp > ref_t - 2 * G.MAX_D))
            assert lo <= int(rk[b, t]) <= hi, (ht, b, t, int(rk[b, t]), lo, hi, margin)
            n_above += int(rk[b, t]) > 1
            if K.decisive(x, 2, 2 * G.MAX_D):
                n_dec += 1
                assert ids[b, t, :2].tolist() == [int(v) for v in order[:2]], (ht, b, t, ids[b, t].tolist(), order[:2].tolist(), margin)
    print(f"top_logprobs[{ht}]: {n_rows} scored rows, {n_dec} decisive at depth 2, {n_above} emitted ids of rank > 1; largest |d logprob| "
          f"{worst_lp:.4g}, deepest id {worst_cut:.4g} below the reference's slot {k}")
    assert n_dec >= K.DECISIVE_SHARE * n_rows, (n_dec, n_rows)
    m.engine.close()


# ---- 4. invariance ----------------------------------------------------------------------------------------------------------------------
def _same(run, one, P, n, k, label):
    """Rows [P, n) of a stream in two runs (``one``: alone, with k + 1 slots): log-probabilities at atol 1e-4 (test_gpu_scores.py's bound for the
    same comparison); ids and ranks equal on the rows whose adjacent gaps among the k + 1 slots of the single-stream run all exceed 1e-3."""
    n_eq = 0
    for t in range(P, n):
        assert torch.allclose(run["top_token_logprobs"][t], one["top_token_logprobs"][t, :k], atol=1e-4), (label, t)
        g = one["top_token_logprobs"][t].double()
        gaps = [float(g[j] - g[j + 1]) for j in range(k) if torch.isfinite(g[j + 1])]
        if all(v > 1e-3 for v in gaps):
            n_eq += 1
            assert torch.equal(run["top_token_ids"][t], one["top_token_ids"][t, :k]), (label, t)
            assert int(run["token_ranks"][t]) == int(one["token_ranks"][t]), (label, t)
    return n_eq


def test_alternatives_do_not_depend_on_the_batch_or_the_pool(gpu, rigs):
    cfg, sd, _ = rigs("base_head")
    B, k = 4, 4
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=B, act_fp16=False)
    m.set_micro_batches(1)
    feats = m.extract_features(G.clips(cfg, B))
    names = ("top_token_ids", "top_token_logprobs", "token_ranks")
    P = len(synth.default_prompt(cfg, timestamps=True))
    batch = m.generate(feats, top_logprobs=k, **KW)
    alone = [m.generate(feats[b: b + 1], top_logprobs=k + 1, **KW) for b in range(B)]       # one slot more: the gap behind slot k
    m.set_micro_batches(2)
    pool = m.generate(feats, top_logprobs=k, **KW)
    assert torch.equal(pool["sequences"], batch["sequences"])
    n_eq = 0
    for b in range(B):
        n = int(alone[b]["lengths"][0])
        assert int(batch["lengths"][b]) == n and batch["sequences"][b, :n].tolist() == alone[b]["sequences"][0, :n].tolist()
        assert torch.allclose(batch["token_logprobs"][b, :n], alone[b]["token_logprobs"][0, :n], atol=1e-4)
        one = {name: alone[b][name][0] for name in names}
        for label, run in (("batch", batch), ("pool", pool)):
            n_eq += _same({name: run[name][b] for name in names}, one, P, n, k, (label, b))
            assert torch.all(run["top_token_ids"][b, n:] == -1) and torch.all(run["token_ranks"][b, n:] == 0)
    assert n_eq > 0
    m.engine.close()


def test_a_skipped_stream_holds_fills(gpu, rigs):
    cfg, m, feats = G._no_speech_model(gpu, rigs, 2)
    P = len(synth.default_prompt(cfg, timestamps=True))
    d = m.generate(feats, return_timestamps=True, no_speech_threshold=0.6, logprob_threshold=None, top_logprobs=4, max_new_tokens=24)
    assert bool(d["skipped"].all()) and d["sequences"].shape[1] == P + 1
    assert d["top_token_ids"].shape == (2, P + 1, 4) and torch.all(d["top_token_ids"] == -1)
    assert torch.all(d["top_token_logprobs"] == NEG) and torch.all(d["token_ranks"] == 0)
    m.engine.close()
