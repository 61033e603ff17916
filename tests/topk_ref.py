"""CPU reference of the token alternatives (include/wm.h wm_score_tokens_topk / wm_topk_rows), on top of tests/scores_ref.py.

A row is HF's processed `scores[i]` (scores_ref.processed_row: transformers' own processors at the row's own length).  The reference order is
`sorted by (-value, id)` over its finite entries, log-probabilities are torch.log_softmax in fp64, the rank of a target is
1 + #{x > x_t or (x == x_t and n < t)} (0 where the target is masked).  Shared by tests/test_topk_cpu.py and tests/test_gpu_topk.py."""
import dataclasses

import numpy as np
import torch

import scores_ref as R

NEG = -float("inf")
GAP_KERNEL = 1e-4       # crafted rows: adjacent gaps among the reference's top 9 (200 x fp32 rounding at |x| < 8, below test_gpu_scores.TIE)
DECISIVE_SHARE = 0.4    # end to end: share of scored rows whose gaps among the reference's top 3 exceed 2 * MAX_D


def order_of(x):
    """ids of the finite entries of the fp32 row ``x`` (numpy), value descending, then id ascending."""
    fin = np.nonzero(np.isfinite(x))[0]
    return fin[np.lexsort((fin, -x[fin].astype(np.float64)))]


def rank_of(x, target):
    xt = x[target]
    if not np.isfinite(xt):
        return 0
    return 1 + int(np.sum(x > xt)) + int(np.sum(x[:target] == xt))


def ref_topk(x, target, k):
    """Reference of one processed fp32 row (torch or numpy) -> (ids [k] with -1 fills, fp64 log-probabilities [k] with -inf fills, rank,
    the full order, the fp64 log-softmax row)."""
    xt = torch.as_tensor(x).float()
    lp = torch.log_softmax(xt.double(), 0).numpy()
    xn = xt.numpy()
    order = order_of(xn)
    ids = [int(n) for n in order[:k]] + [-1] * max(0, k - len(order))
    lps = [float(lp[n]) for n in order[:k]] + [NEG] * max(0, k - len(order))
    return ids, lps, rank_of(xn, target), order, lp


def top_gaps(x, depth):
    """Adjacent gaps among the ``depth`` largest finite entries of the row (fewer where the row keeps fewer)."""
    xn = torch.as_tensor(x).float().numpy()
    v = xn[order_of(xn)[:depth]].astype(np.float64)
    return [float(a - b) for a, b in zip(v[:-1], v[1:])]


def crafted_sets(cfg):
    """The rows, prefixes and targets of test_gpu_scores.crafted_rows under the parameter sets of test_score_rows_matches_hf, the
    max_initial_timestamp_index = 1 variant on the bare prompt (2 tokens left) and the crafted rows with every rule off.
    -> [(label, cfg the HF processor is built from, gp, rows, prefixes, targets)]"""
    import test_gpu_scores as G
    tb = cfg.timestamp_begin
    rows, pre, tgt = G.crafted_rows(cfg)
    sets = [("ts", cfg, G._gp(cfg, True), rows, pre, tgt)]
    gp2 = G._gp(cfg, True, suppress_tokens=[3, 40], begin_suppress_tokens=[tb + 2, 7], exp_decay=(2, 1.3))
    base = list(gp2.prompt)
    sets.append(("ts+processors", cfg, gp2, rows + [rows[0], rows[0], rows[1]], pre + [base, base, base], tgt + [tb + 2, tb + 1, tb + 2]))
    gp3 = G._gp(cfg, False, suppress_tokens=[3, 5], begin_suppress_tokens=[7, cfg.eos_token_id], exp_decay=(1, 1.5))
    b3 = list(gp3.prompt)
    sets.append(("plain", cfg, gp3, [rows[i] for i in range(5)], [b3, b3, b3 + [9], b3 + [9, 10, 11], b3 + [9, 10, 11, 12, 13]],
                 [7, 8, 7, cfg.eos_token_id, cfg.eos_token_id]))
    cfg1 = dataclasses.replace(cfg, max_initial_timestamp_index=1)
    bare = [r for r in range(len(rows)) if pre[r] == pre[0]]
    sets.append(("mit=1", cfg1, G._gp(cfg1, True), [rows[r] for r in bare] + [rows[bare[0]], rows[bare[-1]]], [pre[0]] * (len(bare) + 2),
                 [tgt[r] for r in bare] + [tb, tb + 1]))           # (+ the two tokens the rules leave, as targets)
    sets.append(("rules off", cfg, G._gp(cfg, False), rows, pre, tgt))
    return sets


_CRAFTED = {}


def crafted_reference(cfg):
    """crafted_sets with HF's processed row of every entry: [(label, gp, rows, prefixes, targets, [processed fp32 row])], computed once."""
    key = (cfg.vocab_size, cfg.timestamp_begin)
    if key not in _CRAFTED:
        out = []
        for label, pcfg, gp, rows, pre, tgt in crafted_sets(cfg):
            proc = R.hf_processor(pcfg, gp.begin_index) if gp.timestamps else None
            xs = [R.processed_row(torch.from_numpy(rows[r]), pre[r], gp, proc)[0] for r in range(len(rows))]
            out.append((label, gp, rows, pre, tgt, xs))
        _CRAFTED[key] = out
    return _CRAFTED[key]


def reference_rows(orc, enc, ids, P, gp, cfg):
    """scores_ref.reference_scores keeping the rows: one teacher-forced oracle pass over ``ids`` (prompt ids[:P], the stream's own end) ->
    {t: (processed fp32 row of position t, timestamp-decision margin)} for P <= t < len(ids)."""
    ids = [int(t) for t in ids]
    z = orc.decoder_pass(orc.new_state(enc), ids[:-1], 0, True)[0]
    proc = R.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
    return {t: R.processed_row(z[t - 1], ids[:t], gp, proc) for t in range(P, len(ids))}


def decisive(x, depth, bound):
    """Every adjacent gap among the reference's top ``depth + 1`` exceeds ``bound``: the first ``depth`` ids are settled."""
    return all(g > bound for g in top_gaps(x, depth + 1))
