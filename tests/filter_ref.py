"""CPU reference of the sampling filters (include/wm.h wm_set_sampling_filter): top-k, top-p and min-p as ONE value threshold per
row, in fp64 from the fp32 row and fl(1 / T).  The row, the noise, the draw and the decode loop are tests/sample_ref.py's; this file adds the
threshold, the draw restricted to what it keeps, and the guards ("decided" rows) the tests of both files share."""
import numpy as np
import torch

import sample_ref as S
from sample_ref import EPS, t32  # noqa: F401

OFF = (0, 1.0, 0.0)
# (top_k, top_p, min_p): the filters of the tap test — each alone, and two combinations
FILTERS = ((1, 1.0, 0.0), (5, 1.0, 0.0), (50, 1.0, 0.0), (0, 0.5, 0.0), (0, 0.9, 0.0), (0, 1.0, 0.05), (0, 1.0, 0.5), (50, 0.9, 0.0), (5, 0.9, 0.05))
K_REF = 5                  # the k the crafted rows put their ties at
GUARD = 10.0               # a boundary is decided when its margin exceeds GUARD x the tolerance
UNDECIDED_CAP = 0.02       # at most 2 % of the rows of a case list may be undecided
_CACHE = {}


def inv_t(T):
    """fl(1 / T) as the engine computes it: one fp32 division of 1 by the fp32 temperature."""
    return float(np.float32(1.0) / np.float32(T))


def tolerance(e, a, Z=None, n=0):
    """Bound on the engine's evaluation of the two arithmetic tests, in the units of the test.  One element's mass e_n = exp(a_n):
      argument: a_n = fl(fl(v_n - m) * fl(1 / T)), two roundings of 2^-24 relative each: |da| <= |a| 2^-23 = |a| EPS, which exp turns into a
                RELATIVE error |a| EPS of the mass;
      expf:     the device library's bound, 1 ulp: EPS relative (taken twice: 2 EPS, which also covers the second-order terms);
      so the engine's mass is e_n (1 + d_n), |d_n| <= (|a_n| + 2) EPS.
    min-p (Z is None): the test is expf(a_n) >= min_p on one element: the bound is e (|a| + 2) EPS, against the margin |e - min_p|.
    top-p (Z: the sum of the masses of K1, n = |K1|; e, a: arrays over K1): the engine tests S < top_p Z on S = the mass of the strictly greater
    values, both sums of round(e_n 2^40) in 64-bit integers — the accumulation as implemented adds no error of its own (integer adds), the
    quantisation errs by 2^-41 per element.  The target ceil(top_p Z 2^40) is taken in fp64: the integer total (up to V 2^40, about 2^56 units)
    rounds by up to 4 units on its way to fp64, the product by up to 4 more, the ceiling by one: under 16 units = 2^-36.  S - top_p Z has
    coefficients 1 - top_p and -top_p on the masses, both below 1 in magnitude: |error| <= sum_K1 e_n (|a_n| + 2) EPS + n 2^-41 + 2^-36, and as a
    FRACTION of the mass (the unit of the margin |G - top_p|): that over Z."""
    if Z is None:
        return float(e) * (abs(float(a)) + 2.0) * EPS
    return float((np.sum(e * (np.abs(a) + 2.0)) * EPS + n * 2.0 ** -41 + 2.0 ** -36) / Z)


def threshold(v, T, top_k=0, top_p=1.0, min_p=0.0):
    """v: the processed row AFTER the decision (fp32, -inf masked) -> dict(thr, kept, ratio, tie): the threshold tau as an fp32 value (-inf: nothing
    is cut; a zero threshold is +0.0), the number of finite ids at or above it, the smallest margin / tolerance of the arithmetic boundaries
    (inf for top-k alone: pure ordering) and whether the top-p boundary value occurs more than once (HF's sort may split such a tie)."""
    v32 = np.asarray(v, dtype=np.float32)
    fin = np.isfinite(v32)
    x = v32[fin].astype(np.float64)
    out = dict(thr=-np.inf, kept=int(fin.sum()), ratio=float("inf"), tie=False)
    if x.size == 0:
        return out
    top_p, min_p = float(np.float32(top_p)), float(np.float32(min_p))
    a_all = (x - x.max()) * inv_t(T)
    tau = -np.inf
    if top_k > 0 and x.size > top_k:
        tau = max(tau, float(np.sort(x)[::-1][top_k - 1]))
    if top_p < 1.0:
        k1 = x >= tau
        xs, a = x[k1], a_all[k1]
        e = np.exp(a)
        Z = float(e.sum())
        vals, inv = np.unique(xs, return_inverse=True)                  # ascending distinct values
        mass = np.bincount(inv, weights=e, minlength=len(vals))[::-1]   # descending
        vals = vals[::-1]
        G = (np.cumsum(mass) - mass) / Z                                # the mass of the strictly greater values, as a fraction
        keep = G < top_p
        last = int(np.nonzero(keep)[0][-1])                             # (G[0] = 0 < top_p: the maximum is always kept)
        tol = tolerance(e, a, Z, int(k1.sum()))
        margin = top_p - G[last]
        if last + 1 < len(vals):
            margin = min(margin, G[last + 1] - top_p)
        out["ratio"] = min(out["ratio"], margin / tol)
        out["tie"] = bool((xs == vals[last]).sum() > 1)
        out["hf_margin"] = float(margin)
        tau = max(tau, float(vals[last]))
    if min_p > 0.0:
        e = np.exp(a_all)
        ok = e >= min_p
        i_ok, i_no = np.nonzero(ok)[0], np.nonzero(~ok)[0]              # (the maximum has e = 1 >= min_p: i_ok is never empty)
        for i in [i_ok[np.argmin(x[i_ok])]] + ([i_no[np.argmax(x[i_no])]] if i_no.size else []):       # the two values either side of the boundary
            out["ratio"] = min(out["ratio"], abs(e[i] - min_p) / tolerance(e[i], a_all[i]))
        tau = max(tau, float(x[ok].min()))
    if np.isfinite(tau):
        out["thr"] = float(np.float32(tau) + np.float32(0.0))          # (-0.0 + 0.0 = +0.0)
        out["kept"] = int((x >= tau).sum())
    return out


def decided(th):
    return th["ratio"] > GUARD


def kept(v, T, top_k=0, top_p=1.0, min_p=0.0):
    """The boolean kept set of the row."""
    v32 = np.asarray(v, dtype=np.float32)
    return np.isfinite(v32) & (v32 >= np.float32(threshold(v32, T, top_k, top_p, min_p)["thr"]))


def draw(v, T, seed, key, t, flt=OFF):
    """sample_ref.draw restricted to the kept set, plus the threshold's record."""
    v32 = np.asarray(v, dtype=np.float32)
    th = threshold(v32, T, *flt)
    d = S.draw(np.where(np.isfinite(v32) & (v32 >= np.float32(th["thr"])), v32, -np.inf), T, seed, key, t)
    d.update(thr=th["thr"], kept=th["kept"], ratio=th["ratio"], tie=th["tie"])
    return d


def filter_row(z_row, prefix, gp, cfg, T, seed, key, flt, ts_proc=None):
    x, forced, margin = processed_cached(z_row, prefix, gp, cfg, ts_proc)
    d = draw(x, T, seed, key, len(prefix), flt)
    d.update(forced=forced, margin=margin)
    return d


def processed_cached(z_row, prefix, gp, cfg, ts_proc):
    """sample_ref.processed, once per (row, prefix): the filters and temperatures of a test all read the same processed row."""
    k = ("proc", z_row.tobytes(), tuple(prefix), gp.timestamps, gp.repetition_penalty, gp.no_repeat_ngram_size, cfg.vocab_size)
    if k not in _CACHE:
        x, forced, margin = S.processed(torch.from_numpy(z_row), prefix, gp, cfg, ts_proc)
        _CACHE[k] = (x.numpy().copy(), forced, margin)
    return _CACHE[k]


class FilterRef(S.SampleRef):
    """sample_ref.SampleRef's plain decode loop with the filtered draw.  decode() returns (ids, gaps, ratios): ratios[i] is the smallest margin /
    tolerance of the arithmetic boundaries of the decision that emitted ids[P + i]."""

    def decode(self, enc, gp, T, seed, key, flt=OFF):
        if tuple(flt) == OFF:
            ids, gaps = super().decode(enc, gp, T, seed, key)
            return ids, gaps, [float("inf")] * len(gaps)
        cfg, orc = self.cfg, self.orc
        ts_proc = S._sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
        eos = gp.eos_token_id
        st = orc.new_state(enc)
        ids, gaps, ratios = list(gp.prompt), [], []
        while True:
            L, kv = len(ids), st["kv_len"]
            zr = orc.decoder_pass(st, ids[kv:L], kv, disable_medusa=True, last_only=True)[:, 0]
            st["kv_len"] = L
            x, _, margin = S.processed(zr[0], ids, gp, cfg, ts_proc)
            d = draw(x.numpy(), T, seed, key, L, flt)
            ids.append(d["token"])
            gaps.append(min(d["gap"], margin / t32(T) if margin != float("inf") else float("inf")))
            ratios.append(d["ratio"])
            if d["token"] == eos or len(ids) >= gp.max_length:
                break
        return ids, gaps, ratios


# ---- the crafted rows of tests/test_filter_cpu.py (guards) and tests/test_gpu_filter.py (the tap) -------------------------------------------------
SETTINGS = ("plain", "ts", "ts_rep")
TAP_T = S.TAP_T
TAP_SEED = S.TAP_SEEDS[0]
BIG_V = 51864
SMALL_V = 516


def shape(name):
    """(cfg, gp, timestamp rules): the three settings of sample_ref.tap_cfg, and the two rules-off vocabularies."""
    if name in SETTINGS:
        cfg = S.tap_cfg()
        return cfg, S.tap_gp(cfg, name), name != "plain"
    cfg = S.MedusaConfig.micro(vocab=int(name))
    return cfg, S.plain_gp(cfg), False


SHAPES = SETTINGS + (str(SMALL_V), str(BIG_V))


def cases(name):
    """(rows [R, V] fp32, prefixes, labels): the raw rows.  Crafted values sit on a low background (N(0, 1) - 8; - 20 at V = 51864), so that they ARE the top of the row
    wherever the processors leave them alone; ties are placed at K_REF: four larger values, then 2, 3 or 17 copies of one value at ids either side
    of the first two slice edges, at 0 and V - 1 and either side of tb."""
    cfg, gp, ts = shape(name)
    V, tb = cfg.vocab_size, cfg.timestamp_begin
    if not ts:
        tb = V // 2                                           # (rules off: no regions; the "boundary" is just two more ids)
    rng = np.random.default_rng(29)
    base = list(gp.prompt)
    big = V > 4096
    if ts:
        pre_mix = base + [tb + 3, 41]                         # text after an opening timestamp: text and the timestamps >= tb + 3 are allowed
        pre_rep = base + [tb + 1, 60, 61, 60]                 # (repetition rules: 61 follows 60)
        prefixes = [base + [tb + 3, 40, tb + 9, tb + 9], pre_mix, base + [tb + 3], pre_rep]
    else:
        pre_mix, pre_rep = base + [9], base + [60, 61, 60]
        prefixes = [base, pre_mix, base + [9, 10, 11], pre_rep]
    per = -(-V // S.SEL_SP)
    edges = [per - 1, per, 2 * per - 1, 2 * per, 0, V - 1, tb - 1, tb]
    taken = set(edges) | {3, 40, 7, tb + 2, 60, 61, cfg.eos_token_id}
    free = [n for n in range(20, min(tb, V) - 1) if n not in taken and n not in pre_mix]

    def ground():
        return (rng.standard_normal(V) - (20.0 if big else 8.0)).astype(np.float32)       # (the whole background holds far less mass than any boundary's margin)

    rows, pre, lab = [], [], []

    def add(x, p, label):
        rows.append(np.asarray(x, dtype=np.float32)); pre.append(list(p)); lab.append(label)

    for s in range(4 if big else 8):                                    # random rows (peaked enough that a top-p boundary has room)
        x = (rng.standard_normal(V) * (5.0 if big else 2.0)).astype(np.float32)
        if ts:
            x[tb:] += (-3.0, 3.0)[s % 2]
        add(x, prefixes[s % len(prefixes)], f"random{s}")
    above = [free[1], free[3], free[5], free[7]]
    for copies, ids in ((2, edges[:2]), (3, edges[2:5]), (17, edges + [free[10 + 2 * j] for j in range(9)])):
        x = ground()
        x[above] = (6.0, 5.0, 4.5, 4.0)
        x[ids] = 2.25
        add(x, pre_mix, f"dup{copies}")
    if ts:                                                              # forced to a timestamp whose region holds fewer than K_REF finite values
        x = ground()
        x[tb:] = -np.inf
        x[[tb + 10, tb + 11, tb + 12]] = (9.0, 8.5, 8.0)
        add(x, pre_mix, "forced_few")
    x = np.full(V, -np.inf, dtype=np.float32)
    x[free[2]] = 1.0
    add(x, pre_mix, "one_finite")
    add(np.full(V, 1.5, dtype=np.float32), pre_mix, "all_equal")
    x = ground()
    x[free[4]] = 30.0
    add(x, pre_mix, "dominant")
    x = ground()
    x[above] = (2.0, 1.0, 0.5, 0.25)
    x[[free[9], free[11]]] = (0.0, -0.0)                                # the K_REF-th place is a tie of +0.0 and -0.0, under mixed signs
    x[free[13]] = -0.5
    add(x, pre_mix, "zeros")
    x = ground()
    c = np.float32(2.25)
    x[above[:3]] = (6.0, 5.0, 4.5)
    x[[free[9], free[11], free[13]]] = (np.nextafter(c, np.float32(9)), c, np.nextafter(c, np.float32(-9)))      # 4th, 5th, 6th: one ulp apart
    add(x, pre_mix, "ulp")
    x = (rng.standard_normal(V) * 2.0).astype(np.float32)
    x[61] = 40.0                                                        # lifted above every threshold; the 2-gram rule bans it after 60
    add(x, pre_rep, "banned")
    return np.stack(rows), pre, lab


def keys_of(R):
    return S.tap_keys(R)


def reference(name, T, flt, seed=TAP_SEED):
    """The reference records of every row of cases(name) under one filter."""
    k = ("ref", name, T, tuple(flt), seed)
    if k not in _CACHE:
        cfg, gp, ts = shape(name)
        rows, pre, _ = cases(name)
        proc = S._sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
        keys = keys_of(len(pre))
        _CACHE[k] = [filter_row(rows[r], pre[r], gp, cfg, T, seed, keys[r], flt, proc) for r in range(len(pre))]
    return _CACHE[k]


def region_count(name, r):
    """|R| of row r: the finite ids the decision leaves."""
    cfg, gp, ts = shape(name)
    rows, pre, _ = cases(name)
    proc = S._sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
    return int(np.isfinite(processed_cached(rows[r], pre[r], gp, cfg, proc)[0]).sum())


# ---- the distribution (test 2): sample_ref.dist_row under top_k = 2 keeps its two largest probabilities, 1/2 and 1/4 -> 2/3 : 1/3 -------------------
def dist_reference(V, position, top_k=2):
    k = ("dist", V, position, top_k)
    if k not in _CACHE:
        x = S.dist_row(V)
        keepm = kept(x, 1.0, top_k)
        x64 = np.where(keepm, x.astype(np.float64), -np.inf)
        toks = np.empty(S.DIST_N, dtype=np.int64)
        for key in range(S.DIST_N):
            toks[key] = int(np.argmax(np.where(np.isfinite(x64), x64 + S.noise(S.DIST_SEED, key, position, V), -np.inf)))
        _CACHE[k] = toks
    return _CACHE[k]


# ---- decode runs (test 3): sample_ref's setup (4 streams = two clips twice, 24 new tokens) -----------------------------------------------------------
# case -> (temperature, timestamp rules, repetition rules, filter, sampling seed).  The seeds were chosen on the CPU with this reference alone
# (oracle encoder; `python tests/filter_ref.py --search`): every draw of the four runs clears 10 x TIE / T and every boundary clears the guard
DEC_CASES = {
    "k5_T1.0": (1.0, False, False, (5, 1.0, 0.0), 2),
    "p0.8_T0.4_ts": (0.4, True, False, (0, 0.8, 0.0), 1),
    "k50_p0.9_m0.05_T1.0_rep": (1.0, False, True, (50, 0.9, 0.05), 1),
}
DEC_DIFFERS = "k5_T1.0"             # the case whose ids must differ from the unfiltered reference's
DEC_SECOND_K = 2                    # a second decode on the same context with another top_k (case DEC_DIFFERS)


def dec_guards(ref, gp, T, seed, flt, encs, keys=S.DEC_KEYS, clips=S.DEC_CLIPS):
    """{(clip, key): (ids, gaps, ratios)} of one case on the encoder outputs encs[clip], with the two margins asserted."""
    runs = {(c, k): ref.decode(encs[c], gp, T, seed, k, flt) for c, k in zip(clips, keys)}
    for (c, k), (ids, gaps, ratios) in runs.items():
        assert min(gaps) >= 10 * S.TIE / t32(T), ("a decision under 10 x TIE / T", c, k, min(gaps))
        assert min(ratios) > GUARD, ("a boundary under the guard", c, k, min(ratios))
    return runs



# ---- generate() (test 4): sample_ref's fallback fixture and long-form recording under sampling_top_k = 50 ------------------------------------------
GEN_FILTER = (50, 1.0, 0.0)
LF_FILTER = (5, 1.0, 0.0)           # the long-form recording: top_k = 50 leaves its one sampled window as the unfiltered draw has it; 5 does not


def fb_reference(ref, cfg, gp, encs, flt=GEN_FILTER):
    """sample_ref.fb_reference with the filtered draw: per stream attempt 0 (exact-match Medusa), the sampled run of attempt 1, both ratios."""
    P, eos, T = len(gp.prompt), gp.eos_token_id, S.FB_TEMPS[1]
    out = []
    for b, c in enumerate(S.FB_CLIPS):
        g_ids, g_gap = S.medusa_run(ref, encs[c], gp)
        s_ids, s_gaps, s_ratios = ref.decode(encs[c], S.plain_of(gp), T, S.FB_SEED, S.stream_key(b, 0, 1), flt)
        out.append(dict(greedy=g_ids, greedy_gaps=[g_gap], sampled=s_ids, sampled_gaps=s_gaps, ratios=s_ratios,
                        cr_greedy=S._sr.hf_compression_ratio(S.own_end(g_ids, P, eos)[P:], cfg.vocab_size),
                        cr_sampled=S._sr.hf_compression_ratio(S.own_end(s_ids, P, eos)[P:], cfg.vocab_size)))
    return out


class Filtered:
    """A FilterRef under one fixed filter, with sample_ref.SampleRef's decode signature: what sample_ref.lf_reference / medusa_run take."""

    def __init__(self, ref, flt=GEN_FILTER):
        self.cfg, self.orc, self.ref, self.flt, self.min_ratio = ref.cfg, ref.orc, ref, flt, float("inf")

    def decode(self, enc, gp, T, seed, key):
        ids, gaps, ratios = self.ref.decode(enc, gp, T, seed, key, self.flt)
        self.min_ratio = min([self.min_ratio] + ratios)
        return ids, gaps


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        cfg, sd = S.dec_checkpoint()
        ref = FilterRef(cfg, sd)
        encs = {c: S.oracle_encode(ref.orc, cfg, c) for c in set(S.DEC_CLIPS)}
        for name, (T, ts, rep, flt, _) in DEC_CASES.items():
            for seed in range(1, 40):
                try:
                    runs = dec_guards(ref, S.dec_gp(cfg, ts, rep), T, seed, flt, encs)
                except AssertionError as e:
                    print(name, seed, "no:", str(e)[:80], flush=True)
                    continue
                plain = {ck: ref.decode(encs[ck[0]], S.dec_gp(cfg, ts, rep), T, seed, ck[1])[0] for ck in runs}
                print(name, "seed", seed, "ok; differs from the unfiltered ids:", [runs[ck][0] != plain[ck] for ck in runs], flush=True)
                break
