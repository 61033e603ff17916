"""CPU reference of the seeded sampling contract (include/wm.h wm_set_sampling) and of HF's generate_with_fallback control flow.

The noise is the contract's own: Philox4x32-10 in numpy (pinned to the Random123 known answers by tests/test_sampling_cpu.py), the mapping
u = (2 (x >> 9) + 1) 2^-24 and g = -log(-log u) in fp64.  The processed row is HF's: tests/repeat_ref.py::hf_row (repetition processors,
oracle.process_logits, WhisperTimeStampLogitsProcessor — whose log-softmax decision runs on the row at temperature 1, before the warper).
`decode` is the oracle's plain step function with the draw in place of the arg-max."""
import numpy as np
import torch

from helpers import MedusaConfig, GenParams, synth, ACCEPT_TYPICAL, ACCEPT_GREEDY  # noqa: F401  (also puts the package on sys.path)
from oracle.whisper_medusa_oracle import Oracle
import repeat_ref as _rr
import scores_ref as _sr

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
EPS = 2.0 ** -23          # one fp32 unit in the last place, relative


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays (Random123 philox4x32, 10 rounds)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK32, p1 >> np.uint64(32), p1 & MASK32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [x.astype(np.uint32) for x in c]


def u_of(x):
    """fp32, exact: the odd multiples of 2^-24."""
    x = np.asarray(x, dtype=np.uint32)
    return (2 * (x >> np.uint32(9)).astype(np.float32) + np.float32(1)) * np.float32(2.0 ** -24)


def gumbel64(x):
    u = u_of(x).astype(np.float64)
    return -np.log(-np.log(u))


def noise_words(seed, key, t, V):
    """x_n for n in [0, V): word n & 3 of the block with counter (n >> 2, t, key_lo, key_hi) under key (seed_lo, seed_hi)."""
    seed, key = int(seed) & (2 ** 64 - 1), int(key) & (2 ** 64 - 1)
    q = np.arange((V + 3) // 4, dtype=np.uint64)
    w = philox4x32_10([q, int(t), key & MASK32, key >> 32], (seed & MASK32, seed >> 32))
    return np.stack(w, axis=1).reshape(-1)[:V]


def noise(seed, key, t, V):
    return gumbel64(noise_words(seed, key, t, V))


def t32(T):
    """The temperature as the C-ABI carries it: a float."""
    return float(np.float32(T))


def draw(v, T, seed, key, t):
    """v: the processed row AFTER the decision (fp32 values, -inf masked) -> dict(token, value, gap, tol): the arg-max of v / T + g in fp64 (ties: the
    lower id), the runner-up's distance, and the arithmetic tolerance of an fp32 evaluation of the winner's value (tolerance())."""
    v = np.asarray(v, dtype=np.float64)
    g = noise(seed, key, t, len(v))
    p = np.where(np.isfinite(v), v / t32(T) + g, -np.inf)
    tok = int(np.argmax(p))
    q = p.copy()
    q[tok] = -np.inf
    run = int(np.argmax(q))                 # the runner-up: the maximum of an fp32 evaluation lies within the larger of the two tolerances
    tol = tolerance(v[tok], g[tok], T)
    if np.isfinite(q[run]):
        tol = max(tol, tolerance(v[run], g[run], T))
    return dict(token=tok, value=float(p[tok]), gap=float(p[tok] - q[run]), tol=tol)


def tolerance(v, g, T):
    """Bound on |fp32 value - fp64 value| of one token's v / T + g, in units EPS = 2^-23 (one fp32 ulp, relative; a correctly rounded operation
    errs by half of it):
      v / T:  v itself may differ by 2 ulp from the reference's fp32 v where a processor computed it (the exponential decay: the engine's factor
              table is a double pow rounded to fp32, HF's an fp32 pow — 1 ulp —, and x + |x| k may be one fused multiply-add or two roundings — 1
              ulp; the repetition penalty: one true division, exact to 1/2 ulp on both sides): 2 EPS |v| / T; fl(1 / T) errs by 1/2 EPS relative;
              the product is exact inside the fused multiply-add;
      g:      a = -logf(u) within 1 ulp (the device library's bound): relative error EPS, which the outer logarithm turns into an ABSOLUTE error
              EPS (d log a = da / a); the outer logf itself within 1 ulp: EPS |g|;
      the fused multiply-add rounds once: 1/2 EPS |value|.
    Sum, with the halves rounded up to 1: EPS (3 |v| / T + 1 + |g| + |v / T + g|)."""
    v, g, T = abs(float(v)), float(g), t32(T)
    return EPS * (3.0 * v / T + 1.0 + abs(g) + abs(v / T + g))


def processed(z_row, prefix, gp, cfg, ts_proc=None):
    """The contract's steps 1 and 2 on one raw fp32 row -> (row after the decision, forced, decision margin)."""
    x = _rr.hf_row(z_row, prefix, gp, None, ts_proc)
    forced, margin = 0, float("inf")
    if ts_proc is not None:
        m = _rr.hf_row(z_row, prefix, gp, None, _sr.masks_only(ts_proc))
        tb = cfg.timestamp_begin
        lse, mt = torch.logsumexp(m[tb:].double(), 0), m[:tb].double().max()
        if torch.isfinite(lse):          # (no timestamp left: nothing to decide)
            forced, margin = int(lse > mt), float((lse - mt).abs()) if torch.isfinite(mt) else float("inf")
    return x, forced, margin


def sample_row(z_row, prefix, gp, cfg, T, seed, key, ts_proc=None):
    x, forced, margin = processed(z_row, prefix, gp, cfg, ts_proc)
    d = draw(x.numpy(), T, seed, key, len(prefix))
    d.update(forced=forced, margin=margin)
    return d


class SampleRef:
    """The oracle's plain decode loop (one base-head row per step) with the draw of the contract.  decode() returns (ids, gaps): gaps[i] is the
    reference's top-2 perturbed gap of the decision that emitted ids[P + i]; T = 0 is the greedy arg-max (gap: the top-2 logit gap)."""

    def __init__(self, cfg, sd, sim="bf16", act="hilo"):
        self.cfg, self.orc = cfg, Oracle(cfg, sd, sim=sim, act=act)

    def decode(self, enc, gp, T, seed, key):
        cfg, orc = self.cfg, self.orc
        ts_proc = _sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
        P, eos = len(gp.prompt), gp.eos_token_id
        st = orc.new_state(enc)
        ids, gaps = list(gp.prompt), []
        while True:
            L, kv = len(ids), st["kv_len"]
            zr = orc.decoder_pass(st, ids[kv:L], kv, disable_medusa=True, last_only=True)[:, 0]
            st["kv_len"] = L
            x, _, margin = processed(zr[0], ids, gp, cfg, ts_proc)
            if T:
                d = draw(x.numpy(), T, seed, key, L)
                tok, gap = d["token"], min(d["gap"], margin / t32(T) if margin != float("inf") else float("inf"))
            else:
                tok, gap = int(torch.argmax(x)), min(_rr.top2_gap(x), margin)
            ids.append(tok); gaps.append(gap)
            if tok == eos or len(ids) >= gp.max_length:
                break
        return ids, gaps


def medusa_run(ref, enc, gp):
    """Attempt 0 of a fallback schedule at temperature 0: the engine's configured path, exact-match Medusa acceptance (`gp` not vanilla).  Its
    ids are the greedy ids, but an iteration emits up to K + 1 tokens, so a run may end a few ids behind max_length: the oracle's chain loop
    (tests/repeat_ref.py::RepRef, transformers' processors per row).  Returns (ids, smallest top-2 logit gap of any row it decided on)."""
    r = _rr.RepRef.__new__(_rr.RepRef)
    r.cfg, r.orc = ref.cfg, ref.orc
    ids, marg, _ = r.decode(enc, gp)
    return ids, min(m[0] for m in marg)


def stream_key(stream_id, seek_frames, attempt):
    """The 64-bit stream key of generate(): key_lo = the stream id, key_hi = 16 * window seek (mel frames) + attempt index."""
    return (int(stream_id) & MASK32) | (((16 * int(seek_frames) + int(attempt)) & MASK32) << 32)


def fallback_loop(temperatures, B, decode, judge, keys_of=None):
    """HF WhisperGenerationMixin.generate_with_fallback's control flow on B streams.  decode(idx, T, attempt) -> one result per stream of idx;
    judge(result, T) -> (needs_fallback, skipped).  Attempt i decodes the streams still flagged at temperatures[i]; a stream is final when it
    needs no fallback, was skipped (no speech) or the temperatures are exhausted (the last attempt is kept).
    Returns (results, kept temperature, attempts) per stream and the log of calls [(attempt, T, idx)]."""
    res, temp, att = [None] * B, [None] * B, [0] * B
    todo, log = list(range(B)), []
    for i, T in enumerate(temperatures):
        if not todo:
            break
        out = decode(list(todo), T, i)
        log.append((i, T, list(todo)))
        nxt = []
        for b, r in zip(todo, out):
            res[b], temp[b], att[b] = r, T, i + 1
            need, skipped = judge(r, T)
            if need and not skipped and i + 1 < len(temperatures):
                nxt.append(b)
        todo = nxt
    return res, temp, att, log


# ---- shared inputs of tests/test_sampling_cpu.py (guards, from the reference alone) and tests/test_gpu_sampling.py ---------------------------
SEL_SP = 16               # csrc/wm_select.h: vocabulary slices of the select / sample kernels
TAP_T = (0.4, 1.0)
TAP_SEEDS = (20240607, 0x9E3779B97F4A7C15)
TAP_SETTINGS = ("plain", "ts", "ts_rep")
_CACHE = {}


def tap_cfg():
    return _sr.micro_ts("base_head")


def tap_gp(cfg, setting):
    """(The decay factor is exact in fp32: the C-ABI carries it as a float, and a factor that is not — 1.05, 1.3 — moves the decayed EOS logit
    itself by k ulp at the k-th power before any sampling arithmetic runs; the tap is about the draw.)"""
    ts = setting != "plain"
    rep = dict(repetition_penalty=1.3, no_repeat_ngram_size=2) if setting == "ts_rep" else {}
    tb = cfg.timestamp_begin
    return GenParams(prompt=synth.default_prompt(cfg, timestamps=ts), eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id,
                     suppress_tokens=[3, 40], begin_suppress_tokens=[tb + 2, 7], max_length=cfg.max_target_positions,
                     hard_max_length=cfg.max_length, exp_decay=(2, 1.0625), accept_mode=ACCEPT_GREEDY, temperature=0.0, vanilla=True,
                     timestamps=ts, no_timestamps_token_id=cfg.no_timestamps_token_id if ts else -1,
                     max_initial_timestamp_index=cfg.max_initial_timestamp_index if ts else None, **rep)


def edge_tokens(V):
    """Tokens at both sides of the first two slice edges (a Philox block of four ids straddles them when the slice width is no multiple of 4),
    the last slice's first token, ids 0 and V - 1."""
    per = -(-V // SEL_SP)
    return [per - 1, per, 2 * per - 1, 2 * per, per * ((V - 1) // per), 0, V - 1]


def tap_cases(cfg, setting):
    """(rows [R, V] fp32, prefixes): the crafted rows of tests/test_gpu_scores.py (timestamp block shifted by -3 / +3: rows the decision leaves
    alone and rows it forces to a timestamp), random rows, and rows whose edge token is lifted so that it wins the draw."""
    V, tb = cfg.vocab_size, cfg.timestamp_begin
    ts = setting != "plain"
    base = synth.default_prompt(cfg, timestamps=ts)
    rng = np.random.default_rng(11)
    if ts:
        prefixes = [base, base + [tb + 3], base + [tb + 3, 40], base + [tb + 3, 40, tb + 9], base + [tb + 3, 40, tb + 9, tb + 9],
                    base + [tb + 2, 17, 18, 19], base + [50, 51], base + [tb + 60, 9, tb + 61, tb + 61, 12, 13],
                    base + [tb + 1, 60, 61, 60], base + [tb + 1, 60, 61, 60, 61, 60]]          # (repetition rules: 61 follows 60)
    else:
        prefixes = [base, base + [9], base + [9, 10, 11], base + [60, 61, 60], base + list(range(100, 140))]
    rows, pre = [], []
    for p in prefixes:
        for shift in (-3.0, 3.0):
            x = (rng.standard_normal(V) * 2.0).astype(np.float32)
            x[tb:] += shift
            rows.append(x); pre.append(list(p))
    for k, e in enumerate(edge_tokens(V) + edge_tokens(tb)):        # lifted edge tokens of the vocabulary and of the text region
        x = (rng.standard_normal(V) * 2.0).astype(np.float32)
        x[tb:] -= 3.0
        x[e] = 40.0
        rows.append(x); pre.append(list(prefixes[1 + k % 3]))
    x = (rng.standard_normal(V) * 2.0).astype(np.float32)
    x[61] = 40.0                                                    # a lifted token the 2-gram rule bans after 60
    rows.append(x); pre.append(list(prefixes[-1] if ts else prefixes[3]))
    return np.stack(rows), pre


def tap_keys(R):
    """One stream key per row: both words in use."""
    return [((7 * r + 1) << 32) | (1000 + r) for r in range(R)]


def tap_reference(setting, T, seed):
    key = ("tap", setting, T, seed)
    if key not in _CACHE:
        cfg = tap_cfg()
        gp = tap_gp(cfg, setting)
        rows, pre = tap_cases(cfg, setting)
        proc = _sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
        keys = tap_keys(len(pre))
        _CACHE[key] = [sample_row(torch.from_numpy(rows[r]), pre[r], gp, cfg, T, seed, keys[r], proc) for r in range(len(pre))]
    return _CACHE[key]


def plain_cases(V, seed):
    """Rules off, any vocabulary: random rows and one lifted edge token per row; the prefix is the prompt (+ a few ids)."""
    rng = np.random.default_rng(seed)
    rows = []
    for k, e in enumerate([None, None] + edge_tokens(V)):
        x = (rng.standard_normal(V) * 2.0).astype(np.float32)
        if e is not None:
            x[e] = 40.0
        rows.append(x)
    return np.stack(rows)


def plain_gp(cfg):
    return GenParams(prompt=synth.default_prompt(cfg), eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id, suppress_tokens=[],
                     begin_suppress_tokens=[], max_length=cfg.max_target_positions, hard_max_length=cfg.max_length, accept_mode=ACCEPT_GREEDY,
                     temperature=0.0, vanilla=True)


def plain_reference(V, T, seed):
    key = ("plain", V, T, seed)
    if key not in _CACHE:
        cfg = MedusaConfig.micro(vocab=V)
        gp = plain_gp(cfg)
        rows = plain_cases(V, 23)
        pre = [list(gp.prompt) + [9] * (r % 3) for r in range(len(rows))]
        keys = tap_keys(len(rows))
        _CACHE[key] = (rows, pre, keys, [sample_row(torch.from_numpy(rows[r]), pre[r], gp, cfg, T, seed, keys[r]) for r in range(len(rows))])
    return _CACHE[key]


# the distribution row: four live tokens with probabilities 1/2, 1/4, 1/8, 1/8 at T = 1 (exact in fp32: logits are multiples of log 2 only up to
# rounding, so the reference draws from the fp32 row it is given), everything else masked by the suppress list's effect: -inf in the row itself
DIST_TOKENS = (5, 64, 65, 1030)
DIST_N = 4096
DIST_SEED = 77


def dist_row(V):
    x = np.full(V, -np.inf, dtype=np.float32)
    x[list(DIST_TOKENS)] = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float32)
    return x


def dist_reference(V, position):
    key = ("dist", V, position)
    if key not in _CACHE:
        x = dist_row(V).astype(np.float64)
        toks = np.empty(DIST_N, dtype=np.int64)
        for k in range(DIST_N):
            p = np.where(np.isfinite(x), x + noise(DIST_SEED, k, position, V), -np.inf)
            toks[k] = int(np.argmax(p))
        _CACHE[key] = toks
    return _CACHE[key]


# ---- decode runs (tests 3 and 4): 4 streams = two clips, each twice, stream keys 0 .. 3 -------------------------------------------------------
TIE = 5e-4                # tests/helpers.py check_tokens: the logit distance of two correct implementations
DEC_MAX_NEW = 24
DEC_CLIPS = (0, 1, 0, 1)
DEC_KEYS = (0, 1, 2, 3)
DEC_CKPT_SEED = 21
# case -> (temperature, timestamp rules, repetition rules, sampling seed).  The seeds were chosen on the CPU with this reference alone (oracle
# encoder; `python tests/sample_ref.py --search`): no decision of the four reference runs of a case falls under 10 x TIE / T
DEC_CASES = {
    "T0.4": (0.4, False, False, 1),
    "T1.0": (1.0, False, False, 1),
    "T0.4_ts": (0.4, True, False, 4),
    "T1.0_ts": (1.0, True, False, 1),
    "T0.4_rep": (0.4, False, True, 1),
}
DEC_SECOND_SEED = 2       # test 4: a second decode on the same context under another seed (case "T1.0")


def dec_checkpoint():
    cfg = _sr.micro_ts("base_head")
    return cfg, _sr.ts_state_dict(cfg, DEC_CKPT_SEED)


def dec_gp(cfg, ts, rep, max_new=DEC_MAX_NEW):
    prompt = synth.default_prompt(cfg, timestamps=ts)
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2) if rep else {}
    return GenParams(prompt=prompt, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id, suppress_tokens=[3, 5],
                     begin_suppress_tokens=list(cfg.begin_suppress_tokens), max_length=min(len(prompt) + max_new, cfg.max_target_positions),
                     hard_max_length=cfg.max_length, accept_mode=ACCEPT_GREEDY, temperature=0.0, vanilla=True, timestamps=ts,
                     no_timestamps_token_id=cfg.no_timestamps_token_id if ts else -1,
                     max_initial_timestamp_index=cfg.max_initial_timestamp_index if ts else None, **kw)


def oracle_encode(orc, cfg, clip):
    from oracle.whisper_medusa_oracle import log_mel
    from helpers import clip_for
    w = clip_for(cfg, clip)
    return orc.encode(torch.from_numpy(log_mel(w, cfg.num_mel_bins, len(w))))


def dec_guards(ref, gp, T, seed, encs, keys=DEC_KEYS, clips=DEC_CLIPS):
    """The reference runs of one case on the encoder outputs `encs[clip]` and what the tests ask of them: every decision's gap >= 10 TIE / T,
    sampled ids != greedy ids, one clip under two keys differs, one clip under one key repeats.  Returns {(clip, key): (ids, gaps)}."""
    runs = {(c, k): ref.decode(encs[c], gp, T, seed, k) for c, k in zip(clips, keys)}
    for (c, k), (ids, gaps) in runs.items():
        assert min(gaps) >= 10 * TIE / t32(T), ("a decision under 10 x TIE / T", c, k, min(gaps))
        assert ids != ref.decode(encs[c], gp, 0.0, seed, k)[0], ("the sampled ids are the greedy ids", c, k)
    by_clip = {}
    for (c, k), (ids, _) in runs.items():
        by_clip.setdefault(c, []).append(ids)
    assert all(len(v) == 2 and v[0] != v[1] for v in by_clip.values()), "one clip under two keys gives the same ids"
    (c0, k0) = next(iter(runs))
    assert ref.decode(encs[c0], gp, T, seed, k0)[0] == runs[(c0, k0)][0]
    return runs


def check_run(got, ref_run, T, label, P):
    """Strict equality, or a first difference at a decision whose reference gap is below TIE / T (assert_same's rule).  Returns 1 for a tie."""
    ids, gaps = ref_run
    if list(got) == list(ids):
        return 0
    first = next((i for i, (a, b) in enumerate(zip(got, ids)) if a != b), min(len(got), len(ids)))
    g = gaps[first - P] if 0 <= first - P < len(gaps) else float("inf")
    print(f"sampling[{label}]: first difference at {first}, reference gap {g:.3g} (bound {TIE / t32(T):.3g})")
    assert g < TIE / t32(T), (label, first, g, list(got), list(ids))
    return 1


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        cfg, sd = dec_checkpoint()
        ref = SampleRef(cfg, sd)
        encs = {c: oracle_encode(ref.orc, cfg, c) for c in set(DEC_CLIPS)}
        for name, (T, ts, rep, _) in DEC_CASES.items():
            for seed in range(1, 40):
                try:
                    dec_guards(ref, dec_gp(cfg, ts, rep), T, seed, encs)
                except AssertionError as e:
                    print(name, seed, "no:", str(e)[:80], flush=True)
                    continue
                print(name, "seed", seed, "ok", flush=True)
                break


# ---- generate() with a fallback schedule (test 5): the loop-prone weights of tests/test_gpu_repeat.py ------------------------------------------
FB_MAX_NEW = 40
FB_TEMPS = (0.0, 0.4)
FB_SEED = 8
FB_CLIPS = (1, 7)         # (chosen on the CPU reference: see test_sampling_cpu.py) stream 0 falls back (its greedy run compresses better than the threshold allows), stream 1 passes at once


def fb_checkpoint():
    from test_gpu_repeat import loop_state_dict, SEEDS
    cfg = MedusaConfig.micro(K=4)
    return cfg, loop_state_dict(cfg, SEEDS["base_head"])


def fb_gp(cfg, sd):
    """What generate(temperature=(0.0, ..), max_new_tokens=FB_MAX_NEW) decodes attempt 0 under (no device needed: exact-match Medusa)."""
    from whisper_medusa import WhisperMedusaModel
    return WhisperMedusaModel(cfg, sd)._gen_params(None, None, None, FB_MAX_NEW, None, 0.0, False, None, None, None, None, None)


def plain_of(gp):
    """The plain decode path under the same processors: what every sampled attempt runs on."""
    import dataclasses
    return dataclasses.replace(gp, vanilla=True)


def own_end(ids, P, eos):
    return ids[: ids.index(eos, P) + 1] if eos in ids[P:] else ids


def fb_reference(ref, cfg, gp, encs, clips=FB_CLIPS, temps=FB_TEMPS, seed=FB_SEED):
    """Per stream: attempt 0 (exact-match Medusa), the sampled run of attempt 1 (stream key of stream b, seek 0, attempt 1) and both
    compression ratios."""
    P, eos = len(gp.prompt), gp.eos_token_id
    out = []
    for b, c in enumerate(clips):
        g_ids, g_gap = medusa_run(ref, encs[c], gp)
        g_gaps = [g_gap]
        s_ids, s_gaps = ref.decode(encs[c], plain_of(gp), temps[1], seed, stream_key(b, 0, 1))
        out.append(dict(greedy=g_ids, greedy_gaps=g_gaps, sampled=s_ids, sampled_gaps=s_gaps,
                        cr_greedy=_sr.hf_compression_ratio(own_end(g_ids, P, eos)[P:], cfg.vocab_size),
                        cr_sampled=_sr.hf_compression_ratio(own_end(s_ids, P, eos)[P:], cfg.vocab_size)))
    return out


def fb_threshold(runs):
    """A compression_ratio_threshold between stream 0's greedy ratio and everything that has to pass: stream 0's sampled ratio and stream 1's
    greedy one.  Returns (threshold, low, high); the guard asserts low < high with room."""
    high = runs[0]["cr_greedy"]
    low = max(runs[0]["cr_sampled"], runs[1]["cr_greedy"])
    return 0.5 * (low + high), low, high


# ---- sequential long-form with a fallback schedule (test 6): the loop of tests/longform_seek.py with HF's retry per window ------------------------
LF_TEMPS = (0.0, 0.4)
LF_MAX_NEW = 24
LF_SEED = 1
LF_LENGTH = 70_700                      # about 2.3 windows of the micro shape
LF_CLIP = (374, (1.0, 0.1, 1.0, 1.0, 0.0))      # (clip index, gains of its half windows: longform_seek.recording), chosen on the CPU reference
LF_OTHER = (543, (1.0, 1.0), 30_500)    # the recording it shares a batch with


def lf_setup(max_new=LF_MAX_NEW):
    """(cfg, sd, gp): the checkpoint of tests/longform_seek.py and what attempt 0 of generate(temperature=(0.0, ..), return_timestamps=True)
    decodes every window under (exact-match Medusa)."""
    import longform_seek as LS
    from whisper_medusa import WhisperMedusaModel
    cfg, sd = LS.checkpoint()
    gp = WhisperMedusaModel(cfg, sd)._gen_params(None, None, None, max_new, None, 0.0, False, None, None, None, None, None, timestamps=True)
    return cfg, sd, gp


def lf_reference(ref, cfg, gp, feats, max_frames, stream_id, threshold, temps=LF_TEMPS, seed=LF_SEED):
    """The sequential loop over ONE recording's oracle features [n_mels, frames] with generate_with_fallback per window: attempt i at temps[i]
    under the stream key (stream id, the window's seek, i); a window is flagged while its compression ratio exceeds `threshold` (None: never).
    Returns the window records of tests/longform_seek.py plus attempts, temperature, the ratios of every attempt made and the smallest gap."""
    import torch.nn.functional as F
    import longform_seek as LS
    Fw, P, tb, eos = cfg.n_mel_frames, len(gp.prompt), cfg.timestamp_begin, gp.eos_token_id
    seek, out = 0, []
    while seek < max_frames:
        snf = min(Fw, max_frames - seek)
        enc = ref.orc.encode(F.pad(feats[:, seek: seek + snf], (0, Fw - snf)))
        ratios, gap = [], float("inf")
        for i, T in enumerate(temps):
            if T:
                ids, gaps = ref.decode(enc, plain_of(gp), T, seed, stream_key(stream_id, seek, i))
            else:
                ids, g0 = medusa_run(ref, enc, gp)
                gaps = [g0]
            ratios.append(_sr.hf_compression_ratio(own_end(ids, P, eos)[P:], cfg.vocab_size))
            gap = min(gap, min(gaps) * (t32(T) if T else 1.0))          # in logit units: comparable with TIE at every temperature
            if threshold is None or not ratios[-1] > threshold:
                break
        raw = LS.generated(ids, P, eos)
        segs, so = LS.hf_retrieve(raw, P, tb, seek, snf)
        out.append(dict(seek=seek, seek_num_frames=snf, ids=raw, segments=segs, segment_offset=so, skipped=False, attempts=i + 1,
                        temperature=T, ratios=ratios, gap=gap))
        seek += so
    return out


def lf_threshold(windows):
    """A compression_ratio_threshold that flags exactly one window of the greedy pass: between its two largest ratios."""
    r = sorted((w["ratios"][0] for w in windows), reverse=True)
    return 0.5 * (r[0] + r[1]), r[0], r[1]


def lf_inputs(clip=LF_CLIP, length=LF_LENGTH):
    import longform_seek as LS
    wavs = [LS.recording(clip[0], length, clip[1]), LS.recording(LF_OTHER[0], LF_OTHER[2], LF_OTHER[1])]
    return wavs


def lf_run(ref, cfg, gp, wavs, b=0):
    """The greedy pass of recording b (to place the threshold), then the loop under that threshold."""
    import longform_seek as LS
    feats, frames = LS.oracle_features(cfg, wavs)
    plain = lf_reference(ref, cfg, gp, feats[b], frames[b], b, None)
    thr, hi, lo = lf_threshold(plain)
    return thr, hi, lo, plain, lf_reference(ref, cfg, gp, feats[b], frames[b], b, thr)
