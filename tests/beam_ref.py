"""CPU reference of the engine's beam search (include/wm.h wm_set_beam): HF GenerationMixin._beam_search restated over any
`step(prefixes, beam_idx) -> raw rows [n, V]` function, one clip at a time (the engine takes HF's three-way stop per clip).

Two arithmetics.  mode="fp32" mirrors HF: torch's fp32 log_softmax, HF's own processor objects on the log-probabilities, fp32 accumulation and HF's
fp32 -1e9 arithmetic; tests/test_beam_cpu.py pins it against `model.generate(num_beams=n)`.  mode="fp64" runs the same steps in double: the yardstick
of the GPU tap, and the source of the per-decision margins.  torch.topk leaves ties open; this reference breaks them as the engine does: value
descending, then (beam, token) ascending, and in the finished-table merge older entries before new ones.

Every step records its ordered 2n candidates, beam_idx and the margins of its decisions — the gap between the last kept and the first dropped value:
  cut2n  of the 2n accumulated values kept out of n * V;
  rankn  between ranks n - 1 and n of those, when a candidate hits (only a hit among the first n ranks may enter the finished table);
  cutn   of the n running beams, taken over the live (not -1e9-shifted) candidates;
  fin    of the finished-table merge, over real (set / entering) scores;
  stop   |best possible running score - worst finished score| of the heuristic, where it is evaluated against a set entry;
  dec    the timestamp rules' log-softmax decision, over the rows of live beams;
and, apart (ORDER_KINDS), the smallest gap between neighbours INSIDE what is kept — order2n, ordern, orderfin: they decide the order of the candidates,
of the streams and of the returned ranks, not what is kept.  The tap tests, which compare every candidate and every beam_idx, need them too; an
end-to-end comparison of the returned hypotheses needs orderfin of the final table only (final_order_margin).
A decision between values that HF's fp32 -1e9 arithmetic has collapsed (dead beams, entries that may not enter) is exact in any implementation of
that arithmetic and counts as decided (margin inf) — unless a kept 2n candidate itself comes from a dead beam: then the step is listed as a planted tie."""
import math

import numpy as np
import torch

from helpers import MedusaConfig, GenParams, synth, ACCEPT_GREEDY  # noqa: F401  (also puts the package on sys.path)
from oracle.whisper_medusa_oracle import process_logits
import repeat_ref as _rr
import scores_ref as _sr

EPS = 2.0 ** -23
NEG = -1.0e9
SEL_SP = 16                 # vocabulary slices of the engine's select kernels (csrc/wm_select.h)
DEAD = -5.0e8               # below: a value HF's -1e9 arithmetic has shifted
TOL_LOGIT = 5e-4            # tests/helpers.py check_tokens: the engine-versus-oracle logit tolerance


def tolerance(V, lse, w, acc):
    """Bound on |fp32 value - fp64 value| of ONE accumulated value a = running score + processors(x - lse) as the engine computes it from an exact
    raw row x and an exact running score, in units EPS = 2^-23 (one fp32 ulp, relative; a correctly rounded operation errs by half of it):
      Z:    V terms expf(x - m), each within 1 ulp (the device library's bound; the subtraction x - m is half an ulp of a number <= 0 whose
            exponential turns it into the same relative size: 1 more); a term's path to the sum holds at most ceil(ceil(V / 16) / 256) - 1 adds in
            its thread, 6 in the wave's butterfly, 2 across the block's four waves, 16 across the slices (all terms positive: every add costs at
            most half an ulp of the total, relatively); the slice merge multiplies by expf(m_k - M): 1 ulp + half for the product;
      lse:  logf(Z) turns Z's relative error into an absolute one of the same size, errs itself by 1 ulp of |log Z| <= |lse| + |m| — bounded
            here by 2 |lse| + log V —, and m + log Z rounds once: half an ulp of |lse|;
      w:    x - lse rounds once (half an ulp of |w|); a processor that computes on it (repetition penalty: one multiply; exponential decay: the
            engine's factor is a double pow rounded to fp32, HF's an fp32 pow, and x + |x| k is two roundings) moves it by at most 2 ulp of |w|;
      a:    the add of the running score rounds once: half an ulp of |a|.
    HF's own fp32 log_softmax lies within the same bound of the fp64 value, so two fp32 values differ by at most twice this."""
    per = -(-int(V) // SEL_SP)
    adds = max(-(-per // 256) - 1, 0) + 6 + 2 + SEL_SP
    z_rel = 2.0 + 0.5 * adds + 1.5
    lse, w, acc = abs(float(lse)), abs(float(w)), abs(float(acc))
    return EPS * (z_rel + (2.0 * lse + math.log(max(V, 2))) + 0.5 * lse + 2.5 * w + 0.5 * acc)


def e2e_bound(steps_so_far):
    """Engine against the oracle, accumulated value after `steps_so_far` earlier steps: TOL_LOGIT on the logit, the same again on the lse, per step."""
    return (steps_so_far + 1) * 2.0 * TOL_LOGIT


def _gap(a, b):
    """a >= b in the reference's order.  Two -inf: their order is the index order in every implementation (inf)."""
    if a == -np.inf and b == -np.inf:
        return float("inf")
    return float(a - b)


def _chain_margin(vals):
    """Smallest gap between neighbours of a descending list."""
    m = float("inf")
    for a, b in zip(vals[:-1], vals[1:]):
        m = min(m, _gap(a, b))
    return m


def process_row(w, prefix, gp, ts_proc=None):
    """HF's processors on one row of log-probabilities `w [V]` (torch fp32 or fp64) under `prefix`, at cur_len = len(prefix): the repetition
    processors, the processors of gp (oracle.process_logits), then WhisperTimeStampLogitsProcessor -> (row, forced, decision margin)."""
    ids = torch.tensor([list(prefix)], dtype=torch.long)
    x = w[None].clone()
    for p in _rr.hf_repeat(gp.repetition_penalty, gp.no_repeat_ngram_size):
        x = p(ids, x)
    x = process_logits(x, len(prefix), gp)
    forced, margin = 0, float("inf")
    if ts_proc is not None:
        m = _sr.masks_only(ts_proc)(ids, x.clone())[0]
        tb = ts_proc.timestamp_begin
        lse, mt = torch.logsumexp(m[tb:].double(), 0), m[:tb].double().max()
        if torch.isfinite(lse):
            forced = int(lse > mt)
            margin = float((lse - mt).abs()) if torch.isfinite(mt) else float("inf")
        x = ts_proc(ids, x.clone())
    return x[0], forced, margin


class ClipBeams:
    """One clip's beam search.  prefixes: n id lists of one length (HF: the prompt n times); P: the decoder prompt length of the length penalty."""

    def __init__(self, prefixes, gp, n, V, length_penalty=1.0, early_stopping=False, mode="fp32", init_scores=None, ts_proc=None, P=None):
        assert mode in ("fp32", "fp64") and early_stopping in (False, True, "never")
        self.gp, self.n, self.V, self.lp, self.es, self.mode, self.ts_proc = gp, n, V, float(np.float32(length_penalty)), early_stopping, mode, ts_proc
        self.ft = np.float32 if mode == "fp32" else np.float64
        self.P = len(gp.prompt) if P is None else P
        self.run_ids = [list(p) for p in prefixes]
        self.run = np.array([0.0] + [NEG] * (n - 1) if init_scores is None else init_scores, dtype=self.ft)
        self.fin_ids = [list(p) for p in prefixes]
        self.fin_score = np.full(n, NEG, dtype=self.ft)
        self.fin_set = [False] * n
        self.heur, self.done, self.steps = True, False, []
        self.neg = self.ft(NEG)

    def _den(self, length):
        return self.ft(float(length) ** self.lp)            # (int ** float in double, then the tensor's dtype: what HF's `x / (len ** lp)` reads)

    def step(self, raw, beam_src=None):
        """raw: [n, V] raw logits rows of the current running beams (any float tensor / array).  Returns the step's record."""
        gp, n, V, ft = self.gp, self.n, self.V, self.ft
        cur = len(self.run_ids[0])
        x = torch.as_tensor(np.asarray(raw), dtype=torch.float32 if self.mode == "fp32" else torch.float64)
        w = torch.log_softmax(x, dim=-1)
        lse = (x[:, 0] - w[:, 0]).double().numpy()
        rows, dec = [], float("inf")
        for j in range(n):
            r, _, m = process_row(w[j], self.run_ids[j], gp, self.ts_proc)
            rows.append(r.numpy().astype(ft))
            if self.run[j] > DEAD:
                dec = min(dec, m)
        wp = np.stack(rows)
        acc = (wp + self.run[:, None]).astype(ft)            # log_probs + running_beam_scores[:, :, None]
        flat = acc.reshape(-1)
        order = np.argsort(-flat, kind="stable")             # value descending, then flat index = (beam, token) ascending
        top = order[: 2 * n]
        val, beam, tok = flat[top], top // V, top % V
        drop = flat[order[2 * n]] if flat.size > 2 * n else -np.inf
        planted = bool(((val < DEAD) & (val > -np.inf)).any())      # a kept candidate comes from a dead beam: fp32 has collapsed its values
        m_cut2n = 0.0 if planted else _gap(val[-1], drop)
        m_order2n = 0.0 if planted else _chain_margin(list(val))
        hit = (tok == gp.eos_token_id) | (cur + 1 >= gp.max_length)
        rv = (val + hit.astype(ft) * self.neg).astype(ft)    # topk_log_probs + hits.to(float32) * -1e9
        rorder = sorted(range(2 * n), key=lambda k: (-rv[k], beam[k], tok[k]))
        keep = rorder[:n]
        live = [k for k in rorder if not hit[k]]
        m_cutn = _gap(rv[live[n - 1]], rv[live[n]]) if len(live) > n else float("inf")
        m_ordern = _chain_margin([rv[k] for k in live[:n]])
        m_rankn = _gap(val[n - 1], val[n]) if hit.any() else float("inf")
        run_new = rv[keep].copy()
        beam_idx = [int(beam[k]) for k in keep]
        new_ids = [self.run_ids[beam[k]] + [int(tok[k])] for k in keep]
        # f. finished table
        did = hit & (np.arange(2 * n) < n)
        s = (val / self._den(cur + 1 - self.P)).astype(ft)
        full = all(self.fin_set)
        if full and self.es is True:
            s = (s + self.neg).astype(ft)
        if not self.heur:
            s = (s + self.neg).astype(ft)
        s = (s + (~did).astype(ft) * self.neg).astype(ft)
        ent = [(-float(self.fin_score[i]), 0, i, 0, ("old", i)) for i in range(n)] + \
              [(-float(s[k]), 1, int(beam[k]), int(tok[k]), ("new", k)) for k in range(2 * n)]
        ent.sort(key=lambda e: e[:4])
        real = [-e[0] for e in ent if -e[0] > DEAD]
        m_fin = _gap(real[n - 1], real[n]) if len(real) > n else float("inf")
        m_orderfin = _chain_margin(real[:n])
        f_ids, f_score, f_set = [], [], []
        for e in ent[:n]:
            kind, i = e[4]
            if kind == "old":
                f_ids.append(self.fin_ids[i]); f_score.append(self.fin_score[i]); f_set.append(self.fin_set[i])
            else:
                f_ids.append(self.run_ids[beam[i]] + [int(tok[i])]); f_score.append(s[i]); f_set.append(bool(did[i]))
        self.fin_ids, self.fin_score, self.fin_set = f_ids, np.array(f_score, dtype=ft), f_set
        self.run_ids, self.run = new_ids, run_new
        # g. heuristic and stop (cur_len has advanced)
        curn = cur + 1
        bl = gp.max_length - self.P if (self.es == "never" and self.lp > 0.0) else curn - self.P
        best = ft(self.run[0] / self._den(bl))
        minfs = self.fin_score.min()
        worst = [minfs if st else self.neg for st in self.fin_set]
        m_stop = min([abs(float(best - minfs))] if any(self.fin_set) and best > DEAD else [float("inf")])
        self.heur = bool(self.heur and any(best > wv for wv in worst))
        cont = self.heur and not (all(self.fin_set) and self.es is True) and not bool(hit.all())
        self.done = not cont
        kept_w = [float(wp[beam[k], tok[k]]) for k in range(2 * n) if np.isfinite(val[k])]
        rec = dict(cand_val=val.copy(), cand_beam=beam.astype(np.int64), cand_tok=tok.astype(np.int64), beam_idx=beam_idx, hit=hit.copy(),
                   margins=dict(cut2n=m_cut2n, rankn=m_rankn, cutn=m_cutn, fin=m_fin, stop=m_stop, dec=dec, order2n=m_order2n, ordern=m_ordern,
                                orderfin=m_orderfin), planted=planted, cur_len=cur,
                   tol=max([tolerance(V, np.abs(lse).max(), min(kept_w + [0.0]), np.abs(val[np.isfinite(val)]).max() if np.isfinite(val).any() else 0.0)]),
                   done=self.done)
        self.steps.append(rec)
        return rec

    def result(self, num_return_sequences=1):
        return [(list(self.fin_ids[r]), float(self.fin_score[r])) for r in range(num_return_sequences)]


def beam_search(step, gp, n, V, length_penalty=1.0, early_stopping=False, mode="fp32", ts_proc=None, max_steps=None):
    """One clip from its prompt.  step(prefixes, beam_idx) -> raw rows [n, V] of the n running prefixes (beam_idx: the beam each prefix continues,
    None at the first step: a stateful model reorders its cache by it).  Returns the ClipBeams (steps, fin_*, run_*)."""
    cb = ClipBeams([list(gp.prompt)] * n, gp, n, V, length_penalty, early_stopping, mode, None, ts_proc)
    idx = None
    while not cb.done and (max_steps is None or len(cb.steps) < max_steps):
        rec = cb.step(step(cb.run_ids, idx), idx)
        idx = rec["beam_idx"]
    return cb


def min_margins(cb, skip_planted=False):
    """The smallest margin of every kind over a run's steps, and per step (kind, margin, bound index)."""
    out = {}
    for rec in cb.steps:
        if skip_planted and rec["planted"]:
            continue
        for k, v in rec["margins"].items():
            out[k] = min(out.get(k, float("inf")), v)
    return out


ORDER_KINDS = ("order2n", "ordern", "orderfin")


def indecisive_steps(cb, bound_of, order=True):
    """Steps with a margin not above twice their bound: [(step, kind, margin, bound)].  bound_of(step index, record) -> the error bound.
    order=False leaves the ORDER_KINDS out (what is kept, not in which order)."""
    bad = []
    for i, rec in enumerate(cb.steps):
        b = bound_of(i, rec)
        for k, v in rec["margins"].items():
            if (order or k not in ORDER_KINDS) and not v > 2.0 * b:
                bad.append((i, k, v, b))
    return bad


def final_order_margin(cb, ranks):
    """Smallest gap between neighbouring scores of the first `ranks` + 1 entries of the final finished table (the order of the returned rows)."""
    s = [float(v) for v in cb.fin_score[: ranks + 1] if v > DEAD]
    return _chain_margin(s)


# ---- the oracle as the model (end-to-end cases) -----------------------------------------------------------------------------------------------
class OracleBeams:
    """step() over the oracle's decoder with one K/V state per beam, reordered by beam_idx: the engine's pass structure (the prompt in one pass,
    then one token per step)."""

    def __init__(self, orc, enc, n):
        self.orc, self.n = orc, n
        st = orc.new_state(enc)
        self.states = [dict(st, self_kv=list(st["self_kv"])) for _ in range(n)]

    def __call__(self, prefixes, beam_idx):
        if beam_idx is not None:
            self.states = [dict(self.states[b], self_kv=list(self.states[b]["self_kv"])) for b in beam_idx]
        rows = []
        for st, ids in zip(self.states, prefixes):
            kv, L = st["kv_len"], len(ids)
            rows.append(self.orc.decoder_pass(st, ids[kv:L], kv, disable_medusa=True, last_only=True)[0, 0])
            st["kv_len"] = L
        return torch.stack(rows)


# ---- tap cases (tests/test_gpu_beam.py tests 1 and 2; their decisiveness is checked on the CPU by tests/test_beam_cpu.py) -----------------------
def tap_cfg(V):
    """V = 1031: the timestamp tap config (tests/scores_ref.py micro_ts) with max_initial_timestamp_index raised so that the first step of 8
    beams still finds 16 timestamps; any other V: the plain micro shape with that vocabulary."""
    import dataclasses
    if V == 1031:
        return dataclasses.replace(_sr.micro_ts("base_head"), max_initial_timestamp_index=20)
    return MedusaConfig.micro(vocab=V)


def tap_gp(cfg, setting, max_length=None):
    ts = setting in ("ts", "ts_rep")
    kw = {}
    if setting in ("rep", "ts_rep"):
        kw.update(repetition_penalty=1.25, no_repeat_ngram_size=2)
    if setting == "decay":
        kw.update(exp_decay=(1, 1.0625))        # (exact in fp32, as tests/sample_ref.py tap_gp says)
    sup = [3, 40] if setting != "plain" else []
    bsup = [7, 9] if setting != "plain" else []
    return GenParams(prompt=synth.default_prompt(cfg, timestamps=ts), eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id,
                     suppress_tokens=sup, begin_suppress_tokens=bsup, max_length=max_length or cfg.max_target_positions,
                     hard_max_length=cfg.max_length, accept_mode=ACCEPT_GREEDY, temperature=0.0, vanilla=True, timestamps=ts,
                     no_timestamps_token_id=cfg.no_timestamps_token_id if ts else -1,
                     max_initial_timestamp_index=cfg.max_initial_timestamp_index if ts else None, **kw)


# (V, n, G, setting, first): first = HF's first-step scores [0, -1e9, ..] from the bare prompt; else a mid-decode step with distinct prefixes and
# caller-given running scores.  V = 516: 16 slices of 33 leave the last one short (21); 1031: 65 per slice, the last one 56.
TAP1_CASES = [
    (516, 2, 1, "plain", True), (516, 5, 3, "plain", False), (516, 8, 1, "sup", True), (516, 8, 3, "decay", False), (516, 5, 1, "rep", False),
    (1031, 2, 3, "ts", True), (1031, 5, 1, "ts", False), (1031, 8, 3, "ts_rep", False), (1031, 8, 1, "plain", True), (1031, 5, 3, "decay", False),
    (51864, 5, 1, "sup", False),
]
TAP_SCALE = 2.0


def tap1_case(V, n, G, setting, first, seed=5):
    """One select step: (cfg, gp, logits [1, G, n, V], prefixes [G * n], init_scores or None)."""
    cfg = tap_cfg(V)
    gp = tap_gp(cfg, setting)
    rng = np.random.default_rng(seed + V + 31 * n + 7 * G)
    ts = gp.timestamps
    tb = cfg.timestamp_begin
    base = list(gp.prompt)
    x = (rng.standard_normal((1, G, n, V)) * TAP_SCALE).astype(np.float32)
    if first:
        return cfg, gp, x, [base] * (G * n), None
    pre, init = [], []
    for g in range(G):
        for j in range(n):
            if ts:          # beams differ in their timestamp state: text after a pair, an open timestamp, plain text
                tail = [[tb + 3, 41, 42], [tb + 1, tb + 1, 60], [tb + 2, 50, tb + 4]][(g + j) % 3]
                x[0, g, j, tb:] += [-3.0, 3.0][(g + j) % 2]         # rows the decision leaves alone / forces to a timestamp
            else:
                tail = [[60, 61, 60], [61, 60, 62], [9, 10, 11]][(g + j) % 3]      # (repetition rules: 61 follows 60)
            pre.append(base + tail)
            init.append(-0.75 * j - 0.1 * g - float(rng.random()))
    x[0, :, :, gp.eos_token_id] += 6.0            # EOS inside the ranks (the decay reads it)
    return cfg, gp, x, pre, np.array(init, dtype=np.float32)


def tap_reference(cfg, gp, x, pre, init, n, length_penalty=1.0, early_stopping=False, mode="fp64"):
    """ClipBeams of every clip of a tap case, all its steps."""
    S, G = x.shape[0], x.shape[1]
    proc = _sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
    out = []
    for g in range(G):
        cb = ClipBeams(pre[g * n: (g + 1) * n], gp, n, cfg.vocab_size, length_penalty, early_stopping, mode,
                       None if init is None else init[g * n: (g + 1) * n], proc)
        for s in range(S):
            if cb.done:
                break
            cb.step(x[s, g])
        out.append(cb)
    return out


# planted exact ties (listed apart: compared against the defined order, not against a margin): equal logits in one row and across two beams
def tie_case():
    cfg = tap_cfg(516)
    gp = tap_gp(cfg, "plain")
    n, V = 3, cfg.vocab_size
    x = np.full((1, 1, n, V), -4.0, dtype=np.float32)
    x[0, 0, :, [200, 17, 333]] = 2.0            # three equal winners in every row
    x[0, 0, 1, 450] = 2.0
    init = np.array([-1.0, -1.0, -2.0], dtype=np.float32)       # beams 0 and 1 tie: (beam, token) ascending decides
    return cfg, gp, x, [list(gp.prompt) + [9]] * n, init, n


# ---- scripted steps (test 2) -------------------------------------------------------------------------------------------------------------------
SCRIPT_S = 6
SCRIPT_CASES = [  # (name, n, length_penalty, early_stopping, max_new or None)
    ("lp1_false", 3, 1.0, False, None), ("lp0_true", 3, 0.0, True, None), ("lp2_never", 3, 2.0, "never", None),
    ("lp1_true_fill", 2, 1.0, True, None), ("maxlen", 3, 1.0, False, 4), ("lp2_false", 4, 2.0, False, None),
]


def script_case(name, n, lp, es, max_new, seed=3):
    """S steps for one clip (G = 2: the second clip gets other rows) on the timestamp tap config: EOS is lifted into and out of the first n ranks
    step by step, so that the finished table fills; the rows' timestamp blocks are shifted so that beams sit in different timestamp states."""
    cfg = tap_cfg(1031)
    gp0 = tap_gp(cfg, "ts")
    gp = tap_gp(cfg, "ts", max_length=len(gp0.prompt) + max_new if max_new else None)
    V, tb, eos = cfg.vocab_size, cfg.timestamp_begin, cfg.eos_token_id
    G = 2
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    x = (rng.standard_normal((SCRIPT_S, G, n, V)) * TAP_SCALE).astype(np.float32)
    for s in range(SCRIPT_S):
        for g in range(G):
            for j in range(n):
                x[s, g, j, tb:] += [-2.0, 4.0, 0.5][(s + g + j) % 3]
                # EOS: far out (never), just inside the 2n ranks but outside the first n, or the row's best
                x[s, g, j, eos] += [-6.0, 5.5 + 0.3 * j, 9.0][(s + 2 * g + j) % 3] if s > 0 else -6.0
    return cfg, gp, x, [list(gp.prompt)] * (G * n), None


# ---- end-to-end cases (test 4 and the CPU decisiveness check) ----------------------------------------------------------------------------------
# name -> (heads_type, clips, n, length_penalty, early_stopping, timestamps, prompt_ids, num_return_sequences, max_batch, max_new, checkpoint seed,
#          logit scale).  The seeds and the scale of the output projection were chosen on the CPU with this reference alone (`python tests/beam_ref.py
# --search`): no decision of a case's reference runs falls under twice its bound.  The scale stays 1: the bound is the engine-versus-oracle logit
# tolerance of the project's ordinary checkpoints, and a scaled output projection scales the engine's own error with it.  "groups" is "b3n5" on a context of 8 streams (groups of one clip).
E2E_PROMPT_IDS = tuple(range(11, 27))
E2E_CASES = {
    "b1n2": ("base_head", (0,), 2, 1.0, False, False, None, 1, 2, 18, 36, 1.0),           # (a result longer than 16 generated tokens)
    "b3n5": ("base_head", (0, 1, 2), 5, 1.0, False, False, None, 3, 15, 6, 70, 1.0),
    "block": ("medusa_block", (0, 1), 3, 1.0, True, False, None, 1, 6, 10, 35, 1.0),
    "ts": ("base_head", (0, 1), 2, 1.0, False, True, None, 1, 4, 8, 51, 1.0),
    "prompt": ("base_head", (1,), 4, 2.0, False, False, E2E_PROMPT_IDS, 1, 4, 8, 33, 1.0),
}
E2E_CASES["groups"] = E2E_CASES["b3n5"][:7] + (1, 8) + E2E_CASES["b3n5"][9:]


def e2e_cfg(heads_type, timestamps):
    import dataclasses
    c = _sr.micro_ts(heads_type)
    return dataclasses.replace(c, max_initial_timestamp_index=20, begin_suppress_tokens=[7, c.eos_token_id])


def e2e_state_dict(cfg, seed, scale):
    sd = _sr.ts_state_dict(cfg, seed)
    sd["whisper_model.proj_out.weight"] = sd["whisper_model.proj_out.weight"] * scale
    return sd


def e2e_gp(cfg, timestamps, prompt_ids, max_new):
    prompt = synth.default_prompt(cfg, timestamps=timestamps)
    bsi = None
    if prompt_ids is not None:
        bsi = len(prompt)
        prompt = [cfg.prev_sot_token_id] + list(prompt_ids) + prompt
    return GenParams(prompt=prompt, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id, suppress_tokens=list(cfg.suppress_tokens or []),
                     begin_suppress_tokens=list(cfg.begin_suppress_tokens), max_length=min(len(prompt) + max_new, cfg.max_target_positions),
                     hard_max_length=cfg.max_length, accept_mode=ACCEPT_GREEDY, temperature=0.0, vanilla=True, timestamps=timestamps,
                     begin_suppress_index=bsi, no_timestamps_token_id=cfg.no_timestamps_token_id if timestamps else -1,
                     max_initial_timestamp_index=cfg.max_initial_timestamp_index if timestamps else None)


_E2E = {}


def e2e_setup(case):
    heads, clips, n, lp, es, ts, pid, _, _, max_new, seed, scale = case
    cfg = e2e_cfg(heads, ts)
    return cfg, e2e_state_dict(cfg, seed, scale), e2e_gp(cfg, ts, pid, max_new)


def e2e_run(case, mode="fp32", stop_when_indecisive=False):
    """The oracle-driven reference runs of a case (bf16 hi / lo oracle: the act_fp16=False contract) -> (cfg, sd, gp, [ClipBeams per clip])."""
    from oracle.whisper_medusa_oracle import Oracle
    from sample_ref import oracle_encode
    heads, clips, n, lp, es, ts = case[:6]
    cfg, sd, gp = e2e_setup(case)
    orc = Oracle(cfg, sd, sim="bf16", act="hilo")
    proc = _sr.hf_processor(cfg, gp.begin_index) if ts else None
    runs = []
    for c in clips:
        model = OracleBeams(orc, oracle_encode(orc, cfg, c), n)
        cb = ClipBeams([list(gp.prompt)] * n, gp, n, cfg.vocab_size, lp, es, mode, None, proc)
        idx = None
        while not cb.done:
            idx = cb.step(model(cb.run_ids, idx))["beam_idx"]
            if stop_when_indecisive and e2e_indecisive(cb, case[7], final=False):
                break
        runs.append(cb)
    return cfg, sd, gp, runs


def e2e_indecisive(cb, ranks, final=True):
    """What an end-to-end comparison of the returned hypotheses needs decided: every cut of every step against (steps so far + 1) * 2 * TOL_LOGIT,
    and the order of the returned ranks in the final table."""
    bad = indecisive_steps(cb, lambda i, r: e2e_bound(i), order=False)
    bad += [(i, "planted", 0.0, 0.0) for i, r in enumerate(cb.steps) if r["planted"]]
    if final and not final_order_margin(cb, ranks) > 2.0 * e2e_bound(len(cb.steps) - 1):
        bad.append((len(cb.steps) - 1, "final order", final_order_margin(cb, ranks), e2e_bound(len(cb.steps) - 1)))
    return bad


def e2e_reference(name, mode="fp32"):
    key = (E2E_CASES[name][:7] + E2E_CASES[name][9:], mode)        # ("groups" shares the runs of "b3n5")
    if key not in _E2E:
        _E2E[key] = e2e_run(E2E_CASES[name], mode)
    return _E2E[key]


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:          # seeds / scales under which every case is decisive
        for name, case in E2E_CASES.items():
            if name == "groups":
                continue
            for scale in (1.0,):
                for seed in range(31, 91):
                    c = case[:10] + (seed, scale)
                    runs = e2e_run(c, "fp64", stop_when_indecisive=True)[3]
                    bad = [b for cb in runs for b in e2e_indecisive(cb, case[7], final=cb.done)]
                    gen = [len(cb.fin_ids[0]) - len(cb.gp.prompt) for cb in runs]
                    eos = [sum(int(r["hit"][: case[2]].any()) for r in cb.steps) for cb in runs]
                    print(name, scale, seed, "ok" if not bad else f"indecisive {bad[:2]}", "generated", gen, "steps with a hit", eos, flush=True)
