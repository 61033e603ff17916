"""CPU reference of constrained decoding on the plain decode path (include/wm.h wm_set_constraint).

The reference is transformers' own PrefixConstrainedLogitsProcessor (`hf_processor`, `hf_rows`) over the callback fn(batch_id, sent) =
sorted(allowed(seqs, eos, sent[P:])), composed with the existing references: a -inf mask commutes with every processor HF runs around it, so a greedy
or sampled step is tests/sample_ref.py::processed and the arg-max / tests/filter_ref.py::draw on the HF-masked raw row (`ConsRef`), and a beam step is
tests/beam_ref.py::ClipBeams with the processor — built with num_beams = n — on the log-probabilities in front of beam_ref.process_row
(`constrained_beams`).  tests/test_constraint_cpu.py holds `allowed` against a brute-force scan and holds, from this reference alone, the conditions
the decode cases below were chosen under."""
import contextlib
import dataclasses
import itertools

import numpy as np
import torch

from helpers import MedusaConfig, GenParams, synth, ACCEPT_GREEDY  # noqa: F401  (also puts the package on sys.path)
import sample_ref as S
import filter_ref as F
import beam_ref as R
import seq_bias_ref as B

NEG_INF = float("-inf")
MAX_SEQS, MAX_LEN = 16384, 32           # WM_CONSTRAINT_MAX / WM_CONSTRAINT_MAX_LEN
SLICES = 8                              # csrc/wm_constraint.hip CONS_SLICES: vocabulary slices (blocks) per row


# ---- the function A(g) --------------------------------------------------------------------------------------------------------------------------
_INDEX = {}


def _index(seqs):
    """prefix -> the set of next ids (None stands for the closing eos), for every prefix of every sequence; built once per table."""
    key = id(seqs)
    if key not in _INDEX or _INDEX[key][0] is not seqs:
        ix = {}
        for s in seqs:
            s = tuple(int(t) for t in s)
            for t in range(len(s)):
                ix.setdefault(s[:t], set()).add(s[t])
            ix.setdefault(s, set()).add(None)
        _INDEX[key] = (seqs, ix)
    return _INDEX[key][1]


def allowed(seqs, eos, g):
    """A(g): every s[t] of the sequences s longer than t = len(g) that start with g; eos when some s == g; eos alone when no s starts with g."""
    nxt = _index(seqs).get(tuple(int(t) for t in g))
    if not nxt:
        return {int(eos)}
    return {int(eos) if v is None else v for v in nxt}


def allowed_scan(seqs, eos, g):
    """The same by a scan of the whole table (what `allowed` is held against)."""
    g, t, out, any_ = [int(x) for x in g], len(g), set(), False
    for s in seqs:
        s = [int(x) for x in s]
        if s[:t] == g:
            any_ = True
            out.add(s[t] if len(s) > t else int(eos))
    return out if any_ else {int(eos)}


# ---- HF's processor ---------------------------------------------------------------------------------------------------------------------------
def hf_processor(seqs, eos, P, num_beams=1):
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    return PrefixConstrainedLogitsProcessor(lambda batch_id, sent: sorted(allowed(seqs, eos, sent[P:].tolist())), num_beams)


def hf_rows(rows, prefixes, seqs, eos, P):
    """HF's processor on every row under its own prefix -> numpy float32 [R, V]."""
    proc = hf_processor(seqs, eos, P)
    out = []
    for x, pre in zip(rows, prefixes):
        out.append(proc(torch.tensor([list(pre)], dtype=torch.long), torch.as_tensor(np.asarray(x), dtype=torch.float32)[None].clone())[0].numpy())
    return np.stack(out)


def contract_rows(rows, prefixes, seqs, eos, P):
    """The contract of include/wm.h: x[v] for v in A(g), -inf elsewhere -> (rows, |A| per row)."""
    out = np.full_like(np.asarray(rows, dtype=np.float32), -np.inf)
    n = []
    for r, pre in enumerate(prefixes):
        a = sorted(allowed(seqs, eos, list(pre)[P:]))
        out[r, a] = np.asarray(rows, dtype=np.float32)[r, a]
        n.append(len(a))
    return out, np.array(n, dtype=np.int32)


# ---- tap cases (tests/test_gpu_constraint.py test 1; the CPU file runs the same cases through contract_rows against HF) ----------------------------
TAP_V = (516, 51864)
TAP_R = (1, 15, 16, 33)
TAP_P = (1, 4)
LONG = tuple(100 + k for k in range(32))            # a sequence of WM_CONSTRAINT_MAX_LEN ids


def slice_span(V):
    """ids per vocabulary slice of k_constraint: ceil(ceil(V / 32) / SLICES) bitmap words."""
    return -(-(-(-V // 32)) // SLICES) * 32


def tap_eos(V):
    return V // 2 + 3                               # (in no sequence of the tables below)


def tap_table(V):
    """The crafted table: a single-token sequence; a sequence that is a strict prefix of another; two that differ in the last id only; two that
    differ in the first id only; two of length 32 that differ in the last id; ids 0 and V - 1; ids at both sides of the first slice edge."""
    e = slice_span(V)
    return [(5,), (10, 11), (10, 11, 12), (10, 40), (20, 21, 22), (20, 21, 23), (30, 31, 32), (33, 31, 32), LONG, LONG[:-1] + (99,),
            (0, V - 1), (V - 1, 0), (e - 1, e), (e,), (e, e - 1, 0)]


def tap_prefixes(V, R, P):
    """R prefixes (a prompt of P ids, then g) cycling through: the root; mid-sequence; a whole sequence (eos alone); a whole sequence that is also a
    prefix (eos and the continuation); one id off the trie at depth 0, mid-depth and depth 32; t = 32 on the trie; t = 33 and beyond; eos inside g;
    the table's corner ids."""
    e, eos = slice_span(V), tap_eos(V)
    base = [3, 4, 6, 8][:P]
    kinds = [[], [10], [10, 11], [10, 11, 12], [20, 21], [5], [6], [20, 22], list(LONG[:-1]) + [7], list(LONG), list(LONG[:-1]), list(LONG) + [eos],
             list(LONG) + [1, 2, 3], [10, 11, eos], [0], [V - 1], [e - 1], [e], [e, e - 1], [30], [33, 31], [31], [10, 11, 12, 13], list(LONG[:16])]
    return [base + list(kinds[r % len(kinds)]) for r in range(R)]


def tap_rows(V, R, seed=7):
    rng = np.random.default_rng(seed + V + R)
    x = (rng.standard_normal((R, V)) * 2.0).astype(np.float32)
    x[:, 0] = 0.0
    x[0, 5] = NEG_INF                               # (an allowed element that is -inf already stays -inf)
    return x


def big_table(V, n=MAX_SEQS, seed=11):
    """n distinct random sequences of 1 .. 12 ids over a 5-id alphabet: ranges are wide (thousands of sequences under one first id) and share long
    prefixes."""
    rng = np.random.default_rng(seed)
    alpha = [17, V - 2, 300, 64, 1]
    seen = {}
    while len(seen) < n:
        m = int(rng.integers(1, 13))
        seen.setdefault(tuple(alpha[i] for i in rng.integers(0, len(alpha), m)))
    return list(seen)


def big_prefixes(table, R, P, seed=13):
    """R prefixes under a big table: the root, truncations of its sequences, whole sequences, and every third one bent off the trie at its last id."""
    rng = np.random.default_rng(seed)
    base, out = [3, 4, 6, 8][:P], [[]]
    while len(out) < R:
        s = list(table[int(rng.integers(0, len(table)))])
        g = s[: int(rng.integers(0, len(s) + 1))]
        if len(out) % 3 == 2 and g:
            g[-1] = 9
        out.append(g)
    return [base + g for g in out[:R]]


# ---- greedy / sampled plain decode with HF's processor in front (tests 3 and 4) --------------------------------------------------------------------
class ConsRef:
    """tests/sample_ref.py::SampleRef's loop — the oracle's plain step, S.processed, arg-max or the (filtered) draw — on the raw row after HF's
    SequenceBiasLogitsProcessor (entries) and PrefixConstrainedLogitsProcessor (seqs).  decode() returns (ids, gaps): gaps[i] = the top-2 gap, among
    the ids the mask leaves, of the decision that emitted ids[P + i] (inf where one id is left); a filtered draw's boundary must be decided."""

    def __init__(self, cfg, sd, sim="bf16", act="hilo"):
        self.cfg, self.orc = cfg, S.Oracle(cfg, sd, sim=sim, act=act)

    def decode(self, enc, gp, seqs=None, entries=None, T=0.0, seed=0, key=0, flt=F.OFF):
        cfg, orc = self.cfg, self.orc
        P, eos = len(gp.prompt), gp.eos_token_id
        bias = B.hf_processor(entries) if entries else None
        cons = hf_processor(seqs, eos, P) if seqs else None
        st = orc.new_state(enc)
        ids, gaps = list(gp.prompt), []
        while True:
            L, kv = len(ids), st["kv_len"]
            z = orc.decoder_pass(st, ids[kv:L], kv, disable_medusa=True, last_only=True)[:, 0][0]
            st["kv_len"] = L
            for proc in (bias, cons):
                if proc is not None:
                    z = B.hf_row(z, ids, proc)
            x, _, _ = S.processed(z, ids, gp, cfg, None)
            assert not torch.isnan(x).any() and torch.isfinite(x).any(), "a row of -inf / NaN"
            if T:
                d = F.draw(x.numpy(), T, seed, key, L, flt)
                assert tuple(flt) == F.OFF or F.decided(d), "a filter boundary under the guard"
                tok, gap = d["token"], d["gap"]
            else:
                tok, gap = int(torch.argmax(x)), S._rr.top2_gap(x)
            ids.append(tok); gaps.append(gap)
            if tok == eos or len(ids) >= gp.max_length:
                break
        return ids, gaps


DEC_CLIPS = S.DEC_CLIPS                 # 4 streams = two clips, each twice
DEC_KEYS = S.DEC_KEYS
DEC_MAX_NEW = S.DEC_MAX_NEW


def dec_checkpoint():
    return S.dec_checkpoint()


def dec_gp(cfg, rep=False):
    gp = S.dec_gp(cfg, False, False)
    return dataclasses.replace(gp, repetition_penalty=1.3) if rep else gp


# The greedy / sampled table: 48 sequences of 1 .. 6 ids over six ids no unconstrained run of the checkpoint emits, plus a sequence that is a strict
# prefix of another.  Every decode under it ends in eos within 7 tokens.
DEC_ALPHA = (101, 222, 343, 464, 585, 706)


def dec_table(seed=1, n=48):
    rng = np.random.default_rng(seed)
    seen = {}
    while len(seen) < n:
        m = int(rng.integers(1, 7))
        seen.setdefault(tuple(DEC_ALPHA[i] for i in rng.integers(0, len(DEC_ALPHA), m)))
    t = list(seen)
    longest = max(t, key=len)
    if longest[:-1] not in seen and len(longest) > 1:
        t.append(longest[:-1])
    return t


DEC_TABLE = dec_table()
# case -> (repetition penalty on, sequence-bias boost: index into DEC_TABLE of the boosted sequence or None, its boost)
DEC_CASES = {"plain": (False, None, 0.0), "rep_bias": (True, 7, 6.0)}
SAMPLE_CASE = dict(T=0.4, seed=3, top_k=2)


def boost_entries(seq, boost):
    """The hotword form: every prefix of the sequence is lifted once its predecessors were emitted."""
    return [(tuple(seq[:k]), float(boost)) for k in range(1, len(seq) + 1)]


def case_entries(name):
    rep, idx, boost = DEC_CASES[name]
    return None if idx is None else boost_entries(DEC_TABLE[idx], boost)


def differs_at_root_and_later(ids, plain, P):
    later = len(ids) != len(plain) or any(a != b for a, b in zip(ids[P + 1:], plain[P + 1:]))
    return ids[P] != plain[P] and later


def is_member(ids, P, eos, seqs):
    """The generated part is one of the sequences plus eos."""
    g = list(ids[P:])
    return len(g) >= 2 and g[-1] == eos and tuple(g[:-1]) in {tuple(s) for s in seqs}


def dec_guards(ref, gp, encs, seqs, entries=None):
    """What the tests ask of a greedy case on the encoder outputs `encs[clip]`: the constrained reference differs from the unconstrained one at the
    root and later, every arg-max among the allowed ids clears 10 x TIE, the text is a member of the table.  Returns {clip: (ids, gaps)}."""
    out = {}
    P = len(gp.prompt)
    for c in sorted(encs):
        plain = ref.decode(encs[c], gp, None, entries)[0]
        ids, gaps = ref.decode(encs[c], gp, seqs, entries)
        assert differs_at_root_and_later(ids, plain, P), ("the constrained reference follows the unconstrained one", c, ids, plain)
        assert min(gaps) >= 10 * S.TIE, ("a decision under 10 x TIE", c, min(gaps))
        assert is_member(ids, P, gp.eos_token_id, seqs), (c, ids)
        out[c] = (ids, gaps)
    return out


def sample_guards(ref, gp, encs, seqs, T, seed, flt, keys=DEC_KEYS, clips=DEC_CLIPS):
    runs = {}
    P = len(gp.prompt)
    for c, k in zip(clips, keys):
        ids, gaps = ref.decode(encs[c], gp, seqs, None, T, seed, k, flt)
        plain = ref.decode(encs[c], gp, None, None, T, seed, k, flt)[0]
        assert differs_at_root_and_later(ids, plain, P), ("the constrained reference follows the unconstrained one", c, k)
        assert min(gaps) >= 10 * S.TIE / S.t32(T), ("a decision under 10 x TIE / T", c, k, min(gaps))
        assert is_member(ids, P, gp.eos_token_id, seqs), (c, k, ids)
        runs[(c, k)] = (ids, gaps)
    assert len({tuple(r[0]) for r in runs.values()}) > 1, "every sampled stream gives the same text"
    return runs


# ---- beam search with HF's processor on the log-probabilities (test 5) -----------------------------------------------------------------------------
@contextlib.contextmanager
def constrained_beams(seqs, eos, P, n):
    """Inside: beam_ref.ClipBeams.step runs HF's PrefixConstrainedLogitsProcessor, built with num_beams = n, on log_softmax(raw) in front of
    beam_ref.process_row.  The processor reads its input n rows per clip: the row goes in n times and comes out once."""
    proc = hf_processor(seqs, eos, P, n) if seqs else None
    orig = R.process_row

    def process_row(w, prefix, gp, ts_proc=None):
        if proc is not None:
            w = proc(torch.tensor([list(prefix)] * n, dtype=torch.long), w[None].repeat(n, 1))[0]
        return orig(w, prefix, gp, ts_proc)
    R.process_row = process_row
    try:
        yield
    finally:
        R.process_row = orig


def beam_run(model_step, gp, n, V, lp, es, seqs):
    with constrained_beams(seqs, gp.eos_token_id, len(gp.prompt), n):
        cb = R.ClipBeams([list(gp.prompt)] * n, gp, n, V, lp, es, "fp32", None, None)
        idx = None
        while not cb.done:
            idx = cb.step(model_step(cb.run_ids, idx))["beam_idx"]
    return cb


def beam_table(n, depth, seed=3):
    """Every sequence of 1 .. depth ids whose first id is one of 2n and whose later ids are one of four: 2n * (4 ** depth - 1) / 3 sequences.  A live
    beam at generated length t < depth then has four continuations (and eos, t >= 1); the root has 2n."""
    rng = np.random.default_rng(seed)
    ids = [int(t) for t in rng.permutation(np.arange(100, 800))[: 2 * n + 4]]
    first, later = ids[: 2 * n], ids[2 * n:]
    out = []
    for d in range(1, depth + 1):
        for f in first:
            out += [(f,) + rest for rest in itertools.product(later, repeat=d - 1)]
    return out


# name -> a case tuple in the layout of beam_ref.E2E_CASES: heads_type, clips, n, length_penalty, early_stopping, timestamps, prompt_ids,
# num_return_sequences, max_batch, max_new, checkpoint seed, logit scale.  max_new = the table's depth: the beams never reach a leaf, the last step
# hits on max_length with every beam still inside the trie, so that every step has 2n finite candidates.  Tables: n2 340 sequences (4 first ids,
# depth 4), n4 680 (8 first ids, depth 4).
BEAM_DEPTH = 4
BEAM_CASES = {
    "n2": ("base_head", (0, 1), 2, 1.0, False, False, None, 2, 4, BEAM_DEPTH, 31, 1.0),
    "n4": ("base_head", (1,), 4, 1.0, False, False, None, 4, 4, BEAM_DEPTH, 31, 1.0),
}
BEAM_SEEDS = {"n2": 3, "n4": 4}                  # (beam_table seeds under which beam_guards holds: tests/test_constraint_cpu.py)
# the under-populated case: three sequences under four beams (no HF comparison: its top-k order among -inf candidates is undefined)
FEW_TABLE = [(DEC_ALPHA[0], DEC_ALPHA[1]), (DEC_ALPHA[0],), (DEC_ALPHA[2], DEC_ALPHA[3], DEC_ALPHA[4])]
FEW_CASE = ("base_head", (0,), 4, 1.0, False, False, None, 4, 4, 8, 31, 1.0)


def beam_case_table(name):
    return beam_table(BEAM_CASES[name][2], BEAM_DEPTH, BEAM_SEEDS[name])


def beam_reference(name, encs=None):
    """The reference runs of a beam case -> (cfg, sd, gp, case, [(unconstrained ClipBeams, constrained ClipBeams)] per clip, table).  encs: encoder
    outputs per clip index (None: the oracle's own)."""
    from oracle.whisper_medusa_oracle import Oracle
    case = BEAM_CASES[name]
    heads, clips, n, lp, es = case[:5]
    cfg, sd, gp = R.e2e_setup(case)
    seqs = beam_case_table(name)
    orc = Oracle(cfg, sd, sim="bf16", act="hilo")
    enc_of = (lambda c: S.oracle_encode(orc, cfg, c)) if encs is None else (lambda c: encs[c])
    runs = []
    for c in clips:
        plain = beam_run(R.OracleBeams(orc, enc_of(c), n), gp, n, cfg.vocab_size, lp, es, None)
        runs.append((plain, beam_run(R.OracleBeams(orc, enc_of(c), n), gp, n, cfg.vocab_size, lp, es, seqs)))
    return cfg, sd, gp, case, runs, seqs


def beam_guards(runs, gp, ranks):
    """Every step of every clip's constrained run keeps 2n finite candidates, none of them planted by a dead beam, and is decisive; the returned
    ranks are ordered decisively; the winner differs from the unconstrained one at the root and later."""
    P = len(gp.prompt)
    for c, (plain, cb) in enumerate(runs):
        for i, rec in enumerate(cb.steps):
            assert np.isfinite(rec["cand_val"]).all() and not rec["planted"], ("fewer than 2n finite candidates", c, i)
        bad = R.e2e_indecisive(cb, ranks - 1)
        assert not bad, ("an indecisive step", c, bad[:3])
        assert differs_at_root_and_later(cb.fin_ids[0], plain.fin_ids[0], P), ("the constrained winner follows the unconstrained one", c)
