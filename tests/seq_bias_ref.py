"""CPU reference of the sequence bias on the plain decode path (include/wm.h wm_set_sequence_bias).

The reference is transformers' own SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor (`hf_processor`, `hf_rows`), composed with the existing
references: HF runs it before every other processor, so a greedy or sampled step is tests/sample_ref.py::processed / draw on the HF-biased raw row
(`BiasRef`), and a beam step is tests/beam_ref.py::ClipBeams with the bias applied to the log-probabilities in front of beam_ref.process_row
(`biased_beams`).  `contract_rows` restates the contract of include/wm.h in numpy; tests/test_seq_bias_cpu.py holds it against HF's processor,
and holds — from this reference alone — the conditions the decode cases below were chosen under (`python tests/seq_bias_ref.py --search` finds
them)."""
import contextlib
import math

import numpy as np
import torch

from helpers import MedusaConfig, GenParams, synth, ACCEPT_GREEDY  # noqa: F401  (also puts the package on sys.path)
import sample_ref as S
import beam_ref as R
import scores_ref as _sr

NEG_INF = float("-inf")
MAX_ENTRIES, MAX_LEN = 1024, 16         # WM_SEQ_BIAS_MAX / WM_SEQ_BIAS_MAX_LEN
EPS = 2.0 ** -23


# ---- HF's processors ----------------------------------------------------------------------------------------------------------------------------
def hf_processor(entries):
    """SequenceBiasLogitsProcessor over [(ids, bias), ..] in the caller's order (a dict keeps it); -inf entries are what NoBadWordsLogitsProcessor
    hands its base class."""
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor
    return SequenceBiasLogitsProcessor({tuple(int(t) for t in ids): float(b) for ids, b in entries})


def hf_rows(rows, prefixes, entries):
    """HF's processor on every row under its own prefix -> numpy float32 [R, V]."""
    proc = hf_processor(entries)
    out = []
    for x, pre in zip(rows, prefixes):
        out.append(proc(torch.tensor([list(pre)], dtype=torch.long), torch.as_tensor(np.asarray(x), dtype=torch.float32)[None].clone())[0].numpy())
    return np.stack(out)


def hf_row(z_row, prefix, proc):
    """One torch fp32 row through an HF processor object."""
    return proc(torch.tensor([list(prefix)], dtype=torch.long), z_row[None].float().clone())[0]


# ---- the contract of include/wm.h, restated -----------------------------------------------------------------------------------------------------
def groups_of(entries):
    """One group per target token (the last id) in the order of first appearance: the one-token entry first, then the caller's order."""
    order, by = [], {}
    for ids, b in entries:
        ids = tuple(int(t) for t in ids)
        if ids[-1] not in by:
            by[ids[-1]] = [[], []]
            order.append(ids[-1])
        by[ids[-1]][0 if len(ids) == 1 else 1].append((ids, b))
    return [(n, by[n][0] + by[n][1]) for n in order]


def contract_rows(rows, prefixes, entries):
    """Per row with prefix ids[:len]: for every target n: s = +0; a one-token entry sets s; every longer entry of length m, in the caller's order,
    with m <= len and ids[len - m + 1 .. len - 1] == its first m - 1 ids: s = s + b (fp32); then x[n] = x[n] + s (fp32)."""
    out = np.array(rows, dtype=np.float32, copy=True)
    grp = groups_of(entries)
    with np.errstate(invalid="ignore"):
        for r, pre in enumerate(prefixes):
            pre, L = [int(t) for t in pre], len(pre)
            for n, ents in grp:
                s = np.float32(0.0)
                for ids, b in ents:
                    m = len(ids)
                    if m == 1:
                        s = np.float32(b)
                    elif m <= L and tuple(pre[L - m + 1: L]) == ids[:-1]:
                        s = np.float32(s + np.float32(b))
                out[r, n] = np.float32(out[r, n] + s)
    return out


# ---- tap cases (tests/test_gpu_seq_bias.py test 1; the CPU file runs the same cases through contract_rows against HF) -----------------------------
TAP_V = (516, 51864)
TAP_R = (1, 15, 16, 33)


def tap_prompt(V):
    cfg = MedusaConfig.micro(vocab=V)
    return list(synth.default_prompt(cfg))


def tap_entries(V, singles=True):
    """The crafted table: targets at ids 0 and V - 1 and at both sides of the select kernels' first two slice edges; lengths 1, 2, 15 and 16;
    two and three entries on one target in different caller orders with biases whose fp32 sum depends on the order; -inf mixed with finite
    values on one target."""
    e = S.edge_tokens(V)                            # [per - 1, per, 2 per - 1, 2 per, first of the last slice, 0, V - 1]
    a, b = 21, 22                                   # the ids the matching prefixes end in
    chain15 = tuple(100 + k for k in range(14))     # 14 leading ids + target = length 15
    chain16 = tuple(200 + k for k in range(15))     # 15 leading ids + target = length 16
    ents = [((0,), 0.75), ((V - 1,), -1.5),
            ((a, e[0]), 1.0e-3), ((b, a, e[0]), 1.0), ((a, a, e[0]), -1.0),           # three on one target: 1e-3, 1.0 (no match below), ...
            ((b, a, e[1]), 1.0), ((a, e[1]), 1.0e-3), ((9, b, a, e[1]), -1.0),        # ... and in another caller order
            ((e[2],), 2.5), ((a, e[2]), 1.0e-3), ((b, a, e[2]), 1.0),                 # a one-token entry plus longer ones
            ((a, e[3]), NEG_INF), ((b, a, e[3]), 3.0), ((e[3],), 0.5),                # -inf mixed with finite values, the one-token entry given last
            ((b, a, e[4]), -1.0), ((a, e[4]), 1.0), ((9, b, a, e[4]), 1.0e-3),        # the order-dependent sum again, reversed
            (chain15 + (50,), 4.0), (chain16 + (51,), -4.0), (chain16[1:] + (51,), 1.0e-3),
            ((a, V - 1), 0.25), ((b, a, 0), NEG_INF)]
    return ents if singles else [e for e in ents if len(e[0]) > 1]       # (without one-token entries a row with no match is left alone)


def tap_prefixes(V, R):
    """R prefixes cycling through: no match, the 2- and 3-token matches, the 4-token match, prefixes shorter than / equal to / one longer than the
    15- and 16-token entries' leading ids, and a one-token prefix."""
    base = tap_prompt(V)
    a, b = 21, 22
    c15, c16 = [100 + k for k in range(14)], [200 + k for k in range(15)]
    kinds = [base + [5, 6], base + [b, a], base + [a, a], base + [9, b, a], base + [a], [a], [b, a],
             c15, [7] + c15, c15[1:], c16, [7] + c16, c16[1:], base + c16, base + c15, [9, b, a], base + [6, 5, 4]]
    return [list(kinds[r % len(kinds)]) for r in range(R)]


def tap_rows(V, R, seed=5):
    rng = np.random.default_rng(seed + V + R)
    x = (rng.standard_normal((R, V)) * 2.0).astype(np.float32)
    x[:, 0] = 0.0                                   # (an exact zero under a bias)
    x[:, S.edge_tokens(V)[:2]] = 0.0                # ... and under the order-dependent sums: the sum itself comes back
    return x


def big_table(V, n=MAX_ENTRIES, seed=9):
    """n entries over n // 2 + .. distinct targets (more than one block of 256 groups at n = 1024): one-token entries on even slots, two-token
    entries (21, target) on odd ones, some targets carrying both."""
    rng = np.random.default_rng(seed)
    half = n // 2
    tg = rng.permutation(V)[: half]                 # (V >= 512: half distinct targets, every one carrying a one-token and a two-token entry)
    ents = []
    for k in range(n):
        if k % 2 == 0:
            ents.append(((int(tg[k // 2]),), float(np.float32(rng.standard_normal()))))
        else:
            ents.append(((21, int(tg[(k // 2 + 100) % half])), float(np.float32(rng.standard_normal()))))
    return ents


# ---- greedy / sampled plain decode with HF's bias in front (tests 2 and 3) -------------------------------------------------------------------------
class BiasRef:
    """tests/sample_ref.py::SampleRef's loop — the oracle's plain step, S.processed, arg-max or S.draw — on the HF-biased raw row.  decode()
    returns (ids, gaps, rows): rows[i] = (raw row, processed row) of the decision that emitted ids[P + i] (kept for the case search only when
    keep_rows)."""

    def __init__(self, cfg, sd, sim="bf16", act="hilo"):
        self.cfg, self.orc = cfg, S.Oracle(cfg, sd, sim=sim, act=act)

    def decode(self, enc, gp, entries=None, T=0.0, seed=0, key=0, keep_rows=False):
        cfg, orc = self.cfg, self.orc
        ts_proc = _sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
        bias = hf_processor(entries) if entries else None
        eos = gp.eos_token_id
        st = orc.new_state(enc)
        ids, gaps, rows = list(gp.prompt), [], []
        while True:
            L, kv = len(ids), st["kv_len"]
            zr = orc.decoder_pass(st, ids[kv:L], kv, disable_medusa=True, last_only=True)[:, 0][0]
            st["kv_len"] = L
            zb = hf_row(zr, ids, bias) if bias is not None else zr
            x, _, margin = S.processed(zb, ids, gp, cfg, ts_proc)
            if T:
                d = S.draw(x.numpy(), T, seed, key, L)
                tok, gap = d["token"], min(d["gap"], margin / S.t32(T) if margin != float("inf") else float("inf"))
            else:
                tok, gap = int(torch.argmax(x)), min(S._rr.top2_gap(x), margin)
            if keep_rows:
                rows.append(x.clone())
            ids.append(tok); gaps.append(gap)
            if tok == eos or len(ids) >= gp.max_length:
                break
        return ids, gaps, rows


DEC_CLIPS = S.DEC_CLIPS                 # 4 streams = two clips, each twice
DEC_MAX_NEW = S.DEC_MAX_NEW
DEC_SETTINGS = {"plain": (False, False), "ts": (True, False), "ts_rep": (True, True)}


def dec_checkpoint():
    return S.dec_checkpoint()


def dec_gp(cfg, setting):
    ts, rep = DEC_SETTINGS[setting]
    return S.dec_gp(cfg, ts, rep)


def choose_entries(ref, gp, encs, pick=0):
    """Entries of the three kinds from the UNBIASED reference runs of the two clips: a boost on a runner-up after a two-token prefix clip 0's run
    emits (lifted 4.0 above the winner), a ban on a token clip 1's run emits, a ban on a bigram of clip 0's run behind the boost.  `pick` moves
    the positions (the search tries several)."""
    P = len(gp.prompt)
    runs = {c: ref.decode(encs[c], gp, None, keep_rows=True) for c in sorted(encs)}
    ids0, _, rows0 = runs[0]
    ids1, _, rows1 = runs[1]
    i = min(2 + pick, len(rows0) - 2)                                   # decision i of clip 0 emitted ids0[P + i]
    x = rows0[i].double().clone()
    win = int(torch.argmax(x)); x[win] = NEG_INF
    run = int(torch.argmax(x))
    lift = float(np.float32(math.ceil(float(rows0[i][win] - rows0[i][run])) + 4.0))
    L = P + i
    boost = ((int(ids0[L - 2]), int(ids0[L - 1]), run), lift)
    # a token of clip 1's run UNDER the boost (the clips share their first tokens: the boost may act there too) that clip 0's run does not
    # emit up to the boost: the ban must not cut the path to the boost's prefix
    ids1 = ref.decode(encs[1], gp, [boost])[0]
    j = next((q for q in range(1 + pick, len(ids1) - P) if ids1[P + q] not in ids0[: L + 1]), len(ids1) - P - 1)
    ban_tok = ((int(ids1[P + j]),), NEG_INF)
    # the bigram comes from clip 0's run UNDER the first two entries, two decisions behind the boost: all three entries act
    ids0b = ref.decode(encs[0], gp, [boost, ban_tok])[0]
    k = min(i + 2, len(ids0b) - P - 1)
    ban_bigram = ((int(ids0b[P + k - 1]), int(ids0b[P + k])), NEG_INF)
    return [boost, ban_tok, ban_bigram]


def entries_that_act(ref, gp, encs, entries):
    """Leave one out: entry e acts when the runs without it differ from the runs with all of them, for some clip."""
    full = {c: ref.decode(encs[c], gp, entries)[0] for c in sorted(encs)}
    return [any(ref.decode(encs[c], gp, entries[:e] + entries[e + 1:])[0] != full[c] for c in sorted(encs)) for e in range(len(entries))]


def dec_guards(ref, gp, encs, entries):
    """What the tests ask of a case on the encoder outputs `encs[clip]`: the biased reference differs from the unbiased one for every clip, and
    every decision of every biased run clears 10 x TIE.  Returns {clip: (ids, gaps)}."""
    out = {}
    for c in sorted(encs):
        plain = ref.decode(encs[c], gp, None)[0]
        ids, gaps, _ = ref.decode(encs[c], gp, entries)
        assert ids != plain, ("the biased reference equals the unbiased one", c)
        assert min(gaps) >= 10 * S.TIE, ("a decision under 10 x TIE", c, min(gaps))
        out[c] = (ids, gaps)
    return out


# The entries were chosen on the CPU with this reference alone (oracle encoder; `python tests/seq_bias_ref.py --search`): choose_entries at the
# first `pick` under which dec_guards holds and every entry acts (entries_that_act).  setting -> pick; "plain2": the second table of the plain setting (another pick: other entries)
DEC_PICKS = {"plain": 1, "ts": 9, "ts_rep": 9, "plain2": 6}
SAMPLE_CASE = dict(T=0.4, seed=1, pick=1)          # test 3: one sampled case, a ban and a boost (the first two entries of choose_entries)
# ... and what choose_entries gave there, written down: the tests run on these tables whatever a host's oracle arithmetic does to the search
DEC_ENTRIES = {
    "plain": [((946, 934, 934), 5.0), ((1011,), NEG_INF), ((934, 971), NEG_INF)],
    "ts": [((1018, 358, 1030), 7.0), ((883,), NEG_INF), ((1030, 633), NEG_INF)],
    "ts_rep": [((1018, 358, 1030), 7.0), ((883,), NEG_INF), ((1030, 633), NEG_INF)],
    "plain2": [((945, 947, 938), 6.0), ((1009,), NEG_INF), ((938, 938), NEG_INF)],
}
SAMPLE_ENTRIES = DEC_ENTRIES["plain"][:2]


def sample_guards(ref, gp, encs, entries, T, seed, keys=S.DEC_KEYS, clips=DEC_CLIPS):
    runs = {}
    for c, k in zip(clips, keys):
        ids, gaps, _ = ref.decode(encs[c], gp, entries, T, seed, k)
        plain = ref.decode(encs[c], gp, None, T, seed, k)[0]
        assert min(gaps) >= 10 * S.TIE / S.t32(T), ("a decision under 10 x TIE / T", c, k, min(gaps))
        runs[(c, k)] = (ids, gaps, ids != plain)
    assert any(r[2] for r in runs.values()), "the bias changes no sampled stream"
    return runs


# ---- beam search with HF's bias on the log-probabilities (test 4) ----------------------------------------------------------------------------------
@contextlib.contextmanager
def biased_beams(entries):
    """Inside: beam_ref.ClipBeams.step runs HF's SequenceBiasLogitsProcessor on log_softmax(raw) in front of beam_ref.process_row (HF's order:
    `log_probs = logits_processor(ids, log_probs)`, the sequence bias first)."""
    proc = hf_processor(entries) if entries else None
    orig = R.process_row

    def process_row(w, prefix, gp, ts_proc=None):
        if proc is not None:
            w = proc(torch.tensor([list(prefix)], dtype=torch.long), w[None].clone())[0]
        return orig(w, prefix, gp, ts_proc)
    R.process_row = process_row
    try:
        yield
    finally:
        R.process_row = orig


def beam_run(model_step, gp, n, V, lp, es, ts_proc, entries, mode="fp32"):
    """One clip's beam search under the bias -> (ClipBeams, widen): widen[i] = one fp32 rounding of |x| + |lse| + |s| at step i, the distance
    between the engine's (x + s) - lse and HF's (x - lse) + s."""
    smax = max([abs(b) for _, b in (entries or []) if b != NEG_INF] + [0.0])
    widen = []
    with biased_beams(entries):
        cb = R.ClipBeams([list(gp.prompt)] * n, gp, n, V, lp, es, mode, None, ts_proc)
        idx = None
        while not cb.done:
            raw = model_step(cb.run_ids, idx)
            x = torch.as_tensor(np.asarray(raw)).double()
            widen.append(EPS * (float(x.abs().max()) + float(torch.logsumexp(x, -1).abs().max()) + smax))
            idx = cb.step(raw)["beam_idx"]
    return cb, widen


def beam_indecisive(cb, widen, ranks):
    """beam_ref.e2e_indecisive with every bound widened by the moved add."""
    bad = R.indecisive_steps(cb, lambda i, r: R.e2e_bound(i) + widen[i], order=False)
    bad += [(i, "planted", 0.0, 0.0) for i, r in enumerate(cb.steps) if r["planted"]]
    last = len(cb.steps) - 1
    if not R.final_order_margin(cb, ranks) > 2.0 * (R.e2e_bound(last) + widen[last]):
        bad.append((last, "final order", R.final_order_margin(cb, ranks), R.e2e_bound(last)))
    return bad


# name -> (a case tuple in the layout of beam_ref.E2E_CASES: heads_type, clips, n, length_penalty, early_stopping, timestamps, prompt_ids,
# num_return_sequences, max_batch, max_new, checkpoint seed, logit scale; pick).  Seeds and picks were chosen on the CPU with this reference alone
# (`python tests/seq_bias_ref.py --search-beam`): no step of a case's biased runs is indecisive and the winner of clip 0 changes
BEAM_CASES = {
    "n2": (("base_head", (0,), 2, 1.0, False, False, None, 1, 2, 8, 31, 1.0), 0),
    "n4": (("base_head", (1,), 4, 1.0, False, False, None, 1, 4, 8, 31, 1.0), 1),
    "n2_ts": (R.E2E_CASES["ts"][:1] + ((0, 1),) + R.E2E_CASES["ts"][2:], 0),
}


BEAM_ENTRIES = {                                    # what beam_entries gave on the oracle's encoder output, written down
    "n2": [((973, 1030, 1030), 1.5), ((973, 1030), NEG_INF)],
    "n4": [((1030, 1030, 938), 1.5), ((1030, 1030), NEG_INF)],
    "n2_ts": [((934, 406, 969), 1.5), ((934, 406), NEG_INF)],
}


def beam_case(name):
    return BEAM_CASES[name]


def beam_entries(cb, gp, pick=0):
    """A boost and a ban from the UNBIASED run of a clip so that the winning hypothesis changes: the best hypothesis' token at generated position
    1 + pick is banned after its predecessor (a bigram ban), and the runner-up hypothesis' last-but-one token is boosted after its two
    predecessors."""
    P = len(gp.prompt)
    best = cb.fin_ids[0]
    q = min(P + 1 + pick, len(best) - 1)
    ban = ((int(best[q - 1]), int(best[q])), NEG_INF)
    other = cb.fin_ids[1] if len(cb.fin_ids) > 1 and len(cb.fin_ids[1]) > P + 2 else best
    r = min(P + 2 + pick, len(other) - 1)
    boost = ((int(other[r - 2]), int(other[r - 1]), int(other[r])), 1.5)
    return [boost, ban]


def beam_reference(name, encs=None, entries=None):
    """The reference runs of a beam case -> (cfg, sd, gp, case, [(unbiased ClipBeams, biased ClipBeams, widen)] per clip, entries).  encs: encoder
    outputs per clip index (None: the oracle's own); entries None: beam_entries of clip 0's unbiased run."""
    from oracle.whisper_medusa_oracle import Oracle
    case, pick = beam_case(name)
    heads, clips, n, lp, es, ts = case[:6]
    cfg, sd, gp = R.e2e_setup(case)
    orc = Oracle(cfg, sd, sim="bf16", act="hilo")
    proc = _sr.hf_processor(cfg, gp.begin_index) if ts else None
    enc_of = (lambda c: S.oracle_encode(orc, cfg, c)) if encs is None else (lambda c: encs[c])
    plain = [beam_run(R.OracleBeams(orc, enc_of(c), n), gp, n, cfg.vocab_size, lp, es, proc, None)[0] for c in clips]
    if entries is None:
        entries = beam_entries(plain[0], gp, pick)
    runs = []
    for c, p in zip(clips, plain):
        cb, widen = beam_run(R.OracleBeams(orc, enc_of(c), n), gp, n, cfg.vocab_size, lp, es, proc, entries)
        runs.append((p, cb, widen))
    return cfg, sd, gp, case, runs, entries


def beam_guards(runs, ranks=1):
    """Every clip's biased run is decisive at every step; the winner of clip 0 changes."""
    for c, (p, cb, widen) in enumerate(runs):
        bad = beam_indecisive(cb, widen, ranks)
        assert not bad, ("an indecisive step", c, bad[:3])
    assert runs[0][1].fin_ids[0] != runs[0][0].fin_ids[0], "the bias does not change the winning hypothesis"


# ---- hotwords: a dict-backed tokenizer ---------------------------------------------------------------------------------------------------------
class FakeTokenizer:
    """encode() over a fixed table text -> ids (what hotword_entries needs of a tokenizer)."""

    def __init__(self, table):
        self.table = {k: list(v) for k, v in table.items()}

    def encode(self, text, add_special_tokens=False):
        assert add_special_tokens is False
        return list(self.table[text])


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        cfg, sd = dec_checkpoint()
        ref = BiasRef(cfg, sd)
        encs = {c: S.oracle_encode(ref.orc, cfg, c) for c in set(DEC_CLIPS)}
        for setting in DEC_SETTINGS:
            gp = dec_gp(cfg, setting)
            for pick in range(0, 12):
                ents = choose_entries(ref, gp, encs, pick)
                try:
                    dec_guards(ref, gp, encs, ents)
                    assert all(entries_that_act(ref, gp, encs, ents)), "an entry that does not act"
                except AssertionError as e:
                    print(setting, "pick", pick, "no:", str(e)[:90], flush=True)
                    continue
                print(setting, "pick", pick, "ok", ents, flush=True)
        gp = dec_gp(cfg, "plain")
        for pick in range(0, 8):
            ents = choose_entries(ref, gp, encs, pick)[:2]
            for seed in range(1, 6):
                try:
                    sample_guards(ref, gp, encs, ents, SAMPLE_CASE["T"], seed)
                except AssertionError as e:
                    print("sample pick", pick, "seed", seed, "no:", str(e)[:90], flush=True)
                    continue
                print("sample pick", pick, "seed", seed, "ok", flush=True)
                break
    if "--search-beam" in sys.argv:
        for name in ("n2", "n4"):
            base = BEAM_CASES[name][0]
            found = False
            for seed in range(31, 61):
                for pick in range(0, 4):
                    BEAM_CASES[name] = (base[:10] + (seed, 1.0), pick)
                    cfg, sd, gp, case, runs, ents = beam_reference(name)
                    try:
                        beam_guards(runs)
                    except AssertionError as e:
                        print(name, "seed", seed, "pick", pick, "no:", str(e)[:100], flush=True)
                        continue
                    print(name, "seed", seed, "pick", pick, "ok", ents, [len(r[1].steps) for r in runs], flush=True)
                    found = True
                    break
                if found:
                    break
