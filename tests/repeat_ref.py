"""CPU reference of the repetition rules (include/wm.h wm_set_repeat_rules), pinned to transformers' own
RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor.

Every logits row goes, under the prefix the contract gives it, through HF's two processors (called with `[1, len]` ids and a `[1, V]` row), then
`oracle.process_logits`, then — timestamp rules on — HF's WhisperTimeStampLogitsProcessor: the order of GenerationMixin._get_logits_processor
followed by the processors Whisper appends.  `RepRef` wraps the oracle's chain loop with it the way tests/test_gpu_timestamps.py::Ref wraps the
timestamp processor; `reference_scores` extends tests/scores_ref.py the same way."""
import torch

from helpers import MedusaConfig, GenParams, synth, ACCEPT_TYPICAL, ACCEPT_GREEDY  # noqa: F401  (also puts the package on sys.path)
from oracle.whisper_medusa_oracle import Oracle, process_logits, evaluate_posterior_chain
import scores_ref as _sr


def hf_repeat(penalty=1.0, ngram=0):
    """HF's own processors in HF's order; neutral values build nothing (as _get_logits_processor does)."""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor
    procs = []
    if penalty is not None and float(penalty) != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=float(penalty)))
    if ngram:
        procs.append(NoRepeatNGramLogitsProcessor(int(ngram)))
    return procs


def hf_row(z_row, prefix, gp, cur_len=None, ts_proc=None, rules=True):
    """One raw fp32 row `z_row [V]` under `prefix` -> the processed fp32 row.  cur_len: the length the processors of gp see (the decode loop's
    shared length; None: the row's own)."""
    ids = torch.tensor([list(prefix)], dtype=torch.long)
    x = z_row[None].float().clone()
    if rules:
        for p in hf_repeat(gp.repetition_penalty, gp.no_repeat_ngram_size):
            x = p(ids, x)
    x = process_logits(x, len(prefix) if cur_len is None else cur_len, gp)
    if ts_proc is not None:
        x = ts_proc(ids, x.clone())
    return x[0]


def top2_gap(row):
    t = torch.topk(row.double(), 2).values
    return float(t[0] - t[1])


class RepRef:
    """The oracle's chain loop with HF's repetition processors per row.  Records, per emitted position, the smallest margins of the iteration
    that emitted it (top-2 logit gap over its rows, p_c against the threshold) and whether the rules changed the arg-max of the row that
    emitted it (`moved`: the unprocessed arg-max was banned or overtaken)."""

    def __init__(self, cfg, sd, sim="bf16", act="hilo"):
        self.cfg, self.orc = cfg, Oracle(cfg, sd, sim=sim, act=act)

    def rows(self, prefixes, z, gp, L, ts_proc, rules):
        return torch.stack([hf_row(z[r], pre, gp, L, ts_proc, rules) for r, pre in enumerate(prefixes)])

    def decode(self, enc, gp, rules=True):
        cfg, orc = self.cfg, self.orc
        ts_proc = _sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
        K, P, eos = cfg.medusa_num_heads, len(gp.prompt), gp.eos_token_id
        st = orc.new_state(enc)
        ids, marg, moved = list(gp.prompt), [], []

        def changed(raw_row, pre, L, tok):
            return int(torch.argmax(hf_row(raw_row, pre, gp, L, ts_proc, False))) != tok

        while True:
            L, kv = len(ids), st["kv_len"]
            if gp.vanilla:
                zr = orc.decoder_pass(st, ids[kv:L], kv, disable_medusa=True, last_only=True)[:, 0]
                st["kv_len"] = L
                z = self.rows([ids], zr, gp, L, ts_proc, rules)
                tok = int(torch.argmax(z[0]))
                moved.append(changed(zr[0], ids, L, tok))
                ids.append(tok); marg.append((top2_gap(z[0]), float("inf")))
                if tok == eos or len(ids) >= gp.max_length:
                    break
                continue
            zr = orc.decoder_pass(st, ids[kv:L], kv, disable_medusa=False, last_only=True)[:, 0]
            st["kv_len"] = L
            z = self.rows([ids] * (K + 1), zr, gp, L, ts_proc, rules)          # base pass: every head row sees the committed ids
            cand = torch.argmax(z, dim=-1)
            vr = orc.decoder_pass(st, cand.tolist(), L, disable_medusa=True)[0]
            vpre = [ids + cand[: i + 1].tolist() for i in range(K + 1)]         # verify row i: its own prefix
            v = self.rows(vpre, vr, gp, L, ts_proc, rules)
            a, dbg = evaluate_posterior_chain(v, cand, gp)
            m = (min([top2_gap(r) for r in z] + [top2_gap(r) for r in v]),
                 min(((dbg["p_c"] - dbg["thr"]).abs() / dbg["thr"]).tolist()) if "p_c" in dbg else float("inf"))
            if a == 0:
                emit = [int(cand[0]), int(torch.argmax(v[0]))]
                mv = [changed(zr[0], ids, L, emit[0]), changed(vr[0], vpre[0], L, emit[1])]
                st["kv_len"] = L + 1
            else:
                emit = [int(t) for t in cand[: a + 1]]
                # c_0 is the base row's arg-max; c_j (j >= 1) was accepted on verify row j - 1, whose own arg-max the rules may have moved
                mv = [changed(zr[0], ids, L, emit[0])] + [int(torch.argmax(hf_row(vr[j - 1], vpre[j - 1], gp, L, ts_proc, False))) !=
                                                          int(torch.argmax(v[j - 1])) for j in range(1, a + 1)]
                st["kv_len"] = L + a
            ids += emit
            marg += [m] * len(emit)
            moved += mv
            L = len(ids)
            if eos in emit or L >= gp.max_length or L + K >= gp.hard_max_length:
                break
        if eos in ids[P:]:
            j = ids.index(eos, P)
            ids = ids[: j + 1] + [eos] * (len(ids) - j - 1)
        return ids, marg, moved


def repeated_ngrams(gen, g):
    """Number of g-grams of `gen` that occurred earlier in it."""
    seen, n = set(), 0
    for i in range(len(gen) - g + 1):
        t = tuple(gen[i: i + g])
        n += t in seen
        seen.add(t)
    return n


def reference_scores(orc, enc, ids, P, gp, cfg):
    """tests/scores_ref.py::reference_scores with the repetition rules: position t's row under its own prefix ids[:t] and length t."""
    ids = [int(t) for t in ids]
    T = len(ids)
    z = orc.decoder_pass(orc.new_state(enc), ids[:-1], 0, True)[0]        # [T - 1, V]: row t - 1 is the logits given ids[:t]
    ts_proc = _sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
    lp, gap = [0.0] * T, [float("inf")] * T
    for t in range(P, T):
        x = hf_row(z[t - 1], ids[:t], gp, None, ts_proc)
        lp[t] = float(torch.log_softmax(x.double(), 0)[ids[t]])
    return dict(logprobs=lp, gaps=gap)
