"""Helpers of the long-history tests (tests/test_long_history_cpu.py, tests/test_gpu_long_history.py; no test in here).

The micro shape with Whisper's own target length, n_tgt = 448 (cache rows Tal = 480): the smallest shape at which wave 0 of the self-attention
kernel (csrc/wm_decoder.hip k_attn_mfma<CROSS=false>) runs four 32-key steps (keys 0, 128, 256, 384), i.e. prefetches, alternates its two register
sets and rescales the running softmax.

(i)   checkpoint(): synth.synth_state_dict with the decoder's SELF-attention q_proj scaled by SHARPEN.  With the plain synthetic weights the softmax
      over 400 keys is nearly flat and a kernel that drops a key moves the logits by less than the project's logits tolerance.
(ii)  the teacher-forced walk: 448 fixed ids in tiles, through the oracle (the GPU test walks the same tiles through wm_forward_logits).
(iii) MutantOracle: the oracle with one of three deliberate faults in the masked (self-attention) `_attend` calls; the CPU test proves with them that
      the GPU test's bounds can fail.
(iv)  decode_with_margins(): the oracle's chain loop restated with every decision's margin; DECODE_RUNS: the (checkpoint seed, clip) of the decode
      runs to the length limit, chosen on these margins."""
import torch

from helpers import MedusaConfig, GenParams, synth, clip_for, ACCEPT_TYPICAL, ACCEPT_GREEDY  # noqa: F401
from oracle.whisper_medusa_oracle import Oracle, log_mel, process_logits, evaluate_posterior_chain

N_TGT = 448
SHARPEN = 4.0
WALK_SEED, WALK_CLIP = 51, 2
MAX_D, MEAN_D = 6e-2, 4e-3          # the decoder-logits contract (header of tests/test_gpu_parity.py)
TOL_LOGIT, TOL_REL_P = 5e-4, 2e-3   # the tie tolerances of helpers.check_tokens / Oracle.decode_following
EXP_DECAY = (6, 1.05)               # finite in fp32 up to position 448 (1.05^440 = 2.1e9; the golden recipe's 1.3 overflows before 300)
HEADS = ["base_head", "medusa_block"]


def cfg_for(heads, **kw):
    return MedusaConfig.micro(K=4, heads_type=heads, n_tgt=N_TGT, **kw)


def sharpen(cfg, sd, factor=SHARPEN):
    """Scales the self-attention q_proj (weight and bias) of every decoder layer, and of the Medusa block, in place."""
    ps = [f"whisper_model.model.decoder.layers.{i}.self_attn.q_proj" for i in range(cfg.decoder_layers)]
    if cfg.is_block:
        ps.append("medusa_block.self_attn.q_proj")
    for p in ps:
        sd[p + ".weight"] = sd[p + ".weight"] * factor         # (x 4: exact in bf16)
        sd[p + ".bias"] = sd[p + ".bias"] * factor
    return sd


def checkpoint(heads, seed=WALK_SEED, cfg=None):
    cfg = cfg or cfg_for(heads)
    return cfg, sharpen(cfg, synth.synth_state_dict(cfg, seed=seed))


def features(cfg, clip):
    return torch.from_numpy(log_mel(clip_for(cfg, clip), cfg.num_mel_bins, cfg.n_mel_frames * 160))


def walk_ids(n=N_TGT, seed=7):
    return torch.randint(10, 1000, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def tiles_aligned(n=N_TGT):
    return [(p, min(16, n - p)) for p in range(0, n, 16)]


RAGGED = (16, 5, 11, 16, 1, 15, 7)


def tiles_ragged(n=N_TGT):
    """(pos0, T) with T cycling through RAGGED: pos0 is no multiple of 16 and single tiles straddle 128, 256 and 384."""
    out, p, i = [], 0, 0
    while p < n:
        t = min(RAGGED[i % len(RAGGED)], n - p)
        out.append((p, t))
        p, i = p + t, i + 1
    return out


@torch.no_grad()
def oracle_walk(orc, enc, ids, tiles, disable_medusa=False):
    """Teacher-forced walk: one decoder_pass per tile, the cache length advanced after each.  Returns the logits [heads, len(ids), V]."""
    st = orc.new_state(enc)
    out = []
    for pos0, T in tiles:
        assert st["kv_len"] == pos0
        out.append(orc.decoder_pass(st, ids[pos0: pos0 + T], pos0, disable_medusa))
        st["kv_len"] = pos0 + T
    return torch.cat(out, dim=1)


def tile_stats(d, tiles):
    """|d| [heads, N, V] -> (whole-walk max, whole-walk mean, per-tile maxima, per-tile means)."""
    mx = [float(d[:, p: p + t].max()) for p, t in tiles]
    mn = [float(d[:, p: p + t].mean()) for p, t in tiles]
    return float(d.max()), float(d.mean()), mx, mn


# ---- (iii) mutants ---------------------------------------------------------------------------------------------------------------------------
MUT_LO, MUT_HI = 128, 160           # the second 32-key step of wave 0
MUTANTS = ("dropped step", "stale step", "dropped key")


class MutantOracle(Oracle):
    """Oracle whose self-attention has one fault: "dropped step" hides keys 128..159, "stale step" reads keys 0..31 (K and V) in their place — a
    register set that was not refilled —, "dropped key" hides the single key 128.  Cross-attention (`mask is None`) is untouched."""

    def __init__(self, *a, mutant, **kw):
        super().__init__(*a, **kw)
        assert mutant in MUTANTS
        self.mutant = mutant

    def _attend(self, q, k, v, mask=None, round_p=False, dec=False):
        S = k.shape[1]
        if mask is not None and S > MUT_LO:
            hi = min(S, MUT_HI)
            if self.mutant == "stale step":
                k, v = k.clone(), v.clone()
                k[:, MUT_LO:hi] = k[:, : hi - MUT_LO]
                v[:, MUT_LO:hi] = v[:, : hi - MUT_LO]
            else:
                mask = mask.clone()
                mask[:, MUT_LO: (hi if self.mutant == "dropped step" else MUT_LO + 1)] = -float("inf")
        return super()._attend(q, k, v, mask=mask, round_p=round_p, dec=dec)


# ---- (iv) decode runs to the length limit ----------------------------------------------------------------------------------------------------
def limit_gen_params(cfg, mode, prompt=None, max_new=10 ** 6):
    """helpers.golden_gen_params with EOS suppressed, the finite length penalty and (optionally) a longer prompt."""
    prompt = list(prompt) if prompt is not None else synth.default_prompt(cfg)
    return GenParams(prompt=prompt, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id, suppress_tokens=sorted({cfg.eos_token_id, 3, 5}),
                     begin_suppress_tokens=list(cfg.begin_suppress_tokens), max_length=min(len(prompt) + max_new, cfg.max_target_positions),
                     hard_max_length=cfg.max_length, exp_decay=EXP_DECAY, accept_mode=mode, temperature=1.0 if mode == ACCEPT_TYPICAL else 0.0)


@torch.no_grad()
def decode_with_margins(orc, enc, gp, stop_below=None):
    """Oracle.decode (chain) restated with the margin of every decision that reaches the output: the top-2 margin of the processed logits behind
    every candidate that is examined (heads 0 .. a + 1) and behind every verify arg-max (exact-match: rows 0 .. a; typical: row 0 when nothing is
    accepted), and |p_c - thr| / thr of every examined candidate (typical).  A candidate behind the first rejected one is never looked at: its
    arg-max decides nothing.  Returns (ids, smallest logit margin, smallest relative p_c margin, iterations); `stop_below` = (logit, rel) ends the
    walk early (ids None) once a margin falls below it (the seed search)."""
    K = orc.cfg.medusa_num_heads
    st = orc.new_state(enc)
    ids = list(gp.prompt)
    m_logit, m_rel, n_it = float("inf"), float("inf"), 0
    greedy = gp.accept_mode == ACCEPT_GREEDY or gp.temperature == 0
    while True:
        L, kv = len(ids), st["kv_len"]
        z = process_logits(orc.decoder_pass(st, ids[kv:L], kv, disable_medusa=False, last_only=True)[:, 0], L, gp)
        st["kv_len"] = L
        cand = torch.argmax(z, dim=-1)
        v = process_logits(orc.decoder_pass(st, cand.tolist(), L, disable_medusa=True)[0], L, gp)
        a, dbg = evaluate_posterior_chain(v, cand, gp)
        n_exam = min(a + 1, K)                                   # candidates 1 .. n_exam were examined
        zt = torch.topk(z[: n_exam + 1], 2, dim=-1).values
        m_logit = min(m_logit, float((zt[:, 0] - zt[:, 1]).min()))
        vt = torch.topk(v[:n_exam] if greedy else v[:1], 2, dim=-1).values
        if greedy or a == 0:
            m_logit = min(m_logit, float((vt[:, 0] - vt[:, 1]).min()))
        if not greedy:
            m_rel = min(m_rel, float(((dbg["p_c"] - dbg["thr"]).abs() / dbg["thr"])[:n_exam].min()))
        if a == 0:
            emit = [int(cand[0]), int(torch.argmax(v[0]))]
            st["kv_len"] = L + 1
        else:
            emit = [int(t) for t in cand[: a + 1]]
            st["kv_len"] = L + a
        ids += emit
        n_it += 1
        if stop_below is not None and (m_logit < stop_below[0] or m_rel < stop_below[1]):
            return None, m_logit, m_rel, n_it
        L = len(ids)
        if (gp.eos_token_id in emit) or L >= gp.max_length or L + K >= gp.hard_max_length:
            return ids, m_logit, m_rel, n_it


# (heads type, acceptance) -> (checkpoint seed, clip): searched on the CPU (oracle sim="bf16" on its OWN encoder output, both act contracts) for
# runs whose smallest margins are >= 10 x the tie tolerances; tests/test_long_history_cpu.py asserts it and carries the figures.
DECODE_RUNS = {
    ("base_head", ACCEPT_TYPICAL): (3069, 8),
    ("base_head", ACCEPT_GREEDY): (168, 11),
    ("medusa_block", ACCEPT_TYPICAL): (322, 7),
    ("medusa_block", ACCEPT_GREEDY): (121, 5),
}
# sibling rows behind a 300-id prompt: checkpoint seed and clips at which the ORACLE counts hits (two per clip) within 30 new tokens, exact-match
SIBLING_SEED, SIBLING_CLIPS = 49, (0, 1)
