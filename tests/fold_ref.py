"""References for the folded decoder LayerNorm on rows no synthetic checkpoint produces (DESIGN.md §2 "Domain of validity of the f16 contract").

The decoder folds LayerNorm into the GEMM it feeds (csrc/wm_common.h): the GEMM operand is the RAW row gamma o x, rounded to the contract's
operand format, and the row statistics (one fp32 pass, var = E[x^2] - mean^2) are applied to the product.  `synth.synth_state_dict` only makes
rows of mean ~ 0, std ~ 2 and gains ~ 1; here the same checkpoint is stressed with a DC offset, two outlier channels and a large gain, and three
restatements are set side by side:

  truth        `fp64_oracle`: HF LayerNorm then linear in float64, no rounding point (Oracle(sim="fp32", dtype=torch.float64)); it never enters
               the folded branch of Oracle._lin_ln.
  yardstick    `UnfoldedF16`: the f16 contract with the LayerNorm NOT folded — normalise first, round the operand to fp16 afterwards — which is
               what fp16 inference of the reference does.
  contracts    Oracle(sim="bf16", act="f16" / "hilo"): the suite's oracles.  The f16 one restates the fold with the engine's rounding points; the
               hi / lo one is LayerNorm then a hi / lo operand.  `folded_hilo_oracle` restates the fold for hi / lo too (Oracle(fold_hilo=True)):
               what the engine runs on act_fp16 = 0, recorded next to the others.

python tests/fold_ref.py rewrites the CPU table of profiles/fold_contract.md."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "whisper-medusa_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from whisper_medusa import synth  # noqa: E402
from oracle.whisper_medusa_oracle import Oracle  # noqa: E402

DEC = "whisper_model.model.decoder"
OUT_CH, OUT_CH2 = 5, 77          # the two outlier channels; OUT_CH is also the high-gain channel
RHO_DOMAIN = 4.5                 # |row mean| / row std up to which the contracts are held to the yardstick: the offset-8 rows (rho 4.2 - 4.3) are inside

# (name, offset, outlier, gain): the points of the GPU tests ...
GPU_POINTS = [("control", 0, 0, 1), ("small offset", 8, 0, 1), ("medium offset", 32, 0, 1), ("large offset", 128, 0, 1),
              ("outlier", 0, 1000, 1), ("mixed", 32, 1000, 8), ("overflow", 0, 3000, 30)]
# ... and of the CPU table
CPU_POINTS = [("control", 0, 0, 1), ("small offset", 8, 0, 1), ("medium offset", 32, 0, 1), ("large offset", 128, 0, 1), ("huge offset", 512, 0, 1),
              ("outlier 100", 0, 100, 1), ("outlier", 0, 1000, 1), ("outlier 3000", 0, 3000, 1), ("mixed", 32, 1000, 8), ("overflow", 0, 3000, 30)]
OVERFLOW = "overflow"


def _bf16(x):
    return x.to(torch.bfloat16).to(torch.float32)


def stress_state_dict(cfg, seed, offset=0.0, outlier=0.0, gain=1.0):
    """synth_state_dict(cfg, seed) with the decoder's position table moved by `offset` on every channel, by +outlier on channel OUT_CH and
    -0.7 outlier on channel OUT_CH2, and channel OUT_CH of every decoder LayerNorm gain (the Medusa block's three included) multiplied by
    `gain`.  A pure function of its arguments; every tensor stays bf16-representable."""
    sd = {k: v.clone() for k, v in synth.synth_state_dict(cfg, seed=seed).items()}
    pos = sd[DEC + ".embed_positions.weight"]
    pos += float(offset)
    pos[:, OUT_CH] += float(outlier)
    pos[:, OUT_CH2] -= 0.7 * float(outlier)
    sd[DEC + ".embed_positions.weight"] = _bf16(pos)
    for k in list(sd):
        if k.endswith("layer_norm.weight") and (k.startswith(DEC + ".") or k.startswith("medusa_block.")):
            w = sd[k]
            w[OUT_CH] *= float(gain)
            sd[k] = _bf16(w)
    sd["whisper_model.proj_out.weight"] = sd[DEC + ".embed_tokens.weight"]          # tied
    return sd


def stress_tokens(cfg, T):
    """T token ids of one pass from position 0: the decoder prompt, then a fixed spread of text ids."""
    ids = list(synth.default_prompt(cfg)) + [10 + (7 * i) % 900 for i in range(T)]
    return ids[:T]


def stress_encoder_output(cfg, seed=3):
    """A random bf16-representable encoder output [n_ctx, d] (engine.set_encoder_output / Oracle.new_state): no encoder pass in the way."""
    g = torch.Generator().manual_seed(seed)
    return _bf16(torch.randn(cfg.max_source_positions, cfg.d_model, generator=g))


def row_rho(sd, cfg, tokens):
    """max over the pass's rows of |mean| / std of tok_emb + pos_emb (fp64): how far the decoder's first residual rows are from zero-mean."""
    ids = torch.tensor(list(tokens), dtype=torch.long)
    h = sd[DEC + ".embed_tokens.weight"].double()[ids] + sd[DEC + ".embed_positions.weight"].double()[: len(tokens)]
    return float((h.mean(dim=1).abs() / h.std(dim=1, unbiased=False)).max())


def fp64_oracle(cfg, sd):
    return Oracle(cfg, sd, sim="fp32", dtype=torch.float64)


class UnfoldedF16(Oracle):
    """The f16 contract without the fold: LayerNorm in fp32, THEN the operand rounded to one fp16 plane."""

    def __init__(self, cfg, sd):
        super().__init__(cfg, sd, sim="bf16", act="f16")

    def _lin_ln(self, h, ln_prefix, prefix, bias=True):
        return self._lin(self._ln(h, ln_prefix), prefix, bias=bias, dec=True)


def contract_oracle(cfg, sd, f16):
    return Oracle(cfg, sd, sim="bf16", act="f16" if f16 else "hilo")


def folded_hilo_oracle(cfg, sd):
    return Oracle(cfg, sd, sim="bf16", act="hilo", fold_hilo=True)


@torch.no_grad()
def pass_logits(orc, enc, tokens):
    """All heads' logits [K + 1, T, V] of one pass over `tokens` from position 0."""
    return orc.decoder_pass(orc.new_state(enc), list(tokens), 0, disable_medusa=False)


def rel_err(z, ref):
    """max |z - ref| / max |ref| (inf for a non-finite z), and the scale."""
    scale = float(ref.abs().max())
    z = z.detach().cpu().double()
    if not bool(torch.isfinite(z).all()):
        return float("inf"), scale
    return float((z - ref.double()).abs().max()) / scale, scale


@torch.no_grad()
def cpu_table(cfg, seed=11, T=7, points=CPU_POINTS):
    """One row per stress point: rho and the three restatements' errors against fp64, relative to the logit scale."""
    enc, tokens = stress_encoder_output(cfg), stress_tokens(cfg, T)
    rows = []
    for name, off, out, gain in points:
        sd = stress_state_dict(cfg, seed, off, out, gain)
        ref = pass_logits(fp64_oracle(cfg, sd), enc, tokens)
        row = dict(name=name, offset=off, outlier=out, gain=gain, rho=row_rho(sd, cfg, tokens))
        for key, orc in (("folded_f16", contract_oracle(cfg, sd, True)), ("unfolded_f16", UnfoldedF16(cfg, sd)), ("hilo", contract_oracle(cfg, sd, False)),
                         ("hilo_folded", folded_hilo_oracle(cfg, sd))):
            row[key] = rel_err(pass_logits(orc, enc, tokens), ref)[0]
        rows.append(row)
    return rows


def format_table(rows):
    lines = ["| point | offset | outlier | gain | rho | folded f16 (the contract) | unfolded fp16 | hi / lo oracle | hi / lo, fold restated |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['name']} | {r['offset']} | {r['outlier']} | {r['gain']} | {r['rho']:.2f} | {r['folded_f16']:.1e} | {r['unfolded_f16']:.1e} | {r['hilo']:.1e} | {r['hilo_folded']:.1e} |")
    return "\n".join(lines)


CPU_BEGIN, CPU_END = "<!-- cpu table: python tests/fold_ref.py -->", "<!-- end of cpu table -->"

if __name__ == "__main__":
    from whisper_medusa.config import MedusaConfig
    table = format_table(cpu_table(MedusaConfig.micro(K=4)))
    print(table)
    path = os.path.join(ROOT, "profiles", "fold_contract.md")
    if os.path.exists(path):
        text = open(path).read()
        if CPU_BEGIN in text and CPU_END in text:
            a, b = text.index(CPU_BEGIN) + len(CPU_BEGIN), text.index(CPU_END)
            open(path, "w").write(text[:a] + "\n" + table + "\n" + text[b:])
