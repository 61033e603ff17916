"""The folded decoder LayerNorm on offset, outlier and high-gain rows, on the GPU (references: tests/fold_ref.py; the CPU side of the same
table: tests/test_fold_contract_cpu.py; DESIGN.md §2 "Domain of validity of the f16 contract").

Every synthetic checkpoint of the suite gives the decoder zero-mean rows of std ~ 2 under gains ~ 1.  Here the position table carries a DC
offset and two outlier channels and one LayerNorm channel a large gain; the engine's logits are compared with fp64 (HF LayerNorm then linear,
no rounding point), with the yardstick `UnfoldedF16` (fp16 inference that normalises before it rounds) and with the oracle in the engine's own
contract.  Micro shapes, a random encoder output through set_encoder_output (no encoder pass):
  d128      d = 128: one group of statistics partials
  d256      d = 256: two groups (the group-order sum of fold_row_stat)
  block256  Medusa-Block, d = 256: the final-LayerNorm launch writes the extra layer's operand and partials

Bounds (relative to the fp64 logit scale).  In the domain — rho = max |row mean| / row std <= 4.5, which the outlier, mixed and overflow points
satisfy, and so do the offset-8 rows (rho 4.2 - 4.3) — the f16 contract claims the yardstick's precision: engine error <= 2 x yardstick
error (both are maxima over ~10^4 sums of independent 11-bit roundings: two draws of one distribution stay within 2x, a systematically coarser rounding does not); for hi / lo the
yardstick is the hi / lo oracle's own fp64 error.  Against its own oracle the engine stays within the suite's figures (2e-3 f16, 2e-4 hi / lo:
test_gpu_act.py::test_prompt_pass_logits_in_its_contract).  Outside the domain the contract promises finite logits only; there the engine must
differ from its oracle by no more than the oracle differs from fp64 — the modelled rounding dominates, nothing worse hides under it.  For
hi / lo "its oracle" is everywhere the one that restates the fold (Oracle(fold_hilo=True)); the suite's hi / lo oracle is LayerNorm-then-operand
and does not meet the in-domain 2e-4 on the offset-8 rows (_figures)."""
import functools
import math

import pytest
import torch

import fold_ref
from helpers import MedusaConfig, check_tokens, golden_gen_params, record_table, ACCEPT_TYPICAL
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu
ACTS = [pytest.param(False, id="hilo"), pytest.param(True, id="f16")]
SHAPES = {"d128": lambda: MedusaConfig.micro(K=4), "d256": lambda: MedusaConfig.micro(K=4, d_model=256),
          "block256": lambda: MedusaConfig.micro(K=4, heads_type="medusa_block", d_model=256)}
POINTS = {p[0]: p[1:] for p in fold_ref.GPU_POINTS}
SEED = 11
T_ROWS = (1, 9, 16)               # single-tile passes: one row, an odd count, a full tile
OWN = {True: 2e-3, False: 2e-4}   # engine vs the oracle in its contract


@functools.lru_cache(maxsize=None)
def _refs(shape, point):
    """Everything the CPU computes for one (shape, point), once: checkpoint, inputs, rho, and the 16-token pass of fp64, the yardstick and the two
    contract oracles (a pass of T < 16 tokens is its first T rows: the mask is causal)."""
    cfg = SHAPES[shape]()
    sd = fold_ref.stress_state_dict(cfg, SEED, *POINTS[point])
    enc, tokens = fold_ref.stress_encoder_output(cfg), fold_ref.stress_tokens(cfg, 16)
    r = dict(cfg=cfg, sd=sd, enc=enc, tokens=tokens, rho=fold_ref.row_rho(sd, cfg, tokens))
    r["fp64"] = fold_ref.pass_logits(fold_ref.fp64_oracle(cfg, sd), enc, tokens)
    r["unfolded"] = fold_ref.pass_logits(fold_ref.UnfoldedF16(cfg, sd), enc, tokens)
    r[True] = fold_ref.pass_logits(fold_ref.contract_oracle(cfg, sd, True), enc, tokens)
    r[False] = fold_ref.pass_logits(fold_ref.contract_oracle(cfg, sd, False), enc, tokens)
    r["hilo_folded"] = fold_ref.pass_logits(fold_ref.folded_hilo_oracle(cfg, sd), enc, tokens)
    return r


@functools.lru_cache(maxsize=None)
def _engine(gpu, shape, point, f16):
    """The engine's logits [K + 1, T, V] of the passes over the first T tokens, T in T_ROWS."""
    r = _refs(shape, point)
    model = WhisperMedusaModel(r["cfg"], r["sd"], device=gpu, max_batch=1, act_fp16=f16)
    eng = model.engine
    assert bool(eng.lib.wm_build_act_fp16()) == f16
    out = {}
    for T in T_ROWS:
        eng.set_encoder_output(r["enc"][None])
        out[T] = eng.forward_logits([r["tokens"][:T]], 0, False)[:, 0]
    eng.close()
    return out


def _figures(gpu, shape, point, f16, T):
    """(engine vs fp64, yardstick vs fp64, own oracle vs fp64, engine vs own oracle), rows 0 .. T - 1, relative to the fp64 logit scale"""
    r = _refs(shape, point)
    z = _engine(gpu, shape, point, f16)[T]
    ref = r["fp64"][:, :T]
    e_truth, scale = fold_ref.rel_err(z, ref)
    yard = fold_ref.rel_err(r["unfolded" if f16 else "hilo_folded"][:, :T], ref)[0]
    # own oracle: f16 the suite's; hi / lo the one that restates the fold (Oracle(fold_hilo=True)).  The suite's hi / lo oracle (LayerNorm, then the
    # operand) misses the 2e-4 of the in-domain check on an offset row: block256, offset 8, 1 row: 4.8e-4 (9 and 16 rows: 4.2e-4) on an MI355X —
    # differences of ~1e-5 in front of the K/V rows' bf16 rounding.  Its distance is printed next to the asserted one.
    o = r[True] if f16 else r["hilo_folded"]
    if not f16:
        print(f"    engine vs the suite's hi / lo oracle (not asserted): {float((z.double() - r[False][:, :T].double()).abs().max()) / scale:.2e}")
    own = fold_ref.rel_err(o[:, :T], ref)[0]
    e_own = float((z.double() - o[:, :T].double()).abs().max()) / scale if math.isfinite(e_truth) else float("inf")
    return e_truth, yard, own, e_own


@pytest.mark.parametrize("f16", ACTS)
@pytest.mark.parametrize("point", list(POINTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_logits_against_fp64_by_domain(gpu, shape, point, f16):
    rho = _refs(shape, point)["rho"]
    act = "f16" if f16 else "hilo"
    for T in T_ROWS:
        e_truth, yard, own, e_own = _figures(gpu, shape, point, f16, T)
        print(f"fold contract {shape} {point} {act} T={T}: rho {rho:.2f}  engine-fp64 {e_truth:.2e}  yardstick-fp64 {yard:.2e}  "
              f"oracle-fp64 {own:.2e}  engine-oracle {e_own:.2e}")
        assert math.isfinite(e_truth) and math.isfinite(yard) and math.isfinite(own)
        if rho <= fold_ref.RHO_DOMAIN:
            assert e_truth <= 2.0 * yard, (shape, point, act, T, e_truth, yard)
            assert e_own <= OWN[f16], (shape, point, act, T, e_own)
        else:
            assert e_own <= own, (shape, point, act, T, e_own, own)
        if T == 16:
            record_table(f"fold contract {shape} {point} {act} (16 rows)", rho=round(rho, 2), engine_vs_fp64=float(f"{e_truth:.3g}"),
                         yardstick_vs_fp64=float(f"{yard:.3g}"), oracle_vs_fp64=float(f"{own:.3g}"), engine_vs_oracle=float(f"{e_own:.3g}"))


def test_domain_selection_covers_both_sides():
    """rho selects the branch above: the offsets of 32 and 128 are outside on every shape; control / outlier / mixed / overflow and the offset of 8
    — a row with a real mean, rho > 4 — inside."""
    for shape in SHAPES:
        assert 4.0 < _refs(shape, "small offset")["rho"] <= fold_ref.RHO_DOMAIN, shape
        for p in ("control", "small offset", "outlier", "mixed", fold_ref.OVERFLOW):
            assert _refs(shape, p)["rho"] <= fold_ref.RHO_DOMAIN, (shape, p)
        assert 10 < _refs(shape, "medium offset")["rho"] < 25 and 40 < _refs(shape, "large offset")["rho"] < 100, shape


@pytest.mark.parametrize("f16", ACTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_overflow_point_is_finite_and_accurate(gpu, shape, f16):
    """gamma o x = 33 x 3000 leaves fp16's range; the operand is written with gamma 2^-s and rstd carries 2^s (csrc/wm_common.h FoldIn), so the
    logits are finite and as close to fp64 as fp16 inference that normalises first."""
    r = _refs(shape, fold_ref.OVERFLOW)
    g = r["sd"][fold_ref.DEC + ".layers.0.self_attn_layer_norm.weight"]
    assert float((g * r["sd"][fold_ref.DEC + ".embed_positions.weight"][0]).abs().max()) > 65504.0       # the point is what it says
    for T in T_ROWS:
        z = _engine(gpu, shape, fold_ref.OVERFLOW, f16)[T]
        assert bool(torch.isfinite(z).all()), (shape, f16, T)
        e_truth, yard, _, _ = _figures(gpu, shape, fold_ref.OVERFLOW, f16, T)
        assert e_truth <= 2.0 * yard, (shape, f16, T, e_truth, yard)


@pytest.mark.parametrize("f16", ACTS)
@pytest.mark.parametrize("point", ["control", "mixed"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_row_count_routes_agree_on_stressed_rows(gpu, shape, point, f16):
    """The same rows through the 16-row kernel (1 stream: 5 verify rows), the two-tile kernels (4 streams: 20 rows) and the token-tile kernels
    (8 streams: 40 rows): every stream's tokens are its single-stream run's, and the first and last stream of each batch match the oracle."""
    cfg = SHAPES[shape]()
    sd = fold_ref.stress_state_dict(cfg, SEED, *POINTS[point])
    model = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=8, act_fp16=f16)
    eng = model.engine
    enc = torch.stack([fold_ref.stress_encoder_output(cfg, seed=40 + b) for b in range(8)])
    gp = golden_gen_params(cfg, ACCEPT_TYPICAL, 12)
    alone = []
    for b in range(8):
        eng.set_encoder_output(enc[b: b + 1])
        alone.append(eng.decode(gp, 1)[0])
    # (control: the streams differ.  mixed: the outlier channels sit in the POSITION table, so every stream says the same — the rows still take
    # the three routes with |gamma o x| ~ 8000 in the operand)
    assert point != "control" or len({tuple(a) for a in alone}) > 1
    for B in (1, 4, 8):
        eng.set_encoder_output(enc[:B])
        assert eng.decode(gp, B) == alone[:B], (shape, point, f16, B)
    eng.close()
    orc = fold_ref.contract_oracle(cfg, sd, f16)
    for b in (0, 3, 7):               # streams 0 and B - 1 of the three batches (identical to the single-stream runs, as asserted above)
        check_tokens(orc, enc[b], gp, alone[b], label=f"fold {shape} {point} act={'f16' if f16 else 'hilo'} b={b}")
