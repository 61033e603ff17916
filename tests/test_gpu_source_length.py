"""The key masks at the source length S = n_ctx: k_flash_enc (encoder self-attention) and k_attn_mfma<CROSS> (decoder cross-attention).

Both kernels walk the keys in 64-key steps of two 32-key halves; what they execute depends on S mod 64, on ceil(S / 64) and on
Spad = roundup(S, 128).  The rest of the suite runs S = 96 (no mask instruction executes) and S = 1500 (mask in the first half of the
last step), with tolerances an off-by-one mask passes (tests/test_mask_ref_cpu.py).  Here every branch runs, and the check is the
coefficient of tests/mask_ref.py: the engine's error against the fp32 oracle, projected on what a wrong mask would change.

  |c| < 0.5     for every mutant (last key invisible / first pad row visible / last half step invisible): the midpoint between
                "does not carry the bug" (0) and "carries it" (1); a condition, not a measurement.  test_mask_ref_cpu.py shows that on
                these inputs the rounding points of the engine contract alone stay within +-0.25.
  |c - c_oracle| < 0.5   the same projection of the oracle in the engine's contract, on the same inputs: the two share their rounding
                points, so this difference is the part of c that is the engine's own.
The absolute tolerances of test_gpu_parity.py (encoder 0.12 / 6e-3, logits 6e-2 / 4e-3, oracle in the process's contract) are kept.
"""
import numpy as np
import pytest
import torch

import mask_ref as M
from helpers import record_table
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu


def _fmt(c):
    return "  ".join(f"{m} {v:+.3f}" for m, v in c.items())


def _check_encoder(case, enc, clips, tag):
    """Engine encoder rows `enc[b]` of the case's clips b: coefficients against the fp32 oracle + the absolute tolerance against the bf16 one.
    Every figure is printed before anything is asserted.  Returns {mutant: [c per clip]}."""
    ob = case.bf16()
    out, fails = {m: [] for m in case.mutants}, []
    for b in clips:
        in_contract = ob.encode(torch.from_numpy(case.feats[b]))
        c, c_orc = case.enc_coefficients(enc[b], b), case.enc_coefficients(in_contract, b)
        d = (enc[b] - in_contract).abs()
        print(f"{tag} clip {b} encoder: c {_fmt(c)} | in-contract oracle {_fmt(c_orc)} | max|d| {float(d.max()):.4f} mean|d| {float(d.mean()):.5f}")
        if not (torch.isfinite(enc[b]).all() and d.max() <= 0.12 and d.mean() <= 6e-3):
            fails.append((tag, b, "absolute", float(d.max()), float(d.mean())))
        for m in case.mutants:
            out[m].append(round(c[m], 3))
            if not (abs(c[m]) < 0.5 and abs(c[m] - c_orc[m]) < 0.5):
                fails.append((tag, b, "encoder", m, c[m], c_orc[m]))
    assert not fails, fails
    return out


def _check_logits(case, eng, enc, tag, xkv_fp8=False):
    """set_encoder_output(the engine's own output) — the pad rows of the packed operand are then exactly 0: K = 0, V = bias, the "pad" mutant —
    and one 16-token pass at position 0, all heads, per stream."""
    rows = M.token_rows(case.cfg)
    eng.set_encoder_output(enc)
    z = eng.forward_logits(rows, 0, False)                                  # [K+1, 2, 16, V]
    assert z.shape == (case.cfg.medusa_num_heads + 1, 2, M.N_TOKENS, case.cfg.vocab_size) and torch.isfinite(z).all()
    ob = case.bf16(xkv_fp8=xkv_fp8)                                          # the process's decode contract (WM_ACT)
    out, fails = {m: [] for m in case.mutants}, []
    for b in range(2):
        ref, muts = case.logit_ref(enc[b], rows[b], xkv_fp8=xkv_fp8)
        in_contract = M.logits(ob, enc[b], rows[b])
        c = {m: M.bug_coefficient(z[:, b], ref, muts[m]) for m in case.mutants}
        c_orc = {m: M.bug_coefficient(in_contract, ref, muts[m]) for m in case.mutants}
        d = (z[:, b] - in_contract).abs()
        print(f"{tag} clip {b} logits: c {_fmt(c)} | in-contract oracle {_fmt(c_orc)} | max|d| {float(d.max()):.4f} mean|d| {float(d.mean()):.5f}")
        if xkv_fp8:
            ref0, muts0 = case.logit_ref(enc[b], rows[b])
            print(f"{tag} clip {b} logits against the UNQUANTISED fp32 oracle (not asserted, see test_mask_ref_cpu.py): "
                  + _fmt({m: M.bug_coefficient(z[:, b], ref0, muts0[m]) for m in case.mutants}))
        if not (d.max() <= 6e-2 and d.mean() <= 4e-3):
            fails.append((tag, b, "absolute", float(d.max()), float(d.mean())))
        for m in case.mutants:
            out[m].append(round(c[m], 3))
            if not (abs(c[m]) < 0.5 and abs(c[m] - c_orc[m]) < 0.5):
                fails.append((tag, b, "logits", m, c[m], c_orc[m]))
    assert not fails, fails
    return out


def _sweep(gpu, S):
    case = M.sweep_case(S)
    model = WhisperMedusaModel(case.cfg, case.sd, device=gpu, max_batch=2)
    eng = model.engine
    try:
        eng.encode(torch.from_numpy(case.feats).to(gpu))
        enc = eng.encoder_output(2)
        ce = _check_encoder(case, enc, (0, 1), f"S={S}")
        cl = _check_logits(case, eng, enc, f"S={S}")
        record_table(f"source length {S}: mask coefficients, [full clip, ragged clip]",
                     **{f"enc_{m}": v for m, v in ce.items()}, **{f"logits_{m}": v for m, v in cl.items()})
    finally:
        eng.close()


@pytest.mark.parametrize("S", [s for s in M.SWEEP if s != 8])
def test_source_length_sweep(gpu, S):
    _sweep(gpu, S)


@pytest.mark.parametrize("S", M.FP8_SWEEP)
def test_source_length_with_e4m3_cross_kv(gpu, S):
    """cross_kv_fp8: k_xkv_quant masks its amax by S (decoding key indices out of the V^T fragment layout) and the decode kernel reads the
    e4m3 copy (kv_load8).  Reference: the fp32 oracle of the same operation — attention over the e4m3 image — because the quantisation
    itself moves the logits along the "pad" direction by more than a key at S = 1500 (test_mask_ref_cpu.py)."""
    case = M.sweep_case(S)
    model = WhisperMedusaModel(case.cfg, case.sd, device=gpu, max_batch=2, cross_kv_fp8=True)
    eng = model.engine
    try:
        eng.encode(torch.from_numpy(case.feats).to(gpu))
        enc = eng.encoder_output(2)
        cl = _check_logits(case, eng, enc, f"e4m3 S={S}", xkv_fp8=True)
        record_table(f"source length {S}, e4m3 cross-K/V: mask coefficients, [full clip, ragged clip]", **{f"logits_{m}": v for m, v in cl.items()})
    finally:
        eng.close()


# wm_enc_encode's dispatch (csrc/wm_encoder.hip), with M = B * Spad token rows, H heads, d = 64 H:
#   flash attention:  B * (Spad / 128) * H >= 256 and Spad % 256 == 0 -> k_flash_enc<4>;  else  B * (Spad / 128) * H < 256 -> <1>;  else <2>
#   LayerNorm:        M / 16 < 256 -> k_enc_ln_rows;  else k_enc_ln<10> (d <= 1280)
#   GEMM, N columns:  M % 256 == 0 and N % 256 == 0 and (M / 256) * (N / 256) >= 200 -> k_gemm_256p (persistent grid above 256 tiles;
#                     QKV: V's feature tiles in a sub-launch of their own, token-major)
# Two clips reach <1>, k_enc_ln_rows and the 64-row GEMM tiles only.
#   flash4_masked    d 128, S 1500: Spad 1536, H 2, B 11: 11 * 12 * 2 = 264 >= 256, 1536 % 256 == 0 -> k_flash_enc<4> with S mod 64 = 28 (masked
#                    last step); M / 16 = 1056 -> k_enc_ln<10>
#   flash2_one_key   d 256, S 257: Spad 384 (127 pad rows), H 4, B 22: 22 * 3 * 4 = 264 >= 256 but 384 % 256 != 0 -> k_flash_enc<2>, its last
#                    step holding ONE valid key
#   gemm256p         d 256, S 1500: B 12: M / 256 = 72; QKV N = 768: 72 * 3 = 216 >= 200 (one tile per block, V sub-launch); FC1 N = 1024:
#                    72 * 4 = 288 > 256 (persistent grid).  Ran at large-v2 only before.
@pytest.mark.parametrize("tag", list(M.VARIANTS))
def test_encoder_kernel_variants(gpu, tag):
    """One clip at index 0 and again at the last index: within one launch configuration a row's result cannot depend on its position, so the
    two encoder outputs are bit-equal.  Then the coefficient test on that clip and on the ragged one."""
    d, S, B = M.VARIANTS[tag]
    case = M.variant_case(tag)
    cfg = case.cfg
    H, Spad = cfg.n_heads, -(-S // 128) * 128
    blocks = B * (Spad // 128) * H
    assert blocks >= 256 and (B * Spad) // 16 >= 256                        # the arithmetic above, so that a retuned config is noticed here
    if tag == "flash2_one_key":
        assert Spad % 256 != 0 and S % 64 == 1 and Spad - S == 127
    else:
        assert Spad % 256 == 0 and 0 < S % 64 < 32
    if tag == "gemm256p":
        tm = B * Spad // 256
        assert (B * Spad) % 256 == 0 and 200 <= tm * (3 * d // 256) <= 256 < tm * (cfg.encoder_ffn_dim // 256)
    model = WhisperMedusaModel(cfg, case.sd, device=gpu, max_batch=B)
    eng = model.engine
    try:
        eng.encode(torch.from_numpy(M.variant_batch(case, B)).to(gpu))
        enc = eng.encoder_output(B)
        assert torch.isfinite(enc).all()
        same = torch.equal(enc[0], enc[B - 1])
        print(f"{tag}: clip at index 0 and at index {B - 1} bit-equal: {same}"
              + ("" if same else f" (max |d| {float((enc[0] - enc[B - 1]).abs().max()):.5f})"))
        ce = _check_encoder(case, enc, (0, 1), tag)
        record_table(f"encoder variant {tag} (d {d}, S {S}, {B} clips): mask coefficients, [full clip, ragged clip]", **{f"enc_{m}": v for m, v in ce.items()})
        assert same
    finally:
        eng.close()


def test_shortest_source_length(gpu):
    """n_ctx = 8, the smallest wm_create accepts: one step, mask in its first half, 120 pad rows."""
    _sweep(gpu, 8)
