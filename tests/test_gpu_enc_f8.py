"""Every fp8 encoder GEMM tile kernel behind launch_gemm_f8 (csrc/wm_encoder.hip) on a checkpoint where a wrong dequantisation scale shows.

k_gemm_f8k<64, 3>, k_gemm_f8k<128, 2>, k_gemm_f8k_256 and its WM_F8_STAGGER sibling k_gemm_f8k_256s are dequantised with one scale per token
row and one per weight row.  On a plain synthetic checkpoint all those scales are alike and a kernel that takes the scale of the wrong row,
16-row group or feature stays inside the fp8 allowances; tests/enc_f8_ref.py builds the stress checkpoint on which it does not, and
tests/test_enc_f8_ref_cpu.py proves the margins with the oracle alone (noise <= half of every bound, every one-tile fault >= twice one).

Per variant (enc_f8_ref.VARIANTS: shapes and dispatch arithmetic), one engine:
  * three distinct clips A (full), B (ragged), C (full) fill the batch with period 3; a second pass holds the arrangement reversed.  Every copy
    of a clip, in both passes, is BIT-EQUAL to its first copy, encoder output and cross-K/V: within one launch configuration a row's result
    cannot depend on its index.  At 12 / 13 clips that covers every row tile, both XCD share sizes and every strip without an oracle run per
    index; the two-clip variants hold A and B only, and the comparison there is one moved copy of each (A 0 -> 1, B 1 -> 0).
  * the first copies against Oracle(sim="bf16", enc_fp8=True): max |d| <= 0.35, mean |d| <= 2e-2 (the standing allowances of
    test_gpu_parity.py::test_fp8_mfma_encoder_matches_the_fp8_oracle) and mean |d| of EVERY 16-row group <= 2e-2 (the same allowance where a
    one-tile fault cannot dilute);
  * cross K/V of every kv layer and head against the oracle's projection of the ENGINE's stored encoder output (identical e4m3 codes on both
    sides): 0.07 max, 2e-3 mean, the bounds of the same test.
Every figure is printed before anything is asserted.
"""
import time

import pytest
import torch

import enc_f8_ref as E
from helpers import record_table
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu

NAMES = "ABC"


def _assert_dispatch(c):
    d, S, _, _, B, kernel, qt = E.VARIANTS[c.tag]
    sites = E.gemm_sites(c.cfg, B)
    assert {s: E.f8_kernel(*mn) for s, mn in sites.items()} == dict.fromkeys(sites, kernel), sites
    assert E.flash_variant(B, E.spad(S), c.cfg.n_heads) == qt
    if c.tag == "f8_256":
        assert ((sites["qkv"][0] // 256) * (sites["qkv"][1] // 256)) % 8 == 2        # XCDs 0, 1 take one tile more than the others
    if c.tag == "f8_256_strips":
        tn = sites["cross_kv"][1] // 256
        assert tn // E.gemm256_strip(tn) == 2                                         # two strips
    if kernel != "256":
        assert d // 128 == 4                                                          # K128 = 4: more steps than ring stages


def _all_kv(eng, cfg, B):
    """[B][kv layer] -> (K [H, S, 64], V [H, S, 64]) of the resident encoder pass."""
    out = []
    for b in range(B):
        per = []
        for layer in range(cfg.n_kv_layers):
            kv = [eng.cross_kv(layer, b, h) for h in range(cfg.n_heads)]
            per.append((torch.stack([k for k, _ in kv]), torch.stack([v for _, v in kv])))
        out.append(per)
    return out


def _two_passes(eng, c, gpu):
    """[(clip id, pass, index, encoder output [S, d], cross K/V per layer)] of the period-3 batch and of the reversed one."""
    seen = []
    for p, rev in enumerate((False, True)):
        eng.encode(torch.from_numpy(c.batch(rev)).to(gpu))
        enc, kv = eng.encoder_output(c.B), _all_kv(eng, c.cfg, c.B)
        assert torch.isfinite(enc).all()
        seen += [(clip, p, i, enc[i], kv[i]) for i, clip in enumerate(c.order(rev))]
    return seen


def _first_copies(seen):
    first = {}
    for s in seen:
        first.setdefault(s[0], s)
    return first


def _position_equality(seen, tag):
    """Every copy bit-equal to the first copy of its clip; returns the number of copies compared."""
    first, differ, n = _first_copies(seen), [], 0
    for clip, p, i, enc, kv in seen:
        _, p0, i0, enc0, kv0 = first[clip]
        if (p, i) == (p0, i0):
            continue
        n += 1
        if not torch.equal(enc, enc0):
            rows = (enc != enc0).any(dim=1).nonzero().flatten()
            differ.append((NAMES[clip], f"pass {p} index {i}", "encoder", f"{len(rows)} rows from {int(rows[0])}", float((enc - enc0).abs().max())))
        for layer, ((k, v), (k0, v0)) in enumerate(zip(kv, kv0)):
            if not (torch.equal(k, k0) and torch.equal(v, v0)):
                differ.append((NAMES[clip], f"pass {p} index {i}", f"cross_kv layer {layer}", float(max((k - k0).abs().max(), (v - v0).abs().max()))))
    print(f"{tag}: {n} copies compared with the first copy of their clip; differing: {differ if differ else 'none'}")
    assert n >= 1
    return differ


def _against_the_oracle(c, first, tag, enc_bounds):
    """First copies against the in-contract oracle: ({clip: (max, mean, worst group, its index)}, {clip: (kv max, kv mean)}, failures)."""
    orc = c.oracle()
    enc_fig, kv_fig, fails = {}, {}, []
    for clip in sorted(first):
        _, p, i, enc, kv = first[clip]
        ref = orc.encode(torch.from_numpy(c.feats[clip]))
        mx, mean, grp, at = E.figures(enc, ref)
        print(f"{tag} clip {NAMES[clip]} (pass {p} index {i}) encoder vs fp8 oracle: max|d| {mx:.4f} mean|d| {mean:.5f} worst 16-row group {grp:.5f}"
              f" (group {at}, rows {16 * at}..) |ref| mean {float(ref.abs().mean()):.3f}")
        enc_fig[NAMES[clip]] = (round(mx, 4), round(mean, 5), round(grp, 5), at)
        if not (mx <= enc_bounds[0] and mean <= enc_bounds[1] and grp <= enc_bounds[2]):
            fails.append((tag, NAMES[clip], "encoder", mx, mean, grp, at))
        ref_kv = orc.cross_kv(enc)
        assert max(float(max(k.abs().max(), v.abs().max())) for k, v in ref_kv) < E.KV_BF16_STEP_BELOW      # one bf16 step <= 0.0625: inside the bound
        kmx, kmean = E.kv_figures(kv, ref_kv)
        print(f"{tag} clip {NAMES[clip]} cross K/V, {c.cfg.n_kv_layers} layers x {c.cfg.n_heads} heads: max|d| {kmx:.4f} worst slab mean|d| {kmean:.5f}")
        kv_fig[NAMES[clip]] = (round(kmx, 4), round(kmean, 5))
        if not (kmx <= E.KV_MAX and kmean <= E.KV_MEAN):
            fails.append((tag, NAMES[clip], "cross_kv", kmx, kmean))
    return enc_fig, kv_fig, fails


def _run(gpu, tag, enc_bounds):
    c = E.case(tag)
    _assert_dispatch(c)
    t0 = time.perf_counter()
    model = WhisperMedusaModel(c.cfg, c.sd, device=gpu, max_batch=c.B, enc_fp8=True)
    eng = model.engine
    try:
        seen = _two_passes(eng, c, gpu)
    finally:
        eng.close()
    differ = _position_equality(seen, tag)
    enc_fig, kv_fig, fails = _against_the_oracle(c, _first_copies(seen), tag, enc_bounds)
    d, S, el, dl, B, kernel, _ = E.VARIANTS[tag]
    record_table(f"fp8 tile kernel {kernel} ({tag}: d {d}, S {S}, {el} + {dl} layers, {B} clips) on the stress checkpoint: [max, mean, worst 16-row group, group]",
                 **{f"enc_{k}": v for k, v in enc_fig.items()}, **{f"kv_{k}": v for k, v in kv_fig.items()}, copies_differing=len(differ),
                 seconds=round(time.perf_counter() - t0, 1))
    assert not differ, differ
    assert not fails, fails


@pytest.mark.parametrize("tag", ["f8_256", "f8_64_deepk", "f8_128_deepk"])
def test_fp8_tile_kernels_on_the_stress_checkpoint(gpu, tag):
    _run(gpu, tag, (E.ENC_MAX, E.ENC_MEAN, E.ENC_GROUP_MEAN))


def test_fp8_cross_kv_projection_in_two_strips(gpu):
    """Six decoder layers at d 256: the fused cross-K/V projection has 12 column tiles, walked as two strips of 6 (sb > 0 in the tile order of
    k_gemm_f8k_256), as at large-v2.  Position equality and cross_kv over all 6 kv layers x 4 heads; the encoder itself has one layer here and
    its comparison is the same three bounds as a sanity check."""
    _run(gpu, "f8_256_strips", (E.ENC_MAX, E.ENC_MEAN, E.ENC_GROUP_MEAN))


def test_fp8_staggered_256_kernel_is_bit_equal(gpu, monkeypatch):
    """WM_F8_STAGGER=1 (read per launch in launch_gemm_f8) swaps k_gemm_f8k_256 for k_gemm_f8k_256s: the same tiles, the two token halves of a
    block half a step apart.  Both accumulate each 16 x 16 tile over kt in order on the same MFMA, so nothing legitimate can differ.
    Bit-equality cannot tell "the staggered kernel agrees" from "the knob was not read".  That it is read rests on launch_gemm_f8
    (csrc/wm_encoder.hip): `const int stagger = [] { ... getenv("WM_F8_STAGGER") ... }();` is NOT `static` (its neighbour `use256` is), and
    wm_encode calls wm_enc_encode directly, outside any captured graph, so every launch evaluates it; monkeypatch.setenv goes through
    os.environ -> putenv, which the C getenv sees.  Should that line become `static`, this test passes vacuously: keep it per launch, or give
    the test a way to see which kernel ran."""
    c = E.case("f8_256")
    _assert_dispatch(c)
    monkeypatch.delenv("WM_F8_STAGGER", raising=False)
    feats = torch.from_numpy(c.batch()).to(gpu)
    model = WhisperMedusaModel(c.cfg, c.sd, device=gpu, max_batch=c.B, enc_fp8=True)
    eng = model.engine
    try:
        eng.encode(feats)
        enc0, kv0 = eng.encoder_output(c.B), _all_kv(eng, c.cfg, c.B)
        monkeypatch.setenv("WM_F8_STAGGER", "1")
        eng.encode(feats)
        enc1, kv1 = eng.encoder_output(c.B), _all_kv(eng, c.cfg, c.B)
    finally:
        eng.close()
    bad_enc = [i for i in range(c.B) if not torch.equal(enc0[i], enc1[i])]
    bad_kv = [(i, layer) for i in range(c.B) for layer in range(c.cfg.n_kv_layers)
              if not (torch.equal(kv0[i][layer][0], kv1[i][layer][0]) and torch.equal(kv0[i][layer][1], kv1[i][layer][1]))]
    print(f"staggered vs lock-step 256 kernel: clips whose encoder output differs {bad_enc or 'none'}"
          + (f" (max |d| {float((enc0 - enc1).abs().max()):.5f})" if bad_enc else "") + f"; (clip, kv layer) whose cross K/V differs {bad_kv or 'none'}")
    assert torch.isfinite(enc1).all()
    assert not bad_enc and not bad_kv
