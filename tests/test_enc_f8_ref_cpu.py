"""The fp8 tile-kernel instrument of tests/enc_f8_ref.py, proven with the oracle alone (no GPU).

tests/test_gpu_enc_f8.py compares the engine's fp8 encoder with the in-contract oracle on the stress checkpoint under three bounds: the
standing allowances 0.35 max |d| and 2e-2 mean |d|, and 2e-2 on the mean |d| of every 16-row group.  Here, at the shape of its `f8_256`
variant (d 256, S 1500, 2 layers):
  * noise: a second correct implementation (LayerNorm in fp64: its e4m3 / bf16 codes flip elsewhere) stays within HALF of each bound;
  * faults: a wrong token or weight scale (enc_f8_ref.FAULTS) in ONE 256-row tile of ONE GEMM site of ONE layer exceeds TWICE at least one bound;
    the same faults in the cross-K/V projection exceed twice the cross_kv bound (0.07 max);
  * the same faults on the plain synthetic checkpoint are printed, not asserted: most of them pass the bounds, which is why the stress
    checkpoint exists (profiles/enc_f8_tiles.md keeps the table);
  * the stress checkpoint is a fair input: finite, O(1) activations, stored cross K/V below 16 (one bf16 step inside the absolute bound).
The dispatch arithmetic of every variant is asserted too, so that a retuned threshold is noticed without a GPU.
"""
import pytest
import torch

import enc_f8_ref as E
from oracle.whisper_medusa_oracle import Oracle

TAG = "f8_256"


@pytest.fixture(scope="module")
def ref():
    """Clip A and the ragged clip B of the f8_256 case with their clean in-contract encoder outputs, computed once and never modified."""
    c = E.case(TAG)
    feats = [torch.from_numpy(c.feats[i]) for i in (0, 1)]
    orc, plain = c.oracle(), c.oracle(plain=True)
    return dict(case=c, feats=feats, clean=[orc.encode(f) for f in feats], clean_plain=plain.encode(feats[0]))


@pytest.mark.parametrize("tag", list(E.VARIANTS))
def test_variants_reach_the_kernels_they_name(tag):
    d, S, enc_layers, dec_layers, B, kernel, qt = E.VARIANTS[tag]
    cfg = E.variant_config(tag)
    assert (cfg.d_model, cfg.max_source_positions, cfg.encoder_layers, cfg.decoder_layers) == (d, S, enc_layers, dec_layers)
    sites = E.gemm_sites(cfg, B)
    assert {s: E.f8_kernel(*mn) for s, mn in sites.items()} == {"qkv": kernel, "fc1": kernel, "cross_kv": kernel}
    assert E.flash_variant(B, E.spad(S), cfg.n_heads) == qt
    M = B * E.spad(S)
    if tag == "f8_256":
        assert M == 19968 and M // 256 == 78
        assert [78 * (n // 256) for _, n in sites.values()] == [234, 312, 312] and 234 % 8 == 2          # uneven XCD shares
        assert [E.gemm256_strip(n // 256) for _, n in sites.values()] == [3, 4, 4]                        # one strip each
    if tag == "f8_256_strips":
        assert sites["cross_kv"] == (18432, 3072) and E.gemm256_strip(12) == 6                            # two strips of 6 column tiles
        assert [72 * (n // 256) for _, n in sites.values()] == [216, 288, 864]
    if tag == "f8_64_deepk":
        assert M == 256 and d // 128 == 4 and max((M // 128) * (n // 128) for _, n in sites.values()) == 32
    if tag == "f8_128_deepk":
        assert M == 3072 and d // 128 == 4
        assert [(M // 256) * (n // 256) for _, n in sites.values()] == [72, 96, 96]
        assert [(M // 128) * (n // 128) for _, n in sites.values()] == [288, 384, 384]


def test_dispatch_thresholds():
    assert E.f8_kernel(256 * 50, 1024) == "256" and E.f8_kernel(256 * 49, 1024) == "128x2"               # 200 / 196 tiles of 256 x 256
    assert E.f8_kernel(128 * 25, 1024) == "128x2" and E.f8_kernel(128 * 24, 1024) == "64x3"              # 200 / 192 tiles of 128 x 128
    assert E.f8_kernel(256 * 80 + 128, 1024) == "128x2"                                                   # M not a multiple of 256
    assert [E.gemm256_strip(n) for n in (1, 3, 4, 12, 15, 20, 60)] == [1, 3, 4, 6, 5, 5, 6]
    assert [E.flash_variant(*a) for a in ((1, 1536, 20), (2, 1536, 8), (22, 384, 4), (11, 1536, 2))] == [1, 1, 2, 4]


def test_stress_checkpoint_spreads_the_scales_and_stays_fair(ref):
    c = ref["case"]
    for k, v in c.sd.items():
        assert v.shape == c.plain[k].shape and torch.equal(v, v.to(torch.bfloat16).to(torch.float32)), k
    changed = sorted(k for k in c.sd if not torch.equal(c.sd[k], c.plain[k]))
    assert len(changed) == 1 + 7 * c.cfg.encoder_layers + 3 * c.cfg.n_kv_layers, changed        # positions; q w b, k w, v w b, fc1 w b; cross k w, v w b
    g = E.row_gains(768)
    assert abs(float(g.pow(2).mean()) - 1.0) < 1e-6
    quad = g.view(-1, 4)
    assert float((quad.amax(1) / quad.amin(1)).median()) >= 2.0                 # inside a lane's 4 features
    tile = g.view(-1, 16)
    assert not any(torch.equal(tile[i], tile[i + 1]) for i in range(tile.shape[0] - 1))    # from one 16-feature tile to the next
    o32 = Oracle(c.cfg, c.sd, sim="fp32")
    out = o32.encode(ref["feats"][0])
    mean_abs = float(out.abs().mean())
    print(f"stress checkpoint, fp32 oracle: encoder output mean|x| {mean_abs:.3f} max|x| {float(out.abs().max()):.2f}")
    assert torch.isfinite(out).all() and 0.3 <= mean_abs <= 1.5
    assert all(torch.isfinite(x).all() for x in ref["clean"])
    # token scales of the final LayerNorm (the cross-K/V operand): a row against its neighbour, and against the row a 16-row group further on
    xs = out.abs().amax(dim=1)
    near, far = (xs[1:] / xs[:-1]).log2().abs().median(), (xs[16:] / xs[:-16]).log2().abs().median()
    print(f"max|row| of the final LayerNorm: {float(xs.min()):.2f} .. {float(xs.max()):.2f}; median factor to the next row {2 ** float(near):.2f},"
          f" to row + 16 {2 ** float(far):.2f}")
    assert float(xs.max() / xs.min()) >= 3.0 and float(near) >= 0.5 and float(far) >= 0.5       # typically sqrt(2) or more apart


def test_rounding_point_noise_stays_within_half_of_every_bound(ref):
    c = ref["case"]
    noisy = c.oracle(ln64=True)
    for i, name in enumerate("AB"):
        mx, mean, grp, at = E.figures(noisy.encode(ref["feats"][i]), ref["clean"][i])
        print(f"noise (LayerNorm in fp64), clip {name}: max|d| {mx:.4f} mean|d| {mean:.5f} worst 16-row group {grp:.5f} (group {at})")
        assert mx <= E.ENC_MAX / 2 and mean <= E.ENC_MEAN / 2 and grp <= E.ENC_GROUP_MEAN / 2, (name, mx, mean, grp)


def _exceeds_twice(mx, mean, grp):
    return mx > 2 * E.ENC_MAX or mean > 2 * E.ENC_MEAN or grp > 2 * E.ENC_GROUP_MEAN


@pytest.mark.parametrize("layer", ["first", "last"])
@pytest.mark.parametrize("site", E.ENC_SITES)
@pytest.mark.parametrize("fault", E.FAULTS)
def test_one_tile_fault_exceeds_twice_a_bound_on_the_stress_checkpoint(ref, fault, site, layer):
    c = ref["case"]
    where = f"layers.{0 if layer == 'first' else c.cfg.encoder_layers - 1}.{site}"
    f = ref["feats"][0]
    bad_plain = c.oracle(plain=True, fault=fault, site=where)
    p = E.figures(bad_plain.encode(f), ref["clean_plain"])
    bad = c.oracle(fault=fault, site=where)
    s = E.figures(bad.encode(f), ref["clean"][0])
    assert bad.faulted == 1 and bad_plain.faulted == 1
    print(f"fault {fault} at {where} rows {E.TILE_ROWS}: plain checkpoint max|d| {p[0]:.3f} mean|d| {p[1]:.4f} group {p[2]:.3f}"
          f" ({'caught' if p[0] > E.ENC_MAX or p[1] > E.ENC_MEAN else 'PASSES 0.35 / 2e-2'}) | stress checkpoint max|d| {s[0]:.3f} mean|d| {s[1]:.4f}"
          f" group {s[2]:.3f} (group {s[3]})")
    assert _exceeds_twice(*s[:3]), (fault, where, s)


@pytest.mark.parametrize("fault", E.FAULTS)
def test_one_tile_fault_in_the_cross_kv_projection_exceeds_twice_its_bound(ref, fault):
    c = ref["case"]
    for plain in (True, False):
        enc = ref["clean_plain"] if plain else ref["clean"][0]
        ok = c.oracle(plain=plain).cross_kv(enc)
        bad = c.oracle(plain=plain, fault=fault, site=E.CROSS_KV)
        mx, mean = E.kv_figures(bad.cross_kv(enc), ok)
        assert bad.faulted == 2 * c.cfg.n_kv_layers
        print(f"fault {fault} in the cross-K/V projection rows {E.TILE_ROWS}, {'plain' if plain else 'stress'} checkpoint: max|d| {mx:.3f}"
              f" worst slab mean|d| {mean:.4f}")
        if not plain:
            assert mx > 2 * E.KV_MAX, (fault, mx, mean)


@pytest.mark.parametrize("tag", list(E.VARIANTS))
def test_stored_cross_kv_stays_where_one_bf16_step_is_inside_its_bound(tag):
    """The cross_kv bound is absolute (0.07 max): it can only hold where a single bf16 rounding flip of a stored value is smaller, |value| < 16.
    A condition on the stress checkpoint and the clips, checked with the oracle for every variant's shape."""
    c = E.case(tag)
    orc = c.oracle()
    for i, name in enumerate("ABC"):
        kv = orc.cross_kv(orc.encode(torch.from_numpy(c.feats[i])))
        top = max(float(max(k.abs().max(), v.abs().max())) for k, v in kv)
        print(f"{tag} clip {name}: largest stored cross K / V value {top:.2f}")
        assert top < E.KV_BF16_STEP_BELOW, (tag, name, top)
