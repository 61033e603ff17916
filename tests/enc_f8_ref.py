"""fp8 encoder GEMM references (CPU only; no GPU import): a checkpoint on which a wrong dequantisation scale shows, the oracle with such a
fault injected, and the dispatch of launch_gemm_f8 restated.

The fp8 MFMA encoder (enc_fp8=True) multiplies e4m3 by e4m3 in three GEMM sites — QKV, FC1 and the fused cross-K/V projection — and
dequantises in EpScaled / ep_tiles (csrc/wm_encoder.hip) with one scale per token row, xs[m], and one per weight row, ws[n].  A wave holds
16-row groups of tokens (m0 + 16 j) and, per lane, 4 consecutive features of 16-feature tiles (n0 + 16 i .. + 3).  The ways that indexing goes
wrong are modelled here as faults of the oracle's _lin8, confined to a row range (one 256-row tile):

  "xs_group"  a 16-row group is dequantised with the token scales of the NEIGHBOURING group (row m takes xs[m + 16], wrapping inside the range)
  "ws_quad"   a lane's 4 features all take the weight scale of its first one (ws[n & ~3])
  "ws_group"  a 16-feature tile takes the weight scales of the neighbouring tile (ws[n + 16], wrapping at N)

On a synth_state_dict checkpoint every LayerNorm row has max|row| of about 3.5 and every weight row the same norm, so all of these are about
10 % off and pass the standing fp8 allowances (0.35 max / 2e-2 mean).  stress_checkpoint() spreads both scale vectors over more than an
order of magnitude, between adjacent rows, adjacent 16-row groups, the 4 features of a lane and adjacent 16-feature tiles; the same faults
then exceed the allowances several times while the legitimate rounding-point noise (the `ln64` oracle: a second correct implementation whose
e4m3 / bf16 codes flip elsewhere) stays several times below them.  tests/test_enc_f8_ref_cpu.py asserts both margins with the oracle alone.
"""
import dataclasses
import functools

import numpy as np
import torch
import torch.nn.functional as F

from helpers import MedusaConfig, synth
from oracle.whisper_medusa_oracle import Oracle
import mask_ref

FAULTS = ("xs_group", "ws_quad", "ws_group")
ENC_SITES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "fc1")
CROSS_KV = "cross_kv"                       # site: encoder_attn.k_proj / v_proj of every kv layer = the rows of the fused projection
TILE_ROWS = (256, 512)                      # the second 256-row tile of a clip: what a fault is confined to
SEED = 17

# the standing fp8 allowances (tests/test_gpu_parity.py::test_fp8_mfma_encoder_matches_the_fp8_oracle); the group bound is the mean allowance
# on the 16 rows a wave dequantises with one xs, where a one-tile fault cannot dilute
ENC_MAX, ENC_MEAN, ENC_GROUP_MEAN = 0.35, 2e-2, 2e-2
KV_MAX, KV_MEAN = 0.07, 2e-3

# amplitude on row s: [s % 6].  Row s + 16 takes entry (s + 4) % 6: 0 -> 64, 48 -> 6, 10 -> 0, 3 -> 48, 64 -> 10, 6 -> 3, so a row and the one a
# 16-row group further on are never alike.  (A LayerNorm row of d values cannot exceed sqrt(d) gamma: at d = 256 the amplitudes 24 and 48 of a
# first table, (0, 6, 24, 12, 48, 3), gave max|row| 13 and 15 — a pair the xs_group fault on v_proj of the last layer then missed the factor with,
# 0.392 / 0.0197 / group 0.038; with this table it measures 0.81 / 0.024 / 0.051.)
POS_OUTLIERS = (0.0, 48.0, 10.0, 3.0, 64.0, 6.0)
ROW_GAINS = (1.0, 4.0, 0.5, 2.0, 8.0, 0.25, 1.0, 16.0)          # gain of every third output row n: [(5 n + n // 16) % 8]

CROSS_RMS = 0.5                                                 # RMS of the cross-attention k_proj / v_proj row gains (stress_checkpoint)
KV_BF16_STEP_BELOW = 16.0                                       # |stored K / V| below this: one bf16 step <= 0.0625 < KV_MAX

_ENC = "whisper_model.model.encoder"


def _bf16(x):
    return x.to(torch.bfloat16).to(torch.float32)


def row_gains(n_out, rms=1.0):
    """Gain per output row with RMS `rms`: every third row takes ROW_GAINS[(5 n + n // 16) % 8], the others 1.  5 n walks the table inside a
    lane's 4 features, n // 16 shifts it from one 16-feature tile to the next."""
    n = torch.arange(n_out)
    g = torch.ones(n_out, dtype=torch.float64)
    table = torch.tensor(ROW_GAINS, dtype=torch.float64)
    third = n % 3 == 0
    g[third] = table[((5 * n + n // 16) % 8)[third]]
    return (g * (rms / g.pow(2).mean().sqrt())).to(torch.float32)


def stress_checkpoint(cfg, sd, seed=SEED):
    """A copy of the synth_state_dict checkpoint `sd` (every tensor still bf16-representable) whose token-row scales xs[m] and weight-row
    scales ws[n] differ several-fold between neighbours:
      * encoder embed_positions row s: + POS_OUTLIERS[s % 6] (seeded sign) on one seeded channel.  The outlier rides the residual stream, so the
        LayerNorm rows in front of every fp8 GEMM (QKV, FC1, cross-K/V) have max|row| between ~2.3 and ~21 (d = 256), changing from row to row and
        — the period 6 does not divide 16 — from one 16-row group to the next;
      * q_proj / k_proj / v_proj / fc1 of every encoder layer, and the cross-attention k_proj / v_proj of every kv layer (Medusa block
        included): output row n times row_gains()[n], bias with it.  The cross-attention rows at RMS CROSS_RMS = 0.5: the final LayerNorm's
        outliers (up to 26 at d = 512) times a high-gain row put a few dozen stored K / V values per clip at 16 .. 19 with unit RMS, where
        one bf16 step is 0.125 and a single legitimate rounding flip exceeds the absolute cross_kv bound of 0.07.  At half the size every
        stored value is below 16 (one step <= 0.0625), which tests/test_enc_f8_ref_cpu.py asserts with the oracle for every variant."""
    out = {k: v.clone() for k, v in sd.items()}
    g = torch.Generator().manual_seed(seed)
    pos = out[_ENC + ".embed_positions.weight"]
    S, d = pos.shape
    ch = torch.randint(0, d, (S,), generator=g)
    sign = torch.randint(0, 2, (S,), generator=g).to(torch.float32) * 2.0 - 1.0
    amp = torch.tensor(POS_OUTLIERS)[torch.arange(S) % len(POS_OUTLIERS)]
    pos[torch.arange(S), ch] += sign * amp
    out[_ENC + ".embed_positions.weight"] = _bf16(pos)
    prefixes = [f"{_ENC}.layers.{i}.{s}" for i in range(cfg.encoder_layers) for s in ENC_SITES]
    kv = [f"whisper_model.model.decoder.layers.{i}" for i in range(cfg.decoder_layers)] + (["medusa_block"] if cfg.is_block else [])
    cross = [f"{p}.encoder_attn.{s}" for p in kv for s in ("k_proj", "v_proj")]
    for p in prefixes + cross:
        gain = row_gains(out[p + ".weight"].shape[0], CROSS_RMS if p in cross else 1.0)
        out[p + ".weight"] = _bf16(out[p + ".weight"] * gain[:, None])
        if p + ".bias" in out:
            out[p + ".bias"] = _bf16(out[p + ".bias"] * gain)
    if "whisper_model.proj_out.weight" in sd:                                   # keep the tie of synth_state_dict
        out["whisper_model.proj_out.weight"] = out["whisper_model.model.decoder.embed_tokens.weight"]
    return out


class FaultyOracle(Oracle):
    """Oracle whose fp8 linear dequantises rows `rows` = (first, end) of the GEMM site `site` with wrong scales (`fault`, one of FAULTS).
    site: the suffix of an encoder linear's prefix ("layers.1.fc1": one layer; "fc1": every layer), or CROSS_KV.  fault=None: no fault.
    ln64: LayerNorm evaluated in float64 and cast back — still a correct implementation, with its rounding points elsewhere."""

    def __init__(self, cfg, sd, fault=None, site=None, rows=TILE_ROWS, ln64=False, **kw):
        super().__init__(cfg, sd, **kw)
        assert fault is None or (fault in FAULTS and site is not None)
        self.fault, self.site, self.rows, self.ln64 = fault, site, rows, ln64
        self.faulted = 0                    # GEMMs the fault was applied to

    def _ln(self, x, prefix):
        if not self.ln64:
            return super()._ln(x, prefix)
        w, b = self.sd[prefix + ".weight"].double(), self.sd[prefix + ".bias"].double()
        return F.layer_norm(x.double(), (x.shape[-1],), w, b, 1e-5).to(torch.float32)

    def _hits(self, prefix):
        if self.fault is None:
            return False
        if self.site == CROSS_KV:
            return prefix.endswith(".encoder_attn.k_proj") or prefix.endswith(".encoder_attn.v_proj")
        return prefix.startswith(_ENC + ".") and prefix.endswith("." + self.site)

    def _lin8(self, x, prefix, bias=True):
        y = super()._lin8(x, prefix, bias=bias)
        if not self._hits(prefix):
            return y
        r0, r1 = self.rows
        assert 0 <= r0 < r1 <= x.shape[0] and (r1 - r0) % 16 == 0
        wq, ws = self.w8[prefix]
        xq, xs = self._q8_rows(x)
        xq, xs = xq[r0:r1], xs[r0:r1]
        if self.fault == "xs_group":
            xs = torch.roll(xs, -16)
        elif self.fault == "ws_quad":
            ws = ws[torch.arange(ws.shape[0]) // 4 * 4]
        else:
            ws = torch.roll(ws, -16)
        bad = ((xq @ wq.t()) * xs[:, None]) * ws[None, :]
        if bias and (prefix + ".bias") in self.sd:
            bad = bad + self.sd[prefix + ".bias"]
        y = y.clone()
        y[r0:r1] = bad
        self.faulted += 1
        return y


def figures(got, ref):
    """(max |d|, mean |d|, worst mean |d| of a 16-row group, that group's index) of two [S, d] tensors; the last group may be short."""
    d = (torch.as_tensor(got).double() - torch.as_tensor(ref).double()).abs()
    rows = d.mean(dim=1)
    groups = torch.stack([g.mean() for g in rows.split(16)])
    return float(d.max()), float(d.mean()), float(groups.max()), int(groups.argmax())


def kv_figures(got, ref):
    """(max |d|, mean |d|) over K and V of cross_kv lists [(K [H, S, 64], V [H, S, 64]) per kv layer], the mean being the worst slab's."""
    mx = mean = 0.0
    for (gk, gv), (rk, rv) in zip(got, ref):
        for a, b in ((gk, rk), (gv, rv)):
            d = (a.double() - b.double()).abs()
            mx, mean = max(mx, float(d.max())), max(mean, float(d.mean(dim=(1, 2)).max()))
    return mx, mean


# ---- launch_gemm_f8 / wm_enc_encode dispatch (csrc/wm_encoder.hip), restated ---------------------------------------------------------------
def f8_kernel(M, N):
    """The tile kernel launch_gemm_f8 picks for M token rows x N features."""
    if M % 256 == 0 and N % 256 == 0 and (M // 256) * (N // 256) >= 200:
        return "256"                        # k_gemm_f8k_256 (WM_F8_STAGGER=1: k_gemm_f8k_256s)
    if (M // 128) * (N // 128) < 200:
        return "64x3"                       # k_gemm_f8k<64, 3>
    return "128x2"                          # k_gemm_f8k<128, 2>


def gemm256_strip(tiles_n):
    """Strip width of the 256-tile order: the divisor pn <= 32 of tiles_n with the smallest 32 / pn + pn (the first such)."""
    best, best_cost = 1, 33.0
    for pn in range(1, min(tiles_n, 32) + 1):
        if tiles_n % pn == 0 and 32.0 / pn + pn < best_cost:
            best, best_cost = pn, 32.0 / pn + pn
    return best


def flash_variant(B, Spad, H):
    """QT of the k_flash_enc<QT> wm_enc_encode launches."""
    blocks = B * (Spad // 128) * H
    if blocks >= 256 and Spad % 256 == 0:
        return 4
    return 1 if blocks < 256 else 2


def spad(S):
    return -(-S // 128) * 128


def gemm_sites(cfg, B):
    """{site: (M, N)} of the three fp8 GEMM sites for B clips."""
    M, d = B * spad(cfg.max_source_positions), cfg.d_model
    return {"qkv": (M, 3 * d), "fc1": (M, cfg.encoder_ffn_dim), "cross_kv": (M, cfg.n_kv_layers * 2 * d)}


# tag -> (d_model, n_ctx, encoder layers, decoder layers, clips B, kernel of every fp8 GEMM site, k_flash_enc QT).  Spad = roundup(S, 128), M = B Spad.
VARIANTS = {
    # Spad 1536, M 19968 = 78 row tiles.  QKV N 768: 78 x 3 = 234 >= 200, 234 % 8 = 2 (XCDs 0 and 1 own 30 tiles, the others 29: `xcd < r`);
    # FC1 N 1024: 78 x 4 = 312; cross-K/V N 2 x 2 x 256 = 1024: 312.  Flash: 13 x 12 x 4 = 624 >= 256, 1536 % 256 == 0 -> <4>.  K128 = 2.
    "f8_256": (256, 1500, 2, 2, 13, "256", 4),
    # M 18432 = 72 row tiles.  QKV 72 x 3 = 216, FC1 72 x 4 = 288; cross-K/V N 6 x 2 x 256 = 3072 = 12 column tiles: 864 tiles and
    # gemm256_strip(12) = 6 (32 / 6 + 6 = 11.3 < 12 at pn 4): TWO strips, sb > 0, as at large-v2.  Flash 12 x 12 x 4 = 576 -> <4>.
    "f8_256_strips": (256, 1500, 1, 6, 12, "256", 4),
    # Spad 128, M 256.  QKV N 1536: 1 x 6 = 6 < 200 and 2 x 12 = 24 < 200 -> <64, 3>; FC1 / cross-K/V N 2048: 2 x 16 = 32.  K128 = 4: the ring
    # of 3 stages preloads kt 0, 1, refills at kt 0 (stage 2) and kt 1 (stage 0 again, read at kt 3); `younger >= 1` holds at kt 0 .. 2.
    # Flash 2 x 1 x 8 = 16 -> <1>.
    "f8_64_deepk": (512, 96, 2, 2, 2, "64x3", 1),
    # Spad 1536, M 3072.  QKV N 1536: 12 x 6 = 72 < 200 (not the 256 kernel), 24 x 12 = 288 >= 200 -> <128, 2>; FC1 / cross-K/V N 2048:
    # 12 x 8 = 96 < 200, 24 x 16 = 384.  K128 = 4: four steps through the 2-stage ring.  Flash 2 x 12 x 8 = 192 < 256 -> <1>.
    "f8_128_deepk": (512, 1500, 2, 2, 2, "128x2", 1),
}


def variant_config(tag):
    d, S, enc_layers, dec_layers, _, _, _ = VARIANTS[tag]
    cfg = MedusaConfig.micro(K=4, d_model=d, n_ctx=S)
    return dataclasses.replace(cfg, encoder_layers=enc_layers, decoder_layers=dec_layers)


class Case:
    """One variant: config, the plain and the stress checkpoint, and three distinct feature clips A (full), B (ragged), C (full)."""

    def __init__(self, tag):
        self.tag, self.cfg = tag, variant_config(tag)
        self.B = VARIANTS[tag][4]
        self.plain = synth.synth_state_dict(self.cfg, seed=SEED)
        self.sd = stress_checkpoint(self.cfg, self.plain)
        f = mask_ref.features(self.cfg, clips=3)                  # clips 0, 1, 2 of the seeded set, the last one ragged
        self.feats = np.ascontiguousarray(f[[0, 2, 1]])           # A, B (ragged), C

    def oracle(self, plain=False, **kw):
        """The in-contract oracle (bf16 rounding points, fp8 encoder GEMMs) on the stress checkpoint, optionally faulted / ln64."""
        return FaultyOracle(self.cfg, self.plain if plain else self.sd, sim="bf16", enc_fp8=True, **kw)

    def order(self, reverse=False):
        """Which of A, B, C (0, 1, 2) sits at each of the B batch indices: period 3, or the same arrangement reversed.  A batch of two holds A
        and the ragged B only; reversed, both change their index."""
        o = [i % 3 for i in range(self.B)]
        return o[::-1] if reverse else o

    def batch(self, reverse=False):
        return np.ascontiguousarray(self.feats[self.order(reverse)])


@functools.lru_cache(maxsize=None)
def case(tag):
    return Case(tag)
