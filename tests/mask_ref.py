"""Source-length mask references (CPU only; no GPU import): the oracle's encoder and cross-attention with the key mask at
S = n_ctx deliberately WRONG, and the coefficient that tells whether an implementation carries that wrong mask.

Two kernels mask keys beyond S: k_flash_enc (csrc/wm_encoder.hip, encoder self-attention) and k_attn_mfma<CROSS>
(csrc/wm_decoder.hip, decoder cross-attention).  Both walk the keys in 64-key steps of two 32-key halves.  The ways such a walk goes
wrong are modelled here as mutants of the fp32 oracle:

  "drop"   the last valid key is invisible (S - 1 keys)
  "pad"    the first pad row is a visible key (S + 1 keys), modelled as the engine holds that row:
             encoder: the conv2 epilogue writes 0 into rows >= S; the row then runs through the layers as a row of its own,
                      attending the same S + 1 keys; rows < S are returned
             cross:   one more encoder-output row of zeros, which is what k_pack_hidden leaves behind wm_set_encoder_output:
                      K = 0, V = bias
  "half"   the last 32-key half step is invisible (keys >= 32 * floor((S - 1) / 32)); only for S > 32

An absolute tolerance cannot see these: at S = 1500 one key more or less moves the encoder output by less than the bf16 rounding points
move it (mean 1.2e-3 against 1.8e-3; the allowance is 6e-3).  The projection of the error on the mutant's own direction can:

  ref = fp32 oracle, mut = fp32 oracle with the wrong mask, D = mut - ref, e = got - ref
  c = <e, D> / <D, D>

c is 0 for an implementation without that bug and 1 for one with it; rounding noise is nearly orthogonal to D.  The decision threshold
0.5 is the midpoint of the two hypotheses, not a tolerance (tests/test_mask_ref_cpu.py proves the margins with the oracle alone).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from helpers import MedusaConfig, synth, clip_for
from oracle.whisper_medusa_oracle import Oracle, log_mel, HEAD_DIM

# every residue of S mod 64 that selects another branch of the two kernels' last step (first half masked, first half full and no second half,
# second half masked), one, two, three (the first refill of the 3-stage ring) and more steps, Spad - S from 0 to 127, and the present shape
SWEEP = (8, 31, 32, 33, 63, 64, 65, 97, 127, 128, 129, 161, 193, 255, 256, 257, 289, 513, 1500)
FP8_SWEEP = (33, 97, 161, 257, 1500)        # cross_kv_fp8: a mask in either half, one valid key in a split, the present shape
MUTANTS = ("drop", "pad", "half")
SEED = 13                                   # checkpoint seed: chosen, with the clips, so that the oracle alone keeps the margins (test_mask_ref_cpu.py)
N_TOKENS = 16                               # one full 16-row tile of the decoder's prompt pass


def mutants_for(S):
    return tuple(m for m in MUTANTS if m != "half" or S > 32)


def visible_keys(S, mutant):
    """Number of keys an implementation with that bug attends."""
    if mutant is None:
        return S
    if mutant == "drop":
        return S - 1
    if mutant == "pad":
        return S + 1
    if mutant == "half":
        assert S > 32
        return 32 * ((S - 1) // 32)
    raise ValueError(mutant)


def encode(orc, feats, mutant=None):
    """Oracle.encode (same helpers, same order: bit-equal for mutant=None) with the self-attention key mask of every layer at
    visible_keys(S, mutant) instead of S.  feats [n_mels, 2 S] -> [S, d]."""
    sd, p = orc.sd, "whisper_model.model.encoder"
    x = orc._r(feats.to(torch.float32))[None]
    x = F.gelu(F.conv1d(x, sd[p + ".conv1.weight"], sd[p + ".conv1.bias"], padding=1))
    x = F.gelu(F.conv1d(orc._r(x), sd[p + ".conv2.weight"], sd[p + ".conv2.bias"], stride=2, padding=1))
    h = x[0].t() + sd[p + ".embed_positions.weight"]
    S = h.shape[0]
    nk = visible_keys(S, mutant)
    if mutant == "pad":
        h = torch.cat([h, torch.zeros(1, h.shape[1])])            # the engine's row S: 0 (no bias, no position)
    for i in range(orc.cfg.encoder_layers):
        lp = f"{p}.layers.{i}"
        xn = orc._ln(h, lp + ".self_attn_layer_norm")
        lin = orc._lin8 if orc.enc_fp8 else orc._lin
        q = orc._r(lin(xn, lp + ".self_attn.q_proj") * HEAD_DIM ** -0.5)
        k = orc._r(lin(xn, lp + ".self_attn.k_proj", bias=False))
        v = orc._r(lin(xn, lp + ".self_attn.v_proj"))
        kh, vh = orc._heads(k), orc._heads(v)
        if nk < S:
            kh, vh = kh[:, :nk], vh[:, :nk]
        a = orc._attend(orc._heads(q), kh, vh, round_p=True)
        h = h + orc._lin(a, lp + ".self_attn.out_proj")
        xn = orc._ln(h, lp + ".final_layer_norm")
        h = h + orc._lin(F.gelu(lin(xn, lp + ".fc1")), lp + ".fc2")
    out = orc._r(orc._ln(h, p + ".layer_norm"))
    return out[:S] if mutant == "pad" else out


def _q8_heads_valid(x, S):
    """Oracle._q8_heads with the per-head scale taken over rows < S only: [H, S + 1, 64] -> its dequantised e4m3 image."""
    amax = x[:, :S].abs().amax(dim=(1, 2))
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))[:, None, None]
    return (x / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float32) * scale


def cross_state(orc, enc, mutant=None):
    """Oracle.new_state(enc) with the cross-attention keys of every kv layer cut or extended to visible_keys(S, mutant)."""
    S = enc.shape[0]
    if mutant == "pad":
        if not orc.xkv_fp8:
            return orc.new_state(torch.cat([enc, torch.zeros(1, enc.shape[1])]))
        # e4m3 copy: k_xkv_quant takes each head's scale from the S valid rows and quantises the pad rows with it
        plain = Oracle(orc.cfg, orc.sd, sim=orc.sim, enc_fp8=orc.enc_fp8, act=orc.act)
        st = plain.new_state(torch.cat([enc, torch.zeros(1, enc.shape[1])]))
        st["cross_kv"] = [(_q8_heads_valid(k, S), _q8_heads_valid(v, S)) for k, v in st["cross_kv"]]
        return st
    st = orc.new_state(enc)
    if mutant is not None:
        nk = visible_keys(S, mutant)
        st["cross_kv"] = [(k[:, :nk], v[:, :nk]) for k, v in st["cross_kv"]]
    return st


def logits(orc, enc, tokens, mutant=None):
    """All heads' logits [K+1, T, V] of one pass over `tokens` at position 0 on the stored encoder output `enc`."""
    return orc.decoder_pass(cross_state(orc, enc, mutant), list(tokens), 0, disable_medusa=False)


def bug_coefficient(got, ref, mut):
    """<got - ref, mut - ref> / <mut - ref, mut - ref> in float64: 0 = `got` does not carry the mutant's bug, 1 = it does."""
    ref = torch.as_tensor(ref).to(torch.float64)
    D = torch.as_tensor(mut).to(torch.float64) - ref
    e = torch.as_tensor(got).to(torch.float64) - ref
    dd = float((D * D).sum())
    assert dd > 0.0, "the mutant does not move the output: nothing to project on"
    return float((e * D).sum()) / dd


def token_rows(cfg, n=N_TOKENS):
    """Two 16-token rows (one per stream): the default prompt continued with ordinary ids, and the same row reversed."""
    prompt = synth.default_prompt(cfg)
    row = prompt + [11 + 37 * i for i in range(n - len(prompt))]
    assert len(row) == n and max(row[len(prompt):]) < cfg.vocab_size - 8      # ordinary ids: below the special tokens
    return [row, row[::-1]]


def features(cfg, clips=2):
    """[clips, n_mels, 2 S] log-mel of the seeded clips; the last one ragged (a third of the window, zero-padded) as in test_gpu_parity.Rig."""
    n = cfg.n_mel_frames * 160
    wavs = [clip_for(cfg, i) for i in range(clips)]
    wavs[-1] = wavs[-1][: n // 3]
    return np.stack([log_mel(w, cfg.num_mel_bins, n) for w in wavs])


class Case:
    """One source length: checkpoint, features, the fp32 oracle and the bf16 ones, and the fp32 reference + mutants of the encoder
    output per clip, computed once and never modified."""

    def __init__(self, cfg, seed=SEED, clips=2):
        self.cfg, self.S = cfg, cfg.max_source_positions
        self.sd = synth.synth_state_dict(cfg, seed=seed)
        self.o32 = Oracle(cfg, self.sd, sim="fp32")
        self.feats = features(cfg, clips)
        self.mutants = mutants_for(self.S)
        self._enc = {}

    def bf16(self, **kw):
        return Oracle(self.cfg, self.sd, sim="bf16", **kw)

    def enc_ref(self, b):
        """(fp32 encoder output of clip b, {mutant: fp32 mutated output})"""
        if b not in self._enc:
            f = torch.from_numpy(self.feats[b])
            self._enc[b] = (self.o32.encode(f), {m: encode(self.o32, f, m) for m in self.mutants})
        return self._enc[b]

    def enc_coefficients(self, got, b):
        ref, muts = self.enc_ref(b)
        return {m: bug_coefficient(got, ref, muts[m]) for m in self.mutants}

    def logit_ref(self, enc, tokens, xkv_fp8=False):
        """(fp32 logits [K+1, T, V] of one pass on the stored encoder output `enc`, {mutant: fp32 mutated logits}).  xkv_fp8: the fp32
        oracle of the model whose cross-K/V is the e4m3 image (the quantisation is part of the operation under test, not of its error)."""
        o = Oracle(self.cfg, self.sd, sim="fp32", xkv_fp8=True) if xkv_fp8 else self.o32
        return logits(o, enc, tokens), {m: logits(o, enc, tokens, m) for m in self.mutants}


@functools.lru_cache(maxsize=None)
def sweep_case(S):
    return Case(MedusaConfig.micro(K=4, n_ctx=S))


# Encoder kernel variants the dispatcher of wm_enc_encode picks only at larger shapes: tag -> (d_model, n_ctx, clips in the batch).
# The dispatch arithmetic is spelled out where they are used (tests/test_gpu_source_length.py).
VARIANTS = {
    "flash4_masked": (128, 1500, 11),
    "flash2_one_key": (256, 257, 22),
    "gemm256p": (256, 1500, 12),
}


@functools.lru_cache(maxsize=None)
def variant_case(tag):
    d, S, _ = VARIANTS[tag]
    return sweep_case(S) if d == 128 else Case(MedusaConfig.micro(K=4, d_model=d, n_ctx=S))


def variant_batch(case, B):
    """[B, n_mels, 2 S]: clip 0, the ragged clip 1, fillers (clips 0 / 1 rotated in time: only their presence matters), clip 0 again."""
    f = case.feats
    fill = [np.roll(f[i % 2], 7 * i, axis=1) for i in range(2, B - 1)]
    return np.ascontiguousarray(np.stack([f[0], f[1]] + fill + [f[0]]))
