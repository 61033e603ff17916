"""generate(return_token_timestamps=True) on the GPU: teacher-forced replay + alignment kernels + DTW (include/wm.h wm_token_timestamps,
csrc/wm_align.hip) against HF's own DTW, the recording oracle and tests/token_ts_ref.py.

Measured bounds (nothing here is fitted to the engine's output):
  probabilities  engine vs contract oracle <= 2 x (contract oracle vs fp32 oracle), relative to each row's maximum
  matrix         engine vs fp32 reference on the engine's own probabilities <= 4 x (fp32 reference vs fp64 reference), absolute
  end to end     share of tokens within one frame of the oracle's >= the fp32-vs-contract oracle pair's share - 0.05"""
import dataclasses

import numpy as np
import pytest
import torch

import token_ts_ref as ref
from helpers import MedusaConfig, synth, clip_for, record_table, default_act_f16
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu

SHARPEN = 6.0       # the alignment heads' cross-attention q_proj is scaled by this in the test checkpoints (random-weight attention is diffuse)


def hf_dtw(cost):
    from transformers.models.whisper.generation_whisper import _dynamic_time_warping
    return _dynamic_time_warping(cost)


def checkpoint(shape, heads_type="base_head", seed=31, n_heads=None, choices=None):
    cfg = MedusaConfig.micro(K=4, heads_type=heads_type) if shape == "micro" else MedusaConfig.tiny_en(heads_type, K=4)
    if choices is not None:
        cfg = dataclasses.replace(cfg, medusa_choices=choices)
    heads = synth.synth_alignment_heads(cfg, n_heads or (2 if shape == "micro" else 5))
    cfg = dataclasses.replace(cfg, alignment_heads=heads)
    sd = synth.synth_state_dict(cfg, seed=seed)
    for l, h in heads:
        p = f"whisper_model.model.decoder.layers.{l}.encoder_attn.q_proj"
        sd[p + ".weight"][h * 64:(h + 1) * 64] *= SHARPEN
        sd[p + ".bias"][h * 64:(h + 1) * 64] *= SHARPEN
    return cfg, sd


_MODELS = {}


def model_for(gpu, shape, heads_type="base_head", act_fp16=None, max_batch=3, choices=None):
    key = (shape, heads_type, act_fp16, max_batch, tuple(choices or ()))
    if key not in _MODELS:
        cfg, sd = checkpoint(shape, heads_type, choices=choices)
        _MODELS[key] = (WhisperMedusaModel(cfg, sd, device=gpu, act_fp16=act_fp16, max_batch=max_batch), cfg, sd)
    return _MODELS[key]


def feats_for(model, cfg, clips):
    return torch.cat([model.extract_features(clip_for(cfg, i)) for i in clips], dim=0)


def oracle_for(cfg, sd, sim, f16):
    return ref.RecordingOracle(cfg, sd, sim=sim, act="f16" if f16 else "hilo")


def rel_rowmax(a, b):
    """max over rows of max_f |a - b| / max_f b."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b).abs().amax(-1) / b.amax(-1)).max())


# ---- 1. DTW exact -----------------------------------------------------------------------------------------------------------------------
def dtw_cases():
    g = torch.Generator().manual_seed(7)
    out = []
    for i, (N, F) in enumerate([(1, 1), (1, 50), (2, 1500), (17, 96), (100, 40), (447, 1500)]):
        for seed in ((0, 1, 2) if N * F < 100000 else (0,)):
            out.append((f"normal{N}x{F}s{seed}", torch.randn(N, F, generator=torch.Generator().manual_seed(1000 * i + seed))))
    out.append(("constant", torch.full((23, 61), 0.25)))
    out.append(("quantised", torch.randint(0, 4, (40, 150), generator=g).float() * 0.5 - 1.0))
    d = -torch.ones(30, 120)
    for r in range(30):
        d[r, 4 * r: 4 * r + 4] = 2.0
    out.append(("diagonal", d))
    return out


def test_dtw_equals_transformers(gpu):
    model, cfg, _ = model_for(gpu, "micro")
    for name, m in dtw_cases():
        text, time, first = model.engine.dtw(m.numpy())
        t_ref, x_ref = hf_dtw(-m.double().numpy())
        assert np.array_equal(text, t_ref) and np.array_equal(time, x_ref), name
        jumps = np.pad(np.diff(t_ref), (1, 0), constant_values=1).astype(bool)
        assert np.array_equal(first, x_ref[jumps]), name


# ---- 2. / 3. probabilities and matrix ------------------------------------------------------------------------------------------------------
def random_ids(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    return synth.default_prompt(cfg) + torch.randint(10, min(cfg.vocab_size, 900), (n,), generator=g).tolist()


@pytest.mark.parametrize("shape,heads_type,other", [("micro", "base_head", False), ("micro", "medusa_block", False), ("tiny", "base_head", False),
                                                    ("micro", "base_head", True)])
def test_probabilities_and_matrix(gpu, shape, heads_type, other):
    f16 = default_act_f16() != other                   # `other`: one run on the library of the other decode contract
    model, cfg, sd = model_for(gpu, shape, heads_type, act_fp16=f16)
    eng, heads, P = model.engine, cfg.alignment_heads, len(synth.default_prompt(cfg))
    feats = feats_for(model, cfg, [0, 1, 2])
    eng.encode(feats)
    seqs = [random_ids(cfg, 40 - P, 1), random_ids(cfg, 21, 2), random_ids(cfg, 33, 3)]      # 40 tokens: rows cross two 16-row tiles
    out, ms = eng.token_timestamps(seqs, P, heads, cfg.median_filter_width)
    enc = eng.encoder_output(3)
    S = cfg.max_source_positions
    d_eng = d_ref = e_mat = e_ref = 0.0
    for b in ([0, 1, 2] if shape == "micro" else [0, 1]):
        w_c = oracle_for(cfg, sd, "bf16", f16).alignment_weights(enc[b], seqs[b], P, heads)
        w_f = oracle_for(cfg, sd, "fp32", f16).alignment_weights(enc[b], seqs[b], P, heads)
        got = torch.stack([torch.from_numpy(eng.align_probs(b, a)) for a in range(len(heads))])
        assert got.shape == w_c.shape == (len(heads), len(seqs[b]) - P - 1, S)
        assert float((got.sum(-1) - 1).abs().max()) <= 1e-5
        d_eng, d_ref = max(d_eng, rel_rowmax(got, w_c)), max(d_ref, rel_rowmax(w_f, w_c))
        # matrix: steps 2-4 in fp32 on the engine's OWN probabilities; yardstick fp32 vs fp64 of the same formula
        M = torch.from_numpy(eng.align_matrix(b))
        m32, m64 = ref.align_matrix(got, cfg.median_filter_width), ref.align_matrix(got, cfg.median_filter_width, torch.float64)
        assert torch.isfinite(M).all() and M.shape == m32.shape
        e_mat, e_ref = max(e_mat, float((M.double() - m32.double()).abs().max())), max(e_ref, float((m32.double() - m64).abs().max()))
    tag = f"token_ts[{shape},{heads_type},{'f16' if f16 else 'hilo'}]"
    print(f"{tag}: probs engine-contract {d_eng:.3e}, fp32-contract {d_ref:.3e}; matrix engine-fp32 {e_mat:.3e}, fp32-fp64 {e_ref:.3e}; {ms:.2f} ms")
    record_table(tag, probs_engine_vs_contract=d_eng, probs_fp32_vs_contract=d_ref, matrix_engine_vs_fp32=e_mat, matrix_fp32_vs_fp64=e_ref)
    assert d_eng <= 2 * d_ref, (d_eng, d_ref)
    assert e_mat <= 4 * e_ref, (e_mat, e_ref)


def test_zero_std_frame_gives_nan_like_torch(gpu):
    """Alignment heads sharpened until most frames underflow to probability 0 in every row: their population std is 0, torch's (w - mean) / std
    is 0 / 0 = NaN there, torch.sort puts NaN last in a median window and the mean over the heads carries it.  The engine's matrix must be
    NaN at exactly the cells where the reference on the engine's own probabilities is."""
    cfg, sd = checkpoint("micro")
    for l, h in cfg.alignment_heads:
        pq = f"whisper_model.model.decoder.layers.{l}.encoder_attn.q_proj"
        sd[pq + ".weight"][h * 64:(h + 1) * 64] *= 60.0
        sd[pq + ".bias"][h * 64:(h + 1) * 64] *= 60.0
    model = WhisperMedusaModel(cfg, sd, device=gpu)
    eng, P = model.engine, len(synth.default_prompt(cfg))
    eng.encode(feats_for(model, cfg, [0]))
    eng.token_timestamps([random_ids(cfg, 14, 5)], P, cfg.alignment_heads, 7)
    got = torch.stack([torch.from_numpy(eng.align_probs(0, a)) for a in range(len(cfg.alignment_heads))])
    M, m32 = torch.from_numpy(eng.align_matrix(0)), ref.align_matrix(got, 7)
    print(f"token_ts zero-std: {int(torch.isnan(m32).sum())} of {m32.numel()} cells NaN in the reference, {int((got.std(dim=-2, unbiased=False) == 0).sum())} zero-std frames")
    assert bool((got.std(dim=-2, unbiased=False) == 0).any()), "the checkpoint is not sharp enough to produce a zero-std frame"
    assert torch.equal(torch.isnan(M), torch.isnan(m32)) and torch.equal(torch.isinf(M), torch.isinf(m32))
    model.engine.close()


# ---- 4. composition is exact ---------------------------------------------------------------------------------------------------------------
def check_composition(model, cfg, out, P, num_frames=None):
    seqs, tt = out["sequences"], out["token_timestamps"]
    assert tt.dtype == torch.float32 and tt.shape == seqs.shape and tt.device == seqs.device
    eos = cfg.eos_token_id
    for b in range(seqs.shape[0]):
        row = seqs[b].tolist()
        T = row.index(eos, P) + 1 if eos in row[P:] else len(row)
        nf = num_frames[b] if isinstance(num_frames, (list, tuple)) else num_frames
        F = cfg.max_source_positions if nf is None else nf // 2
        got = tt[b].cpu()
        if T - P - 1 >= 2:
            M = torch.from_numpy(model.engine.align_matrix(b))
            assert M.shape == (T - P - 1, F)
            want = ref.timestamps_from_matrix(M, P, seqs.shape[1], dtw_fn=hf_dtw)
            assert torch.equal(got, want), (b, got, want)
        else:
            assert torch.equal(got, torch.zeros_like(got))
        assert torch.equal(got[:P], torch.zeros(P))
        assert bool((got[1:] >= got[:-1]).all()) and float(got.min()) >= 0.0 and float(got.max()) < F * 0.02
        assert bool((got[T - 1:] == got[T - 2]).all()) if T - P >= 2 else True


@pytest.mark.parametrize("heads_type", ["base_head", "medusa_block"])
def test_generate_composition_exact(gpu, heads_type):
    model, cfg, sd = model_for(gpu, "micro", heads_type)
    P = len(synth.default_prompt(cfg))
    f1, f3 = feats_for(model, cfg, [0]), feats_for(model, cfg, [0, 1, 2])
    kw = dict(exponential_decay_length_penalty=(4, 1.5))
    plain = model.generate(f1, max_new_tokens=30, **kw)
    it = model.last_stats["iterations"]
    out = model.generate(f1, max_new_tokens=30, return_token_timestamps=True, **kw)
    assert torch.equal(out["sequences"], plain) and model.last_stats["iterations"] == it and model.last_stats["ms_token_timestamps"] > 0
    check_composition(model, cfg, out, P)
    out = model.generate(f3, max_new_tokens=34, return_token_timestamps=True, **kw)
    assert torch.equal(out["sequences"], model.generate(f3, max_new_tokens=34, **kw))
    out = model.generate(f3, max_new_tokens=34, return_token_timestamps=True, **kw)
    check_composition(model, cfg, out, P)
    out = model.generate(f3, max_new_tokens=20, return_token_timestamps=True, num_frames=[120, 96, 150], **kw)
    check_composition(model, cfg, out, P, [120, 96, 150])
    out = model.generate(f1, max_new_tokens=20, return_token_timestamps=True, num_frames=100, **kw)
    check_composition(model, cfg, out, P, 100)
    out = model.generate(f1, max_new_tokens=20, return_token_timestamps=True, vanilla=True, **kw)
    check_composition(model, cfg, out, P)
    prompt_ids = torch.tensor([cfg.prev_sot_token_id, 11, 12, 13])
    out = model.generate(f1, max_new_tokens=20, return_token_timestamps=True, prompt_ids=prompt_ids, **kw)
    check_composition(model, cfg, out, len(model._last_prompt))
    # one generated token (N = 0) and two (N = 1): zeros (plain greedy steps: a Medusa iteration may emit several tokens at once)
    for n in (1, 2):
        out = model.generate(f1, max_new_tokens=n, return_token_timestamps=True, vanilla=True)
        assert out["sequences"].shape[1] == P + n
        assert torch.equal(out["token_timestamps"], torch.zeros_like(out["token_timestamps"]))


def test_generate_composition_tree_and_timestamps(gpu):
    model, cfg, _ = model_for(gpu, "micro", choices=[1, 2, 2, 1, 1])
    f1 = feats_for(model, cfg, [0])
    out = model.generate(f1, max_new_tokens=24, return_token_timestamps=True)
    assert torch.equal(out["sequences"], model.generate(f1, max_new_tokens=24))
    out = model.generate(f1, max_new_tokens=24, return_token_timestamps=True)
    check_composition(model, cfg, out, len(synth.default_prompt(cfg)))
    # return_timestamps=True together (needs the timestamp vocabulary block: tests/test_gpu_timestamps.py micro_ts)
    from test_gpu_timestamps import micro_ts, state_dict
    c = micro_ts()
    c = dataclasses.replace(c, alignment_heads=synth.synth_alignment_heads(c, 2))
    m2 = WhisperMedusaModel(c, state_dict(c, 3, 1.0), device=gpu)
    f = m2.extract_features(clip_for(c, 0))
    out = m2.generate(f, max_new_tokens=24, return_timestamps=True, return_token_timestamps=True, return_segments=True)
    assert torch.equal(out["sequences"], m2.generate(f, max_new_tokens=24, return_timestamps=True))
    out = m2.generate(f, max_new_tokens=24, return_timestamps=True, return_token_timestamps=True, return_segments=True)
    check_composition(m2, c, out, len(m2._last_prompt))
    o = len(m2._last_prompt)
    for sg in out["segments"][0]:
        n = sg["tokens"].numel()
        assert torch.equal(sg["token_timestamps"], out["token_timestamps"][0, o: o + n])
        o += n
    m2.engine.close()


# ---- 5. end to end against the recording oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["micro", "tiny"])
def test_end_to_end_against_oracle(gpu, shape):
    f16 = default_act_f16()
    model, cfg, sd = model_for(gpu, shape)
    heads, P = cfg.alignment_heads, len(synth.default_prompt(cfg))
    clips = [0, 1, 2] if shape == "micro" else [0]
    near_e = near_y = tot = 0
    de, dy = [], []
    for c in clips:
        f = feats_for(model, cfg, [c])
        out = model.generate(f, max_new_tokens=36, return_token_timestamps=True)
        ids = out["sequences"][0].tolist()
        if cfg.eos_token_id in ids[P:]:
            ids = ids[: ids.index(cfg.eos_token_id, P) + 1]
        enc = model.engine.encoder_output(1)[0]
        t_c = ref.token_timestamps(oracle_for(cfg, sd, "bf16", f16).alignment_weights(enc, ids, P, heads), P, cfg.median_filter_width, dtw_fn=hf_dtw)
        t_f = ref.token_timestamps(oracle_for(cfg, sd, "fp32", f16).alignment_weights(enc, ids, P, heads), P, cfg.median_filter_width, dtw_fn=hf_dtw)
        got = out["token_timestamps"][0, : len(ids)].cpu()
        e, y = (got - t_c)[P:].abs(), (t_f - t_c)[P:].abs()
        near_e += int((e <= 0.02 + 1e-6).sum()); near_y += int((y <= 0.02 + 1e-6).sum()); tot += e.numel()
        de += e.tolist(); dy += y.tolist()
    share_e, share_y = near_e / tot, near_y / tot
    print(f"token_ts_e2e[{shape}]: engine within one frame {share_e:.3f} (median |d| {np.median(de):.3f} s), fp32-vs-contract oracle {share_y:.3f} "
          f"(median {np.median(dy):.3f} s), {tot} tokens")
    record_table(f"token_ts_e2e[{shape}]", engine_share=share_e, yardstick_share=share_y, engine_median=float(np.median(de)),
                 yardstick_median=float(np.median(dy)), tokens=tot)
    assert share_y >= 0.8, "the reference pair itself disagrees: sharpen the test checkpoint's cross-attention"
    assert share_e >= share_y - 0.05, (share_e, share_y)


# ---- 6. pool, long-form, segments ----------------------------------------------------------------------------------------------------------
def test_pool_longform_segments_match_single_engine(gpu):
    model, cfg, _ = model_for(gpu, "micro", max_batch=4)
    P = len(synth.default_prompt(cfg))
    f4 = feats_for(model, cfg, [0, 1, 2, 3])
    kw = dict(max_new_tokens=22, return_token_timestamps=True)
    single = [model.generate(f4[b: b + 1], **kw) for b in range(4)]
    model.set_micro_batches(2)
    pooled = model.generate(f4, return_segments=True, **kw)
    model.set_micro_batches(1)
    assert model.last_stats["ms_token_timestamps"] > 0
    for b in range(4):
        T = single[b]["sequences"].shape[1]
        assert torch.equal(pooled["sequences"][b, :T], single[b]["sequences"][0])
        assert torch.equal(pooled["token_timestamps"][b, :T], single[b]["token_timestamps"][0])
        sg = pooled["segments"][b][0]
        assert torch.equal(sg["token_timestamps"], pooled["token_timestamps"][b, P: P + sg["tokens"].numel()])
    # two windows of one long clip = the two clips decoded alone, the second offset by the window length
    long = torch.cat([f4[0], f4[1]], dim=-1)[None]
    lf = model.generate(long, chunk_longform=True, **kw)
    eos, pad = cfg.eos_token_id, cfg.pad_token_id
    want_ids, want_tt = list(single[0]["sequences"][0, :P].tolist()), [0.0] * P
    off = torch.tensor(cfg.n_mel_frames * 0.01, dtype=torch.float32)
    assert abs(float(off) - 30.0 * cfg.max_source_positions / 1500) < 1e-6
    for j in range(2):
        row, tt = single[j]["sequences"][0].tolist(), single[j]["token_timestamps"][0].cpu()
        for q in range(P, len(row)):
            if row[q] in (eos, pad):
                break
            want_ids.append(row[q]); want_tt.append(float(tt[q] + j * off))
    want_ids.append(eos); want_tt.append(want_tt[-1])
    assert lf["sequences"][0].tolist() == want_ids
    assert torch.equal(lf["token_timestamps"][0].cpu(), torch.tensor(want_tt, dtype=torch.float32))


# ---- 7. the replays and taps share one driver and leave the decode alone ------------------------------------------------------------------
def _tap_params(cfg):
    """Parameters of the two row taps: ids of their own with a timestamp block at the vocabulary's end (the taps never touch the weights)."""
    from helpers import GenParams, ACCEPT_TYPICAL
    tb = cfg.vocab_size - 30
    return GenParams(prompt=[5, 6], eos_token_id=900, pad_token_id=900, suppress_tokens=[3, 40], begin_suppress_tokens=[7], max_length=cfg.max_target_positions,
                     hard_max_length=cfg.max_length, accept_mode=ACCEPT_TYPICAL, temperature=1.0, exp_decay=(1, 1.3), timestamps=True,
                     no_timestamps_token_id=tb - 1, max_initial_timestamp_index=5), tb


def test_replays_and_taps_leave_the_decode_alone(gpu):
    """Both replays in both orders, then both row taps, between two identical decodes: the orders agree bit for bit and the second decode
    finds ids, statistics and the captured graph of the first.  Hand-made streams of 16, 17 and 33 tokens (prompt + generated): their last
    replayed input positions (len - 2 = 14, 15, 31) sit below the first 16-row tile edge, on it, and on the edge of the second tile."""
    model, cfg, _ = model_for(gpu, "micro")
    eng, heads, P = model.engine, cfg.alignment_heads, len(synth.default_prompt(cfg))
    f3 = feats_for(model, cfg, [0, 1, 2])
    kw = dict(max_new_tokens=30, exponential_decay_length_penalty=(4, 1.5))

    def run():
        ids = model.generate(f3, **kw)
        return ids, {k: model.last_stats[k] for k in ("iterations", "tokens_emitted", "accept_hist", "schedule_steps", "graph_replays")}
    model.generate(f3, **kw)                    # (captures the graph of these parameters)
    ids0, st0 = run()
    seqs = [random_ids(cfg, n - P, seed) for n, seed in ((16, 1), (17, 2), (33, 3))]
    assert [len(s) for s in seqs] == [16, 17, 33]
    gp = model._gen_params(None, None, (4, 1.5), 30, None, None, False, None, None, None, None, None)
    ns = cfg.no_timestamps_token_id - 1
    lp_a, ns_a, _ = eng.score_tokens(seqs, P, gp, no_speech_token_id=ns)
    tt_a, _ = eng.token_timestamps(seqs, P, heads, cfg.median_filter_width)
    tt_b, _ = eng.token_timestamps(seqs, P, heads, cfg.median_filter_width)
    lp_b, ns_b, _ = eng.score_tokens(seqs, P, gp, no_speech_token_id=ns)
    assert np.array_equal(lp_a, lp_b) and np.array_equal(ns_a, ns_b) and np.array_equal(tt_a, tt_b)
    assert np.isfinite(lp_a[2, P:33]).all() and bool((lp_a[2, P:33] < 0).all()) and float(tt_a.max()) > 0
    tgp, tb = _tap_params(cfg)
    rows = np.random.default_rng(3).standard_normal((2, cfg.vocab_size)).astype(np.float32) * 2.0
    pre = [list(tgp.prompt) + [tb + 3, 41], list(tgp.prompt) + [tb + 3, 41, tb + 9, tb + 9, 12]]
    sr = eng.score_rows(tgp, rows, pre, [44, tb + 12])
    sel = eng.select_rows(tgp, rows, pre, [44, tb + 12])
    assert sr.shape == (2,) and not np.isnan(sr).any() and sel["argmax"].shape == (2,)
    ids1, st1 = run()
    assert torch.equal(ids0, ids1) and st0 == st1, (st0, st1)
    assert st0["graph_replays"] > 0
    # the replays after the taps: what they gave before them
    assert np.array_equal(eng.score_tokens(seqs, P, gp, no_speech_token_id=ns)[0], lp_a)
    assert np.array_equal(eng.token_timestamps(seqs, P, heads, cfg.median_filter_width)[0], tt_a)


_GROUPS_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
import test_gpu_token_timestamps as T
model, eng, seqs, P, heads, width = T.groups_rig(torch.device("cuda", 0))
out, _ = eng.token_timestamps(seqs, P, heads, width)
try:
    eng.align_matrix(0)
    split = False
except RuntimeError as e:
    split = "no longer resident" in str(e)
np.savez(sys.argv[2], out=out, split=split, m2=eng.align_matrix(2))
eng.close()
"""


def groups_rig(gpu):
    """Three streams whose alignment workspaces are 480 KB each (2 heads x 40 rows x 1536 frames x 4 bytes) on a micro checkpoint with a long
    encoder: under a 1 MB cap (the smallest WM_ALIGN_WS_MB) they form the groups [0, 1] and [2], so the replay driver runs at b0 = 2."""
    cfg = MedusaConfig.micro(K=4, n_ctx=1536)
    cfg = dataclasses.replace(cfg, alignment_heads=synth.synth_alignment_heads(cfg, 2))
    model = WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=31), device=gpu, max_batch=3)
    P = len(synth.default_prompt(cfg))
    model.engine.encode(feats_for(model, cfg, [0, 1, 2]))
    return model, model.engine, [random_ids(cfg, 42 - P, s) for s in (1, 2, 3)], P, cfg.alignment_heads, cfg.median_filter_width


def test_workspace_groups_equal_one_group(gpu, tmp_path):
    """WM_ALIGN_WS_MB is read once per process: a fresh child runs the call split into two workspace groups; the timestamps and the last
    group's matrix must be those of this process, where all three streams share one group."""
    import os
    import subprocess
    import sys
    model, eng, seqs, P, heads, width = groups_rig(gpu)
    want, _ = eng.token_timestamps(seqs, P, heads, width)
    m2 = eng.align_matrix(2)
    eng.align_matrix(0)                         # one group: every stream is resident
    eng.close()
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, WM_ALIGN_WS_MB="1")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _GROUPS_CHILD, here, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(path)
    assert bool(got["split"]), "the child did not split the streams into more than one workspace group"
    assert float(want.max()) > 0 and np.array_equal(got["out"], want) and np.array_equal(got["m2"], m2, equal_nan=True)


# ---- 8. error paths -------------------------------------------------------------------------------------------------------------------------
def test_error_paths(gpu):
    model, cfg, sd = model_for(gpu, "micro")
    f1 = feats_for(model, cfg, [0])
    with pytest.raises(ValueError):
        model.generate(f1, max_new_tokens=8, return_token_timestamps=True, alignment_heads=[[cfg.decoder_layers, 0]])
    fresh = WhisperMedusaModel(cfg, sd, device=gpu)
    P = len(synth.default_prompt(cfg))
    with pytest.raises(RuntimeError, match="wm_encode"):          # WM_ERR_STATE
        fresh.engine.token_timestamps([random_ids(cfg, 10, 1)], P, cfg.alignment_heads)
    fresh.engine.encode(f1)
    with pytest.raises(ValueError):                               # WM_ERR_ARG from the C-ABI itself
        fresh.engine.token_timestamps([random_ids(cfg, 10, 1)], P, [[0, cfg.decoder_attention_heads]])
    with pytest.raises(ValueError):
        fresh.engine.token_timestamps([random_ids(cfg, 10, 1)], P, cfg.alignment_heads, median_filter_width=4)
    with pytest.raises(ValueError):
        fresh.engine.token_timestamps([random_ids(cfg, 10, 1)], 99, cfg.alignment_heads)
    fresh.engine.close()
    # without alignment heads: the class test_generate_api_end_to_end asserts
    m3 = WhisperMedusaModel(dataclasses.replace(cfg, alignment_heads=None), sd, device=gpu)
    with pytest.raises(NotImplementedError, match="alignment_heads"):
        m3.generate(f1, max_new_tokens=8, return_token_timestamps=True)
    m3.engine.close()
