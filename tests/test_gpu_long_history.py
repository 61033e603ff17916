"""Decoder self-attention histories beyond 128 keys (csrc/wm_decoder.hip k_attn_mfma<CROSS=false>: from the second 32-key step of a wave on, the
in-flight prefetch, the alternation of the two register sets, the running-max rescale and the V^T fragment addressing at kb >= 128 run; below,
none of them does) and everything else that is a function of the sequence position: K/V appends and row moves at rows >= 128, the ancestor mask
with a large base, merged steps with streams on both sides of a 128-key boundary, the 16-row replay tiles deep into the cache, position
embeddings and the length penalty near n_tgt.

One shape: MedusaConfig.micro(K=4, n_tgt=448) (cache rows Tal = 480), Linear and Block, on a checkpoint whose self-attention is visible in the
logits (tests/long_history.py; tests/test_long_history_cpu.py proves on the oracle that a lost step, a stale register set and a lost key leave
the bounds used here by >= 5 x).  Bounds: the decoder-logits contract of tests/test_gpu_parity.py (max |d| <= 6e-2, mean |d| <= 4e-3 given the same
encoder output), token parity by helpers.check_tokens (max_ties = 2).  Measured values: profiles/long_history_parity.md."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import long_history as LH
import scores_ref as R
import token_ts_ref as ref
from helpers import synth, clip_for, check_tokens, record_table, default_act_f16, ACCEPT_TYPICAL, ACCEPT_GREEDY
from long_history import Oracle
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu
ACTS = [pytest.param(False, id="hilo"), pytest.param(True, id="f16")]
MODES = [pytest.param(ACCEPT_TYPICAL, id="typical"), pytest.param(ACCEPT_GREEDY, id="greedy")]
K = 4


def _act(f16):
    return "f16" if f16 else "hilo"


def _long_pid(cfg, plen):
    """prompt_ids of tests/test_gpu_features.py::test_long_prompts_match_the_oracle."""
    return torch.tensor([cfg.vocab_size - 5] + [10 + (7 * i) % 900 for i in range(plen - 1)])


def _gp(model, cfg, pid, max_new=None, temperature=None, decay=LH.EXP_DECAY, eos_free=True):
    sup = sorted({cfg.eos_token_id, 3, 5}) if eos_free else None
    return model._gen_params(None, None, decay, max_new, None, temperature, False, None, None, sup, None, pid)


# ---- 3. teacher-forced walk through the whole cache (wm_forward_logits, single-stream tile path) ---------------------------------------------
@pytest.mark.parametrize("f16", ACTS)
@pytest.mark.parametrize("heads", LH.HEADS)
def test_teacher_forced_walk_through_the_whole_cache(gpu, heads, f16):
    cfg, sd = LH.checkpoint(heads)
    model = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=1, act_fp16=f16)
    eng = model.engine
    eng.encode(model.extract_features(clip_for(cfg, LH.WALK_CLIP)))
    enc = eng.encoder_output(1)[0]
    ids = LH.walk_ids()
    orc = Oracle(cfg, sd, sim="bf16", act=_act(f16))
    numbers = {}
    for kind, tiles in (("aligned", LH.tiles_aligned()), ("ragged", LH.tiles_ragged())):
        assert tiles[-1][0] + tiles[-1][1] == LH.N_TGT                                     # the walk reaches pos0 + T = n_tgt
        want = LH.oracle_walk(orc, enc, ids, tiles)
        got = torch.cat([eng.forward_logits([ids[p: p + t]], p, False)[:, 0] for p, t in tiles], dim=1)
        assert got.shape == want.shape == (K + 1, LH.N_TGT, cfg.vocab_size) and bool(torch.isfinite(got).all())
        mx, mn, tmx, tmn = LH.tile_stats((got - want).abs(), tiles)
        worst = max(range(len(tiles)), key=lambda i: tmx[i])
        print(f"long history walk [{heads}, {_act(f16)}, {kind}]: max |d| {mx:.4g} (tile {worst} at pos0 {tiles[worst][0]}), mean |d| {mn:.4g}")
        numbers[f"{kind}_max"], numbers[f"{kind}_mean"] = round(mx, 6), round(mn, 7)
        first = next((i for i in range(len(tiles)) if tmx[i] > LH.MAX_D or tmn[i] > LH.MEAN_D), None)
        assert first is None, (heads, f16, kind, "first tile outside the contract", first, tiles[first], tmx[first], tmn[first])
        assert mx <= LH.MAX_D and mn <= LH.MEAN_D, (heads, f16, kind, mx, mn)
        if kind == "aligned":
            # base head against the plain fp32 oracle: bound = the contract oracle's own gap to it (measured here) + the contract
            z32 = LH.oracle_walk(Oracle(cfg, sd, sim="fp32"), enc, ids, tiles, disable_medusa=True)[0]
            gap = (want[0] - z32).abs()
            d32 = (got[0] - z32).abs()
            print(f"long history walk [{heads}, {_act(f16)}] base head vs fp32 oracle: engine {float(d32.max()):.4g} / {float(d32.mean()):.4g}, "
                  f"contract oracle {float(gap.max()):.4g} / {float(gap.mean()):.4g}")
            numbers.update(fp32_max=round(float(d32.max()), 6), fp32_mean=round(float(d32.mean()), 7),
                           oracle_gap_max=round(float(gap.max()), 6), oracle_gap_mean=round(float(gap.mean()), 7))
            assert float(d32.max()) <= float(gap.max()) + LH.MAX_D and float(d32.mean()) <= float(gap.mean()) + LH.MEAN_D
    record_table(f"long history walk [{heads}, {_act(f16)}]", **numbers)
    eng.close()


# ---- 4. decode loop to the length limit, single stream --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("heads", LH.HEADS)
def test_decode_runs_to_the_length_limit(gpu, heads, mode):
    """test_gpu_parity.py::test_runs_to_the_hard_length_limit at n_tgt = 448: no EOS, no max_new_tokens, the run stops by `L + K >= max_length` with
    the K/V cache and the position table used up to their last rows.  Checkpoint seed and clip: long_history.DECODE_RUNS — over the oracle's own
    run the smallest decision margins are >= 10 x the tie tolerances (asserted, with the figures, in tests/test_long_history_cpu.py); the engine
    decodes from that very encoder output (wm_set_encoder_output: stored bf16, which the oracle's already is)."""
    seed, clip = LH.DECODE_RUNS[(heads, mode)]
    cfg, sd = LH.checkpoint(heads, seed)
    model = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=1)
    eng = model.engine
    orc = Oracle(cfg, sd, sim="bf16")
    enc = orc.encode(LH.features(cfg, clip))
    eng.set_encoder_output(enc[None])
    assert torch.equal(eng.encoder_output(1)[0], enc)
    gp = LH.limit_gen_params(cfg, mode)
    assert gp.max_length == LH.N_TGT and gp.hard_max_length == LH.N_TGT
    got = eng.decode(gp, 1)[0]
    st = eng.stats()
    _, ties = check_tokens(orc, enc, gp, got, f"long history to the limit {heads} mode {mode}")
    record_table(f"long history decode to the limit [{heads}, {'typical' if mode == ACCEPT_TYPICAL else 'exact-match'}]", ids=len(got),
                 iterations=st["iterations"], ties=len(ties), accept_hist=str(st["accept_hist"]))
    assert LH.N_TGT - K - 1 <= len(got) <= LH.N_TGT
    assert len(got) - 1 >= 384                                         # the last wave-0 step (keys 384 ..) was reached
    assert st["graph_replays"] > 0 or os.environ.get("WM_NO_GRAPH")
    eng.close()


# ---- 5. several streams across the boundaries ------------------------------------------------------------------------------------------------
def _four_streams(gpu, heads):
    cfg, sd = LH.checkpoint(heads, 31)
    model = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=4)
    n = cfg.n_mel_frames * 160
    feats = model.extract_features([clip_for(cfg, i)[: n // (1 + i % 3)] for i in range(4)])
    gp = _gp(model, cfg, _long_pid(cfg, 100))
    assert len(gp.prompt) == 102 and gp.max_length == LH.N_TGT
    return cfg, sd, model, feats, gp


@pytest.mark.parametrize("heads", LH.HEADS)
def test_streams_on_both_sides_of_a_128_key_boundary(gpu, heads, monkeypatch):
    """Four ragged clips behind one shared 100-id prompt, to the limit: acceptance drifts the streams apart, so launches of the merged-step schedule
    mix histories below and above 128 / 256.  Every stream == its own single-stream run; streams 0 and 1 == the oracle; WM_NO_STEP=1 (lock-step
    iteration, fresh model) gives the same ids."""
    monkeypatch.delenv("WM_NO_STEP", raising=False)
    cfg, sd, model, feats, gp = _four_streams(gpu, heads)
    eng = model.engine
    eng.encode(feats)
    enc = eng.encoder_output(4)
    both = eng.decode(gp, 4)
    assert all(LH.N_TGT - K - 1 <= len(s) <= LH.N_TGT for s in both)
    # the same run one iteration per call: per-stream lengths at the start of every step
    lens, cur = [], [len(gp.prompt)] * 4

    def on_it(new):
        lens.append(list(cur))
        for b in range(4):
            cur[b] += len(new[b])
    eng.encode(feats)
    assert eng.decode(gp, 4, on_iteration=on_it) == both
    # a stream of length l holds keys 0 .. l - 1: with l < edge its pass stays below the boundary, with l >= edge it appends key `edge` or beyond;
    # only streams still running (l + K < n_tgt) take part in a launch
    active = [[l for l in step if l + K < LH.N_TGT] for step in lens]
    for edge in (128, 256):
        assert any(a and min(a) < edge <= max(a) for a in active), (edge, "no step with running streams on both sides")
    for b in range(4):
        eng.encode(feats[b: b + 1].contiguous())
        assert eng.decode(gp, 1)[0] == both[b], b
    orc = Oracle(cfg, sd, sim="bf16")
    for b in (0, 1):
        check_tokens(orc, enc[b], gp, both[b], f"long history four streams {heads} b={b}")
    eng.close()
    monkeypatch.setenv("WM_NO_STEP", "1")
    lock = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=4)
    lock.engine.encode(feats)
    assert lock.engine.decode(gp, 4) == both
    lock.engine.close()


@pytest.mark.parametrize("heads", LH.HEADS)
@pytest.mark.parametrize("plen", [127, 130, 250, 400])
def test_long_prompts_match_the_oracle_at_448(gpu, heads, plen):
    """tests/test_gpu_features.py::test_long_prompts_match_the_oracle at n_tgt = 448 with prompts of 127 .. 400 ids: the 16-row prompt chunks (K/V
    only) either side of the 128-key boundaries, then 24 tokens behind them."""
    cfg, sd = LH.checkpoint(heads, 41)
    model = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=2)
    orc = Oracle(cfg, sd, sim="bf16")
    feats = model.extract_features([clip_for(cfg, 3), clip_for(cfg, 4)[: cfg.n_mel_frames * 80]])
    pid = _long_pid(cfg, plen)
    out = model.generate(feats, prompt_ids=pid, max_new_tokens=24, exponential_decay_length_penalty=(6, 1.3))
    gp = model._gen_params(None, None, (6, 1.3), 24, None, None, False, None, None, None, None, pid)
    assert gp.prompt[:plen] == pid.tolist() and out[0, : len(gp.prompt)].tolist() == gp.prompt
    enc = model.engine.encoder_output(2)
    for b in range(2):
        got = out[b].tolist()
        r = orc.decode(enc[b], gp)
        want = r.ids[: r.ids.index(gp.eos_token_id) + 1] if gp.eos_token_id in r.ids[len(gp.prompt):] else r.ids
        if got[: len(want)] != want:
            check_tokens(orc, enc[b], gp, model.engine.tokens(b), label=f"long history prompt {plen} {heads} b={b}")
        else:
            assert all(t == gp.pad_token_id for t in got[len(want):]), (b, got, want)
    model.engine.close()


# ---- 6. the position-dependent extras: each behind a 300-id prompt, 30 new tokens -------------------------------------------------------------
def test_candidate_tree_behind_a_300_id_prompt(gpu, monkeypatch):
    """The ancestor mask `(unsigned)(k - b0) < 64` with b0 >= 302 and the chosen path's K/V row moves up there: ids == Oracle.decode_tree, and the
    hidden-state carry is bit-identical to two passes (tests/test_gpu_tree.py)."""
    from test_gpu_tree import check_tree_tokens, decode_with_groups
    cfg = LH.cfg_for("base_head", medusa_choices=[1, 2, 2, 2, 2])          # 31 nodes: two 16-row query tiles per stream
    assert cfg.is_tree
    cfg, sd = LH.checkpoint("base_head", 25, cfg)
    model = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=2)
    eng = model.engine
    orc = Oracle(cfg, sd, sim="bf16")
    feats = model.extract_features([clip_for(cfg, 0), clip_for(cfg, 1)])
    gp = _gp(model, cfg, _long_pid(cfg, 300), max_new=30)
    assert len(gp.prompt) == 302
    runs = {}
    for carry in (True, False):
        if carry:
            monkeypatch.delenv("WM_NO_CARRY", raising=False)
        else:
            monkeypatch.setenv("WM_NO_CARRY", "1")
        eng.encode(feats)
        runs[carry] = eng.decode(gp, 2)
    monkeypatch.delenv("WM_NO_CARRY", raising=False)
    assert runs[True] == runs[False]
    enc = eng.encoder_output(2)

    def groups_of(b):
        eng.encode(feats)
        streamed, g = decode_with_groups(eng, gp, 2)
        assert streamed == runs[True]
        return g[b]
    for b in range(2):
        assert len(runs[True][b]) >= 302 + 30
        check_tree_tokens(orc, enc[b], gp, runs[True][b], f"long history tree b={b}", groups=lambda b=b: groups_of(b))
    eng.close()


def test_sibling_rows_behind_a_300_id_prompt(gpu, monkeypatch):
    """A sibling row's hidden state and K/V rows moved into place at rows > 300: ids == the chain's, with the rows on and off, and hits occur
    (tests/test_gpu_siblings.py).  Checkpoint seed and clips: long_history.SIBLING_SEED / SIBLING_CLIPS, where the oracle counts hits."""
    from test_gpu_siblings import _models
    cfg, sd = LH.checkpoint("base_head", LH.SIBLING_SEED)
    on, off = _models(gpu, monkeypatch, cfg, sd)
    orc = Oracle(cfg, sd, sim="bf16")
    gp = _gp(on, cfg, _long_pid(cfg, 300), max_new=30, temperature=0.0)
    hits = 0
    for i in LH.SIBLING_CLIPS:
        on.engine.set_encoder_output(orc.encode(LH.features(cfg, i))[None])          # the encoder output the clips were chosen on
        enc = on.engine.encoder_output(1)
        got_on = on.engine.decode(gp, 1)[0]
        st = on.engine.stats()
        off.engine.set_encoder_output(enc)
        got_off = off.engine.decode(gp, 1)[0]
        assert off.engine.stats()["sibling_hits"] == 0
        check_tokens(orc, enc[0], gp, got_on, f"long history siblings on clip {i}")
        if got_off != got_on:
            check_tokens(orc, enc[0], gp, got_off, f"long history siblings off clip {i}")
        r = orc.decode(enc[0], gp, siblings=5)
        if got_on == r.ids:
            assert st["sibling_hits"] == r.sibling_hits, (i, st["sibling_hits"], r.sibling_hits)
        hits += st["sibling_hits"]
    assert hits > 0
    on.engine.close(); off.engine.close()


def test_replays_deep_into_the_cache(gpu):
    """generate(return_token_logprobs=True, return_token_timestamps=True) on a run to the limit: the 16-row tiles of wm_score_tokens and
    wm_token_timestamps up to row 446.  Log-probabilities against tests/scores_ref.py on the oracle's teacher-forced logits at the bound of
    tests/test_gpu_scores.py; token timestamps against tests/token_ts_ref.py on the oracle's cross-attention as
    tests/test_gpu_token_timestamps.py::test_end_to_end_against_oracle does; the ids are the plain call's."""
    from test_gpu_scores import MAX_D as LP_MAX_D, MEAN_D as LP_MEAN_D
    from test_gpu_token_timestamps import SHARPEN as X_SHARPEN, hf_dtw, oracle_for
    cfg = LH.cfg_for("base_head")
    heads = synth.synth_alignment_heads(cfg, 2)
    cfg = dataclasses.replace(cfg, alignment_heads=heads)
    cfg, sd = LH.checkpoint("base_head", 31, cfg)
    for l, h in heads:                                # the recipe of test_gpu_token_timestamps.checkpoint
        p = f"whisper_model.model.decoder.layers.{l}.encoder_attn.q_proj"
        sd[p + ".weight"][h * 64:(h + 1) * 64] *= X_SHARPEN
        sd[p + ".bias"][h * 64:(h + 1) * 64] *= X_SHARPEN
    f16 = default_act_f16()
    model = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=1)
    feats = model.extract_features(clip_for(cfg, 0))
    sup = sorted({cfg.eos_token_id, 3, 5})
    kw = dict(exponential_decay_length_penalty=LH.EXP_DECAY, suppress_tokens=sup)
    plain = model.generate(feats, **kw)
    out = model.generate(feats, return_token_logprobs=True, return_token_timestamps=True, **kw)
    assert torch.equal(out["sequences"], plain)
    ids = out["sequences"][0].tolist()
    P = len(synth.default_prompt(cfg))
    assert LH.N_TGT - K - 1 <= len(ids) <= LH.N_TGT and cfg.eos_token_id not in ids[P:]
    enc = model.engine.encoder_output(1)[0]
    gp = model._gen_params(None, None, LH.EXP_DECAY, None, None, None, False, None, None, sup, None, None)
    # log-probabilities
    want = R.reference_scores(Oracle(cfg, sd, sim="bf16"), enc, ids, P, gp, cfg)
    lp = out["token_logprobs"][0].cpu()
    assert bool(torch.all(lp[:P] == 0)) and bool(torch.isfinite(lp[P: len(ids)]).all())
    d = np.asarray([abs(float(lp[t]) - want["logprobs"][t]) for t in range(P, len(ids))])
    deep = d[384 - P:]
    print(f"long history replays: {len(d)} log-probabilities, max |d| {d.max():.4g}, mean |d| {d.mean():.4g}; rows >= 384: {deep.max():.4g} / {deep.mean():.4g}")
    assert d.max() <= LP_MAX_D and d.mean() <= LP_MEAN_D, (float(d.max()), float(d.mean()))
    assert abs(float(out["avg_logprob"][0]) - want["avg_logprob"]) <= LP_MAX_D
    # token timestamps
    t_c = ref.token_timestamps(oracle_for(cfg, sd, "bf16", f16).alignment_weights(enc, ids, P, heads), P, cfg.median_filter_width, dtw_fn=hf_dtw)
    t_f = ref.token_timestamps(oracle_for(cfg, sd, "fp32", f16).alignment_weights(enc, ids, P, heads), P, cfg.median_filter_width, dtw_fn=hf_dtw)
    got = out["token_timestamps"][0, : len(ids)].cpu()
    e, y = (got - t_c)[P:].abs(), (t_f - t_c)[P:].abs()
    share_e, share_y = float((e <= 0.02 + 1e-6).float().mean()), float((y <= 0.02 + 1e-6).float().mean())
    print(f"long history replays: token timestamps within one frame of the contract oracle: engine {share_e:.3f}, fp32 oracle {share_y:.3f}, {e.numel()} tokens")
    record_table("long history replays", logprob_max=round(float(d.max()), 6), logprob_mean=round(float(d.mean()), 7), ts_engine_share=round(share_e, 4),
                 ts_yardstick_share=round(share_y, 4), tokens=len(d))
    assert share_y >= 0.8, "the reference pair itself disagrees: sharpen the test checkpoint's cross-attention"
    assert share_e >= share_y - 0.05, (share_e, share_y)
    model.engine.close()
