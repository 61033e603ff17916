"""Token log-probabilities, no-speech probability and quality gating on the GPU (include/wm.h wm_score_tokens / wm_score_rows).

The reference is tests/scores_ref.py: one teacher-forced oracle pass per stream, transformers' own processors per row at the row's own length,
fp64 log-softmax, transformers' static methods for the averages and ratios.  The reference always scores the ENGINE's ids."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import scores_ref as R
from helpers import MedusaConfig, GenParams, synth, clip_for, ACCEPT_TYPICAL, ACCEPT_GREEDY
from oracle.whisper_medusa_oracle import Oracle
from whisper_medusa import WhisperMedusaModel, scores as S

pytestmark = pytest.mark.gpu

TIE = 5e-4
ATOL_KERNEL = 2e-5      # 1e-5 (the fp32 Z the project holds to rtol 1e-5 against fp64, in log space) + two fp32 roundings at |lp| < 64 (3.8e-6 each)
MAX_D, MEAN_D = 0.12, 8e-3      # 2 x the logits bound of test_forward_logits_all_heads: |d(z_t - lse)| <= |dz_t| + max|dz|
SEEDS = {"base_head": 21, "medusa_block": 22}
NS_SCALE = 40.0
EXP_DECAY = (2, 1.2)      # ends the streams at different lengths (and puts the length penalty into the end-to-end runs)
# without the timestamp rules two of the four runs end all 12 streams at one length under (2, 1.2): those take another penalty (chosen on the
# reference alone; tests/test_scores_cpu.py asserts on the oracle that every run's streams differ in length)
DECAY_PLAIN = {("base_head", None): (2, 1.2), ("base_head", 0.0): (12, 1.15), ("medusa_block", None): (12, 1.15), ("medusa_block", 0.0): (2, 1.2)}


def decay_for(ht, temperature, ts):
    return EXP_DECAY if ts else DECAY_PLAIN[(ht, temperature)]


def _cfg(ht, ts, choices=None):
    if ts:
        return R.micro_ts(ht)
    return MedusaConfig.micro(K=4, heads_type=ht, medusa_choices=choices)


def _sd(cfg, ht, ts):
    return R.ts_state_dict(cfg, SEEDS[ht]) if ts else synth.synth_state_dict(cfg, seed=SEEDS[ht])


def clips(cfg, B):
    """B clips of different durations (ragged like the parity rig's): with the length penalty their streams end at different lengths."""
    out = []
    for i in range(B):
        c = clip_for(cfg, i)
        out.append(c[: len(c) * (12 - (i % 6) * 2) // 12] if i % 2 else c)
    return out


def _own(row, P, eos):
    s = [int(t) for t in row]
    return s[: s.index(eos, P) + 1] if eos in s[P:] else s


def crafted_rows(cfg):
    """The rows of test_select_rows_matches_hf (same prefixes, rng.standard_normal(V) * 2, timestamp block shifted by -3 / +3) with targets."""
    tb, V = cfg.timestamp_begin, cfg.vocab_size
    base = synth.default_prompt(cfg, timestamps=True)
    prefixes = [base, base + [tb + 3], base + [tb + 3, 40], base + [tb + 3, 40, tb + 9], base + [tb + 3, 40, tb + 9, tb + 9],
                base + [tb + 2, 17, 18, 19], base + [50, 51], base + [tb + 60, 9, tb + 61, tb + 61, 12, 13]]
    rng = np.random.default_rng(5)
    rows, pre, tgt = [], [], []
    for k, p in enumerate(prefixes):
        for scale_ts in (-3.0, 3.0):
            x = rng.standard_normal(V).astype(np.float32) * 2.0
            x[tb:] += scale_ts
            for target in (int(rng.integers(0, tb)), tb + 4, int(rng.integers(tb, V)), cfg.eos_token_id, cfg.no_timestamps_token_id):
                rows.append(x); pre.append(p); tgt.append(target)
    return rows, pre, tgt


def _gp(cfg, timestamps, **kw):
    prompt = synth.default_prompt(cfg, timestamps=timestamps)
    base = dict(prompt=prompt, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id, suppress_tokens=[], begin_suppress_tokens=[],
                max_length=cfg.max_target_positions, hard_max_length=cfg.max_length, accept_mode=ACCEPT_TYPICAL, temperature=1.0,
                timestamps=timestamps, no_timestamps_token_id=cfg.no_timestamps_token_id if timestamps else -1,
                max_initial_timestamp_index=cfg.max_initial_timestamp_index if timestamps else None)
    base.update(kw)
    return GenParams(**base)


def _check_tap(m, cfg, gp, rows, pre, tgt, label):
    got = m.engine.score_rows(gp, np.stack(rows), pre, tgt)
    proc = R.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
    n_masked = 0
    for r in range(len(rows)):
        want, margin = R.row_logprob(torch.from_numpy(rows[r]), pre[r], tgt[r], gp, proc)
        assert margin >= TIE, (label, r, margin)            # no crafted row sits on the timestamp decision
        if want == -float("inf"):
            n_masked += 1
            assert got[r] == -np.inf, (label, r, got[r])
        else:
            assert abs(float(got[r]) - want) <= ATOL_KERNEL, (label, r, float(got[r]), want)
    return n_masked


# ---- 1. the scoring kernels against HF on crafted rows -------------------------------------------------------------------------------------
def test_score_rows_matches_hf(gpu):
    cfg = R.micro_ts("base_head")
    m = WhisperMedusaModel(cfg, R.ts_state_dict(cfg, 21), device=gpu, max_batch=1, act_fp16=False)
    tb = cfg.timestamp_begin
    rows, pre, tgt = crafted_rows(cfg)
    n = _check_tap(m, cfg, _gp(cfg, True), rows, pre, tgt, "ts")
    assert 0 < n < len(rows)
    # suppress list, begin-suppress at t == begin_index, exponential decay on the rows long enough for it
    gp2 = _gp(cfg, True, suppress_tokens=[3, 40], begin_suppress_tokens=[tb + 2, 7], exp_decay=(2, 1.3))
    base = list(gp2.prompt)
    rows2 = rows + [rows[0], rows[0], rows[1]]
    pre2 = pre + [base, base, base]
    tgt2 = tgt + [tb + 2, tb + 1, tb + 2]                    # begin-suppressed timestamp: -inf; its neighbour: finite
    n2 = _check_tap(m, cfg, gp2, rows2, pre2, tgt2, "ts+processors")
    assert n2 > n
    # rules off: plain processors at the row's own length
    gp3 = _gp(cfg, False, suppress_tokens=[3, 5], begin_suppress_tokens=[7, cfg.eos_token_id], exp_decay=(1, 1.5))
    b3 = list(gp3.prompt)
    pre3 = [b3, b3, b3 + [9], b3 + [9, 10, 11], b3 + [9, 10, 11, 12, 13]]
    tgt3 = [7, 8, 7, cfg.eos_token_id, cfg.eos_token_id]
    n3 = _check_tap(m, cfg, gp3, [rows[i] for i in range(5)], pre3, tgt3, "plain")
    assert n3 == 1
    with pytest.raises(ValueError, match="vocabulary"):
        m.engine.score_rows(gp3, np.stack(rows[:1]), pre3[:1], [cfg.vocab_size])
    m.engine.close()


# ---- 2. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rigs():
    cache = {}

    def get(ht, ts, choices=None):
        key = (ht, ts, tuple(choices or ()))
        if key not in cache:
            cfg = _cfg(ht, ts, choices)
            sd = _sd(cfg, ht, ts)
            cache[key] = (cfg, sd, Oracle(cfg, sd, sim="bf16", act="hilo"))
        return cache[key]
    return get


def _compare(m, cfg, orc, out, B, ts, temperature, vanilla, label, max_new, decay=None, prompt_ids=None):
    gp = m._gen_params(None, None, decay, max_new, None, temperature, vanilla, None, None, None, None, prompt_ids, timestamps=ts)
    sot = len(prompt_ids) if prompt_ids is not None else 0
    P, eos = len(gp.prompt), gp.eos_token_id
    seq, lp = out["sequences"].cpu(), out["token_logprobs"].cpu()
    assert lp.dtype == torch.float32 and lp.shape == seq.shape
    enc = m.engine.encoder_output(B)
    ns_tok = cfg.no_speech_token_id
    d_all, n_rows, n_out = [], 0, 0
    lens, avg_fail = [], False
    for b in range(B):
        ids = seq[b].tolist()[: int(out["lengths"][b])]     # (pad == eos: the row alone cannot tell a stream's EOS from its padding)
        assert ids == _own(ids, P, eos)
        lens.append(len(ids))
        ref = R.reference_scores(orc, enc[b], ids, P, gp, cfg, sot, ns_tok)
        kept = []
        assert torch.all(lp[b, :P] == 0) and torch.all(lp[b, len(ids):] == 0)
        assert torch.isfinite(lp[b, P: len(ids)]).all(), (label, b, lp[b])
        for t in range(P, len(ids)):
            n_rows += 1
            if ts and ref["margins"][t] < MAX_D:
                n_out += 1
                continue
            kept.append(t)
            d_all.append(abs(float(lp[b, t]) - ref["logprobs"][t]))
        print(f"scores[{label}] stream {b}: avg_logprob {float(out['avg_logprob'][b]):.5f} (reference {ref['avg_logprob']:.5f}), largest |d| "
              f"{max(abs(float(lp[b, t]) - ref['logprobs'][t]) for t in range(P, len(ids))):.4g} at "
              f"{max(range(P, len(ids)), key=lambda t: abs(float(lp[b, t]) - ref['logprobs'][t]))}")
        if len(kept) == len(ids) - P:
            avg_fail = avg_fail or abs(float(out["avg_logprob"][b]) - ref["avg_logprob"]) > MAX_D
        elif kept:      # a left-out row's score may sit on the other side of the decision: the averages over the kept rows
            a_got = sum(float(lp[b, t]) for t in kept) / len(kept)
            a_ref = sum(ref["logprobs"][t] for t in kept) / len(kept)
            avg_fail = avg_fail or abs(a_got - a_ref) > MAX_D
        assert float(out["compression_ratio"][b]) == pytest.approx(ref["compression_ratio"], rel=1e-6)
        assert abs(math.log(float(out["no_speech_prob"][b])) - math.log(ref["no_speech_prob"])) <= MAX_D, (label, b)
        assert float(out["avg_logprob"][b]) == pytest.approx(S.avg_logprob(lp[b].tolist(), P, len(ids)), abs=1e-5)
    d = np.asarray(d_all)
    print(f"scores[{label}]: {n_rows} rows, {n_out} left out (decision margin < {MAX_D}), max |d| {d.max():.4g}, mean |d| {d.mean():.4g}; lens {lens}")
    assert n_out <= 0.10 * n_rows, (label, n_out, n_rows)
    assert d.max() <= MAX_D and d.mean() <= MEAN_D, (label, float(d.max()), float(d.mean()))
    assert not avg_fail, label
    return lens


def _ragged(m, cfg, orc, out, B, ts, temperature, decay):
    """Streams of different lengths whatever the decode gave: the run's own ids cut to four different lengths, scored in one call."""
    gp = m._gen_params(None, None, decay, 40, None, temperature, False, None, None, None, None, None, timestamps=ts)
    P, eos = len(gp.prompt), gp.eos_token_id
    own = [r[: int(out["lengths"][b])] for b, r in enumerate(out["sequences"].cpu().tolist())]
    cut = [s[: max(P + 2, len(s) - 2 * (b % 4))] for b, s in enumerate(own)]
    assert len({len(c) for c in cut}) > 1
    lp, _, _ = m.engine.score_tokens(cut, P, gp)
    enc = m.engine.encoder_output(B)
    d = []
    for b, c in enumerate(cut):
        ref = R.reference_scores(orc, enc[b], c, P, gp, cfg)
        assert np.all(lp[b, :P] == 0) and np.all(lp[b, len(c):] == 0) and np.isfinite(lp[b, P: len(c)]).all()
        d += [abs(float(lp[b, t]) - ref["logprobs"][t]) for t in range(P, len(c)) if not (ts and ref["margins"][t] < MAX_D)]
    d = np.asarray(d)
    print(f"scores[ragged B={B} ts={ts}]: lens {[len(c) for c in cut]}, max |d| {d.max():.4g}, mean |d| {d.mean():.4g}")
    assert d.max() <= MAX_D and d.mean() <= MEAN_D


@pytest.mark.parametrize("ts", [False, True])
@pytest.mark.parametrize("B", [1, 12])
@pytest.mark.parametrize("temperature", [None, 0.0])
@pytest.mark.parametrize("ht", ["base_head", "medusa_block"])
def test_generate_token_logprobs(gpu, rigs, ht, temperature, B, ts):
    cfg, sd, orc = rigs(ht, ts)
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=B, act_fp16=False)
    feats = m.extract_features(clips(cfg, B))
    decay = decay_for(ht, temperature, ts)
    out = m.generate(feats, return_token_logprobs=True, return_timestamps=ts, temperature=temperature, max_new_tokens=40,
                     exponential_decay_length_penalty=decay)
    lens = _compare(m, cfg, orc, out, B, ts, temperature, False, f"{ht} T={temperature} B={B} ts={ts}", 40, decay)
    if B > 1:
        assert len(set(lens)) > 1, lens         # generate() packs streams of different lengths
        _ragged(m, cfg, orc, out, B, ts, temperature, decay)
    assert m.last_stats["ms_token_logprobs"] > 0
    m.engine.close()


def test_generate_token_logprobs_vanilla_and_tree(gpu, rigs):
    cfg, sd, orc = rigs("base_head", False)
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=2, act_fp16=False)
    feats = m.extract_features([clip_for(cfg, i) for i in range(2)])
    out = m.generate(feats, return_token_logprobs=True, vanilla=True, max_new_tokens=32)
    _compare(m, cfg, orc, out, 2, False, None, True, "vanilla", 32)
    m.engine.close()
    cfg, sd, orc = rigs("base_head", False, [1, 2, 2, 1, 1])
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=2, act_fp16=False)
    out = m.generate(feats, return_token_logprobs=True, max_new_tokens=32)
    _compare(m, cfg, orc, out, 2, False, None, False, "tree", 32)
    m.engine.close()


@pytest.mark.parametrize("n_prev", [17, 30])
def test_long_prompt_ids_with_timestamps(gpu, rigs, n_prev):
    """prompt_ids that fill the first 16-row tile (and the second), a timestamp of the previous text among them: the prompt's tokens reach the
    timestamp state of the later tiles exactly as they reach the decode's, and <|startoftranscript|> sits at index len(prompt_ids)."""
    cfg, sd, orc = rigs("base_head", True)
    tb = cfg.timestamp_begin
    pid = [cfg.prev_sot_token_id] + [10 + i for i in range(n_prev - 4)] + [tb + 7, 44, tb + 9]
    assert len(pid) == n_prev
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=2, act_fp16=False)
    feats = m.extract_features([clip_for(cfg, 0), clip_for(cfg, 1)])
    for rep_ in range(2):       # the second call starts from the state the first one left
        out = m.generate(feats, return_token_logprobs=True, return_timestamps=True, prompt_ids=torch.tensor(pid), max_new_tokens=16)
        assert out["sequences"][0, : n_prev].tolist() == pid
        _compare(m, cfg, orc, out, 2, True, None, False, f"prompt_ids[{n_prev}] call {rep_}", 16, None, pid)
    m.engine.close()


def test_language_groups_carry_their_scores(gpu):
    """language=None on a multilingual checkpoint: the clips are decoded in groups per detected language; every clip's score fields are those of
    a call on the clip alone in its language."""
    cfg = MedusaConfig.micro(K=4)           # the checkpoint of tests/test_gpu_features.py::test_language_detection_groups_clips
    cfg.is_multilingual = True
    cfg.lang_to_id = {"<|en|>": 20, "<|de|>": 21, "<|fr|>": 22}
    cfg.task_to_id = {"transcribe": 30, "translate": 31}
    sd = synth.synth_state_dict(cfg, seed=43)
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=4, act_fp16=False)
    feats = m.extract_features([clip_for(cfg, i) for i in range(4)])
    out = m.generate(feats, return_token_logprobs=True, max_new_tokens=16)
    langs = list(m.detected_languages)
    assert out["token_logprobs"].shape == out["sequences"].shape and out["avg_logprob"].shape == (4,)
    for b in range(4):
        alone = m.generate(feats[b: b + 1], language=langs[b], return_token_logprobs=True, max_new_tokens=16)
        n = int(alone["lengths"][0])
        assert int(out["lengths"][b]) == n and out["sequences"][b, :n].tolist() == alone["sequences"][0, :n].tolist()
        assert torch.allclose(out["token_logprobs"][b, :n], alone["token_logprobs"][0, :n], atol=1e-4)
        assert torch.all(out["token_logprobs"][b, n:] == 0)
        assert float(out["avg_logprob"][b]) == pytest.approx(float(alone["avg_logprob"][0]), abs=1e-4)
        assert float(out["no_speech_prob"][b]) == pytest.approx(float(alone["no_speech_prob"][0]), rel=1e-3)
    m.engine.close()


def test_segments_carry_their_logprobs_and_pool(gpu, rigs):
    cfg, sd, _ = rigs("base_head", True)
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=2, act_fp16=False)
    feats = m.extract_features([clip_for(cfg, 0), clip_for(cfg, 1)])
    d = m.generate(feats, return_timestamps=True, return_segments=True, return_token_logprobs=True, max_new_tokens=40)
    P = len(synth.default_prompt(cfg, timestamps=True))
    for i in range(2):
        o = P
        assert len(d["segments"][i]) >= 1
        for sg in d["segments"][i]:
            n = int(sg["tokens"].numel())
            assert torch.equal(sg["token_logprobs"], d["token_logprobs"][i, o: o + n])
            o += n
    m.set_micro_batches(2)
    p = m.generate(feats, return_timestamps=True, return_token_logprobs=True, max_new_tokens=40)
    assert torch.equal(p["sequences"], d["sequences"])
    assert torch.allclose(p["token_logprobs"], d["token_logprobs"], atol=1e-4)
    with pytest.raises(NotImplementedError):
        class Odd:
            def __call__(self, ids, scores):
                return scores
        m.generate(feats, return_token_logprobs=True, logits_processor=[Odd()], max_new_tokens=8)


# ---- 3. gating ----------------------------------------------------------------------------------------------------------------------------
def _no_speech_model(gpu, rigs, B):
    """The timestamp checkpoint with the proj_out row of <|nospeech|> scaled so that its raw logit dominates the <|startoftranscript|> row."""
    cfg, sd, _ = rigs("base_head", True)
    sd = {k: v.clone() for k, v in sd.items()}
    m0 = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=B, act_fp16=False)
    feats = m0.extract_features([clip_for(cfg, i) for i in range(B)])
    m0.engine.encode(feats)
    z = m0.engine.forward_logits([[cfg.decoder_start_token_id]] * B, 0, True)[0, :, 0]
    sign = torch.sign(z[:, cfg.no_speech_token_id])
    m0.engine.close()
    assert torch.all(sign == sign[0]) and sign[0] != 0, z[:, cfg.no_speech_token_id]
    w = sd["whisper_model.proj_out.weight"]
    w[cfg.no_speech_token_id] *= float(sign[0]) * NS_SCALE
    sd["whisper_model.model.decoder.embed_tokens.weight"] = w
    return cfg, WhisperMedusaModel(cfg, sd, device=gpu, max_batch=B, act_fp16=False), feats


def test_no_speech_skip(gpu, rigs):
    cfg, m, feats = _no_speech_model(gpu, rigs, 2)
    P = len(synth.default_prompt(cfg, timestamps=True))
    d = m.generate(feats, return_timestamps=True, no_speech_threshold=0.6, logprob_threshold=None, return_dict_in_generate=True, max_new_tokens=24)
    assert bool(d["skipped"].all()) and float(d["no_speech_prob"].min()) > 0.9
    for b in range(2):
        assert d["sequences"][b].tolist()[: P + 1] == synth.default_prompt(cfg, timestamps=True) + [cfg.eos_token_id]
        assert d["sequences"].shape[1] == P + 1
    lf = torch.cat([feats[0:1], feats[1:2]], dim=-1)
    o = m.generate(lf, chunk_longform=True, return_timestamps=True, return_segments=True, no_speech_threshold=0.6, max_new_tokens=24)
    assert o["segments"] == [[]] and o["sequences"].shape[1] == P + 1 and bool(o["skipped"].all())
    m.engine.close()


def test_per_window_skip_and_needs_fallback(gpu, rigs):
    cfg, m, feats = _no_speech_model(gpu, rigs, 2)
    P = len(synth.default_prompt(cfg, timestamps=True))
    lf = torch.cat([feats[0:1], feats[1:2]], dim=-1)
    kw = dict(chunk_longform=True, return_timestamps=True, return_segments=True, max_new_tokens=24)
    free = m.generate(lf, return_token_logprobs=True, **kw)
    a = free["window_avg_logprob"][0].tolist()
    assert a[0] != a[1]
    thr = 0.5 * (a[0] + a[1])
    low = 0 if a[0] < a[1] else 1
    g = m.generate(lf, no_speech_threshold=0.6, logprob_threshold=thr, **kw)
    assert g["skipped"][0].tolist() == [low == 0, low == 1]
    win = m.generate(feats, return_timestamps=True, return_segments=True, max_new_tokens=24)
    keep = 1 - low
    want_ids = [t for t in win["sequences"][keep].tolist()[P:] if t not in (cfg.eos_token_id, cfg.pad_token_id)]
    assert g["sequences"][0].tolist()[P:-1] == want_ids
    F = cfg.n_mel_frames
    from whisper_medusa.timestamps import row_segments
    ws = row_segments(win["sequences"][keep].tolist(), P, cfg.eos_token_id, cfg.timestamp_begin, F, time_offset=keep * F * 0.01)
    assert len(g["segments"][0]) == len(ws) >= 1
    for x, y in zip(g["segments"][0], ws):
        assert torch.allclose(x["start"], y["start"]) and torch.allclose(x["end"], y["end"]) and torch.equal(x["tokens"].cpu(), y["tokens"].cpu())
    # needs_fallback: HF's _need_fallback rule on the returned figures
    s = m.generate(feats, return_timestamps=True, return_token_logprobs=True, logprob_threshold=thr, compression_ratio_threshold=1.2, max_new_tokens=24)
    for b in range(2):
        want = S.needs_fallback(float(s["avg_logprob"][b]), float(s["compression_ratio"][b]), thr, 1.2)
        assert bool(s["needs_fallback"][b]) == want
    assert "skipped" not in s
    m.engine.close()


# ---- 4. off means off ---------------------------------------------------------------------------------------------------------------------
def test_off_means_off(gpu, rigs):
    cfg, sd, _ = rigs("base_head", False)
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=2, act_fp16=False)
    feats = m.extract_features([clip_for(cfg, 0), clip_for(cfg, 1)])

    def run():
        ids = m.generate(feats, max_new_tokens=32)
        st = dict(m.last_stats)
        return ids, {k: st[k] for k in ("iterations", "tokens_emitted", "accept_hist", "graph_replays", "schedule_steps")}
    m.generate(feats, max_new_tokens=32)        # first call captures the graph
    ids0, st0 = run()
    sc = m.generate(feats, return_token_logprobs=True, max_new_tokens=32)
    assert torch.equal(sc["sequences"], ids0)
    ids1, st1 = run()
    assert torch.equal(ids0, ids1) and st0 == st1, (st0, st1)
    assert "ms_token_logprobs" not in m.last_stats
    m2 = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=1, act_fp16=False)
    with pytest.raises(RuntimeError, match="wm_encode first"):           # WM_ERR_STATE without a resident encoder pass
        m2.engine.score_tokens([[1, 2, 3]], 1, _gp(cfg, False))
    m2.engine.close()
    with pytest.raises(ValueError, match="n_tgt|lens"):
        m.engine.score_tokens([[1] * (cfg.max_target_positions + 1)], 1, _gp(cfg, False))
    with pytest.raises(ValueError, match="vocabulary"):
        m.engine.score_tokens([[1, cfg.vocab_size, 3]], 1, _gp(cfg, False))
    m.engine.close()
