"""repetition_penalty / no_repeat_ngram_size inside the engine's decode loop (include/wm.h wm_set_repeat_rules).

Every comparison is against transformers' own RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor (tests/repeat_ref.py), applied to
each logits row under the prefix the contract gives it: base / head rows the committed ids, verify row i the committed ids + c_0 .. c_i."""
import dataclasses

import numpy as np
import pytest
import torch

from helpers import MedusaConfig, GenParams, synth, clip_for, ACCEPT_TYPICAL, ACCEPT_GREEDY
from whisper_medusa import WhisperMedusaModel
import repeat_ref as R
import scores_ref as SR

pytestmark = pytest.mark.gpu

TIE = 5e-4          # the project's tie rule (tests/helpers.py check_tokens)
TIE_P = 2e-3
ATOL_KERNEL = 2e-5  # tests/test_gpu_scores.py: the scoring tap's log-prob tolerance
# tests/test_gpu_scores.py MAX_D / MEAN_D bound |d(z_t - lse)| by |dz_t| + max|dz| of the replayed logits; step 1 multiplies a negative logit by p
# (divides a positive one by p), so with p = 1.3 both terms grow by at most max(p, 1 / p) = 1.3
PEN = 1.3
MAX_D, MEAN_D = 0.12 * PEN, 8e-3 * PEN
SEL_SP = 16         # csrc/wm_select.h: vocabulary slices of the select kernels
LOOP = [40, 41, 42, 43, 44, 45, 300, 301]
LOOP_SCALE = 2.0    # random-weight micro models hardly repeat themselves: eight rows of the tied embedding are scaled (as the timestamp tests
#                     scale the timestamp rows) until the plain decode holds >= 8 repeated bigrams (chosen on the CPU reference alone).  A power
#                     of two: the scaled rows stay exact in bf16, so the engine's packed weights and the oracle's are the same numbers
SEEDS = {"base_head": 31, "medusa_block": 32}
SETTINGS = {"g2": (1.0, 2), "p1.3_g3": (PEN, 3)}


def loop_state_dict(cfg, seed):
    sd = synth.synth_state_dict(cfg, seed=seed)
    sd["whisper_model.proj_out.weight"][LOOP] *= LOOP_SCALE          # (tied: the embedding rows change with it; engine and reference share sd)
    return sd


def gen_params(cfg, mode, max_new, pen=1.0, g=0, **kw):
    prompt = synth.default_prompt(cfg)
    base = dict(prompt=prompt, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id, suppress_tokens=[3, 5],
                begin_suppress_tokens=list(cfg.begin_suppress_tokens), max_length=min(len(prompt) + max_new, cfg.max_target_positions),
                hard_max_length=cfg.max_length, accept_mode=mode, temperature=1.0 if mode == ACCEPT_TYPICAL else 0.0,
                repetition_penalty=pen, no_repeat_ngram_size=g)
    base.update(kw)
    return GenParams(**base)


@pytest.fixture(scope="module")
def rig(gpu):
    out = {}
    for ht, seed in SEEDS.items():
        cfg = MedusaConfig.micro(K=4, heads_type=ht)
        sd = loop_state_dict(cfg, seed)
        out[ht] = (cfg, sd, R.RepRef(cfg, sd))
    out["refs"] = {}
    return out


def _model(cfg, sd, gpu, B):
    return WhisperMedusaModel(cfg, sd, device=gpu, max_batch=B, act_fp16=False)       # the oracle's contract (bf16 hi / lo), as the timestamp tests


def _ref(rig, ht, clip, enc, gp, rules=True):
    """One reference decode per (model, clip, parameters), shared by the tests of this module."""
    key = (ht, clip, gp.accept_mode, gp.vanilla, gp.repetition_penalty if rules else 1.0, gp.no_repeat_ngram_size if rules else 0, gp.max_length)
    if key not in rig["refs"]:
        rig["refs"][key] = rig[ht][2].decode(enc, gp, rules=rules)
    return rig["refs"][key]


def assert_same(got, ref, label, P):
    """Strict equality, or a first difference at a decision within TIE (then the runs agree up to it): at most one such tie."""
    ids, marg, _ = ref
    if got == ids:
        return 0
    first = next((i for i, (a, b) in enumerate(zip(got, ids)) if a != b), min(len(got), len(ids)))
    m = marg[first - P] if 0 <= first - P < len(marg) else (float("inf"), float("inf"))
    print(f"repeat[{label}]: first difference at {first}; smallest margins of that iteration: logit {m[0]:.3g}, p_c {m[1]:.3g} (relative)")
    assert m[0] < TIE or m[1] < TIE_P, (label, first, m, got, ids)
    return 1


def check_nonvacuous(rig, ht, clip, enc, gp, ref, label):
    """From the reference alone: the rules change the ids, and at least 3 emitted positions had their unprocessed arg-max banned or overtaken."""
    plain = _ref(rig, ht, clip, enc, gp, rules=False)
    assert plain[0] != ref[0], (label, "the rules change nothing")
    assert sum(ref[2]) >= 3, (label, "fewer than 3 positions moved by the rules", sum(ref[2]))


# ---- 1. the taps against HF on crafted rows ------------------------------------------------------------------------------------------------
def tap_cfg(ts):
    c = MedusaConfig.micro(K=4, n_tgt=448)
    if ts:
        tb = c.vocab_size - (c.max_source_positions + 1)
        c = dataclasses.replace(c, eos_token_id=tb - 4, pad_token_id=tb - 4, decoder_start_token_id=tb - 3, prev_sot_token_id=tb - 2,
                                no_timestamps_token_id=tb - 1, begin_suppress_tokens=[7, tb - 4], max_initial_timestamp_index=5)
        assert c.supports_timestamps
    return c


def crafted(cfg, g, ts, rng):
    """(prefix, [probe tokens]) cases.  The slices of the select kernels are ceil(V / SEL_SP) tokens wide: tokens at both sides of the first two
    slice edges, token 0 and token V - 1 are followers / penalised tokens."""
    V = cfg.vocab_size
    per = -(-V // SEL_SP)
    edge = [per - 1, per, 2 * per - 1, 2 * per, 0, V - 1]
    gg = max(g, 1)
    S = [200 + k for k in range(gg - 1)]                    # the repeated (g - 1)-gram
    cases = []
    for n in sorted({1, max(gg - 1, 1), gg, gg + 1}):        # lengths 1, g - 1, g, g + 1: one token throughout (len == g bans it: the only n-gram)
        cases.append(([edge[0]] * n, [edge[0], edge[1]]))
    a, b = edge[1], edge[5]
    cases.append((S + [a] + S + [b] + S, [a, b, edge[2]]))                  # the suffix occurs three times, two distinct followers
    cases.append((S + [edge[2]] + S + [edge[2]] + S, [edge[2], edge[3]]))   # the same follower twice
    cases.append((edge + S + [edge[4]] + S, [edge[4], edge[3], edge[5]]))   # every edge token in the prefix (penalised), follower 0
    if not ts:
        for n in (255, 256, 257, 447):                       # more ids than one block of threads walks at once
            pre = rng.choice(np.asarray(edge + [300, 301, 302]), size=n).tolist()
            cases.append((pre, [pre[-1], edge[0], 302]))
    if ts:                                                   # the timestamp rules read ids[begin_index:]: every prefix starts with the prompt
        prompt = synth.default_prompt(cfg, timestamps=True)
        tb = cfg.timestamp_begin
        cases = [(prompt + [t if t < tb else tb - 10 for t in p], q) for p, q in cases]
        cases.append((prompt + [tb + 3, 40, tb + 9] + S + [a] + S, [a, tb + 9, tb + 10]))
    return cases


def tap_rows(cfg, cases, rng):
    rows, pre, probe = [], [], []
    for p, probes in cases:
        x = (rng.standard_normal(cfg.vocab_size) * 2.0).astype(np.float32)
        x[p[0]] = abs(x[p[0]]) + 0.5                         # a penalised token with a positive and one with a negative logit, whatever the draw
        x[p[-1]] = (-abs(x[p[-1]]) - 0.5) if p[-1] != p[0] else x[p[-1]]
        for t in probes:
            rows.append(x); pre.append(list(p)); probe.append(int(t))
    return rows, pre, probe


TAP_SETTINGS = [(1.3, 0), (0.8, 0), (1.0, 1), (1.0, 2), (1.0, 3), (1.0, 5), (1.3, 1), (0.8, 2), (1.3, 3), (0.8, 5)]


@pytest.fixture(scope="module")
def tap_models(gpu):
    out = {}
    for ts in (False, True):
        cfg = tap_cfg(ts)
        out[ts] = (cfg, _model(cfg, synth.synth_state_dict(cfg, seed=5), gpu, 1))
    yield out
    for _, m in out.values():
        m.engine.close()


@pytest.mark.parametrize("ts", [False, True])
@pytest.mark.parametrize("pen,g", TAP_SETTINGS)
def test_taps_match_hf(tap_models, pen, g, ts):
    cfg, m = tap_models[ts]
    rng = np.random.default_rng(7 + g)
    prompt = synth.default_prompt(cfg, timestamps=ts)
    gp = GenParams(prompt=prompt, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id, suppress_tokens=[3, 5], begin_suppress_tokens=[],
                   max_length=cfg.max_target_positions, hard_max_length=cfg.max_length, accept_mode=ACCEPT_TYPICAL, temperature=1.0,
                   timestamps=ts, no_timestamps_token_id=cfg.no_timestamps_token_id if ts else -1,
                   max_initial_timestamp_index=cfg.max_initial_timestamp_index if ts else None, repetition_penalty=pen, no_repeat_ngram_size=g)
    rows, pre, probe = tap_rows(cfg, crafted(cfg, g, ts, rng), rng)
    sel = m.engine.select_rows(gp, np.stack(rows), pre, probe)
    sco = m.engine.score_rows(gp, np.stack(rows), pre, probe)
    ts_proc = SR.hf_processor(cfg, gp.begin_index) if ts else None
    n_banned = n_pen = 0
    for r in range(len(rows)):
        z = torch.from_numpy(rows[r])
        want = R.hf_row(z, pre[r], gp, None, ts_proc).double()
        if ts and SR.decision_margin(SR.masks_only(ts_proc)(torch.tensor([pre[r]]), R.hf_row(z, pre[r], gp, None, None)[None].clone())[0],
                                     cfg.timestamp_begin) < TIE:
            continue                                         # (a row on the timestamp decision: either side is right)
        plain = R.hf_row(z, pre[r], gp, None, ts_proc, rules=False)
        n_pen += bool((torch.isfinite(want) & (want != plain.double())).any())      # a penalised token that is not banned or masked as well
        p = torch.softmax(want, 0)
        H = float(-(p * torch.log(p + 1e-5)).sum())
        lp = float(torch.log_softmax(want, 0)[probe[r]])
        assert int(sel["argmax"][r]) == int(torch.argmax(want)) or R.top2_gap(want) < TIE, (r, pre[r][-8:], sel["argmax"][r])
        np.testing.assert_allclose(sel["p_probe"][r], float(p[probe[r]]), rtol=1e-5, atol=1e-7, err_msg=f"row {r}")
        np.testing.assert_allclose(sel["entropy"][r], H, rtol=1e-5, atol=1e-6, err_msg=f"row {r}")
        if want[probe[r]] == -float("inf"):
            n_banned += bool(torch.isfinite(plain[probe[r]]))
            assert sel["p_probe"][r] == 0.0 and sco[r] == -np.inf, (r, sel["p_probe"][r], sco[r])
        else:
            assert abs(float(sco[r]) - lp) <= ATOL_KERNEL, (r, float(sco[r]), lp)
    # the crafted cases are not vacuous (with the timestamp rules on most probes are already masked by those: one banned / penalised probe)
    if g:
        assert n_banned >= (1 if ts else 3), n_banned
    if pen != 1.0 and g != 1:                               # (g == 1 bans every token of the prefix: the penalty then shows nowhere)
        assert n_pen >= 3, n_pen


def test_banned_eos_under_exponential_decay_is_minus_inf(tap_models):
    """The one deviation from HF (which computes -inf + inf * k = NaN there): a banned EOS stays -inf under the exponential decay."""
    cfg, m = tap_models[False]
    eos = cfg.eos_token_id
    gp = gen_params(cfg, ACCEPT_TYPICAL, 40, 1.0, 1, exp_decay=(1, 1.5), begin_suppress_tokens=[], max_length=cfg.max_target_positions)
    pre = list(gp.prompt) + [9, eos, 10, 11]
    x = np.random.default_rng(3).standard_normal(cfg.vocab_size).astype(np.float32)
    got = m.engine.score_rows(gp, np.stack([x, x]), [pre, pre], [eos, 12])
    assert got[0] == -np.inf and np.isfinite(got[1])


# ---- 2. / 5. the decode loop equals the reference loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("B", [1, 12])
@pytest.mark.parametrize("ht", ["base_head", "medusa_block"])
def test_decode_matches_reference(gpu, rig, ht, B, setting):
    """Typical acceptance: one stream (sibling rows on, their default) and 12 streams (merged-step schedule)."""
    cfg, sd, _ = rig[ht]
    pen, g = SETTINGS[setting]
    m = _model(cfg, sd, gpu, B)
    gp = gen_params(cfg, ACCEPT_TYPICAL, 48, pen, g)
    P = len(gp.prompt)
    clips = [clip_for(cfg, i) for i in range(2)]
    got_all = []
    if B == 1:
        for c in clips:
            m.engine.encode(m.extract_features(c))
            got_all.append((m.engine.decode(gp, 1)[0], m.engine.encoder_output(1)[0]))
    else:
        m.engine.encode(m.extract_features(clips * (B // 2)))
        enc = m.engine.encoder_output(B)
        seqs = m.engine.decode(gp, B)
        assert m.engine.stats()["schedule_steps"] > 0
        got_all = [(seqs[i], enc[i]) for i in range(2)]
        assert all(seqs[i] == seqs[i % 2] for i in range(B))
    ties = 0
    for i, (got, enc) in enumerate(got_all):
        label = f"{ht} B={B} {setting} clip {i}"
        r = _ref(rig, ht, i, enc, gp)
        check_nonvacuous(rig, ht, i, enc, gp, r, label)
        ties += assert_same(got, r, label, P)
        own = got[: got.index(gp.eos_token_id, P) + 1] if gp.eos_token_id in got[P:] else got
        if ties == 0:
            assert R.repeated_ngrams(own, g) == 0, (label, own)
    assert ties <= 1
    m.engine.close()


# ---- 3. greedy: Medusa == vanilla == reference --------------------------------------------------------------------------------------------------
def test_greedy_equals_vanilla_equals_reference(gpu, rig):
    cfg, sd, _ = rig["base_head"]
    m = _model(cfg, sd, gpu, 1)
    pen, g = SETTINGS["p1.3_g3"]
    gp = gen_params(cfg, ACCEPT_GREEDY, 40, pen, g)
    gv = dataclasses.replace(gp, vanilla=True)
    P = len(gp.prompt)
    ties = 0
    for i in range(2):
        m.engine.encode(m.extract_features(clip_for(cfg, i)))
        enc = m.engine.encoder_output(1)[0]
        med = m.engine.decode(gp, 1)[0]
        van = m.engine.decode(gv, 1)[0]
        r = _ref(rig, "base_head", i, enc, gv)
        check_nonvacuous(rig, "base_head", i, enc, gv, r, f"vanilla clip {i}")
        n = min(len(med), len(van))
        assert med[:n] == van[:n], (med, van)
        ties += assert_same(van, r, f"vanilla clip {i}", P)
    assert ties <= 1
    m.engine.close()


# ---- 4. sibling rows compose: on / off --------------------------------------------------------------------------------------------------------------
def test_sibling_rows_do_not_change_ids(gpu, rig, monkeypatch):
    cfg, sd, _ = rig["base_head"]
    monkeypatch.setenv("WM_SIBLINGS", "0")
    off = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=1, act_fp16=False)
    monkeypatch.setenv("WM_SIBLINGS", "5")
    on = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=1, act_fp16=False)
    diffs = hits = 0
    for setting, (pen, g) in SETTINGS.items():
        gp = gen_params(cfg, ACCEPT_TYPICAL, 48, pen, g)
        for i in range(2):
            f = on.extract_features(clip_for(cfg, i))
            on.engine.encode(f); off.engine.encode(f)
            a, b = on.engine.decode(gp, 1)[0], off.engine.decode(gp, 1)[0]
            hits += on.engine.stats()["sibling_hits"]
            assert off.engine.stats()["sibling_hits"] == 0
            diffs += a != b
    print(f"repeat[siblings]: {hits} sibling hits over 4 decodes, {diffs} differing")
    assert diffs <= 1
    assert hits > 0
    on.engine.close(); off.engine.close()


# ---- 6. scoring -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
def test_generate_token_logprobs_with_rules(gpu, rig, B):
    cfg, sd, ref = rig["base_head"]
    m = _model(cfg, sd, gpu, B)
    pen, g = SETTINGS["p1.3_g3"]
    feats = m.extract_features([clip_for(cfg, i) for i in range(B)])
    m.set_micro_batches(1)
    out = m.generate(feats, return_token_logprobs=True, max_new_tokens=40, repetition_penalty=pen, no_repeat_ngram_size=g)
    gp = m._gen_params(None, None, None, 40, None, None, False, None, None, None, None, None, repetition_penalty=pen, no_repeat_ngram_size=g)
    P = len(gp.prompt)
    seq, lp = out["sequences"].cpu(), out["token_logprobs"].cpu()
    enc = m.engine.encoder_output(B)
    d = []
    for b in range(B):
        ids = seq[b].tolist()[: int(out["lengths"][b])]
        assert torch.isfinite(lp[b, P: len(ids)]).all(), (b, lp[b])          # an emitted id is never a banned one
        want = R.reference_scores(ref.orc, enc[b], ids, P, gp, cfg)
        d += [abs(float(lp[b, t]) - want["logprobs"][t]) for t in range(P, len(ids))]
        plain = R.reference_scores(ref.orc, enc[b], ids, P, dataclasses.replace(gp, repetition_penalty=1.0, no_repeat_ngram_size=0), cfg)
        assert max(abs(a - c) for a, c in zip(want["logprobs"], plain["logprobs"])) > MAX_D          # a scorer that ignored the rules would miss the bound
    d = np.asarray(d)
    print(f"repeat[scores B={B}]: {len(d)} rows, max |d| {d.max():.4g}, mean |d| {d.mean():.4g}")
    assert d.max() <= MAX_D and d.mean() <= MEAN_D, (float(d.max()), float(d.mean()))
    m.engine.close()


# ---- 7. the public interface ---------------------------------------------------------------------------------------------------------------------------
def _own(row, P, eos):
    s = [int(t) for t in row]
    return s[: s.index(eos, P) + 1] if eos in s[P:] else s


def test_generate_api(gpu, rig):
    cfg, sd, _ = rig["base_head"]
    m = _model(cfg, sd, gpu, 2)
    P, eos = len(synth.default_prompt(cfg)), cfg.eos_token_id
    f = m.extract_features([clip_for(cfg, 0), clip_for(cfg, 1)])
    plain = m.generate(f[0:1], max_new_tokens=40)
    ruled = m.generate(f[0:1], max_new_tokens=40, no_repeat_ngram_size=2)
    assert R.repeated_ngrams(_own(plain[0].tolist(), P, eos), 2) > 0
    assert R.repeated_ngrams(_own(ruled[0].tolist(), P, eos), 2) == 0
    # neutral values: the ids of a call without the arguments (and nothing of an earlier call's rules is left on the context)
    assert torch.equal(m.generate(f[0:1], max_new_tokens=40, repetition_penalty=1.0, no_repeat_ngram_size=0), plain)
    # a batch of 2 through the micro-batch pool equals two single calls
    m.set_micro_batches(2)
    both = m.generate(f, max_new_tokens=40, repetition_penalty=PEN, no_repeat_ngram_size=3)
    m.set_micro_batches(1)
    for b in range(2):
        one = m.generate(f[b: b + 1], max_new_tokens=40, repetition_penalty=PEN, no_repeat_ngram_size=3)
        assert _own(both[b].tolist(), P, eos) == _own(one[0].tolist(), P, eos)
    assert torch.equal(m.generate(f[0:1], max_new_tokens=40), plain)            # the pool's contexts and the model's own: rules cleared
    # generation_config fields are read
    from transformers import GenerationConfig
    via_gc = m.generate(f[0:1], generation_config=GenerationConfig(no_repeat_ngram_size=2), max_new_tokens=40)
    assert torch.equal(via_gc, ruled)
    # two windows of a long clip: every window under the rules
    long = torch.cat([f[0:1], f[1:2]], dim=-1)
    got = m.generate(long, chunk_longform=True, max_new_tokens=24, no_repeat_ngram_size=2)[0].tolist()
    win = m.generate(f, max_new_tokens=24, no_repeat_ngram_size=2)
    want = list(win[0][:P].tolist())
    for b in range(2):
        want += [t for t in _own(win[b].tolist(), P, eos)[P:] if t != eos]
    assert _own(got, P, eos) == want + [eos]
    m.engine.close()


def test_setter_refusals(gpu, rig):
    cfg, sd, _ = rig["base_head"]
    m = _model(cfg, sd, gpu, 1)
    m.engine.encode(m.extract_features(clip_for(cfg, 0)))
    for pen, g in ((0.0, 0), (-1.0, 0), (float("inf"), 0), (float("nan"), 0), (1.0, -1), (1.0, cfg.max_target_positions + 1)):
        with pytest.raises(ValueError, match="wm_set_repeat_rules"):
            m.engine.decode(gen_params(cfg, ACCEPT_TYPICAL, 8, pen, g), 1)
    m.engine.close()
    tree = MedusaConfig.micro(K=4, medusa_choices=[1, 2, 2, 1, 1])
    mt = _model(tree, synth.synth_state_dict(tree, seed=3), gpu, 1)
    mt.engine.encode(mt.extract_features(clip_for(tree, 0)))
    with pytest.raises(ValueError, match="candidate tree"):
        mt.engine.decode(gen_params(tree, ACCEPT_TYPICAL, 8, 1.0, 2), 1)
    mt.engine.close()
