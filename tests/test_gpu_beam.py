"""Beam search on the plain decode path on the GPU (include/wm.h wm_set_beam / wm_beam_rows / wm_beam_reorder_kv).  The reference is
tests/beam_ref.py — HF's _beam_search restated, pinned against transformers by tests/test_beam_cpu.py, which also holds, from that reference alone,
the decisiveness of every case used here."""
import numpy as np
import pytest
import torch

import beam_ref as R
from helpers import clip_for
from whisper_medusa import WhisperMedusaModel, synth

pytestmark = pytest.mark.gpu


def _model(cfg, sd, gpu, B, act_fp16=False):
    return WhisperMedusaModel(cfg, sd, device=gpu, max_batch=B, act_fp16=act_fp16)       # default: the oracle's contract (bf16 hi / lo)


_TAP = {}


def _tap_model(gpu, V):
    """One context per vocabulary, 24 streams (G = 3, n = 8), shared by the tap tests."""
    if V not in _TAP:
        cfg = R.tap_cfg(V)
        _TAP[V] = _model(cfg, synth.synth_state_dict(cfg, seed=3), gpu, 24)
    return _TAP[V]


@pytest.fixture(scope="module", autouse=True)
def _close_tap_models():
    yield
    for m in _TAP.values():
        m.engine.close()
    _TAP.clear()


def _tap(m, gp, x, pre, n, lp=1.0, es=False, init=None):
    return m.engine.beam_rows(gp, x, pre, n, lp, es, init)


# ---- 1. the tap against fp64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,n,G,setting,first", R.TAP1_CASES, ids=lambda v: str(v))
def test_tap_matches_fp64(gpu, V, n, G, setting, first):
    cfg, gp, x, pre, init = R.tap1_case(V, n, G, setting, first)
    m = _tap_model(gpu, V)
    got = _tap(m, gp, x, pre, n, init=init)
    ref = R.tap_reference(cfg, gp, x, pre, init, n)
    worst = 0.0
    for g, cb in enumerate(ref):
        rec = cb.steps[0]
        assert got["cand_beam"][0, g].tolist() == rec["cand_beam"].tolist() and got["cand_tok"][0, g].tolist() == rec["cand_tok"].tolist(), (g, rec)
        for k in range(2 * n):
            want = float(rec["cand_val"][k])
            if np.isfinite(want):
                err = abs(float(got["cand_val"][0, g, k]) - want)
                assert err <= rec["tol"], (g, k, err, rec["tol"])
                worst = max(worst, err / rec["tol"])
            else:
                assert float(got["cand_val"][0, g, k]) == want
        assert got["beam_idx"][0, g * n: (g + 1) * n].tolist() == [g * n + b for b in rec["beam_idx"]]
    print(f"beam tap[V={V} n={n} G={G} {setting}]: largest |value - fp64| = {worst:.3f} of the tolerance")


def test_planted_ties_come_out_in_the_defined_order(gpu):
    cfg, gp, x, pre, init, n = R.tie_case()
    got = _tap(_tap_model(gpu, 516), gp, x, pre, n, init=init)
    rec = R.tap_reference(cfg, gp, x, pre, init, n, mode="fp32")[0].steps[0]
    assert list(zip(got["cand_beam"][0, 0].tolist(), got["cand_tok"][0, 0].tolist())) == list(zip(rec["cand_beam"].tolist(), rec["cand_tok"].tolist()))
    v = got["cand_val"][0, 0].tolist()
    assert v[0] == v[1] == v[2] and v[3] == v[4] == v[5]            # equal logits of one row: equal values, bit for bit; the order is the rule's
    assert np.allclose(v, rec["cand_val"], rtol=0, atol=2 * rec["tol"])


# ---- 2. scripted steps through the tap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,lp,es,max_new", R.SCRIPT_CASES, ids=[c[0] for c in R.SCRIPT_CASES])
def test_scripted_steps_equal_the_reference(gpu, name, n, lp, es, max_new):
    cfg, gp, x, pre, init = R.script_case(name, n, lp, es, max_new)
    got = _tap(_tap_model(gpu, 1031), gp, x, pre, n, lp, es)
    ref = R.tap_reference(cfg, gp, x, pre, init, n, lp, es, "fp32")         # HF's arithmetic: also where it has collapsed values to -1e9
    for g, cb in enumerate(ref):
        steps = len(cb.steps)
        assert int(got["steps"][g]) == (steps if cb.done else R.SCRIPT_S), (g, got["steps"], steps, cb.done)
        for s, rec in enumerate(cb.steps):
            assert got["beam_idx"][s, g * n: (g + 1) * n].tolist() == [g * n + b for b in rec["beam_idx"]], (g, s)
            assert got["cand_tok"][s, g].tolist() == rec["cand_tok"].tolist() and got["cand_beam"][s, g].tolist() == rec["cand_beam"].tolist()
        for s in range(steps, R.SCRIPT_S):          # a clip that is done stops changing
            assert got["beam_idx"][s, g * n: (g + 1) * n].tolist() == list(range(g * n, (g + 1) * n))
        acc = float(np.sum([r["tol"] for r in cb.steps]))
        for j in range(n):
            assert int(got["fin_set"][g, j]) == int(cb.fin_set[j])
            L = int(got["fin_len"][g, j])
            assert got["fin_ids"][g, j, :L].tolist() == cb.fin_ids[j], (g, j)
            assert float(got["fin_score"][g, j]) == pytest.approx(float(cb.fin_score[j]), abs=2 * acc, rel=1e-6)
            Lr = int(got["run_len"][g * n + j])
            assert got["run_ids"][g * n + j, :Lr].tolist() == cb.run_ids[j], (g, j)
            assert float(got["run_score"][g * n + j]) == pytest.approx(float(cb.run[j]), abs=2 * acc, rel=1e-6)


# ---- 3. the K/V reorder is exact -------------------------------------------------------------------------------------------------------------
def test_kv_reorder_is_exact(gpu):
    """Six streams with different prefixes of 19 tokens (two 16-row tiles), reordered by a 3-cycle, a duplicated source and a fixed point; one more
    token forwarded; the logits are bit-equal to those of streams that were fed the permuted prefixes directly."""
    cfg = R.tap_cfg(1031)
    m = _model(cfg, synth.synth_state_dict(cfg, seed=5), gpu, 6)
    eng = m.engine
    eng.encode(m.extract_features([clip_for(cfg, c // 3) for c in range(6)]))      # two clips, three beams each: a beam only ever follows its own clip
    rng = np.random.default_rng(9)
    pre = rng.integers(10, 900, size=(6, 19)).tolist()
    idx = [1, 2, 0, 3, 3, 5]                    # 3-cycle (0 <- 1 <- 2 <- 0), stream 4 takes stream 3's (3 is a fixed point and a source), 5 fixed
    nxt = [[int(t)] for t in rng.integers(10, 900, size=6)]

    def feed(rows):
        eng.forward_logits([r[:16] for r in rows], 0, True)
        eng.forward_logits([r[16:] for r in rows], 16, True)
    feed(pre)
    eng.beam_reorder_kv(idx, 19)
    got = eng.forward_logits(nxt, 19, True)[0, :, 0]
    feed([pre[i] for i in idx])
    want = eng.forward_logits(nxt, 19, True)[0, :, 0]
    assert torch.equal(got, want)
    with pytest.raises(ValueError, match="beam_idx"):
        eng.beam_reorder_kv([0, 7], 4)
    eng.close()


# ---- 4. end to end against beam_ref over the oracle ------------------------------------------------------------------------------------------
_E2E = {}


def _e2e(gpu, name):
    """The engine's generate() of a case and the reference driven by the oracle from the engine's own encoder output (computed once per case;
    "groups" shares "b3n5"'s reference)."""
    if name in _E2E:
        return _E2E[name]
    from oracle.whisper_medusa_oracle import Oracle
    import scores_ref as _sr
    case = R.E2E_CASES[name]
    heads, clips, n, lp, es, ts, pid, nret, max_batch, max_new = case[:10]
    cfg, sd, gp = R.e2e_setup(case)
    m = _model(cfg, sd, gpu, max_batch)
    feats = m.extract_features([clip_for(cfg, c) for c in clips])
    kw = dict(vanilla=True, num_beams=n, length_penalty=lp, early_stopping=es, num_return_sequences=nret, max_new_tokens=max_new, language="en",
              return_dict_in_generate=True)
    if ts:
        kw["return_timestamps"] = True
    if pid is not None:
        kw["prompt_ids"] = torch.tensor([cfg.prev_sot_token_id] + list(pid))
    out = m.generate(feats, **kw)
    assert m._last_prompt == list(gp.prompt)
    ref_key = ("ref", case[:7] + case[9:])
    if ref_key not in _E2E:
        eng = m.engine
        if getattr(eng, "_B", None) != len(clips):
            eng.encode(feats)
        enc = eng.encoder_output(len(clips))
        orc = Oracle(cfg, sd, sim="bf16", act="hilo")
        proc = _sr.hf_processor(cfg, gp.begin_index) if ts else None
        _E2E[ref_key] = [R.beam_search(R.OracleBeams(orc, enc[i], n), gp, n, cfg.vocab_size, lp, es, "fp32", proc) for i in range(len(clips))]
    _E2E[name] = (m, feats, kw, gp, out, _E2E[ref_key])
    return _E2E[name]


@pytest.fixture(scope="module", autouse=True)
def _close_e2e_models():
    yield
    for k, v in _E2E.items():
        if isinstance(k, str):
            v[0].engine.close()
    _E2E.clear()


@pytest.mark.parametrize("name", sorted(R.E2E_CASES))
def test_end_to_end_equals_the_reference(gpu, name):
    m, feats, kw, gp, out, ref = _e2e(gpu, name)
    case = R.E2E_CASES[name]
    n, nret = case[2], case[7]
    seqs, scores = out["sequences"].tolist(), out["sequences_scores"].tolist()
    assert len(seqs) == len(ref) * nret
    for c, cb in enumerate(ref):
        for r, (ids, score) in enumerate(cb.result(nret)):
            row = seqs[c * nret + r]
            assert row[: len(ids)] == ids and all(t == gp.pad_token_id for t in row[len(ids):]), \
                (name, c, r, row, ids, "indecisive on this encoder output:", R.e2e_indecisive(cb, nret))
            assert abs(scores[c * nret + r] - score) <= R.e2e_bound(len(cb.steps) - 1), (name, c, r, scores[c * nret + r], score)
    st = m.last_stats
    if name == "groups":
        assert st["beam_groups"] == 3            # max_batch 8, n = 5: one clip per group
    if name == "b1n2":
        assert max(len(cb.fin_ids[0]) for cb in ref) - len(gp.prompt) > 16 and st["graph_replays"] > 0
    if name == "prompt":
        assert len(gp.prompt) > 16               # the prompt runs through wm_dec_prompt_prefix


# ---- 5. score consistency ----------------------------------------------------------------------------------------------------------------------
def test_score_is_the_sum_of_the_teacher_forced_rows(gpu):
    """The best hypothesis, teacher-forced through wm_forward_logits; beam_ref's fp64 arithmetic on those raw rows reproduces sequences_scores."""
    import scores_ref as _sr
    m, feats, kw, gp, out, ref = _e2e(gpu, "ts")
    case = R.E2E_CASES["ts"]
    nret, lp = case[7], case[3]
    cfg = m.config
    eng = m.engine
    proc = _sr.hf_processor(cfg, gp.begin_index)
    P = len(gp.prompt)
    for c in range(feats.shape[0]):
        eng.encode(feats[c: c + 1])
        L = len(ref[c].fin_ids[0])
        ids = out["sequences"][c * nret].tolist()[:L]
        rows = torch.cat([eng.forward_logits([ids[p0: min(p0 + 16, L - 1)]], p0, True)[0, 0] for p0 in range(0, L - 1, 16)])
        # row t: the raw logits after ids[: t + 1]
        total = 0.0
        for t in range(P, L):
            w = torch.log_softmax(rows[t - 1].double(), -1)
            total += float(R.process_row(w, ids[:t], gp, proc)[0][ids[t]])
        want = total / float(L - P) ** lp
        assert abs(float(out["sequences_scores"][c * nret]) - want) <= R.e2e_bound(L - P - 1), (c, float(out["sequences_scores"][c * nret]), want)


# ---- 6. invariance -----------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_batch_or_on_replay(gpu):
    m, feats, kw, gp, out, ref = _e2e(gpu, "b3n5")
    nret = R.E2E_CASES["b3n5"][7]
    again = m.generate(feats, **kw)             # a second identical call: the captured beam step is replayed
    assert torch.equal(again["sequences"], out["sequences"]) and torch.equal(again["sequences_scores"], out["sequences_scores"])
    alone = m.generate(feats[1:2], **kw)        # clip 1 alone and as one of three: bit-equal ids and scores
    T = alone["sequences"].shape[1]
    rows = out["sequences"][nret: 2 * nret]
    assert torch.equal(alone["sequences"], rows[:, :T]) and bool((rows[:, T:] == gp.pad_token_id).all())
    assert torch.equal(alone["sequences_scores"], out["sequences_scores"][nret: 2 * nret])


def test_default_contract_is_batch_invariant_too(gpu):
    case = R.E2E_CASES["b3n5"]
    cfg, sd, gp = R.e2e_setup(case)
    m = _model(cfg, sd, gpu, 15, act_fp16=True)
    feats = m.extract_features([clip_for(cfg, c) for c in case[1]])
    kw = dict(vanilla=True, num_beams=5, num_return_sequences=2, max_new_tokens=case[9], language="en", return_dict_in_generate=True)
    three = m.generate(feats, **kw)
    alone = m.generate(feats[2:3], **kw)
    T = alone["sequences"].shape[1]
    assert torch.equal(alone["sequences"], three["sequences"][4:6, :T]) and torch.equal(alone["sequences_scores"], three["sequences_scores"][4:6])
    m.engine.close()


# ---- 7. the context afterwards -----------------------------------------------------------------------------------------------------------------
def test_the_context_afterwards(gpu):
    m, feats, kw, gp, out, ref = _e2e(gpu, "block")
    m.set_micro_batches(1)                      # (two clips would go to the pool's contexts: this test is about the model's own)
    # an ordinary Medusa generate() before and after a beam call returns the same ids
    before = m.generate(feats, language="en", max_new_tokens=12)
    lp = m.generate(feats, **dict(kw, return_token_logprobs=True))
    after = m.generate(feats, language="en", max_new_tokens=12)
    assert torch.equal(before, after)
    # the replay behind a beam call scores the same ids as after a fresh encode: the cross K/V moved back to the clips' slots
    eng = m.engine
    eng.encode(feats)
    seqs = [m._own_end(s, gp) for s in lp["sequences"].tolist()]
    fresh, _, _ = eng.score_tokens(seqs, len(gp.prompt), gp, None, 0)
    for b, s in enumerate(seqs):
        assert np.array_equal(lp["token_logprobs"][b, : len(s)].cpu().numpy(), fresh[b, : len(s)]), b
    m.set_micro_batches(None)
    assert torch.equal(lp["sequences"], out["sequences"]) and "sequences_scores" in lp


# ---- 8. fallback -------------------------------------------------------------------------------------------------------------------------------
def test_fallback_keeps_the_beams_for_the_first_attempt_only(gpu):
    m, feats, kw, gp, out, ref = _e2e(gpu, "b1n2")
    base = {k: v for k, v in kw.items() if k not in ("num_beams", "length_penalty", "early_stopping", "num_return_sequences")}
    # a threshold the beam result fails: its average log-probability lies below 0
    fb = m.generate(feats, **dict(kw, temperature=(0.0, 0.4), sampling_seed=11, logprob_threshold=0.0))
    assert m._fallback_beams[0][0][0] == ref[0].fin_ids[0]                  # attempt 0 is the beam result
    assert m._fallback_beams[0][0][1] == float(out["sequences_scores"][0])
    assert fb["fallback_attempts"].tolist() == [2] and fb["fallback_temperature"].tolist() == pytest.approx([0.4])
    # the kept one is the sampled one-beam attempt: the same call without beams at T = 0.4 (attempt index 1 of its own ladder)
    plain = m.generate(feats, **dict(base, temperature=(0.0, 0.4), sampling_seed=11, logprob_threshold=0.0))
    assert plain["fallback_attempts"].tolist() == [2]
    assert torch.equal(fb["sequences"], plain["sequences"])
    assert bool(torch.isnan(fb["sequences_scores"]).all())


# ---- 9. argument errors ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_back_with_their_reason(gpu):
    import dataclasses
    cfg = R.tap_cfg(1031)
    sd = synth.synth_state_dict(cfg, seed=3)
    m = _model(cfg, sd, gpu, 4)
    eng = m.engine
    gp = R.tap_gp(cfg, "plain", max_length=12)
    for bad, word in (((9, 1.0, False), "num_beams"), ((2, float("nan"), False), "length_penalty")):
        with pytest.raises(ValueError, match=word):
            eng.set_beam(*bad)
    eng.encode(m.extract_features([clip_for(cfg, 0), clip_for(cfg, 1)]))
    with pytest.raises(ValueError, match="plain decode path"):
        eng.decode(dataclasses.replace(gp, vanilla=False, num_beams=2), 2)
    with pytest.raises(ValueError, match="max_batch"):
        eng.decode(dataclasses.replace(gp, num_beams=3), 2)
    # sampling and beams together (set directly: the Python layer never asks for both)
    eng.set_sampling(0.5, 1, None, 2)
    eng.set_beam(2)
    g, _keep = eng._gen_struct(gp)
    import ctypes as C
    rc = eng.lib.wm_decode_begin(eng.h, C.byref(g), 2)
    assert rc == -1 and b"sampling" in eng.lib.wm_last_error(eng.h)
    eng.set_sampling(None)
    eng.set_beam(None)
    with pytest.raises((ValueError, RuntimeError), match="no finished beam decode"):
        eng.beam_result(0, 0)
    # after the refusals an ordinary beam decode still runs, and rank 0 is what wm_get_tokens returns
    ids = eng.decode(dataclasses.replace(gp, num_beams=2), 2)
    assert ids[0] == eng.beam_result(0, 0)[0] and ids[1] == eng.beam_result(1, 0)[0]
    eng.close()
    tree = dataclasses.replace(cfg, medusa_choices=[1, 2, 1, 1, 1])
    mt = _model(tree, synth.synth_state_dict(tree, seed=3), gpu, 4)
    mt.engine.encode(mt.extract_features([clip_for(tree, 0)]))
    with pytest.raises(ValueError, match="candidate tree"):
        mt.engine.decode(dataclasses.replace(gp, num_beams=2), 1)
    mt.engine.close()
