"""Beam search on the plain decode path (include/wm.h wm_set_beam) without a GPU: tests/beam_ref.py pinned against HF's own
`generate(num_beams=n)`, the decisiveness of every case tests/test_gpu_beam.py runs (from the reference alone), the C-ABI surface and what
generate() refuses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import beam_ref as R
from helpers import ROOT, GenParams
from whisper_medusa import WhisperMedusaModel, synth
from whisper_medusa import engine as wm_engine


# ---- the pin: beam_ref (fp32 mode) against transformers ----------------------------------------------------------------------------------------
# A tiny random WhisperForConditionalGeneration built from a config (nothing is fetched), on the CPU in fp32.  HF's generate here is
# GenerationMixin.generate — the call WhisperGenerationMixin.generate itself delegates every short-form decode to, with the decoder prompt and the
# Whisper processors it would build (suppress, begin-suppress, timestamp rules) handed over explicitly; Whisper's own wrapper only adds prompt
# handling and output post-processing around it.  EOS is a token the model's greedy path emits early, so that beams finish inside the run.
HF_V, HF_S, HF_TGT = 300, 48, 40
HF_TB = HF_V - (HF_S + 1)
_HF = {}


def _hf_model(seed):
    if seed not in _HF:
        from transformers import WhisperConfig, WhisperForConditionalGeneration
        torch.manual_seed(seed)
        cfg = WhisperConfig(vocab_size=HF_V, num_mel_bins=8, encoder_layers=1, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2,
                            encoder_ffn_dim=64, decoder_ffn_dim=64, d_model=32, max_source_positions=HF_S, max_target_positions=HF_TGT,
                            eos_token_id=HF_TB - 4, bos_token_id=HF_TB - 4, pad_token_id=HF_TB - 4, decoder_start_token_id=HF_TB - 3,
                            suppress_tokens=None, begin_suppress_tokens=None, tie_word_embeddings=False)
        m = WhisperForConditionalGeneration(cfg).eval()
        with torch.no_grad():
            # (an output projection of its own — a tied one makes a random model repeat its last input token — scaled so that the log-probabilities
            # lie far enough apart to decide in fp32)
            m.proj_out.weight.copy_(torch.randn(HF_V, 32, generator=torch.Generator().manual_seed(seed + 7)) * 0.6)
        _HF[seed] = (m, torch.randn(1, 8, 2 * HF_S, generator=torch.Generator().manual_seed(seed + 1)))
    return _HF[seed]


def _hf_processors(gp, ts):
    from transformers import GenerationConfig, LogitsProcessorList
    from transformers.generation.logits_process import (SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor,
                                                        WhisperTimeStampLogitsProcessor)
    procs = LogitsProcessorList()
    if gp.suppress_tokens:
        procs.append(SuppressTokensLogitsProcessor(list(gp.suppress_tokens)))
    if gp.begin_suppress_tokens:
        procs.append(SuppressTokensAtBeginLogitsProcessor(list(gp.begin_suppress_tokens), begin_index=len(gp.prompt)))
    ts_proc = None
    if ts:
        gc = GenerationConfig(no_timestamps_token_id=HF_TB - 1, eos_token_id=gp.eos_token_id)
        gc.max_initial_timestamp_index = 20
        ts_proc = WhisperTimeStampLogitsProcessor(gc, begin_index=len(gp.prompt), _detect_timestamp_from_logprob=True)
        procs.append(ts_proc)
    return procs, ts_proc


def _hf_gp(m, feats, eos, ts, sup, max_new):
    prompt = [HF_TB - 3] if ts else [HF_TB - 3, HF_TB - 1]
    return GenParams(prompt=prompt, eos_token_id=eos, pad_token_id=eos, suppress_tokens=[3, 5] if sup else [],
                     begin_suppress_tokens=[7, eos] if sup else [], max_length=len(prompt) + max_new, hard_max_length=HF_TGT, vanilla=True,
                     timestamps=ts, no_timestamps_token_id=HF_TB - 1 if ts else -1, max_initial_timestamp_index=20 if ts else None)


def _pick_eos(m, feats, ts, sup):
    """A text token the greedy path (under the same processors) emits at its fourth generated position."""
    from transformers import GenerationMixin
    gp = _hf_gp(m, feats, HF_TB - 4, ts, sup, 8)
    gp.suppress_tokens = list(gp.suppress_tokens) + [gp.eos_token_id]           # (this probe run never ends early)
    procs, _ = _hf_processors(gp, ts)
    out = GenerationMixin.generate(m, feats, decoder_input_ids=torch.tensor([gp.prompt]), logits_processor=procs, num_beams=1, do_sample=False,
                                   max_length=gp.max_length, eos_token_id=gp.eos_token_id, pad_token_id=gp.pad_token_id)
    text = [int(t) for t in out[0, len(gp.prompt) + 2:].tolist() if t < HF_TB - 8 and t not in (3, 5, 7)]
    return text[1] if len(text) > 1 else text[0]


# (seed, n, length_penalty, early_stopping, timestamps, suppress lists, num_return_sequences, max_new)
HF_CASES = [
    (0, 2, 1.0, False, False, False, 1, 14), (0, 3, 0.0, True, False, True, 2, 14), (0, 5, 2.0, "never", False, False, 3, 14),
    (1, 3, 1.0, "never", False, True, 1, 14), (1, 5, 0.0, False, False, False, 5, 14), (1, 2, 2.0, True, False, True, 2, 14),
    (2, 3, 1.0, False, True, True, 2, 14), (2, 2, 2.0, True, True, False, 1, 14), (3, 5, 1.0, False, True, True, 1, 12),
    (3, 3, 1.0, False, False, True, 3, 3),          # ends at max_length: every continuation hits
    (4, 5, 1.0, True, False, False, 2, 14), (4, 2, 0.0, "never", False, True, 1, 14),
]


@pytest.mark.parametrize("seed,n,lp,es,ts,sup,nret,max_new", HF_CASES,
                         ids=[f"s{c[0]}-n{c[1]}-lp{c[2]:g}-es{c[3]}-{'ts' if c[4] else 'plain'}-{'sup' if c[5] else 'nosup'}-r{c[6]}-m{c[7]}" for c in HF_CASES])
def test_beam_ref_equals_hf(seed, n, lp, es, ts, sup, nret, max_new):
    from transformers import GenerationMixin
    m, feats = _hf_model(seed)
    gp = _hf_gp(m, feats, _pick_eos(m, feats, ts, sup), ts, sup, max_new)
    procs, ts_proc = _hf_processors(gp, ts)
    with torch.no_grad():
        out = GenerationMixin.generate(m, feats, decoder_input_ids=torch.tensor([gp.prompt]), logits_processor=procs, num_beams=n, do_sample=False,
                                       length_penalty=lp, early_stopping=es, num_return_sequences=nret, max_length=gp.max_length,
                                       eos_token_id=gp.eos_token_id, pad_token_id=gp.pad_token_id, return_dict_in_generate=True, output_scores=True)
        enc = m.model.encoder(feats).last_hidden_state

        def step(prefixes, beam_idx):
            ids = torch.tensor(prefixes)
            return m(encoder_outputs=(enc.expand(len(prefixes), -1, -1),), decoder_input_ids=ids).logits[:, -1].float()
        cb = R.beam_search(step, gp, n, HF_V, lp, es, "fp32", ts_proc)
    got = cb.result(nret)
    T = out.sequences.shape[1]
    for r, (ids, score) in enumerate(got):
        row = ids + [gp.pad_token_id] * (T - len(ids))
        assert row == out.sequences[r].tolist(), (r, row, out.sequences[r].tolist())
        assert score == pytest.approx(float(out.sequences_scores[r]), rel=1e-5), (r, score, float(out.sequences_scores[r]))
    if max_new == 3:
        assert all(rec["hit"].all() for rec in cb.steps[-1:]) and len(cb.steps) == 3        # the run ended by max_length
    else:
        assert any(rec["hit"].any() for rec in cb.steps)                                    # EOS really came up


def test_fp64_mode_takes_the_same_decisions():
    """The double-precision mode is the same algorithm: on a decisive run it returns the fp32 mode's sequences."""
    m, feats = _hf_model(0)
    gp = _hf_gp(m, feats, _pick_eos(m, feats, False, True), False, True, 14)
    with torch.no_grad():
        enc = m.model.encoder(feats).last_hidden_state

        def step(prefixes, beam_idx):
            return m(encoder_outputs=(enc.expand(len(prefixes), -1, -1),), decoder_input_ids=torch.tensor(prefixes)).logits[:, -1].float()
        a = R.beam_search(step, gp, 3, HF_V, 1.0, False, "fp32")
        b = R.beam_search(step, gp, 3, HF_V, 1.0, False, "fp64")
    assert [x[0] for x in a.result(3)] == [x[0] for x in b.result(3)]
    assert [x[1] for x in a.result(3)] == pytest.approx([x[1] for x in b.result(3)], rel=1e-5)


# ---- decisiveness of the GPU cases, from the reference alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,n,G,setting,first", [c for c in R.TAP1_CASES if c[0] != 51864], ids=lambda v: str(v))
def test_tap_cases_are_decisive(V, n, G, setting, first):
    cfg, gp, x, pre, init = R.tap1_case(V, n, G, setting, first)
    runs = R.tap_reference(cfg, gp, x, pre, init, n)
    for cb in runs:
        rec = cb.steps[0]
        assert not rec["planted"]
        bad = R.indecisive_steps(cb, lambda i, r: r["tol"])
        assert not bad, bad
        if gp.timestamps and not first:
            assert np.isfinite(rec["margins"]["dec"])           # the decision was really taken on live rows
    if setting in ("decay", "sup", "rep") and not first:
        assert any(cb.steps[0]["hit"][:n].any() for cb in runs)     # EOS inside the first n ranks (the decay reads it)


def test_tap_case_large_vocabulary_is_decisive():
    V, n, G, setting, first = [c for c in R.TAP1_CASES if c[0] == 51864][0]
    cfg, gp, x, pre, init = R.tap1_case(V, n, G, setting, first)
    for cb in R.tap_reference(cfg, gp, x, pre, init, n):
        assert not R.indecisive_steps(cb, lambda i, r: r["tol"])


def test_forced_rows_exist_in_the_timestamp_tap():
    """Rows that the timestamp rules' decision forces to a timestamp, and rows it leaves alone, both among live beams."""
    cfg, gp, x, pre, init = R.tap1_case(1031, 5, 1, "ts", False)
    import scores_ref as _sr
    proc = _sr.hf_processor(cfg, gp.begin_index)
    forced = []
    for j in range(5):
        w = torch.log_softmax(torch.from_numpy(x[0, 0, j]).double(), -1)
        forced.append(R.process_row(w, pre[j], gp, proc)[1])
    assert 0 in forced and 1 in forced, forced


@pytest.mark.parametrize("name,n,lp,es,max_new", R.SCRIPT_CASES, ids=[c[0] for c in R.SCRIPT_CASES])
def test_scripted_cases_are_decisive_and_cover(name, n, lp, es, max_new):
    cfg, gp, x, pre, init = R.script_case(name, n, lp, es, max_new)
    runs = R.tap_reference(cfg, gp, x, pre, init, n, lp, es, "fp64")
    for cb in runs:
        # a step's values carry the rounding of the steps before it: the bound of step i is the sum of the per-step tolerances so far
        acc = np.cumsum([r["tol"] for r in cb.steps])
        bad = R.indecisive_steps(cb, lambda i, r: acc[i])
        assert not bad and not any(r["planted"] for r in cb.steps), bad
    if name == "maxlen":
        assert all(len(cb.steps) == 4 and cb.steps[-1]["hit"].all() for cb in runs)
    fp32 = R.tap_reference(cfg, gp, x, pre, init, n, lp, es, "fp32")
    for a, b in zip(runs, fp32):
        # (a step that keeps dead beams — fewer than n candidates that do not hit, as at max_length — orders them by HF's collapsed fp32 values:
        # the fp32 mode IS the definition there, the double mode has no say)
        alive = [int((~r["hit"]).sum()) >= n for r in a.steps]
        assert a.fin_ids == b.fin_ids and [r["beam_idx"] for r, ok in zip(a.steps, alive) if ok] == [r["beam_idx"] for r, ok in zip(b.steps, alive) if ok]
        if all(alive):
            assert a.run_ids == b.run_ids


def test_scripted_cases_cover_what_they_are_for():
    runs = {c[0]: R.tap_reference(*R.script_case(*c), c[1], c[2], c[3], "fp64") for c in R.SCRIPT_CASES}
    n_of = {c[0]: c[1] for c in R.SCRIPT_CASES}
    recs = [(k, cb, r) for k, v in runs.items() for cb in v for r in cb.steps]
    assert any(r["hit"][: n_of[k]].any() for k, _, r in recs) and any(r["hit"][n_of[k]:].any() and not r["hit"].all() for k, _, r in recs)
    # a finished table that fills ends the clip under early_stopping=True, and only there
    assert any(all(cb.fin_set) and cb.done and len(cb.steps) < R.SCRIPT_S for cb in runs["lp1_true_fill"] + runs["lp0_true"])
    assert any(all(cb.fin_set) and not cb.done for cb in runs["lp2_never"] + runs["lp2_false"])
    # the heuristic ends a clip (early_stopping=False) before the steps run out
    assert any(cb.done and not cb.heur and len(cb.steps) < R.SCRIPT_S for cb in runs["lp1_false"])
    # beams reorder (a permutation, a duplicated source): the ids, and with them the timestamp states, must follow beam_idx
    assert any(len(set(r["beam_idx"])) < n_of[k] and len(set(r["beam_idx"])) > 1 for k, _, r in recs)


@pytest.mark.parametrize("name", sorted(R.E2E_CASES))
def test_end_to_end_cases_are_decisive(name):
    """Computed from the oracle's decoder_pass (and the oracle's encoder): every cut of every step exceeds twice (steps so far + 1) * 2 * 5e-4,
    and so does the order of the returned ranks in the final table."""
    cfg, sd, gp, runs = R.e2e_reference(name, "fp64")
    nret = R.E2E_CASES[name][7]
    for cb in runs:
        bad = R.e2e_indecisive(cb, nret)
        assert cb.done and not bad, (name, bad)
    if name == "b1n2":
        assert max(len(cb.fin_ids[0]) - len(gp.prompt) for cb in runs) > 16       # a result longer than 16 generated tokens
        fp32 = R.e2e_reference(name, "fp32")[3]                                    # HF's arithmetic takes the same decisions
        assert [a.fin_ids for a in runs] == [b.fin_ids for b in fp32]
    if name == "prompt":
        assert len(gp.prompt) > 16 and gp.begin_index < len(gp.prompt)


def test_planted_ties_come_out_in_the_defined_order():
    cfg, gp, x, pre, init, n = R.tie_case()
    cb = R.tap_reference(cfg, gp, x, pre, init, n, mode="fp32")[0]
    rec = cb.steps[0]
    # value descending, then (beam, token) ascending: beams 0 and 1 tie at -1, their four equal winners come in (beam, token) order
    assert list(zip(rec["cand_beam"].tolist(), rec["cand_tok"].tolist())) == [(0, 17), (0, 200), (0, 333), (1, 17), (1, 200), (1, 333)]
    assert rec["margins"]["cut2n"] == 0.0


def test_tolerance_is_a_few_ulp_of_the_values_it_bounds():
    t = R.tolerance(51864, 12.0, -9.0, -30.0)
    assert 20 * R.EPS < t < 200 * R.EPS and R.tolerance(516, 12.0, -9.0, -30.0) < t
    assert R.e2e_bound(0) == pytest.approx(1e-3) and R.e2e_bound(9) == pytest.approx(1e-2)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported(built_lib):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert re.search(r"#define WM_ABI_VERSION 9\b", hdr) and re.search(r"#define WM_BEAM_MAX 8\b", hdr)
    names = ("wm_set_beam", "wm_get_beam_result", "wm_beam_rows", "wm_beam_reorder_kv")
    for name in names:
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in wm_engine.EXPORTS
    m = re.search(r"typedef struct wm_beam_params \{([^}]*)\}", hdr)
    fields = [f.split()[-1].lstrip("*") for f in re.sub(r"/\*.*?\*/", "", m.group(1)).split(";") if f.strip()]
    assert fields == [n for n, _ in wm_engine.WmBeamParams._fields_] == ["num_beams", "length_penalty", "early_stopping"]
    for word in ("_get_top_k_continuations", "_get_running_beams_for_next_iteration", "_update_finished_beams", "_check_early_stop_heuristic",
                 "_beam_search_has_unfinished_sequences", "log_softmax", "-1e9"):
        assert word in hdr, word
    for path in (wm_engine.LIB_PATH, wm_engine.LIB_PATH_F16):
        assert os.path.exists(path), f"{path}: build the engine first"
        lib = ctypes.CDLL(path)
        assert lib.wm_abi_version() == 9 and all(hasattr(lib, n) for n in names)


def test_gen_params_carry_the_request():
    gp = GenParams(prompt=[1], eos_token_id=2, pad_token_id=2)
    assert gp.num_beams == 1 and gp.length_penalty == 1.0 and gp.early_stopping is False
    gp.num_beams = 4
    assert WhisperMedusaModel._sampled_gp(gp, 0.4, 9, [5]).num_beams == 1           # HF: a sampled retry runs with one beam
    b = wm_engine.Engine._beam_struct(5, 2.0, "never")
    assert (b.num_beams, b.length_penalty, b.early_stopping) == (5, 2.0, 2)
    assert wm_engine.Engine._beam_struct(2, 0.0, True).early_stopping == 1 and wm_engine.Engine._beam_struct(2).early_stopping == 0
    with pytest.raises(ValueError, match="early_stopping"):
        wm_engine.Engine._beam_struct(2, 1.0, "sometimes")


# ---- refusals (no engine is reached: the model sits on the CPU) --------------------------------------------------------------------------------
def _cpu_model(cfg=None, max_batch=8):
    cfg = cfg or R.tap_cfg(1031)
    return WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=3), max_batch=max_batch)


def _x(m, B=1, frames=1):
    return torch.zeros(B, m.config.num_mel_bins, frames * m.config.n_mel_frames)


def test_without_vanilla_the_reference_exception_stands():
    m = _cpu_model()
    with pytest.raises(Exception, match="Beam search is not supported with medusa for now") as e:
        m.generate(_x(m), num_beams=4)
    assert type(e.value) is Exception and "vanilla=True" in str(e.value)


REFUSED = [
    (dict(logits_processor=[object()]), NotImplementedError, "host processor path"),
    (dict(stopping_criteria=[object()]), NotImplementedError, "host processor path"),
    (dict(streamer=object()), NotImplementedError, "streamer"),
    (dict(chunk_longform=True), NotImplementedError, "chunk_longform"),
    (dict(sequential_longform=True, return_timestamps=True), NotImplementedError, "sequential_longform"),
    (dict(num_beams=9), NotImplementedError, "num_beams > 8"),
    (dict(do_sample=True, sampling_seed=1), NotImplementedError, "do_sample with beams"),
    (dict(temperature=0.4, sampling_seed=1), NotImplementedError, "do_sample with beams"),
    (dict(do_sample=True), NotImplementedError, "do_sample"),
    (dict(num_return_sequences=5), ValueError, "num_return_sequences"),
    (dict(early_stopping="sometimes"), ValueError, "early_stopping"),
    (dict(length_penalty=float("inf")), ValueError, "length_penalty"),
    (dict(num_return_sequences=2, return_token_logprobs=True), NotImplementedError, "num_return_sequences > 1"),
]


@pytest.mark.parametrize("kw,exc,word", REFUSED, ids=[f"{i}-{w}" for i, (_, _, w) in enumerate(REFUSED)])
def test_refused_by_name(kw, exc, word):
    m = _cpu_model()
    frames = 3 if kw.get("sequential_longform") else 1
    with pytest.raises(exc, match=word):
        m.generate(_x(m, frames=frames), **dict(dict(vanilla=True, num_beams=4), **kw))


def test_refused_candidate_tree_pool_and_small_context():
    import dataclasses
    tree = dataclasses.replace(R.tap_cfg(1031), medusa_choices=[1, 2, 1, 1, 1])
    m = _cpu_model(tree)
    with pytest.raises(NotImplementedError, match="candidate tree"):
        m.generate(_x(m), vanilla=True, num_beams=2)
    m = _cpu_model()
    m.set_micro_batches(2)
    with pytest.raises(NotImplementedError, match="micro-batch pool"):
        m.generate(_x(m, 2), vanilla=True, num_beams=2)
    m = _cpu_model(max_batch=2)
    with pytest.raises(ValueError, match="set_max_batch"):
        m.generate(_x(m), vanilla=True, num_beams=4)


def test_generation_config_fields_are_read():
    """length_penalty / early_stopping / num_return_sequences / num_beams from a passed generation_config reach the request."""
    from types import SimpleNamespace
    m = _cpu_model()
    seen = {}

    def req(kwargs, *a, **k):
        seen.update(kwargs)
        raise RuntimeError("stop here")
    m._beam_request = req
    gc = SimpleNamespace(num_beams=3, length_penalty=2.0, early_stopping="never", num_return_sequences=2)
    with pytest.raises(RuntimeError, match="stop here"):
        m.generate(_x(m), generation_config=gc, vanilla=True)
    assert (seen["num_beams"], seen["length_penalty"], seen["early_stopping"], seen["num_return_sequences"]) == (3, 2.0, "never", 2)
