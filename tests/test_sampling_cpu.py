"""Seeded sampling and the temperature fallback (include/wm.h wm_set_sampling / wm_sample_rows) without a GPU: the reference's
Philox against the Random123 known answers, the noise mapping, the C-ABI surface, what generate() refuses with and without `sampling_seed`, the
fallback loop on a scripted engine, and — from the reference alone — the conditions the inputs of tests/test_gpu_sampling.py were chosen under."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import sample_ref as S
from helpers import ROOT, MedusaConfig, GenParams, synth
from whisper_medusa import WhisperMedusaModel
from whisper_medusa import engine as wm_engine
from whisper_medusa.config import ACCEPT_GREEDY


# ---- the noise -----------------------------------------------------------------------------------------------------------------------------
KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = S.philox4x32_10(ctr, key)
    assert " ".join("%08x" % int(w) for w in got) == want


def test_philox_vectorised_equals_scalar():
    q = np.arange(5, dtype=np.uint64)
    vec = S.philox4x32_10([q, 7, 3, 9], (11, 13))
    for i in range(5):
        one = S.philox4x32_10([i, 7, 3, 9], (11, 13))
        assert [int(w[i]) for w in vec] == [int(w) for w in one]
    # word n & 3 of block n >> 2
    w = S.noise_words(seed=(13 << 32) | 11, key=(9 << 32) | 3, t=7, V=18)
    assert [int(x) for x in w[:4]] == [int(v[0]) for v in vec] and int(w[17]) == int(vec[1][4])


def test_noise_mapping_is_exact_and_finite():
    lo, hi = S.u_of(0), S.u_of(0xffffffff)
    assert lo.dtype == np.float32 and float(lo) == 2.0 ** -24 and float(hi) == 1.0 - 2.0 ** -24
    assert float(S.gumbel64(0)) == pytest.approx(-2.8115, abs=1e-4) and float(S.gumbel64(0xffffffff)) == pytest.approx(16.6355, abs=1e-4)
    x = np.random.default_rng(0).integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32)
    u = S.u_of(x)
    k = u.astype(np.float64) * 2.0 ** 24
    assert np.all(k == np.round(k)) and np.all(k.astype(np.int64) % 2 == 1) and np.all((u > 0) & (u < 1))        # odd multiples of 2^-24
    assert np.all(k.astype(np.int64) == 2 * (x.astype(np.int64) >> 9) + 1)
    assert np.isfinite(S.gumbel64(x)).all()


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported(built_lib):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert re.search(r"#define WM_ABI_VERSION 9\b", hdr) and wm_engine.WM_ABI_VERSION == 9
    for name in ("wm_set_sampling", "wm_sample_rows"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in wm_engine.EXPORTS
    m = re.search(r"typedef struct wm_sample_params \{([^}]*)\}", hdr)
    fields = [f.split()[-1].lstrip("*") for f in re.sub(r"/\*.*?\*/", "", m.group(1)).split(";") if f.strip()]
    assert fields == [n for n, _ in wm_engine.WmSampleParams._fields_] == ["temperature", "seed", "stream_keys", "n_keys"]
    for word in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "top_k"):
        assert word in hdr, word
    for path in (wm_engine.LIB_PATH, wm_engine.LIB_PATH_F16):
        assert os.path.exists(path), f"{path}: build the engine first"
        lib = ctypes.CDLL(path)
        assert lib.wm_abi_version() == 9 and hasattr(lib, "wm_set_sampling") and hasattr(lib, "wm_sample_rows")


def test_gen_params_carry_the_request():
    gp = GenParams(prompt=[1], eos_token_id=2, pad_token_id=2)
    assert gp.sampling_temperature == 0.0 and gp.sampling_keys is None
    g = WhisperMedusaModel._sampled_gp(gp, 0.4, 9, [5, 6])
    assert g.vanilla and g.accept_mode == ACCEPT_GREEDY and g.sampling_temperature == 0.4 and g.sampling_seed == 9 and g.sampling_keys == [5, 6]
    assert not gp.vanilla
    assert WhisperMedusaModel.sampling_stream_key(3, 148, 2) == S.stream_key(3, 148, 2) == 3 | ((16 * 148 + 2) << 32)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _cpu_model(cfg=None):
    cfg = cfg or S.tap_cfg()
    return WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=3), max_batch=2)


def test_without_a_seed_everything_raises_as_before():
    m = _cpu_model()
    cfg = m.config
    x = torch.zeros(1, cfg.num_mel_bins, cfg.n_mel_frames)
    with pytest.raises(NotImplementedError, match="do_sample"):
        m.generate(x, do_sample=True)
    with pytest.raises(NotImplementedError, match="temperature > 0"):
        m.generate(x, temperature=0.4)
    long = torch.zeros(1, cfg.num_mel_bins, 3 * cfg.n_mel_frames)
    with pytest.raises(NotImplementedError, match="temperature") as e:
        m.generate(long, sequential_longform=True, return_timestamps=True, temperature=(0.0, 0.2))
    assert "sequential_longform" in str(e.value) and "sampling_seed" in str(e.value)
    # a seed alone asks for nothing: the refusals of a call that does not sample are the old ones
    with pytest.raises(NotImplementedError, match="condition_on_prev_tokens"):
        m.generate(long, sequential_longform=True, return_timestamps=True, condition_on_prev_tokens=True, sampling_seed=1)


REFUSED_WITH_A_SEED = [
    (dict(top_k=50), "top_k"),
    (dict(top_p=0.9), "top_p"),
    (dict(streamer=object()), "streamer"),
    (dict(logits_processor=[object()]), "host processor path"),
    (dict(chunk_longform=True), "chunk_longform"),
]


@pytest.mark.parametrize("kw,word", REFUSED_WITH_A_SEED, ids=[w for _, w in REFUSED_WITH_A_SEED])
@pytest.mark.parametrize("temperature", [0.4, (0.0, 0.4)], ids=["scalar", "ladder"])
def test_refused_with_a_seed_by_name(kw, word, temperature):
    m = _cpu_model()
    x = torch.zeros(1, m.config.num_mel_bins, m.config.n_mel_frames)
    with pytest.raises(NotImplementedError, match=word):
        m.generate(x, temperature=temperature, sampling_seed=7, **kw)


def test_refused_with_a_seed_candidate_tree_and_bad_values():
    import dataclasses
    tree = dataclasses.replace(S.tap_cfg(), medusa_choices=[1, 2, 1, 1, 1])
    m = _cpu_model(tree)
    x = torch.zeros(1, tree.num_mel_bins, tree.n_mel_frames)
    with pytest.raises(NotImplementedError, match="candidate tree"):
        m.generate(x, do_sample=True, sampling_seed=7)
    m = _cpu_model()
    for bad in ((0.0, -0.2), (0.0, float("nan")), ()):
        with pytest.raises(ValueError, match="temperature"):
            m.generate(x, temperature=bad, sampling_seed=7)
    # sequential long-form lets the tuple through with a seed: the next refusal in line is reached
    long = torch.zeros(1, tree.num_mel_bins, 3 * tree.n_mel_frames)
    with pytest.raises(NotImplementedError, match="return_timestamps"):
        m.generate(long, sequential_longform=True, temperature=(0.0, 0.4), sampling_seed=7)


# ---- the fallback loop on a scripted engine ------------------------------------------------------------------------------------------------
class ScriptedEngine:
    """encode / decode / stats of whisper_medusa.engine.Engine: a decode returns, per stream, [attempt marker, global stream]."""

    def __init__(self):
        self.calls, self.resident = [], None

    def encode(self, feats):
        self.resident = [int(v) for v in feats[:, 0, 0].tolist()]
        self._B = len(self.resident)
        self.calls.append(("encode", list(self.resident)))

    def decode(self, gp, B):
        assert B == len(self.resident)
        self.calls.append(("decode", list(self.resident), gp.sampling_temperature, None if gp.sampling_keys is None else list(gp.sampling_keys),
                           gp.vanilla))
        return [[b, round(gp.sampling_temperature * 10)] for b in self.resident]

    def stats(self):
        return dict(ms_decode=1.0, ms_encode=1.0)


def _run_fallback(temps, verdicts, B=4, sc_req=True, ids=None, seeks=None):
    """verdicts[(stream, attempt)] = (needs_fallback, skipped); default (False, False)."""
    m = _cpu_model()
    eng = ScriptedEngine()
    attempt_of = {round(t * 10): i for i, t in enumerate(temps)}

    def score(e, seqs, gp, req):
        infos = [dict(needs_fallback=verdicts.get((s[0], attempt_of[s[1]]), (False, False))[0],
                      skipped=verdicts.get((s[0], attempt_of[s[1]]), (False, False))[1]) for s in seqs]
        return seqs, infos, 0.5
    m._score_run = score
    feats = torch.arange(B, dtype=torch.float32)[:, None, None].expand(B, 2, 3).contiguous()
    gp = GenParams(prompt=[1], eos_token_id=2, pad_token_id=2)
    samp = dict(seed=99, ids=ids, seeks=seeks, temps=list(temps), fallback=True)
    *out, beams, m.last_stats = m._decode_with_fallback(eng, feats, gp, samp, {} if sc_req else None, encoded=False)
    return m, eng, tuple(out)


def test_fallback_loop_follows_hf():
    temps = (0.0, 0.2, 0.4)
    # stream 0 passes at once; 1 passes at the second attempt; 2 never passes (the last attempt is kept); 3 is skipped: no retry although flagged
    verdicts = {(1, 0): (True, False), (2, 0): (True, False), (2, 1): (True, False), (2, 2): (True, False), (3, 0): (True, True)}
    m, eng, (seqs, infos, kept, att, ms) = _run_fallback(temps, verdicts, ids=[10, 11, 12, 13], seeks=[0, 5, 148, 0])
    assert att == [1, 2, 3, 1] and kept == pytest.approx([0.0, 0.2, 0.4, 0.0])
    assert seqs == [[0, 0], [1, 2], [2, 4], [3, 0]]
    dec = [c for c in eng.calls if c[0] == "decode"]
    assert [c[1] for c in dec] == [[0, 1, 2, 3], [1, 2], [2]]                      # only the flagged streams are decoded again
    assert [c[1] for c in eng.calls if c[0] == "encode"] == [[0, 1, 2, 3], [1, 2], [2]]      # ... after their sub-batch was re-encoded
    assert dec[0][2] == 0.0 and dec[0][3] is None and dec[0][4] is False          # temperature 0: the configured path, no sampling
    assert dec[1][2] == pytest.approx(0.2) and dec[1][4] is True                  # above 0: the sampled plain decode
    assert dec[1][3] == [S.stream_key(11, 5, 1), S.stream_key(12, 148, 1)] and dec[2][3] == [S.stream_key(12, 148, 2)]
    assert m.last_stats["fallback_decodes"] == 2 and ms == pytest.approx(1.5)
    # the same control flow as the reference's loop
    want = S.fallback_loop(temps, 4, lambda idx, T, i: [[b, round(T * 10)] for b in idx],
                           lambda r, T: verdicts.get((r[0], temps.index(T)), (False, False)))
    assert want[0] == seqs and want[2] == att and [c[2] for c in want[3]] == [c[1] for c in dec]


def test_fallback_without_thresholds_runs_one_attempt():
    m, eng, (seqs, infos, kept, att, ms) = _run_fallback((0.4, 0.8), {}, B=2, sc_req=False)
    assert att == [1, 1] and kept == pytest.approx([0.4, 0.4]) and infos is None
    dec = [c for c in eng.calls if c[0] == "decode"]
    assert len(dec) == 1 and dec[0][3] == [S.stream_key(0, 0, 0), S.stream_key(1, 0, 0)]       # default stream ids: range(B), seek 0
    assert m.last_stats["fallback_decodes"] == 0


def test_fallback_all_flagged_keeps_the_batch_resident():
    """Every stream flagged: the second attempt decodes the whole batch again, without a second encoder pass."""
    verdicts = {(b, 0): (True, False) for b in range(2)}
    m, eng, (seqs, infos, kept, att, ms) = _run_fallback((0.0, 0.4), verdicts, B=2)
    assert att == [2, 2] and [c[0] for c in eng.calls] == ["encode", "decode", "decode"]


# ---- guards of the GPU inputs, from the reference alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", S.TAP_SETTINGS)
def test_tap_inputs_are_decisive_and_not_vacuous(setting):
    """At most 2 % of the tap rows may be left out of a check as indecisive; the crafted rows reach what they were crafted for."""
    cfg = S.tap_cfg()
    rows, pre = S.tap_cases(cfg, setting)
    V, tb = cfg.vocab_size, cfg.timestamp_begin
    n = out = forced = 0
    winners = set()
    for T in S.TAP_T:
        for seed in S.TAP_SEEDS:
            for d in S.tap_reference(setting, T, seed):
                n += 1
                out += d["gap"] <= 10 * d["tol"] or d["margin"] <= d["tol"]
                forced += d["forced"]
                winners.add(d["token"])
                assert math.isfinite(d["value"]) and 0.0 < d["tol"] < float("inf")
    assert out <= 0.02 * n, (setting, out, n)
    edges = set(S.edge_tokens(V) + S.edge_tokens(tb)) - {3, 40}
    if setting == "plain":
        assert forced == 0 and edges <= winners, sorted(edges - winners)           # every lifted edge token wins its row
    else:
        assert 0 < forced < n and (set(S.edge_tokens(tb)) - {tb - 1, 0}) & winners and any(w >= tb for w in winners)
    assert 61 not in winners if setting == "ts_rep" else True                     # the lifted token the 2-gram rule bans


@pytest.mark.parametrize("V", [516, 51864])
def test_plain_vocabulary_inputs(V):
    rows, pre, keys, ref = S.plain_reference(V, 1.0, S.TAP_SEEDS[0])
    assert sum(d["gap"] <= 10 * d["tol"] for d in ref) == 0
    assert set(S.edge_tokens(V)) <= {d["token"] for d in ref}


def test_distribution_reference_is_the_distribution():
    """4096 keys on the row with probabilities 1/2, 1/4, 1/8, 1/8: every count within 4 sigma of its binomial expectation."""
    V = S.tap_cfg().vocab_size
    toks = S.dist_reference(V, 9)
    N = S.DIST_N
    for tok, p in zip(S.DIST_TOKENS, (0.5, 0.25, 0.125, 0.125)):
        c = int((toks == tok).sum())
        assert abs(c - N * p) <= 4.0 * math.sqrt(N * p * (1 - p)), (tok, c)
    assert set(toks.tolist()) == set(S.DIST_TOKENS)
    assert not np.array_equal(toks, S.dist_reference(V, 10))                      # the position is part of the counter


def test_decode_seeds_clear_the_guards():
    """The seeds of tests/test_gpu_sampling.py's decode runs (oracle encoder here, the engine's there): no reference decision under 10 x TIE / T,
    sampled != greedy, two keys differ, one key repeats."""
    cfg, sd = S.dec_checkpoint()
    ref = S.SampleRef(cfg, sd)
    encs = {c: S.oracle_encode(ref.orc, cfg, c) for c in set(S.DEC_CLIPS)}
    for name, (T, ts, rep, seed) in S.DEC_CASES.items():
        S.dec_guards(ref, S.dec_gp(cfg, ts, rep), T, seed, encs)
    S.dec_guards(ref, S.dec_gp(cfg, False, False), 1.0, S.DEC_SECOND_SEED, encs)
    # the repetition rules bite in their case
    gp = S.dec_gp(cfg, False, True)
    T, _, _, seed = S.DEC_CASES["T0.4_rep"]
    import dataclasses
    plain = dataclasses.replace(gp, repetition_penalty=1.0, no_repeat_ngram_size=0)
    assert ref.decode(encs[0], gp, T, seed, 0)[0] != ref.decode(encs[0], plain, T, seed, 0)[0]


def test_fallback_inputs_have_a_gap():
    cfg, sd = S.fb_checkpoint()
    ref = S.SampleRef(cfg, sd)
    gp = S.fb_gp(cfg, sd)
    encs = {c: S.oracle_encode(ref.orc, cfg, c) for c in S.FB_CLIPS}
    runs = S.fb_reference(ref, cfg, gp, encs)
    thr, low, high = S.fb_threshold(runs)
    assert low < thr < high and high - low > 0.005
    for r in runs:
        assert min(r["greedy_gaps"]) >= 10 * S.TIE and min(r["sampled_gaps"]) >= 10 * S.TIE / S.t32(S.FB_TEMPS[1])
        assert r["greedy"] != r["sampled"]
    assert runs[1]["cr_sampled"] < thr


def test_longform_inputs_flag_exactly_one_window():
    """The recording of the long-form test: three windows, exactly one window above the threshold in the greedy pass (it
    falls back and passes), every decision of every attempt 10 x TIE away from its runner-up (in logit units)."""
    cfg, sd, gp = S.lf_setup()
    ref = S.SampleRef(cfg, sd)
    thr, hi, lo, plain, rec = S.lf_run(ref, cfg, gp, S.lf_inputs())
    assert lo < thr < hi
    assert [w["attempts"] for w in rec] == [2, 1, 1] and [w["temperature"] for w in rec] == [S.LF_TEMPS[1], 0.0, 0.0]
    assert sum(w["ratios"][0] > thr for w in plain) == 1 and rec[0]["ratios"][1] < thr
    assert min(w["gap"] for w in rec) >= 10 * S.TIE
    assert rec[0]["ids"] != plain[0]["ids"] and [w["seek"] for w in rec] == [w["seek"] for w in plain]
