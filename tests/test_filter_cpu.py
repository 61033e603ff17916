"""Top-k, top-p and min-p filters of the seeded draw (include/wm.h wm_set_sampling_filter / wm_filter_rows) without a GPU: the
reference of tests/filter_ref.py against transformers' warpers, the guards the inputs of tests/test_gpu_filter.py were chosen under (from the
reference alone), and the surface: header, exports, GenParams, the keywords of generate()."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import filter_ref as F
import sample_ref as S
from helpers import ROOT, GenParams, synth
from whisper_medusa import WhisperMedusaModel
from whisper_medusa import engine as wm_engine


def _processed(name):
    cfg, gp, _ = F.shape(name)
    rows, pre, lab = F.cases(name)
    proc = S._sr.hf_processor(cfg, gp.begin_index) if gp.timestamps else None
    return [F.processed_cached(rows[r], pre[r], gp, cfg, proc)[0] for r in range(len(pre))], lab


# ---- 1. the reference against transformers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.SHAPES)
def test_reference_keeps_what_transformers_keeps(name):
    """The kept set of the reference equals TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper on v / T, except where HF's own fp32 cumsum
    sits within the tolerance of the boundary (its error: one rounding per addend, n 2^-24 of the mass) or a tie straddles the top-p boundary —
    the two exclusions, both of top-p rows only; top-k and min-p rows are all compared.  That band grows with the vocabulary (3e-3 of the mass
    at V = 51864), so the share of rows compared is asserted against the whole list, not against the excluded ones: three quarters at least."""
    from transformers.generation.logits_process import TopKLogitsWarper, TopPLogitsWarper, MinPLogitsWarper
    vs, lab = _processed(name)
    compared = excluded = 0
    for T in F.TAP_T:
        for (k, p, mp) in F.FILTERS:
            for r, v in enumerate(vs):
                th = F.threshold(v, T, k, p, mp)
                n = int(np.isfinite(v).sum())
                if n == 0:
                    continue
                if p < 1.0 and (th["tie"] or th["hf_margin"] <= n * 2.0 ** -24):
                    excluded += 1
                    continue
                s = (torch.from_numpy(v) / float(np.float32(T)))[None]
                ids = torch.zeros(1, 1, dtype=torch.long)
                if k > 0:
                    s = TopKLogitsWarper(top_k=k)(ids, s)
                if p < 1.0:
                    s = TopPLogitsWarper(top_p=p)(ids, s)
                if mp > 0.0:
                    s = MinPLogitsWarper(min_p=mp)(ids, s)
                want = torch.isfinite(s[0]).numpy()
                got = F.kept(v, T, k, p, mp)
                assert np.array_equal(got, want), (name, T, (k, p, mp), lab[r], int(got.sum()), int(want.sum()))
                compared += 1
    assert compared >= 0.75 * (compared + excluded), (compared, excluded)


def test_threshold_by_hand():
    v = np.append(np.log(np.array([0.5, 0.25, 0.125, 0.125])), -np.inf).astype(np.float32)
    assert F.threshold(v, 1.0, 2)["kept"] == 2 and F.threshold(v, 1.0, 3)["kept"] == 4               # a tie at the k-th place is kept whole
    assert np.isneginf(F.threshold(v, 1.0, 4)["thr"]) and np.isneginf(F.threshold(v, 1.0, 9)["thr"])  # |R| <= k: nothing to cut
    assert F.threshold(v, 1.0, 0, 0.4)["kept"] == 1 and F.threshold(v, 1.0, 0, 0.6)["kept"] == 2 and F.threshold(v, 1.0, 0, 0.8)["kept"] == 4
    assert F.threshold(v, 1.0, 0, 1.0, 0.3)["kept"] == 2 and F.threshold(v, 1.0, 0, 1.0, 0.2)["kept"] == 4
    assert F.threshold(v, 0.5, 0, 1.0, 0.3)["kept"] == 1                                            # the ratio is taken at the temperature
    z = np.array([1.0, 0.0, -0.0, -1.0], dtype=np.float32)
    th = F.threshold(z, 1.0, 2)
    assert th["kept"] == 3 and np.float32(th["thr"]).view(np.uint32) == 0                           # +0.0 and -0.0 are one value; tau is +0.0
    assert F.tolerance(1.0, 0.0) == 2 * F.EPS


# ---- 2. the guards ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.SHAPES)
def test_tap_inputs_are_decided_and_not_vacuous(name):
    rows, pre, lab = F.cases(name)
    for T in F.TAP_T:
        for flt in F.FILTERS:
            ref = F.reference(name, T, flt)
            if flt[1] < 1.0 or flt[2] > 0.0:
                und = [lab[r] for r, d in enumerate(ref) if not F.decided(d)]
                assert len(und) <= F.UNDECIDED_CAP * len(ref), (name, T, flt, und)
            assert all(d["margin"] > d["tol"] for d in ref)
            assert all(d["gap"] > 10 * d["tol"] for d in ref)             # every row's token is compared on the GPU: none sits on a tie of the draw
    # the crafted properties are there after the processors
    k5 = {lab[r]: d for r, d in enumerate(F.reference(name, 1.0, (F.K_REF, 1.0, 0.0)))}
    assert k5["dup2"]["kept"] == 6 and k5["dup3"]["kept"] == 7 and k5["dup17"]["kept"] >= 19 and k5["dup2"]["thr"] == 2.25
    assert k5["one_finite"]["kept"] == 1 and np.isneginf(k5["one_finite"]["thr"])
    assert k5["zeros"]["kept"] == 6 and k5["zeros"]["thr"] == 0.0 and k5["ulp"]["kept"] == 5
    assert k5["all_equal"]["kept"] == F.region_count(name, lab.index("all_equal")) > 50
    assert F.reference(name, 1.0, (0, 0.9, 0.0))[lab.index("dominant")]["kept"] == 1
    if name in ("ts", "ts_rep"):
        assert k5["forced_few"]["forced"] == 1 and k5["forced_few"]["kept"] == 3 and np.isneginf(k5["forced_few"]["thr"])
        assert any(d["forced"] for l, d in k5.items() if l.startswith("random")) and not all(d["forced"] for d in k5.values())
    if name == "ts_rep":
        assert k5["banned"]["token"] != 61 and F.reference("ts", 1.0, (F.K_REF, 1.0, 0.0))[lab.index("banned")]["token"] == 61


def test_distribution_reference():
    V = S.tap_cfg().vocab_size
    toks = F.dist_reference(V, 11)
    assert set(toks.tolist()) == set(S.DIST_TOKENS[:2])
    n0 = int((toks == S.DIST_TOKENS[0]).sum())
    assert abs(n0 - S.DIST_N * 2 / 3) <= 4 * (S.DIST_N * 2 / 9) ** 0.5
    assert not np.array_equal(toks, S.dist_reference(V, 11))


def test_decode_seeds_clear_the_guards():
    """The seeds of the decode cases (oracle encoder here, the engine's on the GPU): every draw clears 10 x TIE / T, every boundary the guard; the
    case DEC_DIFFERS differs from the unfiltered run and from the run under the second top_k."""
    cfg, sd = S.dec_checkpoint()
    ref = F.FilterRef(cfg, sd)
    encs = {c: S.oracle_encode(ref.orc, cfg, c) for c in set(S.DEC_CLIPS)}
    runs = {}
    for name, (T, ts, rep, flt, seed) in F.DEC_CASES.items():
        runs[name] = F.dec_guards(ref, S.dec_gp(cfg, ts, rep), T, seed, flt, encs)
    T, ts, rep, flt, seed = F.DEC_CASES[F.DEC_DIFFERS]
    gp = S.dec_gp(cfg, ts, rep)
    second = F.dec_guards(ref, gp, T, seed, (F.DEC_SECOND_K, 1.0, 0.0), encs)
    plain = {ck: ref.decode(encs[ck[0]], gp, T, seed, ck[1]) for ck in second}
    assert all(min(g) >= 10 * S.TIE / S.t32(T) for _, g, _ in plain.values())
    mine = runs[F.DEC_DIFFERS]
    assert any(mine[ck][0] != plain[ck][0] for ck in mine) and [mine[ck][0] for ck in mine] != [second[ck][0] for ck in mine]
    assert mine[(0, 0)][0] != plain[(0, 0)][0] or mine[(1, 1)][0] != plain[(1, 1)][0]


def test_generate_inputs_have_a_gap():
    cfg, sd = S.fb_checkpoint()
    ref = F.FilterRef(cfg, sd)
    gp = S.fb_gp(cfg, sd)
    encs = {c: S.oracle_encode(ref.orc, cfg, c) for c in S.FB_CLIPS}
    runs = F.fb_reference(ref, cfg, gp, encs)
    thr, low, high = S.fb_threshold(runs)
    assert low < thr < high and high - low > 0.005
    for r in runs:
        assert min(r["greedy_gaps"]) >= 10 * S.TIE and min(r["sampled_gaps"]) >= 10 * S.TIE / S.t32(S.FB_TEMPS[1])
    unfiltered = S.fb_reference(S.SampleRef(cfg, sd), cfg, gp, encs)
    assert runs[0]["sampled"] != unfiltered[0]["sampled"]          # the filter changes the retry the fallback keeps: an engine that dropped it would fail
    # long-form: exactly one window of the greedy pass is flagged and passes under the filtered draw, and that window's ids are not the
    # unfiltered draw's (an engine that dropped the filter under sequential_longform would fail)
    cfg, sd, gp = S.lf_setup()
    ref = F.Filtered(F.FilterRef(cfg, sd), F.LF_FILTER)
    thr, hi, lo, plain, rec = S.lf_run(ref, cfg, gp, S.lf_inputs())
    assert lo < thr < hi and [w["attempts"] for w in rec] == [2, 1, 1]
    assert min(w["gap"] for w in rec) >= 10 * S.TIE and ref.min_ratio > F.GUARD
    _, _, _, _, rec0 = S.lf_run(S.SampleRef(cfg, sd), cfg, gp, S.lf_inputs())
    assert [w["attempts"] for w in rec0] == [2, 1, 1] and rec[0]["ids"] != rec0[0]["ids"]


# ---- 3. the surface --------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported(built_lib):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert re.search(r"#define WM_ABI_VERSION 9\b", hdr) and wm_engine.WM_ABI_VERSION == 9
    for name in ("wm_set_sampling_filter", "wm_filter_rows"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in wm_engine.EXPORTS
    m = re.search(r"typedef struct wm_sample_filter \{([^}]*)\}", hdr)
    fields = [f.split()[-1] for f in m.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in wm_engine.WmSampleFilter._fields_] == ["top_k", "top_p", "min_p"]
    assert ctypes.sizeof(wm_engine.WmSampleFilter) == 12
    m = re.search(r"typedef struct wm_sample_params \{([^}]*)\}", hdr)          # the sampling request keeps its four fields
    assert len([f for f in re.sub(r"/\*.*?\*/", "", m.group(1)).split(";") if f.strip()]) == 4
    for path in (wm_engine.LIB_PATH, wm_engine.LIB_PATH_F16):
        assert os.path.exists(path), f"{path}: build the engine first"
        lib = ctypes.CDLL(path)
        assert lib.wm_abi_version() == 9 and hasattr(lib, "wm_set_sampling_filter") and hasattr(lib, "wm_filter_rows")


def test_gen_params_default_to_off_and_carry_the_filter():
    gp = GenParams(prompt=[1], eos_token_id=2, pad_token_id=2)
    assert (gp.sampling_top_k, gp.sampling_top_p, gp.sampling_min_p) == (0, 1.0, 0.0) == F.OFF
    g = WhisperMedusaModel._sampled_gp(gp, 0.4, 9, [5, 6], (50, 0.9, 0.05))
    assert (g.sampling_top_k, g.sampling_top_p, g.sampling_min_p) == (50, 0.9, 0.05) and g.vanilla and g.sampling_temperature == 0.4
    g = WhisperMedusaModel._sampled_gp(gp, 0.4, 9, [5, 6])
    assert (g.sampling_top_k, g.sampling_top_p, g.sampling_min_p) == F.OFF


def test_generate_keywords():
    cfg = S.tap_cfg()
    m = WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=3), max_batch=2)
    x = torch.zeros(1, cfg.num_mel_bins, cfg.n_mel_frames)
    for kw, word in ((dict(sampling_top_k=-1), "sampling_top_k"), (dict(sampling_top_k=2.5), "sampling_top_k"), (dict(sampling_top_k=True), "sampling_top_k"),
                     (dict(sampling_top_p=0.0), "sampling_top_p"), (dict(sampling_top_p=1.5), "sampling_top_p"),
                     (dict(sampling_min_p=-0.1), "sampling_min_p"), (dict(sampling_min_p=1.01), "sampling_min_p")):
        for T in (0.4, (0.0, 0.4)):
            with pytest.raises(ValueError, match=f"`{word}` has to be"):
                m.generate(x, temperature=T, sampling_seed=7, **kw)
    # on a call that does not sample: refused by name, with or without a seed
    for kw in (dict(sampling_top_k=50), dict(sampling_top_p=0.9), dict(sampling_min_p=0.05)):
        name = next(iter(kw))
        with pytest.raises(ValueError, match=name + ".*does not sample"):
            m.generate(x, **kw)
        with pytest.raises(ValueError, match=name + ".*does not sample"):
            m.generate(x, temperature=0.0, sampling_seed=7, **kw)
    # the request carries the filter; values that mean "off" ask for nothing
    req = m._sampling_request(0.4, dict(sampling_seed=7, sampling_top_k=50, sampling_min_p=0.05), None)
    assert req["filter"] == (50, 1.0, 0.05)
    assert m._sampling_request(0.4, dict(sampling_seed=7), None)["filter"] == F.OFF
    assert m._sampling_request(None, dict(sampling_top_k=0, sampling_top_p=1.0, sampling_min_p=0.0), None) is None
    # HF's own keywords stay refused with a seed, and the message names the engine's
    with pytest.raises(NotImplementedError, match="sampling_top_k="):
        m.generate(x, temperature=0.4, sampling_seed=7, top_k=50)
