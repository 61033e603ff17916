"""VAD long-form on the GPU (include/wm.h wm_vad_windows).  The kernels against the restated contract of tests/vad_ref.py —
regions and windows as integers, E, R and the thresholds as bit patterns — at the frame counts where a tile, a wave or a block ends, in batches,
twice, inside a decode, with every argument error; then generate_from_wav(vad_longform=True) end to end on the micro checkpoint against the same
cuts decoded one by one."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import vad_ref as V
from helpers import synth
from test_gpu_token_timestamps import checkpoint
from whisper_medusa import WhisperMedusaModel, engine as E_

pytestmark = pytest.mark.gpu
TILE = E_.VAD_TILE


@pytest.fixture(scope="module")
def rig(gpu):
    cfg, sd = checkpoint("micro")       # micro shape with alignment heads (they do not touch the decode)
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=8)
    yield cfg, m
    m.engine.close()


@pytest.fixture(scope="module")
def long_ref():
    buf, n, P = V.long_case(tile=TILE)
    return buf, n, P, V.vad_windows_ref(buf, n, P)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _batch(bufs, dev):
    """The padded buffer [C, n_max]: every recording's own buffer, GARBAGE behind it up to n_max."""
    n_max = max(len(b) for b in bufs)
    x = np.full((len(bufs), n_max), V.GARBAGE, dtype=np.float32)
    for c, b in enumerate(bufs):
        x[c, :len(b)] = b
    return torch.from_numpy(x).to(dev)


def _same(got, ref, tag):
    regions, windows, taps, c = got
    assert regions[c] == ref["regions"], (tag, regions[c][:6], ref["regions"][:6])
    assert windows[c] == ref["windows"], (tag, windows[c][:6], ref["windows"][:6])
    assert np.array_equal(_bits(taps["E"][c]), _bits(ref["E"])), tag
    for k in ("R", "thr_on", "thr_off"):
        assert _bits(taps[k][c: c + 1])[0] == _bits([ref[k]])[0], (tag, k)


def _run_grouped(eng, dev, cases, refs=None):
    """Cases grouped by their parameters, one call per group; every recording against the restatement."""
    groups = {}
    for k, (name, buf, n, P) in enumerate(cases):
        groups.setdefault(tuple(sorted((a, float(b)) for a, b in P.items())), []).append(k)
    for ks in groups.values():
        P = cases[ks[0]][3]
        got = eng.vad_windows(_batch([cases[k][1] for k in ks], dev), [cases[k][2] for k in ks], P, taps=True)
        for c, k in enumerate(ks):
            ref = refs[k] if refs else V.vad_windows_ref(cases[k][1], cases[k][2], P)
            _same(got + (c,), ref, cases[k][0])


# ---- 1. the kernels: parity -----------------------------------------------------------------------------------------------------------------------
def test_kernels_equal_the_restatement_on_the_seeded_list(rig, gpu):
    _, m = rig
    _run_grouped(m.engine, gpu, V.seeded_cases())
    assert m.engine.last_vad_ms > 0


def test_frame_counts_at_lane_wave_tile_and_block_edges(rig, gpu):
    """T at the edges of a thread's 4 positions, a wave, the energy kernel's 256-frame quarter and the 1024-position tile (a recording owns
    T // TILE + 1 tiles: position T is the first of a tile of its own when T is a multiple)."""
    _, m = rig
    counts = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1]
    rng = np.random.default_rng(21)
    cases = []
    for T in counts:
        for cut in (0, 53):
            # speech in bursts up to the last frame, so that the last run closes at T
            plan, t = [], 0
            while t < T:
                k = min(T - t, int(rng.integers(1, 40)))
                plan.append(("LQTD"[len(plan) % 4] if T - t > k else "L", k))
                t += k
            buf, n = V.render(rng, plan, cut)
            cases.append((f"T={T}-{cut}", buf, n, V.default_params(min_silence=3, min_speech=2, pad=2, F=50)))
    _run_grouped(m.engine, gpu, cases)


def test_one_long_recording_across_the_blocks_of_every_kernel(rig, gpu, long_ref):
    _, m = rig
    buf, n, P, ref = long_ref
    T, F, s, E = ref["T"], P["F"], ref["s"], ref["E"]
    assert 38 * TILE < T < 40 * TILE
    edges = np.arange(TILE, T, TILE)
    dead = (E < ref["thr_on"]) & (E >= ref["thr_off"])
    # from the restatement alone: a dead-band run crosses a block edge after speech and after silence, a region crosses one, a split search
    # crosses one, and the last run closes at T
    assert any(dead[e - 1] and dead[e] and s[e] == 1 for e in edges) and any(dead[e - 1] and dead[e] and s[e] == 0 for e in edges)
    assert any(a < e < b for a, b in ref["regions"] for e in edges)
    cuts = [(a, b) for a, b in ref["pieces"] if (a, b) not in ref["regions"]]
    assert len(cuts) >= 6
    starts = {a for a, _ in ref["regions"]}
    searched = [(a + F // 2, a + F) for a, b in ref["pieces"] if any(ra <= a and b < rb for ra, rb in ref["regions"])]
    assert any(lo < e <= hi for lo, hi in searched for e in edges)
    assert ref["regions"][-1][1] == T and starts
    got = m.engine.vad_windows(_batch([buf], gpu), [n], P, taps=True)
    _same(got + (0,), ref, "long")


def test_batches_of_ragged_recordings_in_both_orders(rig, gpu, long_ref):
    _, m = rig
    P = V.default_params()
    pool = [c for c in V.seeded_cases(range(2)) if c[3] == P]
    rng = np.random.default_rng(4)
    big, nb = V.render(rng, [("Q", 700), ("L", 900), ("D", 30), ("Q", 500), ("T", 300), ("Q", 100)], cut=91)       # spans three tiles
    five = [pool[0], ("big", big, nb, P), pool[5], pool[9], pool[3]]
    alone = [m.engine.vad_windows(_batch([b], gpu), [n], P, taps=True) for _, b, n, _ in five]
    for sel in ([0], [0, 1], [1, 0], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0]):
        got = m.engine.vad_windows(_batch([five[k][1] for k in sel], gpu), [five[k][2] for k in sel], P, taps=True)
        for c, k in enumerate(sel):
            assert got[0][c] == alone[k][0][0] and got[1][c] == alone[k][1][0], (sel, k)
            assert np.array_equal(_bits(got[2]["E"][c]), _bits(alone[k][2]["E"][0]))
            _same(got + (c,), V.vad_windows_ref(five[k][1], five[k][2], P), (sel, k))


# ---- 2. the kernels: determinism, state and errors --------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes(rig, gpu, long_ref):
    _, m = rig
    buf, n, P, _ = long_ref
    x = _batch([buf, buf[: 5000 * 160]], gpu)
    a = m.engine.vad_windows(x, [n, 5000 * 160 - 3], P, taps=True)
    b = m.engine.vad_windows(x, [n, 5000 * 160 - 3], P, taps=True)
    assert a[0] == b[0] and a[1] == b[1]
    for c in range(2):
        assert _bits(a[2]["E"][c]).tobytes() == _bits(b[2]["E"][c]).tobytes()
    for k in ("R", "thr_on", "thr_off"):
        assert _bits(a[2][k]).tobytes() == _bits(b[2][k]).tobytes()


def test_a_call_inside_a_decode_leaves_the_decode_alone(rig, gpu):
    cfg, m = rig
    eng = m.engine
    feats = m.extract_features([synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160) for i in (0, 1)])
    gp = m._gen_params(None, None, None, 20, None, None, False, None, None, None, None, None)
    eng.encode(feats)
    want = eng.decode(gp, 2)
    name, buf, n, P = V.seeded_cases(range(1))[0]
    x = _batch([buf], gpu)
    ref = V.vad_windows_ref(buf, n, P)
    eng.encode(feats)
    g, _alive = eng._gen_struct(gp)
    eng._check(eng.lib.wm_decode_begin(eng.h, C.byref(g), 2), "wm_decode_begin")
    regions, windows = eng.vad_windows(x, [n], P)
    assert regions == [ref["regions"]] and windows == [ref["windows"]]
    left = C.c_int32(0)
    eng._check(eng.lib.wm_decode_run(eng.h, 1 << 30, C.byref(left)), "wm_decode_run")
    assert [eng.tokens(b) for b in range(2)] == want
    assert eng.decode(gp, 2) == want            # the captured graphs still replay


def _raw(eng, x, ns, P, C_=None, n_max=None, cap_r=64, cap_w=64, null=()):
    i32p = C.POINTER(C.c_int32)
    ns = np.ascontiguousarray(ns, dtype=np.int64)
    prm = E_.WmVadParams(**P)
    nr, nw = np.full(len(ns), -7, np.int32), np.full(len(ns), -7, np.int32)
    reg, win = np.full((max(cap_r, 1), 2), -7, np.int32), np.full((max(cap_w, 1), 2), -7, np.int32)
    arg = dict(samples=C.c_void_p(x.data_ptr()), n_samples=ns.ctypes.data_as(C.POINTER(C.c_int64)), params=C.byref(prm),
               n_regions=nr.ctypes.data_as(i32p), regions=reg.ctypes.data_as(i32p), n_windows=nw.ctypes.data_as(i32p), windows=win.ctypes.data_as(i32p))
    for k in null:
        arg[k] = None
    rc = eng.lib.wm_vad_windows(eng.h, len(ns) if C_ is None else C_, arg["samples"], x.shape[1] if n_max is None else n_max, arg["n_samples"],
                                arg["params"], arg["n_regions"], arg["regions"], cap_r, arg["n_windows"], arg["windows"], cap_w,
                                None, None, None, None, None)
    untouched = bool(np.all(nr == -7) and np.all(nw == -7) and np.all(reg == -7) and np.all(win == -7))
    return rc, eng.lib.wm_last_error(eng.h).decode(), untouched


def test_argument_and_capacity_errors_come_back_with_their_reason(rig, gpu):
    _, m = rig
    eng = m.engine
    name, buf, n, P0 = next(c for c in V.seeded_cases(range(1)) if c[0].startswith("gaps"))
    x = _batch([buf], gpu)
    ref = V.vad_windows_ref(buf, n, P0)
    assert len(ref["regions"]) == 3 and len(ref["windows"]) >= 2
    inf, nan = float("inf"), float("nan")
    bad = [(dict(k_off=0.0), "k_off <= k_on"), (dict(k_off=2.0, k_on=1.0), "k_off <= k_on"), (dict(k_on=inf), "k_off <= k_on"), (dict(k_on=nan), "k_off <= k_on"),
           (dict(abs_off=-1.0), "abs_off <= abs_on"), (dict(abs_off=1.0, abs_on=0.5), "abs_off <= abs_on"), (dict(abs_on=inf), "abs_off <= abs_on"),
           (dict(abs_on=nan), "abs_off <= abs_on"), (dict(q_permille=-1), "q_permille"), (dict(q_permille=1001), "q_permille"),
           (dict(min_silence=0), "min_silence"), (dict(min_speech=0), "min_speech"), (dict(pad=-1), "pad must"), (dict(F=1), "F must be at least 2")]
    for change, word in bad:
        rc, err, untouched = _raw(eng, x, [n], dict(P0, **change))
        assert rc == -1 and re.search(word, err) and untouched, (change, rc, err)
    for null in ("samples", "n_samples", "params", "n_regions", "regions", "n_windows", "windows"):
        rc, err, _ = _raw(eng, x, [n], P0, null=(null,))
        assert rc == -1 and "null pointer" in err, null
    for kw, word in ((dict(C_=0), "C must be"), (dict(C_=E_.VAD_CLIPS_MAX + 1), "C must be"), (dict(n_max=0), "n_max must be"),
                     (dict(cap_r=-1), "must not be negative")):
        rc, err, untouched = _raw(eng, x, [n], P0, **kw)
        assert rc == -1 and re.search(word, err) and untouched, (kw, err)
    for ns, word in (([0], r"n_samples\[0\] = 0 outside"), ([x.shape[1] + 1], r"n_samples\[0\] = \d+ outside")):
        rc, err, untouched = _raw(eng, x, ns, P0)
        assert rc == -1 and re.search(word, err) and untouched, (ns, err)
    # a result that does not fit: the needed counts by name, the outputs untouched
    rc, err, untouched = _raw(eng, x, [n], P0, cap_r=2)
    assert rc == -1 and f"needs 3 regions and {len(ref['windows'])} windows" in err and untouched, err
    rc, err, untouched = _raw(eng, x, [n], P0, cap_w=len(ref["windows"]) - 1)
    assert rc == -1 and f"needs 3 regions and {len(ref['windows'])} windows" in err and untouched, err
    rc, err, untouched = _raw(eng, x, [n], P0, cap_r=3, cap_w=len(ref["windows"]))
    assert rc == 0 and not untouched
    # more windows than a call may return: a ValueError that says to split the call
    Tw = E_.VAD_WINDOWS_MAX + 40
    tone = torch.full((1, Tw * 2 * 160), 0.1, device=gpu)
    with pytest.raises(ValueError, match="split the call"):
        eng.vad_windows(tone, [tone.shape[1]], dict(P0, F=2, pad=0, min_speech=1, min_silence=1))
    with pytest.raises(ValueError, match="one entry per recording"):
        eng.vad_windows(x, [n, n], P0)
    regions, windows = eng.vad_windows(x, [n], P0)                   # still usable
    assert regions == [ref["regions"]] and windows == [ref["windows"]]


# ---- 3. end to end on the micro checkpoint ----------------------------------------------------------------------------------------------------------------
NEW = 10
DIV = dict(no_repeat_ngram_size=1)      # random weights repeat one id for ever; no id twice: rows of many different tokens


def _strip(row, P, cfg):
    gen = row[P:]
    return gen[: next((q for q, t in enumerate(gen) if t in (cfg.eos_token_id, cfg.pad_token_id)), len(gen))]


@pytest.fixture(scope="module")
def recordings(rig):
    """Three recordings and what the restatement alone says of them under the default options on the micro window (192 frames): at least 3
    windows for the two with speech, a split region, a dropped burst, and one recording of digital silence."""
    from whisper_medusa import vad
    cfg, _ = rig
    assert cfg.n_mel_frames == 192
    P = vad.lower_options(None, cfg.n_mel_frames)
    rng = np.random.default_rng(8)
    plans = [[("Q", 30), ("L", 80), ("Q", 80), ("L", 400), ("Q", 90), ("L", 10), ("Q", 90), ("T", 60), ("Q", 40)],
             [("L", 150), ("Q", 100), ("T", 100), ("Q", 70), ("L", 120), ("Q", 60)],
             [("Z", 250)]]
    wavs, refs = [], []
    for plan, cut in zip(plans, (0, 55, 0)):
        buf, n = V.render(rng, plan, cut, tail=0)
        wavs.append(buf[:n].copy())
        refs.append(V.vad_windows_ref(buf, n, P))
    assert all(len(r["windows"]) >= 3 for r in refs[:2]) and refs[2]["windows"] == [] and refs[2]["R"] == 0
    assert any(b - a > P["F"] for r in refs for a, b in r["regions"])                       # a split region
    assert any(b - a < P["min_speech"] for a, b in refs[0]["merged"])                        # a dropped burst
    assert all(v - u <= 192 for r in refs for u, v in r["windows"])
    return wavs, refs


def _one_by_one(m, cfg, wavs, refs, langs=None, **kw):
    """The restatement's cuts [160 u, min(160 v, n)) decoded one window per generate_from_wav call; per recording the calls' outputs."""
    outs = []
    for b, (x, r) in enumerate(zip(wavs, refs)):
        lang = {} if langs is None else dict(language=langs[b])
        outs.append([m.generate_from_wav(x[160 * u: min(160 * v, len(x))], max_new_tokens=NEW, **DIV, **lang, **kw) for u, v in r["windows"]])
    return outs


def _seq(o):
    return (o["sequences"] if isinstance(o, dict) else o)[0].tolist()


def test_vad_longform_equals_the_same_cuts_decoded_one_by_one(rig, recordings):
    cfg, m = rig
    wavs, refs = recordings
    P = len(synth.default_prompt(cfg))
    out = m.generate_from_wav(wavs, vad_longform=True, max_new_tokens=NEW, **DIV, return_dict_in_generate=True)
    assert m.last_stats["ms_vad"] > 0 and m.last_stats["longform_windows"] == [len(r["windows"]) for r in refs]
    alone = _one_by_one(m, cfg, wavs, refs)
    for b, r in enumerate(refs):
        want = synth.default_prompt(cfg) + [t for o in alone[b] for t in _strip(_seq(o), P, cfg)] + [cfg.eos_token_id]
        assert out["sequences"][b, : len(want)].tolist() == want, b
        assert torch.all(out["sequences"][b, len(want):] == cfg.pad_token_id)
        n = len(r["windows"])
        assert out["vad_windows"][b, :n].tolist() == [list(w) for w in r["windows"]] and torch.all(out["vad_windows"][b, n:] == -1)
        assert out["speech_regions"][b] == [(a * 0.01, e * 0.01) for a, e in r["regions"]]
    assert out["sequences"][2, : P + 1].tolist() == synth.default_prompt(cfg) + [cfg.eos_token_id]      # digital silence: prompt + EOS
    assert sum(len(_strip(out["sequences"][b].tolist(), P, cfg)) for b in range(2)) > 6
    t = m.generate_from_wav(wavs, vad_longform=True, max_new_tokens=NEW, **DIV)
    assert isinstance(t, torch.Tensor) and torch.equal(t, out["sequences"])


def test_detect_speech_is_the_restatement_in_seconds(rig, recordings):
    cfg, m = rig
    wavs, refs = recordings
    got = m.detect_speech(wavs)
    for g, r in zip(got, refs):
        assert g == dict(regions=[(a * 0.01, b * 0.01) for a, b in r["regions"]], windows=[(a * 0.01, b * 0.01) for a, b in r["windows"]])
    from whisper_medusa import vad
    opts = dict(onset_db=-25.0, min_silence_ms=300, speech_pad_ms=50, max_window_s=1.0)
    P = vad.lower_options(opts, cfg.n_mel_frames)
    got = m.detect_speech(wavs[0], **opts)
    r = V.vad_windows_ref(wavs[0], len(wavs[0]), P)
    assert got == [dict(regions=[(a * 0.01, b * 0.01) for a, b in r["regions"]], windows=[(a * 0.01, b * 0.01) for a, b in r["windows"]])]
    assert all(b - a <= 1.0 + 1e-9 for a, b in got[0]["windows"])


@pytest.fixture(scope="module")
def mix_rig(gpu):
    """The micro shape whose vocabulary ends in Whisper's timestamp block, multilingual (tests/lang_ref.py)."""
    import lang_ref as L
    cfg, sd = L.mix_checkpoint()
    assert cfg.n_mel_frames == 192 and cfg.supports_timestamps and cfg.is_multilingual
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=8)
    yield cfg, m
    m.engine.close()


def test_vad_longform_segments_are_offset_by_the_window_start(mix_rig, recordings):
    cfg, m = mix_rig
    wavs, refs = recordings
    kw = dict(return_timestamps=True, return_segments=True, language="en")
    out = m.generate_from_wav(wavs[:2], vad_longform=True, max_new_tokens=NEW, **DIV, **kw)
    alone = _one_by_one(m, cfg, wavs[:2], refs[:2], **kw)
    total = 0
    for b, r in enumerate(refs[:2]):
        want = [(float(sg["start"]) + u * 0.01, float(sg["end"]) + u * 0.01, sg["tokens"].tolist())
                for o, (u, _) in zip(alone[b], r["windows"]) for sg in o["segments"][0]]
        got = [(float(sg["start"]), float(sg["end"]), sg["tokens"].tolist()) for sg in out["segments"][b]]
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g[2] == w[2] and g[0] == pytest.approx(w[0], abs=1e-6) and g[1] == pytest.approx(w[1], abs=1e-6)
        total += len(got)
    assert total > 0


def test_vad_longform_token_timestamps_and_logprobs(rig, recordings):
    cfg, m = rig
    wavs, refs = recordings
    P = len(synth.default_prompt(cfg))
    kw = dict(return_token_timestamps=True, return_token_logprobs=True)
    out = m.generate_from_wav(wavs, vad_longform=True, max_new_tokens=NEW, **DIV, **kw)
    assert m.last_stats["ms_token_timestamps"] > 0
    alone = _one_by_one(m, cfg, wavs, refs, **kw)
    for b, r in enumerate(refs):
        tt, lp, eos_lp = [0.0] * P, [0.0] * P, 0.0
        for o, (u, _) in zip(alone[b], r["windows"]):
            k = len(_strip(_seq(o), P, cfg))
            tt += (o["token_timestamps"][0, P: P + k].cpu() + torch.tensor(u * 0.01, dtype=torch.float32)).tolist()
            lp += o["token_logprobs"][0, P: P + k].tolist()
            if P + k < int(o["lengths"][0]):
                eos_lp = float(o["token_logprobs"][0, P + k])
        n = len(tt) + 1
        assert int(out["lengths"][b]) == n
        assert out["token_timestamps"][b, :n].tolist() == [float(np.float32(v)) for v in tt + [tt[-1]]], b
        # the tolerance tests/test_gpu_scores.py holds between a batch's scoring pass and the one-clip call's
        assert torch.allclose(out["token_logprobs"][b, :n].cpu(), torch.tensor(lp + [eos_lp], dtype=torch.float32), atol=1e-4), b
    nmax = max(len(r["windows"]) for r in refs)
    assert out["window_avg_logprob"].shape == (3, nmax) and torch.isnan(out["window_avg_logprob"][2]).all()


def test_vad_longform_word_timestamps(rig, recordings):
    import words_ref as W
    from test_gpu_words import _equal
    cfg, m = rig
    wavs, refs = recordings
    tok, _ = W.whole_char_tokenizer(cfg.eos_token_id)
    P = len(synth.default_prompt(cfg))
    out = m.generate_from_wav(wavs[:2], vad_longform=True, max_new_tokens=NEW, **DIV, return_word_timestamps=True, tokenizer=tok)
    assert m.last_stats["ms_words"] > 0 and "vad_windows" in out
    _equal(tok, cfg, out, P, 2)
    # the words of a later window lie on the recording's clock: not before the window's start
    last_u = refs[0]["windows"][-1][0] * 0.01
    assert max(w["timestamp"][1] for w in out["words"][0]) >= last_u


def test_vad_longform_two_languages(mix_rig, recordings):
    cfg, m = mix_rig
    wavs, refs = recordings
    langs = ["de", "fr", "de"]
    out = m.generate_from_wav(wavs, vad_longform=True, max_new_tokens=NEW, **DIV, language=langs)
    alone = _one_by_one(m, cfg, wavs, refs, langs=langs)
    for b, r in enumerate(refs):
        prompt = synth.default_prompt(cfg, f"<|{langs[b]}|>", "transcribe")
        P = len(prompt)
        want = prompt + [t for o in alone[b] for t in _strip(_seq(o), P, cfg)] + [cfg.eos_token_id]
        assert out[b, : len(want)].tolist() == want, b
        assert cfg.lang_to_id[f"<|{langs[b]}|>"] in want[:4]
