"""VAD long-form (vad_longform) without a GPU: the invariants of the restated contract (tests/vad_ref.py) on the seeded list, the
classes that list has to hold, the host build of the kernels' arithmetic (csrc/wm_vad.h) against the restatement, the lowering of vad_options, the
routes over an engine double whose vad_windows IS the restatement, every refusal, and the surface (header, export, sources, ABI)."""
import os
import re

import numpy as np
import pytest
import torch

import vad_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = V.seeded_cases()
REF = [V.vad_windows_ref(buf, n, P) for _, buf, n, P in CASES]


# ---- the restated contract: invariants ---------------------------------------------------------------------------------------------------------------
def test_invariants_hold_on_every_seeded_case():
    for (name, _, n, P), r in zip(CASES, REF):
        T, F = r["T"], P["F"]
        assert T == -(-n // 160)
        prev = 0
        for a, b in r["regions"]:
            assert prev <= a < b <= T, name                   # ordered, disjoint, inside [0, T]
            prev = b
        prev = 0
        for u, v in r["windows"]:
            assert prev <= u < v <= T and v - u <= F, name    # ordered, disjoint, at most F frames
            prev = v
        in_region = np.zeros(T + 1, dtype=np.int32)
        for a, b in r["regions"]:
            in_region[a:b] += 1
        assert in_region.max(initial=0) <= 1, name
        cover = np.zeros(T + 1, dtype=np.int32)
        starts, stops = {a for a, _ in r["regions"]}, {b for _, b in r["regions"]}
        for u, v in r["windows"]:
            cover[u:v] += 1
            # no window starts or ends outside a region: its first and its last frame are region frames
            assert in_region[u] == 1 and in_region[v - 1] == 1, name
        assert np.all(cover[in_region == 1] == 1), name       # every region frame lies in exactly one window
        assert starts or not r["windows"]
        assert stops or not r["windows"]
        for a, b in r["pieces"]:
            assert 0 < b - a <= F, name


def test_the_seeded_list_holds_every_case_class():
    """Counted from the restatement alone: at least 5 cases of every class, or the list is too weak."""
    cls = {}

    def hit(key, cond):
        cls[key] = cls.get(key, 0) + int(bool(cond))

    for (name, buf, n, P), r in zip(CASES, REF):
        ms, sp, pad, F, T = P["min_silence"], P["min_speech"], P["pad"], P["F"], r["T"]
        gaps = [r["runs"][i + 1][0] - r["runs"][i][1] for i in range(len(r["runs"]) - 1)]
        for d in (-1, 0, 1):
            hit(f"gap = min_silence {d:+d}", ms + d in gaps)
        lens = [b - a for a, b in r["merged"]]
        hit("region of min_speech - 1", sp - 1 in lens and sp > 1)
        hit("region of min_speech", sp in lens)
        kgaps = [r["kept"][i + 1][0] - r["kept"][i][1] for i in range(len(r["kept"]) - 1)]
        for d in (-1, 0, 1):
            hit(f"gap = 2 pad {d:+d}", pad > 0 and 2 * pad + d in kgaps)
        hit("odd gap split at g / 2", any(g < 2 * pad and g % 2 for g in kgaps))
        hit("padding clipped at 0", r["kept"] and r["kept"][0][0] - pad < 0)
        hit("padding clipped at T", r["kept"] and r["kept"][-1][1] + pad > T)
        rl = [b - a for a, b in r["regions"]]
        hit("region of F", F in rl)
        hit("region of F + 1", F + 1 in rl)
        hit("region above 2 F", any(x > 2 * F for x in rl))
        hit("split argmin ties", r["ties"] > 0 and name.startswith("tie"))
        E, s = r["E"], r["s"]
        dead = (E < r["thr_on"]) & (E >= r["thr_off"])
        hit("dead band after speech", any(dead[t] and s[t - 1] == 1 for t in range(1, T)))
        hit("dead band after silence", any(dead[t] and s[t - 1] == 0 for t in range(1, T)))
        hit("abs_on decides", np.float32(r["R"]) * np.float32(P["k_on"]) < P["abs_on"] and r["R"] > 0)
        hit("abs_on decides, with speech", np.float32(r["R"]) * np.float32(P["k_on"]) < P["abs_on"] and r["R"] > 0 and r["regions"])
        hit("digital silence", r["R"] == 0 and not np.any(buf[:n]) and not r["windows"])
        hit("all speech", bool(np.all(s == 1)) and T > 1)
        hit("n_samples no multiple of 160", n % 160 != 0)
        hit("T = 1", T == 1)
        hit("packing absorbs two or more pieces", any(k >= 2 for k in r["absorbed"]))
        hit("packing refuses by one frame", F + 1 in r["refused"])
        hit("packing fits to the frame", any(v - u == F and k >= 1 for (u, v), k in zip(r["windows"], r["absorbed"])))
    weak = {k: v for k, v in cls.items() if v < 5}
    assert not weak, weak


def test_a_tie_is_won_by_the_smallest_frame():
    for (name, _, n, P), r in zip(CASES, REF):
        if name.startswith("tie"):
            a = r["regions"][0][0]
            assert r["pieces"][0] == (a, a + P["F"] // 2)


def test_garbage_behind_n_samples_is_not_audio():
    for name, buf, n, P in CASES[:40]:
        clean = buf.copy()
        clean[n:] = 0
        assert np.array_equal(V.frame_energy(buf, n), V.frame_energy(clean, n)), name


def test_the_energy_is_the_contracts_serial_float32_loop():
    """frame_energy's vectorised form against the contract written out one float32 operation at a time."""
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, 5 * 160 - 37).astype(np.float32)
    E = V.frame_energy(x, len(x))
    xp = np.concatenate([x, np.zeros(37, dtype=np.float32)])
    for t in range(5):
        p = [np.float32(0)] * 16
        for j in range(16):
            for i in range(10):
                v = xp[160 * t + 16 * i + j]
                p[j] = np.float32(p[j] + np.float32(v * v))
        for o in (8, 4, 2, 1):
            for j in range(o):
                p[j] = np.float32(p[j] + p[j + o])
        assert p[0].view(np.uint32) == E[t].view(np.uint32)


# ---- the kernels' arithmetic, built for the host -----------------------------------------------------------------------------------------------------
def test_host_build_of_the_kernels_arithmetic_equals_the_restatement(tmp_path):
    """csrc/wm_vad.h is plain C++: the energy of a frame, the per-region stage and the split-and-pack loop the kernels run, compiled by the host
    compiler (tests/vad_host.cpp), against the restatement on the seeded list and on 3000 random recordings."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "vad_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "whisper-medusa_amd", "csrc"),
                    os.path.join(ROOT, "tests", "vad_host.cpp"), "-o", exe], check=True)
    cases = [(buf, n, P) for _, buf, n, P in CASES]
    rng = np.random.default_rng(11)
    cases += [V.random_case(rng) for _ in range(3000)]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for buf, n, P in cases:
            f.write(np.int32(n).tobytes())
            f.write(np.asarray([P["k_on"], P["k_off"], P["abs_on"], P["abs_off"]], dtype=np.float32).tobytes())
            f.write(np.asarray([P["q_permille"], P["min_silence"], P["min_speech"], P["pad"], P["F"]], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(buf[:n], dtype=np.float32).tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.txt")], check=True)
    lines = open(tmp_path / "out.txt").read().split("\n")
    assert len(lines) >= 3 * len(cases)
    for k, (buf, n, P) in enumerate(cases):
        r = REF[k] if k < len(CASES) else V.vad_windows_ref(buf, n, P)
        assert [int(x, 16) for x in lines[3 * k].split()] == [int(x) for x in r["E"].view(np.uint32)], k
        got = [int(x) for x in lines[3 * k + 1].split()]
        assert list(zip(got[0::2], got[1::2])) == r["regions"], (k, P)
        got = [int(x) for x in lines[3 * k + 2].split()]
        assert list(zip(got[0::2], got[1::2])) == r["windows"], (k, P)


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------------
def test_surface_header_exports_sources_and_abi():
    from whisper_medusa import engine
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert re.search(r"int wm_vad_windows\(wm_ctx\* ctx, int C, const float\* samples", hdr)
    body = re.search(r"typedef struct wm_vad_params \{(.*?)\} wm_vad_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [n for n, _ in engine.WmVadParams._fields_]
    for word in ("q_permille", "fmaxf", "min_silence", "bit pattern", "WM_VAD_WINDOWS_MAX", "wm_decode_begin", "split the call"):
        assert word in hdr
    assert "wm_vad_windows" in engine.EXPORTS
    assert re.search(r"#define WM_ABI_VERSION\s+9\b", hdr) and engine.WM_ABI_VERSION == 9
    for name, val in (("WM_VAD_CLIPS_MAX", engine.VAD_CLIPS_MAX), ("WM_VAD_FRAMES_MAX", engine.VAD_FRAMES_MAX),
                      ("WM_VAD_TOTAL_FRAMES_MAX", engine.VAD_TOTAL_FRAMES_MAX), ("WM_VAD_WINDOWS_MAX", engine.VAD_WINDOWS_MAX)):
        assert eval(re.search(r"#define " + name + r"\s+(\(.*?\)|\d+)", hdr).group(1)) == val
    assert engine.VAD_FRAMES_MAX >= 1 << 22 and engine.VAD_WINDOWS_MAX >= 4096
    import build as wm_build
    assert "wm_vad.hip" in wm_build.SOURCES
    src = open(os.path.join(ROOT, "whisper-medusa_amd", "csrc", "wm_vad.hip")).read()
    assert f"#define VAD_TILE {engine.VAD_TILE}" in src


# ---- vad_options -----------------------------------------------------------------------------------------------------------------------------------
def test_vad_options_lowering():
    from whisper_medusa import vad
    P = vad.lower_options(None, 3000)
    assert np.float32(P["k_on"]) == np.float32(10.0 ** -3.0) and np.float32(P["k_off"]) == np.float32(10.0 ** -3.5)
    abs_on = np.float32(160.0 * 10.0 ** -6.0)
    assert np.float32(P["abs_on"]) == abs_on
    assert np.float32(P["abs_off"]) == np.float32(np.float32(abs_on * np.float32(P["k_off"])) / np.float32(P["k_on"]))
    assert 0 <= P["abs_off"] <= P["abs_on"] and 0 < P["k_off"] <= P["k_on"]
    assert (P["q_permille"], P["min_silence"], P["min_speech"], P["pad"], P["F"]) == (950, 50, 25, 20, 3000)
    P = vad.lower_options(dict(onset_db=-20, offset_db=-20, loud_percentile=99.5, min_level_dbfs=-45.0, min_silence_ms=10, min_speech_ms=10,
                               speech_pad_ms=0, max_window_s=1.5), 192)
    assert P["k_on"] == P["k_off"] == float(np.float32(0.01)) and P["abs_off"] <= P["abs_on"] == float(np.float32(160.0 * 10.0 ** -4.5))
    assert (P["q_permille"], P["min_silence"], P["min_speech"], P["pad"], P["F"]) == (995, 1, 1, 0, 150)
    assert vad.lower_options(dict(max_window_s=1.92), 192)["F"] == 192 and vad.lower_options(dict(max_window_s=0.02), 192)["F"] == 2
    assert set(P) == {"k_on", "k_off", "abs_on", "abs_off", "q_permille", "min_silence", "min_speech", "pad", "F"}
    for bad, word in ((dict(onset=-3), "unknown key"), (dict(onset_db="x"), "finite number"), (dict(onset_db=float("nan")), "finite number"),
                      (dict(onset_db=True), "finite number"), (dict(offset_db=-10.0), "must not lie above"), (dict(onset_db=-500, offset_db=-600), "float32 range"),
                      (dict(onset_db=400), "float32 range"), (dict(loud_percentile=101), r"\[0, 100\]"), (dict(loud_percentile=-1), r"\[0, 100\]"),
                      (dict(min_level_dbfs=None), "finite number"), (dict(min_level_dbfs=400.0), "float32 range"),
                      (dict(min_silence_ms=505), "whole multiple of 10 ms"), (dict(min_silence_ms=0), "at least 10 ms"),
                      (dict(min_speech_ms=12.5), "whole multiple of 10 ms"), (dict(min_speech_ms=0), "at least 10 ms"), (dict(speech_pad_ms=-10), "at least 0 ms"),
                      (dict(speech_pad_ms=5), "whole multiple"), (dict(max_window_s=1.93), "max_window_s"), (dict(max_window_s=0.01), "max_window_s"),
                      (dict(max_window_s=1.005), "max_window_s"), (dict(max_window_s="30"), "finite number")):
        with pytest.raises(ValueError, match=word):
            vad.lower_options(bad, 192)
    with pytest.raises(ValueError, match="has to be a dict"):
        vad.lower_options([("onset_db", -3)], 192)


# ---- the routes: an engine double whose vad_windows IS the restatement ---------------------------------------------------------------------------------
from helpers import synth                                                          # noqa: E402
from test_merge_cpu import DE, EN, SCRIPT, _cfg, _lp, _padded, _prompt, _StrideEng, _ts   # noqa: E402
from test_topk_cpu import _Eng, _model                                              # noqa: E402


class _VadEng(_StrideEng):
    """A window decodes to the script of its first sample's code; vad_windows is the restatement on the audio it is handed."""

    def vad_windows(self, samples_dev, n_samples, params, taps=False):
        self.calls.append(("vad_windows", tuple(samples_dev.shape), [int(n) for n in n_samples], dict(params)))
        self.last_vad_ms = 0.25
        refs = [V.vad_windows_ref(samples_dev[c].numpy(), int(n), params) for c, n in enumerate(n_samples)]
        return [r["regions"] for r in refs], [r["windows"] for r in refs]

    def resample(self, t, sr_in, sr_out):
        self.calls.append(("resample", tuple(t.shape), sr_in, sr_out))
        return t.mean(dim=1)[:, ::sr_in // sr_out]


def _audio(plan, frames, tail=0):
    """plan: [(code, first frame, stop frame)..]: constant audio of the code's value there, digital silence elsewhere."""
    x = np.zeros(frames * 160 - tail, np.float32)
    for code, a, b in plan:
        x[a * 160: b * 160] = float(code)
    return x


OPTS = dict(speech_pad_ms=0)                    # no padding: a window starts on its burst's first sample, which carries the code
A = _audio([(1, 10, 110), (2, 210, 330), (9, 430, 470)], 500, tail=33)          # three windows (micro window: 192 frames)
SILENT = np.zeros(300 * 160, np.float32)
C6 = _audio([(6, 0, 50), (5, 120, 160)], 200)                                   # two bursts, one window (0, 160)
WIN_A, WIN_C = [(10, 110), (210, 330), (430, 470)], [(0, 160)]


def test_vad_route_ids_offsets_and_new_outputs():
    cfg = _cfg()
    eng = _VadEng(cfg)
    m = _model(cfg, eng, 8)
    out = m.generate_from_wav([A, SILENT, C6], vad_longform=True, vad_options=OPTS, language="en", return_dict_in_generate=True)
    vcalls = [c for c in eng.calls if c[0] == "vad_windows"]
    assert len(vcalls) == 1 and vcalls[0][1] == (3, len(A)) and vcalls[0][2] == [len(A), len(SILENT), len(C6)]       # one call for all recordings
    assert vcalls[0][3]["pad"] == 0 and vcalls[0][3]["F"] == 192 and vcalls[0][3]["min_silence"] == 50
    assert [c[1] for c in eng.calls if c[0] == "logmel"] == [5]                  # 3 + 1 placeholder + 1 rows
    assert [c[:2] for c in eng.calls if c[0] in ("encode", "decode")] == [("encode", 4), ("decode", 4)]      # the silent recording is not decoded
    eos = cfg.eos_token_id
    rows = [_prompt(cfg, EN) + SCRIPT[1] + SCRIPT[2] + SCRIPT[9] + [eos], _prompt(cfg, EN) + [eos], _prompt(cfg, EN) + SCRIPT[6] + [eos]]
    assert torch.equal(out["sequences"], _padded(rows, cfg.pad_token_id, torch.long))
    assert out["vad_windows"].tolist() == [[list(w) for w in WIN_A], [[-1, -1]] * 3, [list(WIN_C[0]), [-1, -1], [-1, -1]]]
    assert out["speech_regions"] == [[(a * 0.01, b * 0.01) for a, b in WIN_A], [], [(0.0, 0.5), (1.2, 1.6)]]
    assert m.last_stats["ms_vad"] == 0.25 and m.last_stats["longform_windows"] == [3, 0, 1]
    # the plain tensor without the dict form: the same rows
    t = m.generate_from_wav([A, SILENT, C6], vad_longform=True, vad_options=OPTS, language="en")
    assert isinstance(t, torch.Tensor) and torch.equal(t, out["sequences"])
    # all recordings silent: one placeholder row is decoded for the prompt, every recording returns prompt + EOS
    eng.calls.clear()
    t = m.generate_from_wav([SILENT, SILENT[:5000]], vad_longform=True, language="en", return_dict_in_generate=True)
    assert [c[:2] for c in eng.calls if c[0] == "decode"] == [("decode", 1)]
    assert t["sequences"].tolist() == [_prompt(cfg, EN) + [eos]] * 2 and t["vad_windows"].shape == (2, 0, 2) and t["speech_regions"] == [[], []]


def test_vad_route_cuts_in_the_sample_domain_and_zero_pads():
    cfg = _cfg()
    eng = _VadEng(cfg)
    m = _model(cfg, eng, 2)
    x = _audio([(2, 5, 60)], 61, tail=100)
    x[60 * 160:] = 7.0                                                            # a ragged last frame of speech: T = 61, n = 61 * 160 - 100
    win, plan = m._vad_wav_windows([A, x], 16000, OPTS)
    assert plan["windows"] == [WIN_A, [(5, 61)]] and plan["first"] == [0, 3, 4]
    assert [c[1] for c in eng.calls if c[0] == "logmel"] == [2, 2]               # groups of at most max_batch windows
    assert win[:, 0, 0].tolist() == [1.0, 2.0, 9.0, 2.0]
    seen = []
    eng.logmel = lambda buf: seen.append(buf.clone()) or _StrideEng.logmel(eng, buf)
    m._vad_wav_windows([x], 16000, OPTS)
    row = seen[0][0]
    n = len(x) - 5 * 160
    assert torch.equal(row[:n], torch.from_numpy(x[5 * 160:])) and torch.all(row[n:] == 0)          # [160 u, min(160 v, n)), then zeros
    # the front door: a stereo recording at 32 kHz is downmixed and resampled first
    eng.calls.clear()
    st = np.stack([np.repeat(A, 2), np.repeat(A, 2)])
    _, plan2 = m._vad_wav_windows([st], 32000, OPTS)
    assert eng.calls[0][0] == "resample" and plan2["windows"] == [WIN_A]


def test_vad_route_token_timestamps_and_logprobs_carry_the_window_offsets():
    cfg = _cfg()
    eng = _VadEng(cfg, no_speech={2: 0.95})
    m = _model(cfg, eng, 8)
    out = m.generate_from_wav([A, C6], vad_longform=True, vad_options=OPTS, language="en", return_token_timestamps=True, return_token_logprobs=True,
                              no_speech_threshold=0.6)
    P = len(_prompt(cfg, EN))
    eos = cfg.eos_token_id

    def at(code, u, q):      # the window's own value at text position q, offset by the window's start in float32
        return float(torch.tensor(_ts(code, P + q), dtype=torch.float32) + torch.tensor(u * 0.01, dtype=torch.float32))

    # recording 0: its middle window (code 2) is gated and contributes nothing; the others keep their own offsets
    rows = [_prompt(cfg, EN) + SCRIPT[1] + SCRIPT[9] + [eos], _prompt(cfg, EN) + SCRIPT[6] + [eos]]
    assert torch.equal(out["sequences"], _padded(rows, cfg.pad_token_id, torch.long))
    tt = [[0.0] * P + [at(1, 10, q) for q in range(len(SCRIPT[1]))] + [at(9, 430, q) for q in range(len(SCRIPT[9]))],
          [0.0] * P + [at(6, 0, q) for q in range(len(SCRIPT[6]))]]
    assert torch.equal(out["token_timestamps"], _padded([r + [r[-1]] for r in tt], None, torch.float32))
    lp = [[0.0] * P + [_lp(1, P + q) for q in range(len(SCRIPT[1]))] + [_lp(9, P + q) for q in range(len(SCRIPT[9]))] + [_lp(9, P + len(SCRIPT[9]))],
          [0.0] * P + [_lp(6, P + q) for q in range(len(SCRIPT[6]))] + [_lp(6, P + len(SCRIPT[6]))]]
    assert torch.equal(out["token_logprobs"], _padded(lp, 0.0, torch.float32))
    assert out["skipped"].tolist() == [[False, True, False], [False, False, False]]
    assert out["no_speech_prob"][0].tolist() == pytest.approx([0.1, 0.95, 0.1])
    assert torch.isnan(out["no_speech_prob"][1]).tolist() == [False, True, True]
    assert out["window_avg_logprob"].shape == (2, 3) and torch.isnan(out["window_avg_logprob"][1]).tolist() == [False, True, True]
    assert out["lengths"].tolist() == [len(r) for r in rows]
    assert m.last_stats["ms_token_timestamps"] == 2.0 and m.last_stats["ms_vad"] == 0.25


def test_vad_route_segments_are_offset_by_the_window_start():
    cfg = _cfg()

    class TsEng(_VadEng):
        def decode(self, gp, B, **kw):
            return _Eng.decode(self, gp, B)

    eng = TsEng(cfg)
    m = _model(cfg, eng, 8)
    out = m.generate_from_wav([A], vad_longform=True, vad_options=OPTS, language="en", return_timestamps=True, return_segments=True)
    segs = out["segments"][0]
    assert len(segs) == 6                                                        # _Eng's row: two segments per window, (0.0, 0.2) and (0.2, 0.3)
    for j, (u, _) in enumerate(WIN_A):
        for k, (a, b) in enumerate(((0.0, 0.2), (0.2, 0.3))):
            sg = segs[2 * j + k]
            assert float(sg["start"]) == pytest.approx(u * 0.01 + a, abs=1e-6) and float(sg["end"]) == pytest.approx(u * 0.01 + b, abs=1e-6)
    assert out["vad_windows"].tolist() == [[list(w) for w in WIN_A]]


def test_vad_route_language_groups_and_detection():
    cfg = _cfg()
    eng = _VadEng(cfg, lang_ids={1: 20, 6: 21, 0: 20})
    m = _model(cfg, eng, 8)
    eos = cfg.eos_token_id
    out = m.generate_from_wav([A, C6, SILENT], vad_longform=True, vad_options=OPTS, language=["de", "en", "de"])
    rows = [_prompt(cfg, DE) + SCRIPT[1] + SCRIPT[2] + SCRIPT[9] + [eos], _prompt(cfg, EN) + SCRIPT[6] + [eos], _prompt(cfg, DE) + [eos]]
    assert torch.equal(out, _padded(rows, cfg.pad_token_id, torch.long))
    assert [c[1:] for c in eng.calls if c[0] == "decode"] == [(3, tuple(_prompt(cfg, DE))), (1, tuple(_prompt(cfg, EN)))]
    assert len([c for c in eng.calls if c[0] == "vad_windows"]) == 1
    # detection: once per recording, on its first row (the silent one on its placeholder)
    eng.calls.clear()
    out = m.generate_from_wav([A, C6, SILENT], vad_longform=True, vad_options=OPTS)
    assert [c for c in eng.calls if c[0] == "encode"][0] == ("encode", 3)
    rows = [_prompt(cfg, EN) + rows[0][4:], _prompt(cfg, DE) + rows[1][4:], _prompt(cfg, EN) + [eos]]
    assert torch.equal(out, _padded(rows, cfg.pad_token_id, torch.long))
    with pytest.raises(ValueError):
        m.generate_from_wav([A, C6], vad_longform=True, language=["de", "en", "en"])


def test_detect_speech_is_the_restatement_in_seconds():
    cfg = _cfg()
    m = _model(cfg, _VadEng(cfg), 8)
    got = m.detect_speech([A, SILENT], speech_pad_ms=20, max_window_s=1.0)
    from whisper_medusa import vad
    for x, g in zip((A, SILENT), got):
        r = V.vad_windows_ref(x, len(x), vad.lower_options(dict(speech_pad_ms=20, max_window_s=1.0), 192))
        assert g == dict(regions=[(a * 0.01, b * 0.01) for a, b in r["regions"]], windows=[(a * 0.01, b * 0.01) for a, b in r["windows"]])
    assert got[0]["regions"][0] == (0.08, 1.12) and len(got[0]["windows"]) > 3 and got[1] == dict(regions=[], windows=[])
    with pytest.raises(ValueError, match="unknown key"):
        m.detect_speech(A, pad_ms=3)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_vad_longform_refusals():
    cfg = _cfg()
    m = _model(cfg, _VadEng(cfg), 8)
    ok = dict(vad_longform=True, language="en")
    for other in (dict(chunk_longform=True), dict(sequential_longform=True, return_timestamps=True), dict(stride_length_s=0.32),
                  dict(chunk_longform=True, stride_length_s=0.32)):
        with pytest.raises(ValueError, match="alternatives"):
            m.generate_from_wav(A, **ok, **other)
    f = torch.zeros(1, cfg.num_mel_bins, 192)
    with pytest.raises(ValueError, match="needs the waveform"):
        m.generate(f, **ok)
    with pytest.raises(ValueError, match="needs the waveform"):
        m.generate(torch.zeros(1, cfg.num_mel_bins, 500), **ok)
    for kw in (dict(language="en"), dict(language="en", vad_longform=False), dict(language="en", chunk_longform=True)):
        with pytest.raises(ValueError, match="only valid together with vad_longform"):
            m.generate_from_wav(A, vad_options=OPTS, **kw)
        with pytest.raises(ValueError, match="only valid together with vad_longform"):
            m.generate(f, vad_options=OPTS, **kw)
    with pytest.raises(ValueError, match="unknown key"):
        m.generate_from_wav(A, vad_options=dict(threshold=0.5), **ok)
    with pytest.raises(ValueError, match="has to be a dict"):
        m.generate_from_wav(A, vad_options=0.5, **ok)
    for kw, word in ((dict(vanilla=True, num_beams=2), "beam search"), (dict(sampling_seed=1, temperature=0.5), "sampling"), (dict(do_sample=True), "sampling"),
                     (dict(top_logprobs=2), "top_logprobs"), (dict(vanilla=True, sequence_bias={(5,): 1.0}), "sequence_bias"),
                     (dict(vanilla=True, bad_words_ids=[[5]]), "bad_words_ids"), (dict(vanilla=True, allowed_sequences=[[5, 6]]), "allowed_sequences"),
                     (dict(return_token_timestamps=True, num_frames=[100]), "num_frames"), (dict(streamer=object()), "streamer")):
        with pytest.raises(NotImplementedError, match=word + r".*vad_longform"):
            m.generate_from_wav(A, **ok, **kw)
    # the other routes are what they were: no VAD call without the keyword
    eng = _VadEng(cfg)
    m = _model(cfg, eng, 8)
    m.generate_from_wav(A[:20000] + 9.0, language="en")
    assert [c[0] for c in eng.calls] == ["logmel", "encode", "decode"]
