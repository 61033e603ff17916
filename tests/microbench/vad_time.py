"""Time of finding the speech windows of long recordings: wm_vad_windows (a fixed chain of kernel launches for all recordings) against
the vectorised numpy parts of the restated contract (tests/vad_ref.py vad_numpy_parts: energy, loud level, thresholds, the two comparisons) on the
same audio, on the same machine.

    python tests/microbench/vad_time.py [--reps 10] [--np-reps 2] [--bench-call] [--only-bench-call] [--out FILE.md]

The audio is synthetic: bursts of noise of 0.3 .. 6 s separated by quiet gaps of 0.1 .. 2 s (about 600 regions per hour), and one burst of 90 s per
ten minutes that has to be split.  Shapes: 1 recording x 1 h, 32 x 1 h (32 x 10 min where the memory does not allow it), 1 x 30 s.  Engine: the
call's own hipEvent time (upload of the plan, kernels, download), median and minimum of --reps calls after two warm-up calls, and the host clock
around Engine.vad_windows (which adds the Python lists).  numpy: the host clock around vad_numpy_parts, recording by recording, best of --np-reps;
the serial Python loops of the restatement (hysteresis, regions) are not in that time, the full restatement is timed once for the single hour.  The
windows of the two are compared on the first recording.  --bench-call: on the bench checkpoint (large-v2 shape, K = 10, synthetic weights) a
10 min recording with pauses through vad_longform, chunk_longform, chunk_longform + stride_length_s=5 and sequential_longform, each from the
waveform (the log-mel inside the time; chunk_longform alone has no waveform door of its own: extract_features(truncation=False), then generate)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "whisper-medusa_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from whisper_medusa import WhisperMedusaModel, MedusaConfig, synth, weights, vad  # noqa: E402
import vad_ref as V  # noqa: E402


def recording(seconds, seed):
    """Noise bursts and quiet gaps, float32 [seconds * 16000]."""
    rng = np.random.default_rng(seed)
    n = int(seconds * 16000)
    x = (1e-4 * rng.standard_normal(n)).astype(np.float32)
    t, k = 0, 0
    while t < n:
        dur = 90.0 if k % 100 == 50 else float(rng.uniform(0.3, 6.0))
        m = min(n - t, int(dur * 16000))
        x[t: t + m] = (0.1 * rng.standard_normal(m)).astype(np.float32)
        t += m + int(float(rng.uniform(0.1, 2.0)) * 16000)
        k += 1
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--np-reps", type=int, default=2)
    ap.add_argument("--bench-call", action="store_true")
    ap.add_argument("--only-bench-call", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = MedusaConfig.micro()
    eng = WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=1), device=dev).engine
    P = vad.lower_options(None, 3000)
    hour = recording(3600, 1)
    rows = []
    for n_rec, seconds in () if a.only_bench_call else ((1, 3600), (32, 3600), (1, 30)):
        base = hour[: seconds * 16000]
        try:
            x = torch.from_numpy(base).to(dev)[None].repeat(n_rec, 1)
            if n_rec > 1:                                   # recordings that differ: each one rolled by its index in seconds
                for c in range(1, n_rec):
                    x[c] = torch.roll(x[0], 16000 * c)
        except RuntimeError:
            seconds = 600
            base = hour[: seconds * 16000]
            x = torch.stack([torch.roll(torch.from_numpy(base).to(dev), 16000 * c) for c in range(n_rec)])
        ns = [x.shape[1]] * n_rec
        ev, wall = [], []
        for rep in range(a.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            regions, windows = eng.vad_windows(x, ns, P)
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(eng.last_vad_ms)
        ev, wall = ev[2:], wall[2:]
        host = x[: min(n_rec, 4)].cpu().numpy()             # numpy: at most four recordings, scaled to n_rec
        nps = []
        for rep in range(a.np_reps):
            t0 = time.perf_counter()
            for c in range(len(host)):
                V.vad_numpy_parts(host[c], ns[c], P)
            nps.append(1e3 * (time.perf_counter() - t0) * n_rec / len(host))
        full = None
        if n_rec == 1:
            t0 = time.perf_counter()
            ref = V.vad_windows_ref(host[0], ns[0], P)
            full = 1e3 * (time.perf_counter() - t0)
            same = ref["regions"] == regions[0] and ref["windows"] == windows[0]
        else:
            same = None
        row = dict(recordings=n_rec, seconds=seconds, frames=-(-ns[0] // 160), regions=len(regions[0]), windows=len(windows[0]),
                   engine_event_ms_median=round(statistics.median(ev), 3), engine_event_ms_min=round(min(ev), 3),
                   engine_wall_ms_median=round(statistics.median(wall), 2), numpy_parts_ms_best=round(min(nps), 1),
                   numpy_over_event=round(min(nps) / statistics.median(ev), 1), restatement_ms=None if full is None else round(full, 1), equal=same)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x
    lines = ["| recordings x seconds | regions / windows of the first | wm_vad_windows, hipEvent ms (median / min) | Engine.vad_windows, host clock ms (median) | "
             "numpy parts, host clock ms (best) | numpy / event | whole restatement ms | equal |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['recordings']} x {r['seconds']} | {r['regions']} / {r['windows']} | {r['engine_event_ms_median']} / {r['engine_event_ms_min']} | "
                     f"{r['engine_wall_ms_median']} | {r['numpy_parts_ms_best']} | {r['numpy_over_event']} | {r['restatement_ms']} | {r['equal']} |")
    eng.close()
    if a.bench_call or a.only_bench_call:
        big = MedusaConfig.large_v2(K=10)
        from whisper_medusa.engine import default_act_fp16
        f16 = default_act_fp16()
        sd = synth.synth_state_dict(big, seed=0, device=str(dev), logit_std=4.5)
        blob, offs = weights.build_blob(big, sd, device=dev, act_fp16=f16)
        del sd
        model = WhisperMedusaModel.from_blob(big, blob, offs, max_batch=32, act_fp16=f16)
        wav = recording(600, 2)
        kw = dict(max_new_tokens=100, suppress_tokens=sorted(set(list(big.suppress_tokens or []) + [big.eos_token_id])))
        arms = (("vad_longform", dict(vad_longform=True)), ("chunk_longform", dict(chunk_longform=True)),
                ("chunk_longform + stride_length_s=5", dict(chunk_longform=True, stride_length_s=5.0)),
                ("sequential_longform", dict(sequential_longform=True, return_timestamps=True)))
        res = {}
        for rnd in range(3):                                # (the first round warms every arm up)
            for arm, extra in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if arm == "chunk_longform":
                    model.generate(model.extract_features(wav, truncation=False), **kw, **extra)
                else:
                    model.generate_from_wav(wav, **kw, **extra)
                torch.cuda.synchronize()
                res.setdefault(arm, []).append((1e3 * (time.perf_counter() - t0), dict(model.last_stats)))
        lines += ["", "| route (10 min recording with pauses, bench checkpoint, 100 new ids per window) | windows decoded | call ms (best of 2) | ms_vad | share |",
                  "|---|---|---|---|---|"]
        for arm, _ in arms:
            ms, st = min(res[arm][1:], key=lambda v: v[0])
            w = st.get("longform_windows")
            w = (w[0] if isinstance(w, (list, tuple)) else w) if w is not None else -(-60000 // big.n_mel_frames)
            mv = st.get("ms_vad")
            call = dict(route=arm, windows=w, call_ms=round(ms, 1), ms_vad=None if mv is None else round(mv, 3), share=None if mv is None else round(mv / ms, 5))
            print(json.dumps(call), flush=True)
            lines.append(f"| {arm} | {call['windows']} | {call['call_ms']} | {call['ms_vad']} | {call['share']} |")
        model.engine.close()
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
