"""Time of stitching overlapping long-form windows: wm_merge_windows (one kernel launch for all boundaries of all recordings) against
transformers' _find_longest_common_sequence on the same token lists, on the same machine.

    python tests/microbench/merge_time.py [--reps 20] [--hf-reps 3] [--bench-call] [--out FILE.md]

The lists are cut from one random id stream per recording the way 30 s windows with 5 s strides each side cut a transcript: a window holds n ids,
the next one starts 2/3 n further on, so neighbours share a third (10 s of 30 s).  Shapes: 1 recording x 120 windows x 100 ids (one hour), 32
recordings x 120 windows x 100 ids, 1 x 120 x 448 ids; each without and with times (one ascending float32 per id, the same on both sides of an
overlap).  Engine: the call's own hipEvent time (upload + kernel + download), median and minimum of --reps calls after two warm-up calls, and the
host clock around Engine.merge_windows (which adds the packing of the Python lists).  transformers: the host clock around the function, recording by
recording, best of --hf-reps (1 rep where one takes over 5 s).  The merged ids of the two are compared.  --bench-call: one strided generate() on the
bench checkpoint (large-v2 shape, K = 10, synthetic weights) over a 10 min recording — 30 windows of one batch — and its ms_merge share."""
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

from whisper_medusa import WhisperMedusaModel, MedusaConfig, synth, weights  # noqa: E402
import merge_ref as M  # noqa: E402


def recordings(n_rec, n_win, n_tok, seed):
    rng = np.random.default_rng(seed)
    step = (2 * n_tok) // 3
    wins, times = [], []
    for _ in range(n_rec):
        stream = rng.integers(0, 50000, step * (n_win - 1) + n_tok)
        wins.append([[int(t) for t in stream[j * step: j * step + n_tok]] for j in range(n_win)])
        times.append([[float(np.float32((j * step + q) * 30.0 / n_tok)) for q in range(n_tok)] for j in range(n_win)])
    return wins, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hf-reps", type=int, default=3)
    ap.add_argument("--bench-call", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = MedusaConfig.micro()
    eng = WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=1), device=dev).engine
    rows = []
    for n_rec, n_win, n_tok in ((1, 120, 100), (32, 120, 100), (1, 120, 448)):
        wins, times = recordings(n_rec, n_win, n_tok, 11 * n_rec + n_tok)
        for timed in (False, True):
            ts = times if timed else None
            ev, wall = [], []
            for rep in range(a.reps + 2):
                t0 = time.perf_counter()
                keep = eng.merge_windows(wins, ts)
                wall.append(1e3 * (time.perf_counter() - t0))
                ev.append(eng.last_merge_ms)
            ev, wall = ev[2:], wall[2:]
            hf, merged = [], None
            for rep in range(a.hf_reps):
                t0 = time.perf_counter()
                merged = [M.hf_merge(wins[c], None if ts is None else ts[c]) for c in range(n_rec)]
                hf.append(1e3 * (time.perf_counter() - t0))
                if hf[-1] > 5000:
                    break
            same = all(M.assemble(wins[c], keep[c]) == (merged[c][0] if timed else merged[c]) for c in range(n_rec))
            cut = sum(1 for c in range(n_rec) for k, w in zip(keep[c], wins[c]) if k != (0, len(w)))
            row = dict(recordings=n_rec, windows=n_win, ids=n_tok, times=timed, engine_event_ms_median=round(statistics.median(ev), 3),
                       engine_event_ms_min=round(min(ev), 3), engine_wall_ms_median=round(statistics.median(wall), 2), hf_wall_ms_best=round(min(hf), 1),
                       hf_reps=len(hf), hf_over_engine_event=round(min(hf) / statistics.median(ev), 1),
                       hf_over_engine_wall=round(min(hf) / statistics.median(wall), 1), ids_equal=same, windows_cut=cut)
            rows.append(row)
            print(json.dumps(row), flush=True)
    lines = ["| recordings x windows x ids | times | wm_merge_windows, hipEvent ms (median / min) | Engine.merge_windows, host clock ms (median) | "
             "transformers, host clock ms (best of n) | transformers / event | transformers / host clock | merged ids equal |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['recordings']} x {r['windows']} x {r['ids']} | {'yes' if r['times'] else 'no'} | {r['engine_event_ms_median']} / {r['engine_event_ms_min']} | "
                     f"{r['engine_wall_ms_median']} | {r['hf_wall_ms_best']} (n = {r['hf_reps']}) | {r['hf_over_engine_event']} | {r['hf_over_engine_wall']} | {r['ids_equal']} |")
    eng.close()
    if a.bench_call:
        big = MedusaConfig.large_v2(K=10)
        from whisper_medusa.engine import default_act_fp16
        f16 = default_act_fp16()
        sd = synth.synth_state_dict(big, seed=0, device=str(dev), logit_std=4.5)
        blob, offs = weights.build_blob(big, sd, device=dev, act_fp16=f16)
        del sd
        model = WhisperMedusaModel.from_blob(big, blob, offs, max_batch=32, act_fp16=f16)
        F = big.n_mel_frames
        wav = torch.from_numpy(synth.synth_clip(0, 600 * 16000))[None].to(dev)
        feats = model.engine.logmel_long(wav)                       # [1, 80, 60000]: 10 min
        kw = dict(chunk_longform=True, max_new_tokens=100, suppress_tokens=sorted(set(list(big.suppress_tokens or []) + [big.eos_token_id])))
        res = {}
        for arm, extra in (("strided", dict(stride_length_s=5.0)), ("plain", {})) * 3:          # (the first pair warms both up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate(feats, **kw, **extra)
            torch.cuda.synchronize()
            res.setdefault(arm, []).append((1e3 * (time.perf_counter() - t0), dict(model.last_stats)))
        s_ms, s_st = min(res["strided"][1:], key=lambda v: v[0])
        p_ms, p_st = min(res["plain"][1:], key=lambda v: v[0])
        n_s, n_p = s_st["longform_windows"][0], -(-feats.shape[-1] // F)
        call = dict(frames=int(feats.shape[-1]), strided_windows=n_s, plain_windows=n_p, strided_call_ms=round(s_ms, 1), plain_call_ms=round(p_ms, 1),
                    ms_merge=round(s_st["ms_merge"], 3), merge_share=round(s_st["ms_merge"] / s_ms, 5), windows_per_hour_strided=3600 / 20, windows_per_hour_plain=3600 / 30)
        print(json.dumps(call), flush=True)
        lines += ["", f"Strided call on the bench checkpoint, {call['frames']} frames, 100 new ids per window: {n_s} windows, {call['strided_call_ms']} ms per call, "
                      f"ms_merge {call['ms_merge']} ({100 * call['merge_share']:.3f} % of the call); without strides {n_p} windows, {call['plain_call_ms']} ms."]
        model.engine.close()
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
