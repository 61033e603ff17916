"""Cost of the sampling filters on the plain decode path (wm_set_sampling_filter): ms per plain decode step with sampling off, on,
and on with top_k = 50, with top_p = 0.95 alone (the full-vocabulary case), and with all three filters.

    python tests/microbench/filter_time.py [--streams 1 32] [--new-tokens 64] [--reps 5] [--temperature 0.4]

large-v2 shape, K = 10, synthetic weights (seed 0), the default decode contract, as tests/microbench/sample_time.py.  Per stream count the arms
are run alternately, --reps times each, on one context and one encoder pass; EOS is suppressed so that every run makes --new-tokens steps.  Prints
one JSON line per stream count: ms per step of every arm (the engine's hipEvent time of wm_decode_run / steps; best and all) and the launches of
its select stage per step (plain: k_select1 + k_select_argmax; sampling: k_sample1 + k_sample_fin; a filter: k_sample1 + k_filter_prep +
k_filter_row)."""
import argparse
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "whisper-medusa_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from whisper_medusa import WhisperMedusaModel, MedusaConfig, synth  # noqa: E402

ARMS = (("off", None, 2), ("sample", (0, 1.0, 0.0), 2), ("top_k50", (50, 1.0, 0.0), 3), ("top_p0.95", (0, 0.95, 0.0), 3),
        ("all", (50, 0.95, 0.05), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--temperature", type=float, default=0.4)
    a = ap.parse_args()
    cfg = MedusaConfig.large_v2(K=10)
    sd = synth.synth_state_dict(cfg, seed=0)
    model = WhisperMedusaModel(cfg, sd, device=torch.device("cuda", 0), max_batch=max(a.streams))
    eng = model.engine
    for B in a.streams:
        feats = torch.cat([model.extract_features(synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160)) for i in range(B)], dim=0)
        gp = model._gen_params("en", None, None, a.new_tokens, None, 0.0, True, None, None, [cfg.eos_token_id], None, None)
        gps = {}
        for name, flt, _ in ARMS:
            gps[name] = gp if flt is None else dataclasses.replace(gp, sampling_temperature=a.temperature, sampling_seed=1, sampling_keys=list(range(B)),
                                                                   sampling_top_k=flt[0], sampling_top_p=flt[1], sampling_min_p=flt[2])
        eng.encode(feats)
        ms = {name: [] for name, _, _ in ARMS}
        steps = {}
        for _ in range(a.reps + 1):             # (the first round warms every arm's graphs up and is dropped)
            for name, _, _ in ARMS:
                eng.decode(gps[name], B)
                st = eng.stats()
                steps[name] = int(st["iterations"])
                ms[name].append(st["ms_decode"] / max(steps[name], 1))
        ms = {k: v[1:] for k, v in ms.items()}
        print(json.dumps(dict(streams=B, steps=steps, select_launches={name: n for name, _, n in ARMS},
                              ms_per_step={k: round(min(v), 4) for k, v in ms.items()},
                              all={k: [round(x, 4) for x in v] for k, v in ms.items()})), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
