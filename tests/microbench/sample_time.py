"""Cost of seeded sampling on the plain decode path (wm_set_sampling): ms per plain decode step with sampling off and on.

    python tests/microbench/sample_time.py [--streams 1 32] [--new-tokens 64] [--reps 5] [--temperature 0.4]

large-v2 shape, K = 10, synthetic weights (seed 0), the default decode contract.  Per stream count the plain decode (`vanilla`: one base-head row
per stream and step, select = k_select1 + k_select_argmax) and the same decode with sampling on (k_sample1 + k_sample_fin in their place) are run
alternately, --reps times each, on one context and one encoder pass; EOS is suppressed so that every run makes --new-tokens steps.  Prints one
JSON line per stream count: ms per step of both (the engine's hipEvent time of wm_decode_run / steps; best and all)."""
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
        on = dataclasses.replace(gp, sampling_temperature=a.temperature, sampling_seed=1, sampling_keys=list(range(B)))
        eng.encode(feats)
        ms = {"off": [], "on": []}
        steps = {}
        for _ in range(a.reps + 1):             # (the first pair warms both graphs up and is dropped)
            for name, g in (("off", gp), ("on", on)):
                seqs = eng.decode(g, B)
                st = eng.stats()
                steps[name] = int(st["iterations"])
                ms[name].append(st["ms_decode"] / max(steps[name], 1))
        ms = {k: v[1:] for k, v in ms.items()}
        print(json.dumps(dict(streams=B, steps=steps, ms_per_step_off=round(min(ms["off"]), 4), ms_per_step_on=round(min(ms["on"]), 4),
                              all_off=[round(v, 4) for v in ms["off"]], all_on=[round(v, 4) for v in ms["on"]])), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
