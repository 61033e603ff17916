"""Cost of constrained decoding on the plain decode path (wm_set_constraint): ms per plain decode step with no table and with tables
of N sequences.

    python tests/microbench/constraint_time.py [--streams 1 32] [--sequences 1 1024 16384] [--new-tokens 32] [--reps 3] [--out FILE.md]

large-v2 shape, K = 10, synthetic weights (seed 0), the default decode contract.  Per stream count and table size the plain greedy decode
(`vanilla`: one base-head row per stream and step) and the same decode under a table of that many sequences (one k_constraint launch per step behind
the base pass) are run alternately, --reps times each after one warm-up pair, on one context and one encoder pass.  Every sequence is
WM_CONSTRAINT_MAX_LEN = 32 ids long over a four-id alphabet and EOS is suppressed, so that every run makes --new-tokens <= 32 steps and no stream
reaches a leaf: the ranges the kernel marks start at N / 4 sequences and shrink by four per step.  Prints one JSON line per case — ms per step of
both (the engine's hipEvent time of wm_decode_run / steps; the best and all) and the added microseconds — and the table (also written to --out)."""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "whisper-medusa_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from whisper_medusa import WhisperMedusaModel, MedusaConfig, synth  # noqa: E402
from whisper_medusa.engine import CONSTRAINT_MAX_LEN  # noqa: E402


def table(n, avoid, seed=1):
    rng = np.random.default_rng(seed)
    alpha = [t for t in (1000, 2000, 3000, 4000, 5000, 6000) if t not in avoid][:4]
    seen = {}
    while len(seen) < n:
        seen.setdefault(tuple(alpha[i] for i in rng.integers(0, 4, CONSTRAINT_MAX_LEN)))
    return list(seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--sequences", type=int, nargs="+", default=[1, 1024, 16384])
    ap.add_argument("--new-tokens", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.new_tokens <= CONSTRAINT_MAX_LEN
    cfg = MedusaConfig.large_v2(K=10)
    sd = synth.synth_state_dict(cfg, seed=0)
    model = WhisperMedusaModel(cfg, sd, device=torch.device("cuda", 0), max_batch=max(a.streams))
    eng = model.engine
    rows = []
    for B in a.streams:
        feats = torch.cat([model.extract_features(synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160)) for i in range(B)], dim=0)
        gp = model._gen_params("en", None, None, a.new_tokens, None, 0.0, True, None, None, [cfg.eos_token_id], [], None)
        eng.encode(feats)
        for n in a.sequences:
            seqs = table(n, {cfg.eos_token_id})
            on = dataclasses.replace(gp, allowed_sequences=seqs)
            ms = {"off": [], "on": []}
            steps, ids = {}, {}
            for _ in range(a.reps + 1):                 # (the first pair warms both graphs up and is dropped)
                for name, g in (("off", gp), ("on", on)):
                    ids[name] = eng.decode(g, B)
                    st = eng.stats()
                    steps[name] = int(st["iterations_launched"])
                    ms[name].append(st["ms_decode"] / max(steps[name], 1))
            P = len(gp.prompt)
            assert all(tuple(s[P:]) in {q[: len(s) - P] for q in seqs} for s in ids["on"]), "a constrained stream left the table"
            ms = {k: v[1:] for k, v in ms.items()}
            row = dict(streams=B, sequences=n, steps=steps, ms_per_step_off=round(min(ms["off"]), 4), ms_per_step_on=round(min(ms["on"]), 4),
                       delta_us=round(1000 * (min(ms["on"]) - min(ms["off"])), 2), all_off=[round(v, 4) for v in ms["off"]],
                       all_on=[round(v, 4) for v in ms["on"]])
            rows.append(row)
            print(json.dumps(row), flush=True)
    lines = ["| streams | sequences N | no table (ms / step) | table (ms / step) | added (us / step) |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['streams']} | {r['sequences']} | {r['ms_per_step_off']} ({', '.join(str(v) for v in r['all_off'])}) | "
                     f"{r['ms_per_step_on']} ({', '.join(str(v) for v in r['all_on'])}) | {r['delta_us']} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
