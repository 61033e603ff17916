"""Cost of the sequence bias on the plain decode path (wm_set_sequence_bias): ms per plain decode step with the table off and on.

    python tests/microbench/seq_bias_time.py [--streams 1 32] [--entries 64 1024] [--beams 4] [--new-tokens 64] [--reps 5]

large-v2 shape, K = 10, synthetic weights (seed 0), the default decode contract.  Per stream count and table size the plain decode (`vanilla`: one
base-head row per stream and step) and the same decode with a table of that many entries (one k_seq_bias launch per step behind the base pass) are
run alternately, --reps times each, on one context and one encoder pass; EOS is suppressed so that every run makes --new-tokens steps.  With
--beams n the same pair is run as a beam decode of streams // n clips (k_seq_bias behind k_beam_lse).  The table: a third one-token entries, the
rest 2 .. 16 tokens long over random ids, every entry on a target of its own (as many groups as entries: the widest launch a table of that size
can ask for).  Prints one JSON line per case: ms per step of both (the engine's hipEvent time of wm_decode_run / steps; best and all)."""
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


def table(n, V, avoid, seed=1):
    rng = np.random.default_rng(seed)
    targets = [int(t) for t in rng.permutation(V) if int(t) not in avoid][:n]
    ents = []
    for k, t in enumerate(targets):
        m = 1 if k % 3 == 0 else int(rng.integers(2, 17))
        ents.append((tuple(int(x) for x in rng.integers(0, V, size=m - 1)) + (t,), float(np.float32(rng.standard_normal()))))
    return ents


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--entries", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    cfg = MedusaConfig.large_v2(K=10)
    sd = synth.synth_state_dict(cfg, seed=0)
    model = WhisperMedusaModel(cfg, sd, device=torch.device("cuda", 0), max_batch=max(a.streams + [a.beams]))
    eng = model.engine
    for B in a.streams:
        for nb in (1, a.beams):
            if nb > 1 and B < nb and B != 1:
                continue
            clips = 1 if B < nb else B // nb
            feats = torch.cat([model.extract_features(synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160)) for i in range(clips)], dim=0)
            gp = model._gen_params("en", None, None, a.new_tokens, None, 0.0, True, None, None, [cfg.eos_token_id], None, None)
            gp = dataclasses.replace(gp, num_beams=nb)
            eng.encode(feats)
            for n in a.entries:
                on = dataclasses.replace(gp, sequence_bias=table(n, cfg.vocab_size, {cfg.eos_token_id}))
                ms = {"off": [], "on": []}
                steps = {}
                for _ in range(a.reps + 1):             # (the first pair warms both graphs up and is dropped)
                    for name, g in (("off", gp), ("on", on)):
                        eng.decode(g, clips)
                        st = eng.stats()
                        steps[name] = int(st["iterations_launched"])
                        ms[name].append(st["ms_decode"] / max(steps[name], 1))
                ms = {k: v[1:] for k, v in ms.items()}
                print(json.dumps(dict(streams=clips * nb, beams=nb, entries=n, steps=steps, ms_per_step_off=round(min(ms["off"]), 4),
                                      ms_per_step_on=round(min(ms["on"]), 4), delta_us=round(1000 * (min(ms["on"]) - min(ms["off"])), 2),
                                      all_off=[round(v, 4) for v in ms["off"]], all_on=[round(v, 4) for v in ms["on"]])), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
