"""Cost of generate(return_token_timestamps=True) next to the decode it follows.

    python tests/microbench/token_timestamps_time.py [--streams 1 32] [--new-tokens 128] [--heads 23]
    rocprofv3 --kernel-trace --stats -d OUT -- python tests/microbench/token_timestamps_time.py --streams 1 --reps 1 --extra 4
    python tests/prof_summary.py OUT/.../*.db

large-v2 shape, synthetic weights, `--heads` alignment heads over the upper decoder layers.  Prints one JSON line per stream count:
ms_decode and ms_token_timestamps (hipEvent times of the engine).  `--extra N` repeats the timestamp call alone N times on the ids of the
last decode (`ms_token_timestamps_alone`): in a kernel trace of such a run, k_align_probs, k_align_stats + k_align_norm and k_dtw are told
apart by name (their time / (reps + N) is one call's share); the replay is the rest of ms_token_timestamps."""
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
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--heads", type=int, default=23)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--extra", type=int, default=0)
    a = ap.parse_args()
    cfg = MedusaConfig.large_v2(K=10)
    cfg = dataclasses.replace(cfg, alignment_heads=synth.synth_alignment_heads(cfg, a.heads))
    sd = synth.synth_state_dict(cfg, seed=0)
    dev = torch.device("cuda", 0)
    model = WhisperMedusaModel(cfg, sd, device=dev, max_batch=max(a.streams))
    for B in a.streams:
        feats = torch.cat([model.extract_features(synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160)) for i in range(B)], dim=0)
        rows = []
        for _ in range(a.reps):
            out = model.generate(feats, max_new_tokens=a.new_tokens, language="en", return_token_timestamps=True,
                                 suppress_tokens=[cfg.eos_token_id])
            st = model.last_stats
            rows.append((st["ms_decode"], st["ms_token_timestamps"]))
        dec, tt = min(r[0] for r in rows), min(r[1] for r in rows)
        alone = []
        P, eos = len(model._last_prompt), cfg.eos_token_id
        seqs = [r[: r.index(eos, P) + 1] if eos in r[P:] else r for r in out["sequences"].tolist()]
        for _ in range(a.extra):
            alone.append(model.engine.token_timestamps(seqs, P, cfg.alignment_heads, cfg.median_filter_width)[1])
        print(json.dumps(dict(ms_token_timestamps_alone=[round(v, 3) for v in alone], streams=B, new_tokens=int(out["sequences"].shape[1]) - len(model._last_prompt), alignment_heads=a.heads,
                              ms_decode=round(dec, 3), ms_token_timestamps=round(tt, 3), ratio=round(tt / dec, 3))), flush=True)
    model.engine.close()


if __name__ == "__main__":
    main()
