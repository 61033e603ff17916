"""Cost of the scoring pass of generate(return_token_logprobs=True) next to the decode it follows.

    python tests/microbench/token_logprobs_time.py [--streams 1 32] [--new-tokens 128]
    rocprofv3 --kernel-trace --stats -d OUT -- python tests/microbench/token_logprobs_time.py --streams 1 --reps 1 --extra 4
    python tests/prof_summary.py OUT/.../*.db

large-v2 shape, K = 10, synthetic weights (the bench shape).  Prints one JSON line per stream count: ms_decode and ms_token_logprobs (hipEvent
times of the engine, best of --reps).  `--extra N` repeats the scoring call alone N times on the ids of the last decode: in a kernel trace of
such a run the scoring stage (k_score1, k_score2, k_score_build) is told apart by name, the vocabulary projection as the `k_skinny_gemm<..., EpF32T<false>, false>` launches beyond the decode's own;
the replay is the rest of ms_token_logprobs."""
import argparse
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--extra", type=int, default=0)
    a = ap.parse_args()
    cfg = MedusaConfig.large_v2(K=10)
    sd = synth.synth_state_dict(cfg, seed=0)
    dev = torch.device("cuda", 0)
    model = WhisperMedusaModel(cfg, sd, device=dev, max_batch=max(a.streams))
    for B in a.streams:
        feats = torch.cat([model.extract_features(synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160)) for i in range(B)], dim=0)
        rows = []
        for _ in range(a.reps):
            out = model.generate(feats, max_new_tokens=a.new_tokens, language="en", return_token_logprobs=True, suppress_tokens=[cfg.eos_token_id])
            st = model.last_stats
            rows.append((st["ms_decode"], st["ms_token_logprobs"]))
        dec, sc = min(r[0] for r in rows), min(r[1] for r in rows)
        P = len(model._last_prompt)
        seqs = [r[: int(n)] for r, n in zip(out["sequences"].tolist(), out["lengths"].tolist())]
        gp = model._gen_params("en", None, None, a.new_tokens, None, None, False, None, None, [cfg.eos_token_id], None, None)
        alone = [model.engine.score_tokens(seqs, P, gp, cfg.no_speech_token_id)[2] for _ in range(a.extra)]
        print(json.dumps(dict(streams=B, new_tokens=int(out["sequences"].shape[1]) - P, ms_decode=round(dec, 3), ms_token_logprobs=round(sc, 3),
                              ratio=round(sc / dec, 3), ms_token_logprobs_alone=[round(v, 3) for v in alone])), flush=True)
    model.engine.close()


if __name__ == "__main__":
    main()
