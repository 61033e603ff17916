"""Cost of the token alternatives next to the scoring pass they ride on (generate(top_logprobs=k)).

    python tests/microbench/topk_time.py [--streams 1] [--new-tokens 128] [--top-logprobs 8] [--reps 3]

large-v2 shape, K = 10, synthetic weights: the call of tests/microbench/token_logprobs_time.py, once with return_token_logprobs=True and once
with top_logprobs=k on the same clips.  Prints one JSON line per stream count: ms_token_logprobs of both calls (hipEvent time of the engine:
replay + vocabulary projection + scoring, with k also the two top-k kernels and their copies; best of --reps) and ms_decode."""
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
    ap.add_argument("--streams", type=int, nargs="+", default=[1])
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--top-logprobs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    cfg = MedusaConfig.large_v2(K=10)
    sd = synth.synth_state_dict(cfg, seed=0)
    model = WhisperMedusaModel(cfg, sd, device=torch.device("cuda", 0), max_batch=max(a.streams))
    for B in a.streams:
        feats = torch.cat([model.extract_features(synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160)) for i in range(B)], dim=0)
        kw = dict(max_new_tokens=a.new_tokens, language="en", suppress_tokens=[cfg.eos_token_id])
        plain, top, dec = [], [], []
        for _ in range(a.reps):
            out = model.generate(feats, return_token_logprobs=True, **kw)
            plain.append(model.last_stats["ms_token_logprobs"]); dec.append(model.last_stats["ms_decode"])
            alt = model.generate(feats, top_logprobs=a.top_logprobs, **kw)
            top.append(model.last_stats["ms_token_logprobs"])
            assert torch.equal(alt["sequences"], out["sequences"]) and torch.equal(alt["token_logprobs"], out["token_logprobs"])
        P = len(model._last_prompt)
        print(json.dumps(dict(streams=B, new_tokens=int(out["sequences"].shape[1]) - P, top_logprobs=a.top_logprobs, ms_decode=round(min(dec), 3),
                              ms_token_logprobs=round(min(plain), 3), ms_token_logprobs_topk=round(min(top), 3),
                              all_ms_token_logprobs=[round(v, 3) for v in plain], all_ms_token_logprobs_topk=[round(v, 3) for v in top])), flush=True)
    model.engine.close()


if __name__ == "__main__":
    main()
