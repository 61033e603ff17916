"""Wall time of generate(language=None) on a batch of several languages: the grouped path (detect on the host, one encoder pass and one decode
per language group) against group_by_language=False (detect on the device, one encoder pass and one decode batch).

    python tests/microbench/lang_batch_time.py [--clips 32] [--groups 1 2 4 8] [--new-tokens 64] [--reps 3] [--out FILE.md]

large-v2 shape, K = 10, synthetic weights (seed 0) as bench.py uses, the default decode contract, one context.  A random-init checkpoint detects
one language for every clip, so the MIX is imposed: both detection entries run as they are (their cost is paid) and their answer is then replaced by
the drawn languages — clip b gets language b mod G of the first G of lang_to_id.  EOS is suppressed so that every stream makes --new-tokens tokens.
Per group count the two arms are run alternately, --reps times each after one warm-up pair; the time is the host clock around generate(), which
ends in the device synchronise of the token read-back.  The ids of the two arms are compared.  Prints one JSON line per group count and, at the end,
the table (also written to --out)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "whisper-medusa_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from whisper_medusa import WhisperMedusaModel, MedusaConfig, synth, weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = MedusaConfig.large_v2(K=10)
    from whisper_medusa.engine import default_act_fp16
    f16 = default_act_fp16()
    sd = synth.synth_state_dict(cfg, seed=0, device=str(dev), logit_std=4.5)
    blob, offs = weights.build_blob(cfg, sd, device=dev, act_fp16=f16)
    del sd
    model = WhisperMedusaModel.from_blob(cfg, blob, offs, max_batch=a.clips, act_fp16=f16)
    eng = model.engine
    B = a.clips
    wav = torch.stack([torch.from_numpy(synth.synth_clip(i, cfg.n_mel_frames * 160)) for i in range(B)]).to(dev)
    feats = eng.logmel(wav)
    toks = sorted(cfg.lang_to_id, key=lambda k: cfg.lang_to_id[k])
    kw = dict(max_new_tokens=a.new_tokens, suppress_tokens=sorted(set(list(cfg.suppress_tokens or []) + [cfg.eos_token_id])))
    drawn = []
    host_detect, dev_detect = model.detect_language, eng.detect_language
    model.detect_language = lambda f: (host_detect(f), list(drawn[: f.shape[0]]))[1]                       # the real host path runs, the mix is imposed
    eng.detect_language = lambda ids, st: (dev_detect(ids, st), [cfg.lang_to_id[l] for l in drawn[: eng._B]])[1]     # ... and the real entry
    encodes, real_encode = [], eng.encode
    eng.encode = lambda f: (encodes.append(f.shape[0]), real_encode(f))[1]
    rows = []
    for G in a.groups:
        drawn[:] = [toks[b % G] for b in range(B)]
        t = {"grouped": [], "one_batch": []}
        ids, enc = {}, {}
        for rep in range(a.reps + 1):                   # (the first pair warms both paths up — graphs, workspaces — and is dropped)
            for arm, extra in (("grouped", {}), ("one_batch", {"group_by_language": False})):
                del encodes[:]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.generate(feats, **kw, **extra)
                torch.cuda.synchronize()
                t[arm].append(1e3 * (time.perf_counter() - t0))
                ids[arm], enc[arm] = out.tolist(), list(encodes)
                assert model.detected_languages == drawn
        t = {k: v[1:] for k, v in t.items()}
        row = dict(clips=B, groups=G, new_tokens=a.new_tokens, grouped_ms=round(min(t["grouped"]), 1), one_batch_ms=round(min(t["one_batch"]), 1),
                   ratio=round(min(t["grouped"]) / min(t["one_batch"]), 3), ids_equal=ids["grouped"] == ids["one_batch"],
                   encodes_grouped=enc["grouped"], encodes_one_batch=enc["one_batch"], detect_ms_device=round(eng.last_detect_ms, 2),
                   all_grouped=[round(v, 1) for v in t["grouped"]], all_one_batch=[round(v, 1) for v in t["one_batch"]])
        rows.append(row)
        print(json.dumps(row), flush=True)
    lines = [f"| languages | grouped path (ms) | one batch, group_by_language=False (ms) | grouped / one batch | encoder passes (clips each) | ids equal |",
             "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['groups']} | {r['grouped_ms']} ({', '.join(str(v) for v in r['all_grouped'])}) | {r['one_batch_ms']} "
                     f"({', '.join(str(v) for v in r['all_one_batch'])}) | {r['ratio']} | {r['encodes_grouped']} vs {r['encodes_one_batch']} | {r['ids_equal']} |")
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table + "\n")
    eng.close()


if __name__ == "__main__":
    main()
