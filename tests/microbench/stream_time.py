"""Time of the streaming agreement step: wm_stream_agree (one kernel launch for all live sessions of a tick) against the Python
statement of the same policy (tests/stream_ref.py agree_ref) on the same lists, on the same machine; and what a tick of 32 sessions costs.

    python tests/microbench/stream_time.py [--reps 50] [--ref-reps 3] [--tick] [--out FILE.md]

Lists: S sessions (1, 32, 1024), each with a new hypothesis of 60 words of one or two tokens, a previous hypothesis that repeats its words under
another tokenisation up to a seeded mismatch, and a tail of five committed words of which the new hypothesis repeats the last two.  Engine: the
call's own hipEvent time (upload + kernel + download), median and minimum of --reps calls after three warm-up calls, and the host clock around
Engine.stream_agree (which adds the packing of the Python lists).  agree_ref: the host clock around the loop over the sessions, best of --ref-reps.
The outputs of the two are compared.  --tick: on the bench checkpoint (large-v2 shape, K = 10, synthetic weights, alignment heads) 32 sessions
hold 10 s of audio each and receive 1 s per tick; ms_feed of a tick is split into ms_generate, ms_agree and the rest (the session layer itself),
next to a plain 32-clip extract_features + generate(return_word_timestamps=True) on the same audio, alternating, after two warm-up ticks."""
import argparse
import dataclasses
import datetime
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
from whisper_medusa import words as WD  # noqa: E402
import stream_ref as SR  # noqa: E402

N_WORDS = 60


def table():
    rng = np.random.default_rng(5)
    stems = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(2, 9)))) for _ in range(2000)]
    return [bytes([b]) for b in range(256)] + [(" " + s).encode() for s in stems] + [s.encode() for s in stems] + [b".", b",", b"?"]


def sessions(token_bytes, S, seed):
    rng = np.random.default_rng(seed)
    whole = lambda: [int(rng.integers(256, 2256))] + ([int(rng.integers(2256, 4256))] if rng.random() < 0.4 else []) + ([4256] if rng.random() < 0.1 else [])   # noqa: E731
    spell = lambda w: [int(b) for t in w for b in token_bytes[t]]                                       # noqa: E731  (byte ids are the bytes)
    out = []
    for _ in range(S):
        new = [whole() for _ in range(N_WORDS)]
        tail = [whole() for _ in range(3)] + [spell(w) for w in new[:2]]
        stop = int(rng.integers(20, N_WORDS - 2))
        prev = [spell(w) if rng.random() < 0.5 else list(w) for w in new[2: 2 + stop]] + [whole() for _ in range(N_WORDS - 2 - stop)]
        starts = 1000 + np.cumsum(rng.integers(5, 40, N_WORDS))
        out.append(dict(new=new, prev=prev, tail=tail, times=[(int(s), int(s) + 5) for s in starts], last_cs=1000))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--tick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = MedusaConfig.micro()
    eng = WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=1), device=dev).engine
    tb = table()
    t = WD.WordTable(tb)
    eng.set_word_table(t.blob, t.offsets)
    rows = []
    for S in (1, 32, 1024):
        cs = sessions(tb, S, 100 + S)
        args = ([c["new"] for c in cs], [c["prev"] for c in cs], [c["tail"] for c in cs], [c["times"] for c in cs], [c["last_cs"] for c in cs])
        ev, wall, got = [], [], None
        for rep in range(a.reps + 3):
            t0 = time.perf_counter()
            got = eng.stream_agree(*args)
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(eng.last_stream_ms)
        ev, wall = ev[3:], wall[3:]
        ref_ms, ref = [], None
        for rep in range(a.ref_reps):
            t0 = time.perf_counter()
            ref = [SR.agree_ref(tb, c["new"], c["prev"], c["tail"], c["times"], c["last_cs"]) for c in cs]
            ref_ms.append(1e3 * (time.perf_counter() - t0))
        same = [tuple(int(x[k]) for x in got) for k in range(S)] == ref
        row = dict(sessions=S, words=N_WORDS, ids=sum(len(w) for c in cs for l in ("new", "prev", "tail") for w in c[l]),
                   event_ms_median=round(statistics.median(ev), 4), event_ms_min=round(min(ev), 4), wall_ms_median=round(statistics.median(wall), 3),
                   ref_wall_ms_best=round(min(ref_ms), 2), ref_over_event=round(min(ref_ms) / statistics.median(ev), 1),
                   ref_over_wall=round(min(ref_ms) / statistics.median(wall), 1), equal=same, committed=sum(r[1] for r in ref), skipped=sum(r[0] for r in ref))
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    lines = [f"`python tests/microbench/stream_time.py{' --tick' if a.tick else ''} --reps {a.reps}`, {datetime.datetime.now().strftime('%Y-%m-%d')}, "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Clocks: hipEvent pair of the call (upload + kernel + download) and "
             "time.perf_counter around calls that end in a device synchronise.", "",
             "| sessions x words | ids | wm_stream_agree, hipEvent ms (median / min) | Engine.stream_agree, host clock ms (median) | agree_ref, host clock ms (best) | "
             "agree_ref / event | agree_ref / host clock | outputs equal |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['sessions']} x {r['words']} | {r['ids']} | {r['event_ms_median']} / {r['event_ms_min']} | {r['wall_ms_median']} | {r['ref_wall_ms_best']} | "
                     f"{r['ref_over_event']} | {r['ref_over_wall']} | {r['equal']} |")
    if a.tick:
        big = MedusaConfig.large_v2(K=10)
        big = dataclasses.replace(big, alignment_heads=synth.synth_alignment_heads(big, 6))
        from whisper_medusa.engine import default_act_fp16
        f16 = default_act_fp16()
        sd = synth.synth_state_dict(big, seed=0, device=str(dev), logit_std=4.5)
        blob, offs = weights.build_blob(big, sd, device=dev, act_fp16=f16)
        del sd
        model = WhisperMedusaModel.from_blob(big, blob, offs, max_batch=32, act_fp16=f16)
        n_text = big.eos_token_id
        wt = WD.WordTable([(b" " if k % 3 else b"") + b"t%d" % k + (b"." if k % 17 == 0 else b"") for k in range(n_text)])
        kw = dict(max_new_tokens=64, suppress_tokens=sorted(set(list(big.suppress_tokens or []) + [big.eos_token_id])), no_repeat_ngram_size=3)
        S = 32
        ss = model.stream_sessions(S, word_table=wt, min_chunk_s=1.0, **kw)
        clips = [synth.synth_clip(40 + k, 20 * 16000) for k in range(S)]
        ss.feed([c[: 9 * 16000] for c in clips])                               # 9 s each, the first decode
        ticks, plain, feats_ms = [], [], []
        for tck in range(7):
            chunk = [c[(9 + tck) * 16000: (10 + tck) * 16000] for c in clips]
            torch.cuda.synchronize()
            res = ss.feed(chunk)
            torch.cuda.synchronize()
            st = dict(ss.last_stats)
            st["committed"] = sum(len(r["committed"]) for r in res)
            st["pending"] = sum(len(r["pending"]) for r in res)
            ticks.append(st)
            t0 = time.perf_counter()
            f = model.extract_features(ss.buf)
            torch.cuda.synchronize()
            feats_ms.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            model.generate(f, return_word_timestamps=True, word_table=wt, **kw)
            torch.cuda.synchronize()
            plain.append(feats_ms[-1] + 1e3 * (time.perf_counter() - t0))
            print(json.dumps(dict(tick=tck, **{k: round(v, 3) if isinstance(v, float) else v for k, v in st.items()}, plain_ms=round(plain[-1], 2),
                                  features_ms=round(feats_ms[-1], 2))), flush=True)
        use = ticks[2:]
        med = lambda k: statistics.median(x[k] for x in use)                   # noqa: E731
        rest = statistics.median(x["ms_feed"] - x["ms_generate"] - x["ms_agree"] for x in use)
        lines += ["", f"One tick of {S} sessions on the bench checkpoint (large-v2 shape, K = 10, synthetic weights, 6 alignment heads; buffers of 10 - 16 s, 1 s of new "
                      f"audio per session and tick, 64 new ids per hypothesis, EOS suppressed), medians of {len(use)} ticks after 2 warm-up ticks:", "",
                  "| ms_feed | ms_generate (extract_features + generate, host clock) | ms_agree (hipEvent) | rest (the session layer) | rest / ms_feed | "
                  "plain 32-clip extract_features + generate(return_word_timestamps=True) | of which extract_features | words committed / pending per tick |",
                  "|---|---|---|---|---|---|---|---|",
                  f"| {med('ms_feed'):.2f} | {med('ms_generate'):.2f} | {med('ms_agree'):.3f} | {rest:.2f} | {100 * rest / med('ms_feed'):.2f} % | "
                  f"{statistics.median(plain[2:]):.2f} | {statistics.median(feats_ms[2:]):.2f} | {med('committed'):.0f} / {med('pending'):.0f} |"]
        model.engine.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
