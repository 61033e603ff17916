"""Time of grouping token ids into words: wm_word_spans (one kernel launch for all rows of a call) against transformers'
_combine_tokens_into_words on the same id lists, on the same machine.

    python tests/microbench/words_time.py [--reps 20] [--hf-reps 3] [--bench-call] [--out FILE.md]

The rows are drawn from the atoms of tests/words_ref.py over its byte-level WhisperTokenizer (multi-byte characters split across byte tokens,
punctuation of both passes), whole atoms only, so every row is inside the domain of equality.  Workloads: 120 rows of 100 ids (an hour of 30 s
windows), one row of 12 000 ids (an hour as one assembled text), 32 times the first.  Engine: the call's own hipEvent time (upload + kernel +
download), median and minimum of --reps calls after two warm-up calls, and the host clock around Engine.word_spans (which adds the packing of the
Python lists); both with times and log-probabilities.  transformers: the host clock around the function, row by row, best of --hf-reps.  The
word starts of the two are compared.  --bench-call: one strided generate(return_word_timestamps=True) on the bench checkpoint (large-v2 shape,
K = 10, synthetic weights, synthetic alignment heads) over a 10 min recording and its ms_words share."""
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
from whisper_medusa import words as WD  # noqa: E402
import words_ref as W  # noqa: E402


def make_rows(token_bytes, n_rows, n_ids, seed):
    index = {b: t for t, b in reversed(list(enumerate(token_bytes)))}
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_rows):
        ids = []
        while True:
            a = W.ATOMS[int(rng.integers(len(W.ATOMS)))].encode()
            new = [index[a]] if a in index and rng.random() < 0.6 else [index[bytes([x])] for x in a]
            if len(ids) + len(new) > n_ids:
                break
            ids += new
        rows.append(ids)
    return rows


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
    tok, token_bytes, _ = W.byte_level_whisper_tokenizer()
    table = WD.WordTable(token_bytes)
    eng.set_word_table(table.blob, table.offsets)
    out = []
    for n_rows, n_ids in ((120, 100), (1, 12000), (32 * 120, 100)):
        rows = make_rows(token_bytes, n_rows, n_ids, 13 * n_rows + n_ids)
        rng = np.random.default_rng(1)
        times = [np.stack([np.arange(len(r), dtype=np.float32), np.arange(1, len(r) + 1, dtype=np.float32)], axis=1) * np.float32(0.02) for r in rows]
        lps = [(-rng.random(len(r))).astype(np.float32) for r in rows]
        modes = [W.SPACES] * n_rows
        ev, wall = [], []
        for rep in range(a.reps + 2):
            t0 = time.perf_counter()
            got = eng.word_spans(rows, modes, times, lps)
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(eng.last_words_ms)
        ev, wall = ev[2:], wall[2:]
        hf, ref = [], None
        for rep in range(a.hf_reps):
            t0 = time.perf_counter()
            ref = [W.hf_words(tok, r, "english")[1] for r in rows]
            hf.append(1e3 * (time.perf_counter() - t0))
            if hf[-1] > 20000:
                break
        same = all([i[0] for i in idx] + [len(r)] == list(g[0]) for r, idx, g in zip(rows, ref, got))
        row = dict(rows=n_rows, ids=n_ids, ids_total=sum(len(r) for r in rows), words=sum(len(g[0]) - 1 for g in got),
                   engine_event_ms_median=round(statistics.median(ev), 3), engine_event_ms_min=round(min(ev), 3),
                   engine_wall_ms_median=round(statistics.median(wall), 2), hf_wall_ms_best=round(min(hf), 1), hf_reps=len(hf),
                   hf_over_engine_event=round(min(hf) / statistics.median(ev), 1), hf_over_engine_wall=round(min(hf) / statistics.median(wall), 1),
                   starts_equal=same)
        out.append(row)
        print(json.dumps(row), flush=True)
    lines = ["| rows x ids | ids / words | wm_word_spans, hipEvent ms (median / min) | Engine.word_spans, host clock ms (median) | "
             "transformers, host clock ms (best of n) | transformers / event | transformers / host clock | word starts equal |", "|---|---|---|---|---|---|---|---|"]
    for r in out:
        lines.append(f"| {r['rows']} x {r['ids']} | {r['ids_total']} / {r['words']} | {r['engine_event_ms_median']} / {r['engine_event_ms_min']} | "
                     f"{r['engine_wall_ms_median']} | {r['hf_wall_ms_best']} (n = {r['hf_reps']}) | {r['hf_over_engine_event']} | {r['hf_over_engine_wall']} | {r['starts_equal']} |")
    eng.close()
    if a.bench_call:
        import dataclasses
        big = MedusaConfig.large_v2(K=10)
        big = dataclasses.replace(big, alignment_heads=synth.synth_alignment_heads(big, 6))
        from whisper_medusa.engine import default_act_fp16
        f16 = default_act_fp16()
        sd = synth.synth_state_dict(big, seed=0, device=str(dev), logit_std=4.5)
        blob, offs = weights.build_blob(big, sd, device=dev, act_fp16=f16)
        del sd
        model = WhisperMedusaModel.from_blob(big, blob, offs, max_batch=32, act_fp16=f16)
        btok, bbytes = W.whole_char_tokenizer(big.eos_token_id)
        wav = torch.from_numpy(synth.synth_clip(0, 600 * 16000))[None].to(dev)
        feats = model.engine.logmel_long(wav)                       # [1, 80, 60000]: 10 min
        kw = dict(chunk_longform=True, stride_length_s=5.0, max_new_tokens=100, word_table=WD.WordTable(bbytes), language="en",
                  suppress_tokens=sorted(set(list(big.suppress_tokens or []) + [big.eos_token_id])))
        res = []
        for rep in range(3):                                        # (the first call warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = model.generate(feats, return_word_timestamps=True, **kw)
            torch.cuda.synchronize()
            res.append((1e3 * (time.perf_counter() - t0), dict(model.last_stats), sum(len(w) for w in o["words"]), int(o["sequences"].shape[1])))
        ms, st, n_words, T = min(res[1:], key=lambda v: v[0])
        t0 = time.perf_counter()
        row = o["sequences"][0].tolist()
        P = len(model._last_prompt)
        hf_n = sum(len(W.hf_words(btok, row[p:q], "english")[1]) for p, q in WD.text_rows(row, P, big.eos_token_id))
        hf_ms = 1e3 * (time.perf_counter() - t0)
        call = dict(frames=int(feats.shape[-1]), windows=st["longform_windows"][0], call_ms=round(ms, 1), ms_words=round(st["ms_words"], 3),
                    words_share=round(st["ms_words"] / ms, 6), ms_token_timestamps=round(st.get("ms_token_timestamps", 0.0), 1), ms_merge=round(st["ms_merge"], 3),
                    row_ids=T, words=n_words, hf_words=hf_n, hf_ms_on_the_same_row=round(hf_ms, 1))
        print(json.dumps(call), flush=True)
        lines += ["", f"Strided call with return_word_timestamps on the bench checkpoint, {call['frames']} frames, 100 new ids per window: {call['windows']} windows, "
                      f"{call['call_ms']} ms per call, ms_words {call['ms_words']} ({100 * call['words_share']:.4f} % of the call; token timestamps "
                      f"{call['ms_token_timestamps']} ms, merge {call['ms_merge']} ms); {call['words']} words over {call['row_ids']} positions; "
                      f"transformers on the same row: {call['hf_ms_on_the_same_row']} ms, {call['hf_words']} words."]
        model.engine.close()
    table_md = "\n".join(lines)
    print(table_md)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table_md + "\n")


if __name__ == "__main__":
    main()
