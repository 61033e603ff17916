"""generate(return_timestamps=True): HF's WhisperTimeStampLogitsProcessor inside the engine's decode loop (include/wm.h wm_decode_begin_ts,
DESIGN.md §2b).

The reference here is the oracle's chain loop (Oracle.decoder_pass + oracle.process_logits) followed, on every logits row, by transformers' own
WhisperTimeStampLogitsProcessor with the prefix the contract gives that row: base / head rows the committed ids, verify row i the committed ids
+ c_0 .. c_i.  The rule is pinned to HF's code, not to a restatement."""
import dataclasses

import numpy as np
import pytest
import torch

from helpers import MedusaConfig, GenParams, synth, clip_for, ACCEPT_TYPICAL, ACCEPT_GREEDY
from oracle.whisper_medusa_oracle import Oracle, process_logits, evaluate_posterior_chain
from whisper_medusa import WhisperMedusaModel
from whisper_medusa.timestamps import row_segments

pytestmark = pytest.mark.gpu

TIE = 5e-4          # the project's tie rule (tests/helpers.py check_tokens): logits closer than this, or p_c within TIE_P (relative) of the threshold
TIE_P = 2e-3


def micro_ts(heads_type="base_head", K=4):
    """micro shape remapped so that its vocabulary ends in a max_source_positions + 1 timestamp block with EOS, SOT and <|notimestamps|>
    below it (1031 - 934 = 97 = 96 + 1)."""
    c = MedusaConfig.micro(K=K, heads_type=heads_type)
    tb = c.vocab_size - (c.max_source_positions + 1)
    c = dataclasses.replace(c, eos_token_id=tb - 4, pad_token_id=tb - 4, decoder_start_token_id=tb - 3, prev_sot_token_id=tb - 2,
                            no_timestamps_token_id=tb - 1, begin_suppress_tokens=[7, tb - 4], max_initial_timestamp_index=5)
    assert c.supports_timestamps
    return c


def state_dict(cfg, seed, ts_scale):
    """Synthetic weights; the timestamp rows of the tied embedding are scaled so that the decode holds both timestamp pairs and text."""
    sd = synth.synth_state_dict(cfg, seed=seed)
    w = sd["whisper_model.proj_out.weight"]
    w[cfg.timestamp_begin:] *= ts_scale                    # (tied: the embedding rows change with it; engine and reference share sd)
    return sd


def ts_gen_params(cfg, mode, max_new):
    prompt = synth.default_prompt(cfg, timestamps=True)
    return GenParams(prompt=prompt, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id, suppress_tokens=[3, 5],
                     begin_suppress_tokens=list(cfg.begin_suppress_tokens), max_length=min(len(prompt) + max_new, cfg.max_target_positions),
                     hard_max_length=cfg.max_length, accept_mode=mode, temperature=1.0 if mode == ACCEPT_TYPICAL else 0.0,
                     timestamps=True, no_timestamps_token_id=cfg.no_timestamps_token_id,
                     max_initial_timestamp_index=cfg.max_initial_timestamp_index)


def hf_processor(cfg, begin_index):
    from transformers import GenerationConfig
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    gc = GenerationConfig(no_timestamps_token_id=cfg.no_timestamps_token_id, eos_token_id=cfg.eos_token_id)
    gc.max_initial_timestamp_index = cfg.max_initial_timestamp_index
    return WhisperTimeStampLogitsProcessor(gc, begin_index=begin_index, _detect_timestamp_from_logprob=True)


def decision_margin(row, tb):
    """|logsumexp(ts) - max(text)| of a row (after the per-token masks) and whether the decision masked the text."""
    lse = torch.logsumexp(row[tb:].double(), 0)
    mt = row[:tb].double().max()
    return float((lse - mt).abs()), bool(lse > mt)


def top2_gap(row):
    t = torch.topk(row.double(), 2).values
    return float(t[0] - t[1])


class Ref:
    """The oracle's loop with HF's timestamp processor per row.  Records, per emitted position, the smallest decision margin of the iteration
    that emitted it, and every row's decision."""

    def __init__(self, cfg, sd):
        self.cfg, self.orc = cfg, Oracle(cfg, sd, sim="bf16", act="hilo")

    def rows(self, proc, prefixes, x, gp, L):
        x = process_logits(x, L, gp)                   # the processors the engine already fuses: one cur_len = L for every row
        out, margins, flips = [], [], []
        for r, pre in enumerate(prefixes):
            pre_masked = proc(torch.tensor([pre]), x[r: r + 1].clone())
            _detect = proc._detect_timestamp_from_logprob
            proc._detect_timestamp_from_logprob = False    # the per-token masks alone, for the decision margin
            masks_only = proc(torch.tensor([pre]), x[r: r + 1].clone())
            proc._detect_timestamp_from_logprob = _detect
            m, f = decision_margin(masks_only[0], self.cfg.timestamp_begin)
            out.append(pre_masked[0]); margins.append(m); flips.append(f)
        return torch.stack(out), margins, flips

    def decode(self, enc, gp):
        cfg, orc = self.cfg, self.orc
        proc = hf_processor(cfg, gp.begin_index)
        K, P, eos = cfg.medusa_num_heads, len(gp.prompt), gp.eos_token_id
        st = orc.new_state(enc)
        ids, marg, flips = list(gp.prompt), [], []
        while True:
            L, kv = len(ids), st["kv_len"]
            if gp.vanilla:
                z = orc.decoder_pass(st, ids[kv:L], kv, disable_medusa=True, last_only=True)[:, 0]
                st["kv_len"] = L
                z, m, f = self.rows(proc, [ids], z, gp, L)
                tok = int(torch.argmax(z[0]))
                ids.append(tok); marg.append((min(m + [top2_gap(z[0])]), float("inf"))); flips += f
                if tok == eos or len(ids) >= gp.max_length:
                    break
                continue
            z = orc.decoder_pass(st, ids[kv:L], kv, disable_medusa=False, last_only=True)[:, 0]
            st["kv_len"] = L
            z, mz, fz = self.rows(proc, [ids] * (K + 1), z, gp, L)         # base pass: every head row sees the committed ids
            cand = torch.argmax(z, dim=-1)
            v = orc.decoder_pass(st, cand.tolist(), L, disable_medusa=True)[0]
            v, mv, fv = self.rows(proc, [ids + cand[: i + 1].tolist() for i in range(K + 1)], v, gp, L)   # verify row i: its own prefix
            a, dbg = evaluate_posterior_chain(v, cand, gp)
            m = (min(mz + mv + [top2_gap(r) for r in z] + [top2_gap(r) for r in v]),
                 min(((dbg["p_c"] - dbg["thr"]).abs() / dbg["thr"]).tolist()) if "p_c" in dbg else float("inf"))
            if a == 0:
                emit = [int(cand[0]), int(torch.argmax(v[0]))]
                st["kv_len"] = L + 1
            else:
                emit = [int(t) for t in cand[: a + 1]]
                st["kv_len"] = L + a
            ids += emit
            marg += [m] * len(emit)
            flips += [fz[0]] + fv[: a + 1]
            L = len(ids)
            if eos in emit or L >= gp.max_length or L + K >= gp.hard_max_length:
                break
        if eos in ids[P:]:
            j = ids.index(eos, P)
            ids = ids[: j + 1] + [eos] * (len(ids) - j - 1)
        return ids, marg, flips


def count_pairs(ids, P, tb):
    g = ids[P:]
    return sum(1 for i in range(len(g) - 1) if g[i] >= tb and g[i + 1] >= tb)


def assert_same(got, ref, label, P):
    """Strict equality, or a first difference at a decision within TIE (then the runs agree up to it): at most one such tie."""
    ids, marg, _ = ref
    if got == ids:
        return 0
    first = next((i for i, (a, b) in enumerate(zip(got, ids)) if a != b), min(len(got), len(ids)))
    m = marg[first - P] if 0 <= first - P < len(marg) else (float("inf"), float("inf"))
    print(f"timestamps[{label}]: first difference at {first}; smallest margins of that iteration: logit {m[0]:.3g} "
          f"(top-2 gap / |lse_ts - max_text|), p_c {m[1]:.3g} (relative to the threshold)")
    assert m[0] < TIE or m[1] < TIE_P, (label, first, m, got, ids)
    return 1


def check_nonvacuous(ref, P, tb, label):
    ids, _, flips = ref
    assert count_pairs(ids, P, tb) >= 2, (label, "fewer than 2 timestamp pairs", ids[P:])
    assert any(flips) and not all(flips), (label, "no decision flip", flips)


TS_SCALE = 3.0


@pytest.fixture(scope="module")
def micro_rig(gpu):
    out = {}
    for ht, seed in (("base_head", 21), ("medusa_block", 22)):
        cfg = micro_ts(ht)
        sd = state_dict(cfg, seed, TS_SCALE)
        out[ht] = (cfg, sd, Ref(cfg, sd))
    return out


def _model(cfg, sd, gpu, B):
    # the bf16 hi / lo operand contract (~17 bits): the scaled timestamp rows make the fp16 contract's logit error (~1e-3 here) as large
    # as the tie tolerance; the rules under test do not depend on the contract
    return WhisperMedusaModel(cfg, sd, device=gpu, max_batch=B, act_fp16=False)


# ---- the selection tap against HF on crafted rows -----------------------------------------------------------------------------------------
def test_select_rows_matches_hf(gpu, micro_rig):
    cfg, sd, _ = micro_rig["base_head"]
    m = _model(cfg, sd, gpu, 1)
    tb, V = cfg.timestamp_begin, cfg.vocab_size
    gp = ts_gen_params(cfg, ACCEPT_TYPICAL, 16)
    gp.begin_suppress_tokens = []
    gp.suppress_tokens = []
    P = len(gp.prompt)
    base = list(gp.prompt)
    prefixes = [
        base,                                  # at begin: timestamps only, <= tb + max_initial
        base + [tb + 3],                       # one timestamp: ts,ts rule (penultimate counts as timestamp) -> text only
        base + [tb + 3, 40],                   # text after ts: monotone floor last + 1
        base + [tb + 3, 40, tb + 9],           # text, ts -> no text below EOS, floor = last (may repeat)
        base + [tb + 3, 40, tb + 9, tb + 9],   # ts, ts -> text only
        base + [tb + 2, 17, 18, 19],           # plain text after a timestamp
        base + [50, 51],                       # no timestamp at all (no floor)
        base + [tb + 60, 9, tb + 61, tb + 61, 12, 13],
    ]
    rng = np.random.default_rng(5)
    rows, pre, probes = [], [], []
    for k, p in enumerate(prefixes):
        for scale_ts in (-3.0, 0.0, 3.0):     # decision false / near / true
            x = rng.standard_normal(V).astype(np.float32) * 2.0
            x[tb:] += scale_ts
            rows.append(x); pre.append(p)
            probes.append(int(rng.integers(0, V)) if k % 2 else tb + 12)
    out = m.engine.select_rows(gp, np.stack(rows), pre, probes)
    proc = hf_processor(cfg, gp.begin_index)
    n_forced = 0
    for r in range(len(rows)):
        want = proc(torch.tensor([pre[r]]), torch.from_numpy(rows[r][None]).clone())[0].double()
        am = int(torch.argmax(want))
        p = torch.softmax(want, 0)
        H = float(-(p * torch.log(p + 1e-5)).sum())
        m_, forced = decision_margin(_masks_only(proc)(torch.tensor([pre[r]]), torch.from_numpy(rows[r][None]).clone())[0], tb)
        n_forced += forced
        assert int(out["ts_forced"][r]) == int(forced) or m_ < TIE, (r, out["ts_forced"][r], forced, m_)
        assert int(out["argmax"][r]) == am or top2_gap(want) < TIE, (r, out["argmax"][r], am)
        np.testing.assert_allclose(out["p_probe"][r], float(p[probes[r]]), rtol=1e-5, atol=1e-7, err_msg=f"row {r}")
        np.testing.assert_allclose(out["entropy"][r], H, rtol=1e-5, atol=1e-6, err_msg=f"row {r}")
    assert 0 < n_forced < len(rows)


def _masks_only(proc):
    import copy
    q = copy.copy(proc)
    q._detect_timestamp_from_logprob = False
    return q


# ---- the decode loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ht", ["base_head", "medusa_block"])
@pytest.mark.parametrize("B", [1, 12])
def test_decode_matches_reference(gpu, micro_rig, ht, B):
    """Typical acceptance: one stream (sibling rows on, their default) and 12 streams (merged-step schedule)."""
    cfg, sd, ref = micro_rig[ht]
    m = _model(cfg, sd, gpu, B)
    gp = ts_gen_params(cfg, ACCEPT_TYPICAL, 48)
    P, tb = len(gp.prompt), cfg.timestamp_begin
    clips = [clip_for(cfg, i) for i in range(2)]
    feats = m.extract_features(clips * (B // 2) if B > 1 else clips[:1])
    got_all = []
    if B == 1:
        for c in clips:
            f = m.extract_features(c)
            m.engine.encode(f)
            got_all.append((m.engine.decode(gp, 1)[0], m.engine.encoder_output(1)[0]))
    else:
        m.engine.encode(feats)
        enc = m.engine.encoder_output(B)
        seqs = m.engine.decode(gp, B)
        assert m.engine.stats()["schedule_steps"] > 0
        got_all = [(seqs[i], enc[i]) for i in range(2)]
        assert all(seqs[i] == seqs[i % 2] for i in range(B))
    ties = 0
    for i, (got, enc) in enumerate(got_all):
        r = ref.decode(enc, gp)
        check_nonvacuous(r, P, tb, f"{ht} B={B} clip {i}")
        ties += assert_same(got, r, f"{ht} B={B} clip {i}", P)
    assert ties <= 1


def test_greedy_equals_vanilla_equals_reference(gpu, micro_rig):
    cfg, sd, ref = micro_rig["base_head"]
    m = _model(cfg, sd, gpu, 1)
    gp = ts_gen_params(cfg, ACCEPT_GREEDY, 40)
    gv = dataclasses.replace(gp, vanilla=True)
    P, tb = len(gp.prompt), cfg.timestamp_begin
    ties = 0
    for i in range(2):
        m.engine.encode(m.extract_features(clip_for(cfg, i)))
        enc = m.engine.encoder_output(1)[0]
        med = m.engine.decode(gp, 1)[0]
        van = m.engine.decode(gv, 1)[0]
        r = ref.decode(enc, gv)
        check_nonvacuous(r, P, tb, f"vanilla clip {i}")
        n = min(len(med), len(van))
        assert med[:n] == van[:n], (med, van)
        ties += assert_same(van, r, f"vanilla clip {i}", P)
    assert ties <= 1


def test_sibling_rows_do_not_change_ids(gpu, micro_rig, monkeypatch):
    cfg, sd, _ = micro_rig["base_head"]
    gp = ts_gen_params(cfg, ACCEPT_TYPICAL, 48)
    monkeypatch.setenv("WM_SIBLINGS", "0")
    off = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=1, act_fp16=False)
    monkeypatch.setenv("WM_SIBLINGS", "5")
    on = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=1, act_fp16=False)
    diffs = 0
    for i in range(2):
        f = on.extract_features(clip_for(cfg, i))
        on.engine.encode(f); off.engine.encode(f)
        a, b = on.engine.decode(gp, 1)[0], off.engine.decode(gp, 1)[0]
        diffs += a != b
    assert diffs <= 1


def test_generate_segments_follow_hf_rule(gpu, micro_rig):
    cfg, sd, _ = micro_rig["base_head"]
    m = _model(cfg, sd, gpu, 2)
    feats = m.extract_features([clip_for(cfg, 0), clip_for(cfg, 1)])
    d = m.generate(feats, return_timestamps=True, return_segments=True, max_new_tokens=40)
    t = d["sequences"]
    P = len(synth.default_prompt(cfg, timestamps=True))
    assert cfg.no_timestamps_token_id not in t[:, :P].tolist()[0]
    assert (t[:, P:] >= cfg.timestamp_begin).any()
    for i in range(2):
        want = row_segments(t[i].tolist(), P, cfg.eos_token_id, cfg.timestamp_begin, cfg.n_mel_frames)
        got = d["segments"][i]
        assert len(got) == len(want) and len(got) >= 1
        for g, w in zip(got, want):
            assert g["start"].dtype == torch.float64 and torch.equal(g["start"], w["start"]) and torch.equal(g["end"], w["end"])
            assert torch.equal(g["tokens"], w["tokens"])
    plain = m.generate(feats, max_new_tokens=40)
    assert plain.shape[0] == 2 and cfg.no_timestamps_token_id in plain[0].tolist()


def test_longform_two_windows(gpu, micro_rig):
    cfg, sd, _ = micro_rig["base_head"]
    m = _model(cfg, sd, gpu, 2)
    f = m.extract_features([clip_for(cfg, 0), clip_for(cfg, 1)])
    feats = torch.cat([f[0:1], f[1:2]], dim=-1)              # one clip of two windows
    d = m.generate(feats, chunk_longform=True, return_timestamps=True, return_segments=True, max_new_tokens=24)
    win = m.generate(f, return_timestamps=True, max_new_tokens=24)
    P = len(synth.default_prompt(cfg, timestamps=True))
    segs = d["segments"][0]
    w0 = row_segments(win[0].tolist(), P, cfg.eos_token_id, cfg.timestamp_begin, cfg.n_mel_frames)
    w1 = row_segments(win[1].tolist(), P, cfg.eos_token_id, cfg.timestamp_begin, cfg.n_mel_frames, time_offset=cfg.n_mel_frames * 0.01)
    assert len(segs) == len(w0) + len(w1)
    for g, w in zip(segs, w0 + w1):
        assert torch.allclose(g["start"], w["start"]) and torch.allclose(g["end"], w["end"])
    assert float(segs[-1]["start"]) >= cfg.n_mel_frames * 0.01


def test_tiny_en_layout(gpu):
    """tiny.en: the real 1501-token timestamp block; prompt [sot], every emitted token obeys the pairing / monotone rules."""
    cfg = MedusaConfig.tiny_en(K=4)
    assert cfg.supports_timestamps
    sd = state_dict(cfg, 0, TS_SCALE)
    m = _model(cfg, sd, gpu, 1)
    x = m.extract_features(clip_for(cfg, 0))
    out = m.generate(x, return_timestamps=True, return_segments=True, max_new_tokens=32)
    ids = out["sequences"][0].tolist()
    assert ids[0] == cfg.decoder_start_token_id and cfg.no_timestamps_token_id not in ids
    proc = hf_processor(cfg, 1)
    gen = [t for t in ids[1:]]
    tb = cfg.timestamp_begin
    for j, tok in enumerate(gen):
        if tok == cfg.eos_token_id:
            break
        s = torch.zeros(1, cfg.vocab_size)
        allowed = proc(torch.tensor([ids[: 1 + j]]), s)[0]
        if tok >= tb:               # a timestamp must be one the per-token masks allow (the decision can only remove text)
            assert allowed[tok] != -float("inf"), (j, tok, gen)
