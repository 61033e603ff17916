"""Word grouping on the GPU (include/wm.h wm_set_word_table / wm_word_spans, csrc/wm_words.hip).  The kernel against the restated
contract of tests/words_ref.py — word starts, float32 times and mean log-probabilities, exactly — on the seeded list, at the lane, tile and row
count edges, under a replaced table and inside a decode in progress; the entry's argument errors; then generate(return_word_timestamps=True) end
to end on the micro checkpoint against transformers' own functions on the call's own sequences and token timestamps."""
import ctypes as C
import dataclasses
import math
import re

import numpy as np
import pytest
import torch

import scores_ref as R
import words_ref as W
from helpers import synth
from test_gpu_token_timestamps import SHARPEN, checkpoint
from whisper_medusa import WhisperMedusaModel
from whisper_medusa import engine as E
from whisper_medusa import words as WD

pytestmark = pytest.mark.gpu
DIV = dict(no_repeat_ngram_size=1)      # random weights repeat one id for ever; no id twice: rows of many different tokens, so many words
TILE = E.WORDS_TILE
TOK, TOKEN_BYTES, N_TEXT = W.byte_level_whisper_tokenizer()
INDEX = {b: t for t, b in reversed(list(enumerate(TOKEN_BYTES)))}
NEW = 12


@pytest.fixture(scope="module")
def rig(gpu):
    cfg, sd = checkpoint("micro")       # micro shape with alignment heads
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=8)
    yield cfg, m
    m.engine.close()


@pytest.fixture()
def eng(rig):
    e = rig[1].engine
    t = WD.WordTable(TOKEN_BYTES)
    e.set_word_table(t.blob, t.offsets)
    e._word_table = None                # (generate() uploads its own table again)
    return e


def _values(rows, seed=0):
    rng = np.random.default_rng(seed)
    times, lps = [], []
    for r in rows:
        t = np.cumsum(rng.random(len(r) + 1)).astype(np.float32)
        times.append(np.stack([t[:-1], t[1:]], axis=1))
        lps.append((-3 * rng.random(len(r))).astype(np.float32))
    return times, lps


def _check(eng, rows, modes, token_bytes=TOKEN_BYTES, values=True):
    """One call: every row's word starts, times and log-probabilities are the restatement's, bit for bit; and the same call without the inputs."""
    times, lps = _values(rows)
    got = eng.word_spans(rows, modes, times, lps) if values else eng.word_spans(rows, modes)
    assert len(got) == len(rows)
    for r, (ids, (wf, wt, wl)) in enumerate(zip(rows, got)):
        rf, rt, rl = W.word_spans_ref(token_bytes, ids, modes[r], times[r] if values else None, lps[r] if values else None)
        assert wf.dtype == np.int32 and np.array_equal(wf, rf), (r, len(ids), wf[:12], rf[:12])
        if values:
            assert wt.dtype == wl.dtype == np.float32 and np.array_equal(wt, rt) and np.array_equal(wl, rl), r
        else:
            assert wt is None and wl is None
    return got


def _atoms_row(n, seed):
    """n ids drawn like the seeded list's rows."""
    rng = np.random.default_rng(seed)
    ids = []
    while len(ids) < n:
        a = W.ATOMS[int(rng.integers(len(W.ATOMS)))].encode()
        ids += [INDEX[a]] if a in INDEX and rng.random() < 0.6 else [INDEX[bytes([x])] for x in a]
    return ids[:n]


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------------
def test_kernel_equals_the_restatement_on_the_seeded_list_in_both_modes(eng):
    cases = W.seeded_cases(TOKEN_BYTES)
    rows = cases + cases
    modes = [W.SPACES] * len(cases) + [W.UNICODE] * len(cases)
    _check(eng, rows, modes)
    assert eng.last_words_ms > 0
    _check(eng, rows[::7], modes[::7], values=False)
    # with one of the two inputs alone
    sub, md = rows[:200], [W.SPACES, W.UNICODE] * 100          # both modes mixed in one call
    times, lps = _values(sub)
    for (wf, wt, wl), (wf2, wt2, wl2), (wf3, wt3, wl3) in zip(eng.word_spans(sub, md, times, lps), eng.word_spans(sub, md, times), eng.word_spans(sub, md, None, lps)):
        assert np.array_equal(wf, wf2) and np.array_equal(wf, wf3) and np.array_equal(wt, wt2) and np.array_equal(wl, wl3) and wl2 is None and wt3 is None


def test_row_lengths_at_lane_wave_and_tile_edges(eng):
    lens = [0, 1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 12000]
    rows = [_atoms_row(n, 100 + n) for n in lens]
    _check(eng, rows, [W.SPACES] * len(rows))
    _check(eng, rows, [W.UNICODE, W.SPACES] * (len(rows) // 2))
    for r in rows[:8]:                  # and a call of its own each (R = 1)
        _check(eng, [r], [W.SPACES])


def test_characters_and_punctuation_runs_across_a_tile_edge(eng):
    i = INDEX
    a, sp = i[b"a"], i[b" "]
    rows = []
    for shift in (0, 1, 2):             # "你" = E4 BD A0 over three byte tokens, the tile edge behind its first / second byte / in front of it
        head = [i[b" the"]] + [a] * (TILE - 2 - shift)
        rows.append(head + [i[b"\xe4"], i[b"\xbd"], i[b"\xa0"], a, i[b"."]])
        rows.append(head[:-1] + [sp, i[b"\xe3"], i[b"\x80"], i[b"\x80"], a])               # U+3000 behind a space: a whitespace-only word
    for k in range(5):                  # a prepend run ' ( [ " -' and an append chain 'a.,!?)' that straddle the edge at every offset
        rows.append([a] * (TILE - k) + [i[b" ("], i[b" ["], i[b" \""], i[b" -"], i[b" hello"], a])
        rows.append([a] * (TILE - k) + [i[b"."], i[b","], i[b"!"], i[b"?"], i[b")"], i[b" hello"]])
        rows.append([a] * (TILE - k) + [i[b"e "], i[b"."], i[b","], i[b" ("], i[b"."]])     # refused: the left word ends in a space
    rows.append([a] * (TILE - 1) + [i[b"\xe4"], i[b"\xbd"]])                                 # a truncated character at the end, across the edge
    assert all(len(r) > TILE for r in rows)
    _check(eng, rows, [W.SPACES] * len(rows))
    _check(eng, rows, [W.UNICODE] * len(rows))


def test_the_tables_longest_token_row_counts_and_both_orders(eng):
    longest = max(range(N_TEXT), key=lambda t: len(TOKEN_BYTES[t]))
    assert len(TOKEN_BYTES[longest]) > 8                       # beyond the bytes kept with a token's summary
    dots = INDEX["。。。！？……".encode()]
    rows = [[longest], [longest, INDEX[b"."]], [INDEX[b" ("], longest], [dots], [INDEX[b"a"], dots], [dots, longest, dots], [longest] * 70]
    _check(eng, rows, [W.SPACES] * len(rows))
    pool = W.seeded_cases(TOKEN_BYTES)[100:133]
    for R in (1, 2, 33):
        rs, md = pool[:R], [k % 2 for k in range(R)]
        fwd = _check(eng, rs, md)
        back = _check(eng, rs[::-1], md[::-1])
        assert all(np.array_equal(f[0], b[0]) for f, b in zip(fwd, back[::-1]))


def test_a_second_table_replaces_the_first(eng):
    rows = [[0, 1, 2, 3], [3, 2, 1, 0, 2]]
    t1 = [b" a", b"b", b".", b" ("]
    t2 = [b".", b" x", b" y", b"\xe4\xbd\xa0"]
    for tb in (t1, t2, t1):
        t = WD.WordTable(tb)
        eng.set_word_table(t.blob, t.offsets)
        _check(eng, rows, [W.SPACES, W.SPACES], token_bytes=tb)
    assert W.word_first_ref(t1, rows[0], 0) != W.word_first_ref(t2, rows[0], 0)
    with pytest.raises(ValueError, match=r"ids\[0\] = 4 outside the table"):                # the smaller table's bound holds now
        eng.word_spans([[4]], [0])


def test_a_call_inside_a_decode_leaves_the_decode_alone(rig, eng):
    cfg, m = rig
    feats = m.extract_features([synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160) for i in (0, 1)])
    gp = m._gen_params(None, None, None, 20, None, None, False, None, None, None, None, None)
    eng.encode(feats)
    want = eng.decode(gp, 2)
    rows = W.seeded_cases(TOKEN_BYTES)[200:240]
    ref = [W.word_first_ref(TOKEN_BYTES, r, 0) for r in rows]
    eng.encode(feats)
    g, _alive = eng._gen_struct(gp)
    eng._check(eng.lib.wm_decode_begin(eng.h, C.byref(g), 2), "wm_decode_begin")
    assert [list(w[0]) for w in eng.word_spans(rows, [0] * len(rows))] == ref
    left = C.c_int32(0)
    eng._check(eng.lib.wm_decode_run(eng.h, 1 << 30, C.byref(left)), "wm_decode_run")
    assert [eng.tokens(b) for b in range(2)] == want
    assert eng.decode(gp, 2) == want    # the captured graphs still replay


def _raw(eng, R, first, ids, modes, times=None, logprobs=None, nw=True, wf=True, wt=True, wl=True):
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    arr = lambda v, t: None if v is None else np.ascontiguousarray(v, dtype=t)          # noqa: E731
    p = lambda a, ty: None if a is None else a.ctypes.data_as(ty)                        # noqa: E731
    f, i, md, tm, lp = arr(first, np.int32), arr(ids, np.int32), arr(modes, np.int32), arr(times, np.float32), arr(logprobs, np.float32)
    o_nw, o_wf = (np.zeros(64, np.int32) if nw else None), (np.zeros(256, np.int32) if wf else None)
    o_wt, o_wl = (np.zeros(256, np.float32) if wt else None), (np.zeros(256, np.float32) if wl else None)
    rc = eng.lib.wm_word_spans(eng.h, R, p(f, i32p), p(i, i32p), p(md, i32p), p(tm, f32p), p(lp, f32p), p(o_nw, i32p), p(o_wf, i32p), p(o_wt, f32p),
                               p(o_wl, f32p), None)
    return rc, eng.lib.wm_last_error(eng.h).decode()


def test_argument_errors_come_back_with_their_reason(rig, eng):
    ok = dict(R=2, first=[0, 2, 3], ids=[1, 2, 3], modes=[0, 1])
    for change, word in ((dict(first=None), "null pointer"), (dict(ids=None), "null pointer"), (dict(modes=None), "null pointer"),
                         (dict(nw=False), "null pointer"), (dict(wf=False), "null pointer"),
                         (dict(times=np.zeros((3, 2)), wt=False), "times given without word_times"),
                         (dict(logprobs=np.zeros(3), wl=False), "logprobs given without word_logprobs"),
                         (dict(R=0), "R must be in"), (dict(R=E.WORDS_ROWS_MAX + 1), "R must be in"), (dict(first=[1, 2, 3]), r"first\[0\] must be 0"),
                         (dict(first=[0, 2, 1]), "first must ascend"), (dict(first=[0, 2, E.WORDS_IDS_MAX + 1]), "more than WM_WORDS_IDS_MAX"),
                         (dict(modes=[0, 2]), r"modes\[1\] = 2"), (dict(ids=[1, N_TEXT, 3]), r"ids\[1\] = %d outside" % N_TEXT),
                         (dict(ids=[-1, 2, 3]), r"ids\[0\] = -1 outside")):
        rc, err = _raw(eng, **dict(ok, **change))
        assert rc == -1, (change, rc)
        assert re.search(word, err), (change, err)
        assert list(eng.word_spans([[INDEX[b" a"], INDEX[b"."]]], [0])[0][0]) == [0, 2]                  # still usable
    # without the outputs that go with absent inputs: fine
    assert _raw(eng, **dict(ok, wt=False, wl=False))[0] == 0
    blob, off = np.zeros(4, np.uint8), np.asarray([0, 1, 2, 4], np.int32)
    u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    for args, word in (((None, off.ctypes.data_as(i32p), 3), "null pointer"), ((blob.ctypes.data_as(u8p), None, 3), "null pointer"),
                       ((blob.ctypes.data_as(u8p), off.ctypes.data_as(i32p), 0), "n_tokens must be"),
                       ((blob.ctypes.data_as(u8p), np.asarray([1, 2, 3, 4], np.int32).ctypes.data_as(i32p), 3), r"offsets\[0\] must be 0"),
                       ((blob.ctypes.data_as(u8p), np.asarray([0, 2, 2, 4], np.int32).ctypes.data_as(i32p), 3), "at least one byte")):
        assert eng.lib.wm_set_word_table(eng.h, *args) == -1 and re.search(word, eng.lib.wm_last_error(eng.h).decode()), word
    assert list(eng.word_spans([[INDEX[b" a"], INDEX[b"."]]], [0])[0][0]) == [0, 2]                      # a refused table leaves the old one in place
    with pytest.raises(ValueError, match="one entry per row"):
        eng.word_spans([[1]], [0, 0])
    with pytest.raises(ValueError, match="shape of rows"):
        eng.word_spans([[1, 2]], [0], [np.zeros((1, 2))])
    assert eng.word_spans([], []) == []
    # a context without a table: a state error that says so
    cfg, sd = checkpoint("micro")
    m2 = WhisperMedusaModel(cfg, sd, device=rig[1].device, max_batch=1)
    with pytest.raises(RuntimeError, match="no vocabulary table"):
        m2.engine.word_spans([[1]], [0])
    m2.engine.close()


# ---- 2. end to end on the micro checkpoint ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vocab(rig):
    cfg, _ = rig
    tok, token_bytes = W.whole_char_tokenizer(cfg.eos_token_id)
    return tok, WD.WordTable(token_bytes)


def _hf(tok, cfg, out, b, P, language="english"):
    """transformers' _collate_word_timestamps on every text run of row b of the call's own output, under the pipeline's pairing and rounding."""
    row = out["sequences"][b].tolist()
    tt = out["token_timestamps"][b].tolist()
    words = []
    for a, z in WD.text_rows(row, P, cfg.eos_token_id):
        pairs = [(round(tt[p - 1], 2), round(tt[p], 2)) for p in range(a, z)]
        words += [(w["text"], w["timestamp"]) for w in W.hf_words(tok, row[a:z], language, pairs)]
    return words


def _equal(tok, cfg, out, P, n_clips):
    total = 0
    for b in range(n_clips):
        got = out["words"][b]
        assert [(w["text"], w["timestamp"]) for w in got] == _hf(tok, cfg, out, b, P), b
        row = out["sequences"][b].tolist()
        assert all(0 < w["tokens"][0] < w["tokens"][1] <= len(row) for w in got)
        total += len(got)
    assert total > 0
    print(f"  {total} words over {n_clips} clips: {[w['text'] for w in out['words'][0]][:8]}")
    return total


def test_short_form_words_are_transformers(rig, vocab):
    cfg, m = rig
    tok, table = vocab
    P = len(synth.default_prompt(cfg))
    feats = m.extract_features([synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160) for i in (0, 1, 2)])
    out = m.generate(feats, max_new_tokens=NEW, **DIV, return_word_timestamps=True, tokenizer=tok)
    n = _equal(tok, cfg, out, P, 3)
    assert m.last_stats["ms_words"] > 0 and m.last_stats["ms_token_timestamps"] > 0
    print(f"short-form: {n} words over 3 clips, rows {[[z - a for a, z in WD.text_rows(r, P, cfg.eos_token_id)] for r in out['sequences'].tolist()]}, ms_words {m.last_stats['ms_words']:.3f}")
    # the same call with the table itself, on the plain decode path, with probabilities
    out = m.generate(feats, max_new_tokens=NEW, **DIV, return_word_timestamps=True, word_table=table, vanilla=True, return_token_logprobs=True)
    _equal(tok, cfg, out, P, 3)
    for b in range(3):
        lp = out["token_logprobs"][b].cpu().numpy().astype(np.float32)
        for w in out["words"][b]:
            acc = np.float32(0)
            for k in range(*w["tokens"]):
                acc = np.float32(acc + lp[k])
            assert w["probability"] == math.exp(float(np.float32(acc / np.float32(w["tokens"][1] - w["tokens"][0]))))
    # without the keyword: the token timestamps call as it was
    plain = m.generate(feats, max_new_tokens=NEW, **DIV, return_token_timestamps=True)
    assert "words" not in plain and "ms_words" not in m.last_stats


def test_segments_carry_their_words_and_no_word_crosses_a_timestamp_token(gpu):
    cfg = R.micro_ts("base_head")       # the micro shape whose vocabulary ends in a timestamp block, with alignment heads
    heads = synth.synth_alignment_heads(cfg, 2)
    cfg = dataclasses.replace(cfg, alignment_heads=heads)
    sd = R.ts_state_dict(cfg, seed=33)
    for l, h in heads:
        p = f"whisper_model.model.decoder.layers.{l}.encoder_attn.q_proj"
        sd[p + ".weight"][h * 64:(h + 1) * 64] *= SHARPEN
        sd[p + ".bias"][h * 64:(h + 1) * 64] *= SHARPEN
    m = WhisperMedusaModel(cfg, sd, device=gpu, max_batch=2)
    tok, _ = W.whole_char_tokenizer(cfg.eos_token_id)
    feats = m.extract_features([synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160) for i in (0, 1)])
    out = m.generate(feats, max_new_tokens=24, **DIV, return_timestamps=True, return_segments=True, return_word_timestamps=True, tokenizer=tok)
    P = len(m._last_prompt)
    n = _equal(tok, cfg, out, P, 2)
    rows = [[z - a for a, z in WD.text_rows(r, P, cfg.eos_token_id)] for r in out["sequences"].tolist()]
    print(f"timestamp rules: {n} words, text runs {rows}, segments {[len(s) for s in out['segments']]}")
    for b in range(2):
        row = out["sequences"][b].tolist()
        assert all(all(t < cfg.eos_token_id for t in row[w["tokens"][0]: w["tokens"][1]]) for w in out["words"][b])
        # every segment carries the words inside its own tokens; text behind the last closed segment (HF drops an unfinished one) is in none
        o, held = P, 0
        for sg in out["segments"][b]:
            n_tok = int(sg["tokens"].numel())
            assert sg["words"] == [w for w in out["words"][b] if o <= w["tokens"][0] and w["tokens"][1] <= o + n_tok]
            o, held = o + n_tok, held + len(sg["words"])
        assert held > 0 and [w for sg in out["segments"][b] for w in sg["words"]] == [w for w in out["words"][b] if w["tokens"][0] < o]
    m.engine.close()


def test_pool_words_are_transformers(rig, vocab):
    cfg, m = rig
    tok, _ = vocab
    P = len(synth.default_prompt(cfg))
    feats = m.extract_features([synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160) for i in (0, 1, 2, 3)])
    one = m.generate(feats, max_new_tokens=NEW, **DIV, return_word_timestamps=True, tokenizer=tok)
    m.set_micro_batches(2)
    try:
        out = m.generate(feats, max_new_tokens=NEW, **DIV, return_word_timestamps=True, tokenizer=tok)
    finally:
        m.set_micro_batches(None)
    _equal(tok, cfg, out, P, 4)
    assert torch.equal(out["sequences"], one["sequences"]) and [[w["text"] for w in c] for c in out["words"]] == [[w["text"] for w in c] for c in one["words"]]


def test_strided_words_through_both_doors(rig, vocab):
    cfg, m = rig
    tok, _ = vocab
    F, P = cfg.n_mel_frames, len(synth.default_prompt(cfg))
    assert F == 192
    wavs = [synth.synth_clip(i, n_samples=(2 * F + 37) * 160) for i in (3, 4)]         # three windows of 192 frames with strides of 32
    feats = m.extract_features(wavs, truncation=False)
    kw = dict(chunk_longform=True, stride_length_s=0.32, max_new_tokens=NEW, return_word_timestamps=True, tokenizer=tok, **DIV)
    out = m.generate(feats, **kw)
    assert m.last_stats["longform_windows"] == [3, 3] and m.last_stats["ms_words"] > 0 and "window_keep" in out
    _equal(tok, cfg, out, P, 2)
    out = m.generate_from_wav(wavs, **kw)
    assert m.last_stats["longform_windows"] == [3, 3]
    _equal(tok, cfg, out, P, 2)
    # the unstrided chunked route
    out = m.generate(feats, chunk_longform=True, max_new_tokens=NEW, return_word_timestamps=True, tokenizer=tok, **DIV)
    _equal(tok, cfg, out, P, 2)
