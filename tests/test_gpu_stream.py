"""Live transcription on the GPU (include/wm.h wm_stream_agree, csrc/wm_stream.hip, whisper_medusa/streaming.py).  The kernel against
the restated contract of tests/stream_ref.py — skip, commit and ender, exactly — on the seeded list in one call and one session at a time, at the
lane and block edges, under a replaced table and inside a decode in progress; the entry's argument and state errors; then stream_sessions end to
end on the micro checkpoint against the one-session reference driver, its batch independence and its keywords."""
import ctypes as C
import re

import numpy as np
import pytest

import stream_ref as SR
import words_ref as W
from helpers import synth
from test_gpu_token_timestamps import checkpoint
from whisper_medusa import WhisperMedusaModel
from whisper_medusa import engine as E
from whisper_medusa import words as WD

pytestmark = pytest.mark.gpu
TOK, TOKEN_BYTES, N_TEXT = W.byte_level_whisper_tokenizer()
INDEX = {b: t for t, b in reversed(list(enumerate(TOKEN_BYTES)))}
CASES = SR.seeded_cases(TOKEN_BYTES)


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


def _ref(cases, token_bytes=TOKEN_BYTES, **kw):
    return [SR.agree_ref(token_bytes, c["new"], c["prev"], c["tail"], c["times"], c["last_cs"], **kw) for c in cases]


def _run(eng, cases, **kw):
    skip, commit, ender = eng.stream_agree([c["new"] for c in cases], [c["prev"] for c in cases], [c["tail"] for c in cases], [c["times"] for c in cases],
                                           [c["last_cs"] for c in cases], **kw)
    assert skip.dtype == commit.dtype == ender.dtype == np.int32 and len(skip) == len(commit) == len(ender) == len(cases)
    return list(zip(skip.tolist(), commit.tolist(), ender.tolist()))


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------------
def test_kernel_equals_the_restatement_on_the_seeded_list_in_one_call_and_one_session_at_a_time(eng):
    ref = _ref(CASES)
    assert len(CASES) >= 257
    got = _run(eng, CASES)
    assert eng.last_stream_ms > 0
    bad = [(n, g, r) for n, (g, r) in enumerate(zip(got, ref)) if g != r]
    assert not bad, bad[:10]
    assert _run(eng, CASES) == got                          # two runs, the same bytes
    assert _run(eng, CASES[::-1]) == ref[::-1]
    for n, c in enumerate(CASES):                           # S = 1
        assert _run(eng, [c]) == [ref[n]], n
    # other parameters than the defaults
    for kw in (dict(late_cs=0, near_cs=30, max_ngram=2), dict(late_cs=25, near_cs=1000, max_ngram=1), dict(late_cs=10, near_cs=0, max_ngram=5)):
        assert _run(eng, CASES, **kw) == _ref(CASES, **kw), kw
    print(f"{len(CASES)} sessions, {sum(len(c['new']) for c in CASES)} words: {eng.last_stream_ms:.3f} ms")


def test_edges_in_one_call_and_the_tables_longest_token_inside_a_key(eng):
    edge = [c for c in CASES if len(c["new"]) in SR.EDGES or len(c["prev"]) in SR.EDGES]
    assert {len(c["new"]) for c in edge} >= set(SR.EDGES) and len(edge) >= 40
    longest = INDEX[b" internationalisation"]
    assert len(TOKEN_BYTES[longest]) == max(len(b) for b in TOKEN_BYTES) > 16
    by = [INDEX[bytes([x])] for x in TOKEN_BYTES[longest]]
    a, sp, dot = INDEX[b" a"], INDEX[b" "], INDEX[b"."]
    far = [(2000 + 10 * k, 2005 + 10 * k) for k in range(4)]
    extra = [dict(new=[[a], [sp, longest, dot, sp], [a]], prev=[[a], by + [dot], [a]], tail=[], times=far[:3], last_cs=1000),
             dict(new=[[a], [longest, longest]], prev=[[a], by + by[1:]], tail=[], times=far[:2], last_cs=1000),                  # an inner space is kept
             dict(new=[[a], [longest, longest]], prev=[[a], by + by], tail=[], times=far[:2], last_cs=1000),
             dict(new=[[longest, dot], [a]], prev=[[a]], tail=[by + [dot, sp]], times=[(1001, 1005), (1010, 1020)], last_cs=1000)]
    ref = _ref(edge + extra)
    assert ref[len(edge):] == [(0, 3, 1), (0, 1, -1), (0, 2, -1), (1, 1, -1)]
    assert _run(eng, edge + extra) == ref
    assert _run(eng, extra + edge) == ref[len(edge):] + ref[:len(edge)]


# ---- 2. state, errors, side effects ----------------------------------------------------------------------------------------------------------------------
def test_a_second_table_replaces_the_first(eng):
    cases = [dict(new=[[0, 1], [2]], prev=[[3], [2]], tail=[], times=[(500, 510), (520, 530)], last_cs=100),
             dict(new=[[1], [2, 0]], prev=[[1], [2]], tail=[[1]], times=[(101, 110), (120, 130)], last_cs=100)]
    t1 = [b" a", b"b", b".", b" ab"]
    t2 = [b"c", b"x", b"y", b" xc"]
    for tb in (t1, t2, t1):
        t = WD.WordTable(tb)
        eng.set_word_table(t.blob, t.offsets)
        assert _run(eng, cases) == _ref(cases, tb)
    assert _ref(cases, t1) != _ref(cases, t2)
    with pytest.raises(ValueError, match=r"new\.ids\[0\] = 4 outside the table"):          # the smaller table's bound holds now
        eng.stream_agree([[[4]]], [[]], [[]], [[(0, 1)]], [0])


def test_a_call_inside_a_decode_leaves_the_decode_alone(rig, eng):
    cfg, m = rig
    feats = m.extract_features([synth.synth_clip(i, n_samples=cfg.n_mel_frames * 160) for i in (0, 1)])
    gp = m._gen_params(None, None, None, 20, None, None, False, None, None, None, None, None)
    eng.encode(feats)
    want = eng.decode(gp, 2)
    cases = CASES[60:120]
    eng.encode(feats)
    g, _alive = eng._gen_struct(gp)
    eng._check(eng.lib.wm_decode_begin(eng.h, C.byref(g), 2), "wm_decode_begin")
    assert _run(eng, cases) == _ref(cases)
    left = C.c_int32(0)
    eng._check(eng.lib.wm_decode_run(eng.h, 1 << 30, C.byref(left)), "wm_decode_run")
    assert [eng.tokens(b) for b in range(2)] == want
    assert eng.decode(gp, 2) == want    # the captured graphs still replay


OK = dict(S=2, new=([0, 2, 3], [0, 1, 3, 4], [1, 2, 3, 4]), prev=([0, 1, 1], [0, 1], [1]), tail=([0, 0, 1], [0, 2], [5, 6]), times=np.zeros((3, 2)),
          last=[0, 0], params=(10, 100, 5))


def _raw(eng, S, new, prev, tail, times, last, params, outs=(True, True, True)):
    i32p = C.POINTER(C.c_int32)
    keep = []

    def arr(v):
        if v is None:
            return None
        a = np.ascontiguousarray(v, dtype=np.int32)
        keep.append(a)
        return a.ctypes.data_as(i32p)

    def lst(l):
        if l is None:
            return None
        s = E.WmStreamList(arr(l[0]), arr(l[1]), arr(l[2]))
        keep.append(s)
        return C.byref(s)
    p = None if params is None else E.WmStreamParams(*params)
    out = [np.zeros(8, dtype=np.int32) if k else None for k in outs]
    o = [None if a is None else a.ctypes.data_as(i32p) for a in out]
    rc = eng.lib.wm_stream_agree(eng.h, S, lst(new), lst(prev), lst(tail), arr(times), arr(last), None if p is None else C.byref(p), o[0], o[1], o[2], None)
    return rc, eng.lib.wm_last_error(eng.h).decode(), [None if a is None else a.tolist() for a in out]


def test_argument_and_state_errors_come_back_with_their_reason(rig, eng):
    rc, _, out = _raw(eng, **OK)
    assert rc == 0 and [o[:2] for o in out] == [[0, 0], [1, 0], [-1, -1]]
    assert _raw(eng, **dict(OK, params=None))[0] == 0                                       # NULL: the defaults
    big_w, big_i = E.STREAM_WORDS_MAX, E.STREAM_IDS_MAX
    half = big_w // 2
    for change, word in ((dict(new=None), "null pointer"), (dict(prev=None), "null pointer"), (dict(tail=None), "null pointer"), (dict(times=None), "null pointer"),
                         (dict(last=None), "null pointer"), (dict(outs=(False, True, True)), "null pointer"), (dict(outs=(True, True, False)), "null pointer"),
                         (dict(new=(None, [0], [0])), r"new: null pointer \(words, tok, ids\)"), (dict(tail=([0, 0, 1], [0, 2], None)), "tail: null pointer"),
                         (dict(S=0), "S must be in"), (dict(S=E.STREAM_SESSIONS_MAX + 1), "S must be in"),
                         (dict(new=([1, 2, 3], [0, 1, 3, 4], [1, 2, 3, 4])), r"new\.words\[0\] must be 0"),
                         (dict(prev=([0, 1, 0], [0, 1], [1])), r"prev\.words must ascend \(words\[2\] < words\[1\]\)"),
                         (dict(new=([0, 2, 3], [1, 1, 3, 4], [1, 2, 3, 4])), r"new\.tok\[0\] must be 0"),
                         (dict(new=([0, 2, 3], [0, 1, 1, 4], [1, 2, 3, 4])), r"new: a word without ids \(tok\[2\] <= tok\[1\]\)"),
                         (dict(tail=([0, 6, 6], [0, 1, 2, 3, 4, 5, 6], [1] * 6)), "tail: session 0 has 6 words, more than WM_STREAM_TAIL = 5"),
                         (dict(new=([0, 2, 3], [0, 1, 3, 4], [1, 2, N_TEXT, 4])), r"new\.ids\[2\] = %d outside the table" % N_TEXT),
                         (dict(tail=([0, 0, 1], [0, 2], [5, -1])), r"tail\.ids\[1\] = -1 outside"),
                         (dict(prev=([0, 1, big_w + 1], [0, 1], [1])), "prev: more than WM_STREAM_WORDS_MAX"),
                         (dict(prev=([0, 1, 1], [0, big_i + 1], [1])), "prev: more than WM_STREAM_IDS_MAX"),
                         (dict(new=([0, half, half], np.arange(half + 1), [1]), prev=([0, half + 1, half + 1], np.arange(half + 2), [1])),
                          "the three lists hold more than WM_STREAM_WORDS_MAX"),          # (each list alone fits; the sum is checked before any id is read)
                         (dict(params=(-1, 100, 5)), "late_cs = -1"), (dict(params=(10, -1, 5)), "near_cs = -1"), (dict(params=(10, 100, 0)), "max_ngram = 0"),
                         (dict(params=(10, 100, 6)), "max_ngram = 6")):
        rc, err, _ = _raw(eng, **dict(OK, **change))
        assert rc == -1, (change.keys(), rc, err)
        assert re.search(word, err), (word, err)
        assert _run(eng, CASES[:40]) == _ref(CASES[:40])                                    # still usable
    # the Python glue's own checks
    with pytest.raises(ValueError, match="one entry per session"):
        eng.stream_agree([[]], [[], []], [[]], [[]], [0])
    with pytest.raises(ValueError, match="at most STREAM_TAIL = 5"):
        eng.stream_agree([[]], [[]], [[[1]] * 6], [[]], [0])
    with pytest.raises(ValueError, match="one .start, end. per word"):
        eng.stream_agree([[[1]]], [[]], [[]], [[]], [0])
    with pytest.raises(ValueError, match="prev: every word needs at least one id"):
        eng.stream_agree([[]], [[[]]], [[]], [[]], [0])
    s, c, e = eng.stream_agree([], [], [], [], [])
    assert len(s) == len(c) == len(e) == 0
    # a context without a table: a state error that says so
    cfg, sd = checkpoint("micro")
    m2 = WhisperMedusaModel(cfg, sd, device=rig[1].device, max_batch=1)
    with pytest.raises(RuntimeError, match="no vocabulary table"):
        m2.engine.stream_agree([[[1]]], [[]], [[]], [[(0, 1)]], [0])
    m2.engine.close()


# ---- 3. end to end on the micro checkpoint ---------------------------------------------------------------------------------------------------------------
KW = dict(min_chunk_s=0.2, trim_s=1.0, hard_trim_s=1.6, no_repeat_ngram_size=1, max_new_tokens=12)
SEEDS = (20, 21, 22)


@pytest.fixture(scope="module")
def vocab(rig):
    cfg, _ = rig
    tok, token_bytes = W.whole_char_tokenizer(cfg.eos_token_id)
    return tok, token_bytes


def _schedule(seed, first, step, every, ticks=14):
    """Real audio, then a chunk of exact zeros (the zero-padded buffer is then bit-identical: the second hypothesis equals the first), then more
    real audio, ``step`` samples on every ``every``-th tick, until the buffer has passed hard_trim_s."""
    clip = synth.synth_clip(seed, n_samples=4 * 16000)
    out, pos = [clip[:first], np.zeros(step, np.float32)], first
    for t in range(ticks - 2):
        if t % every == 0:
            out.append(clip[pos: pos + step]); pos += step
        else:
            out.append(None)
    return out


SCHEDULES = [_schedule(SEEDS[0], 8000, 4000, 1), _schedule(SEEDS[1], 6400, 6400, 2), _schedule(SEEDS[2], 9600, 3200, 1)]


@pytest.fixture(scope="module")
def reference(rig, vocab):
    """drive_ref's run of every schedule, computed once: one session and one one-clip generate() per tick."""
    _, m = rig
    tok, token_bytes = vocab
    return [SR.drive_ref(m, token_bytes, s, tokenizer=tok, **KW) for s in SCHEDULES]


def _feed_all(m, tok, schedules, n=None, **kw):
    ss = m.stream_sessions(n or len(schedules), tokenizer=tok, **kw)
    calls, per_tick = [0], []
    orig = m.generate

    def counted(*a, **k):
        calls[0] += 1
        return orig(*a, **k)
    m.generate = counted
    try:
        got = [[] for _ in schedules]
        for t in range(len(schedules[0])):
            before = calls[0]
            res = ss.feed([s[t] for s in schedules] + [None] * (ss.n - len(schedules)))
            per_tick.append((calls[0] - before, ss.last_stats["n_due"], dict(ss.last_stats)))
            for k in range(len(schedules)):
                got[k].append(res[k])
    finally:
        del m.generate
    return ss, got, per_tick


def test_three_sessions_at_different_rates_equal_the_reference_driver(rig, vocab, reference):
    _, m = rig
    tok, _ = vocab
    # conditions on the reference driver's run, not on the code under test
    cuts = 0
    for k, ref in enumerate(reference):
        words = [w for r in ref for w in r["committed"]]
        offs = sorted({r["offset_s"] for r in ref})
        cuts += len(offs) - 1
        print(f"  session {k}: {len(words)} words committed {[w['text'] for w in words][:6]}, offsets {offs}, decodes {sum(r['decoded'] for r in ref)}")
        assert len(words) >= 1, k
    assert cuts >= 1
    ss, got, per_tick = _feed_all(m, tok, SCHEDULES, **KW)
    for k in range(3):
        for t, (g, r) in enumerate(zip(got[k], reference[k])):
            assert g == r, (k, t, g, r)
    # one generate() call and one agreement launch per tick, whatever the number of sessions that are due
    assert all(c == (1 if due else 0) for c, due, _ in per_tick) and max(due for _, due, _ in per_tick) == 3
    assert all(st["ms_agree"] > 0 and st["ms_generate"] > 0 and st["batches"] == 1 for _, due, st in per_tick if due)
    assert ss.transcript(0) == "".join(w["text"] for r in reference[0] for w in r["committed"]).strip()


def test_a_session_alone_and_among_eight_commits_the_same_stream(rig, vocab, reference):
    _, m = rig
    tok, _ = vocab
    _, alone, _ = _feed_all(m, tok, SCHEDULES[:1], **KW)
    others = [_schedule(30 + k, 8000, 4000 + 800 * k, 1 + k % 2) for k in range(7)]
    _, eight, per_tick = _feed_all(m, tok, SCHEDULES[:1] + others, **KW)
    assert max(due for _, due, _ in per_tick) == 8 and all(c <= 1 for c, _, _ in per_tick)
    assert alone[0] == eight[0] == reference[0]


def test_keywords_reach_the_decode_and_words_carry_probabilities(rig, vocab):
    _, m = rig
    tok, token_bytes = vocab
    kw = dict(KW, vanilla=True, return_token_logprobs=True)
    _, got, _ = _feed_all(m, tok, SCHEDULES, **kw)
    words = [w for s in got for r in s for w in r["committed"]]
    assert words and all(0.0 < w["probability"] <= 1.0 for w in words)
    assert all("probability" in w for s in got for r in s for w in r["pending"])
    assert got[1] == SR.drive_ref(m, token_bytes, SCHEDULES[1], tokenizer=tok, **kw)
