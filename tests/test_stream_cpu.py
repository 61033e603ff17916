"""Live transcription (stream_sessions) without a GPU: the two restatements of the agreement policy in tests/stream_ref.py against
each other on the seeded list, the classes that list has to hold, the host build of the kernel's arithmetic (csrc/wm_stream.h) under the address
and undefined-behaviour sanitizers, the session layer over a model double whose stream_agree IS the restatement and whose generate() is scripted
from the audio it is handed, and the surface (header, export, sources, ABI)."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import stream_ref as SR
import words_ref as W
from whisper_medusa import streaming as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOK, TOKEN_BYTES, N_TEXT = W.byte_level_whisper_tokenizer()
CASES = SR.seeded_cases(TOKEN_BYTES)
REF = [SR.agree_ref(TOKEN_BYTES, c["new"], c["prev"], c["tail"], c["times"], c["last_cs"]) for c in CASES]


# ---- the two restatements ---------------------------------------------------------------------------------------------------------------------------
def test_four_steps_equal_the_list_popping_formulation_on_ordered_cases():
    n = 0
    for c, r in zip(CASES, REF):
        st = [t[0] for t in c["times"]]
        if all(a <= b for a, b in zip(st, st[1:])):
            assert SR.buffer_ref(TOKEN_BYTES, c) == r[:2], c
            n += 1
    print(f"{n} of {len(CASES)} cases with non-decreasing starts; commits {sum(r[1] for r in REF)}, enders {sum(r[2] >= 0 for r in REF)}")
    assert n > 350 and len(CASES) >= 257


def test_case_list_holds_every_class():
    total = {}
    for c in CASES:
        for k in SR.case_classes(TOKEN_BYTES, c):
            total[k] = total.get(k, 0) + 1
    print("classes:", total)
    assert all(total.get(k, 0) >= 1 for k in SR.CLASSES), [k for k in SR.CLASSES if not total.get(k)]


def test_the_boundaries_by_hand():
    i = {b: t for t, b in reversed(list(enumerate(TOKEN_BYTES)))}
    hel, lo, hello, sp = [i[b" "], i[b"h"], i[b"e"], i[b"l"]], [i[b"l"], i[b"o"]], [i[b" hello"]], [i[b" "]]
    plain = [i[b"h"], i[b"e"], i[b"l"], i[b"l"], i[b"o"]]
    assert SR.key(TOKEN_BYTES, hel + lo) == SR.key(TOKEN_BYTES, hello) == SR.key(TOKEN_BYTES, plain) == b"hello" and SR.key(TOKEN_BYTES, sp + sp) == b""
    a = lambda *k, **kw: SR.agree_ref(TOKEN_BYTES, *k, **kw)                        # noqa: E731
    the = [i[b" the"]]
    # late: start == last - late is dropped, one centisecond later is kept
    assert a([hello, the], [the], [], [(90, 95), (300, 310)], 100) == (1, 1, -1)
    assert a([hello, the], [the], [], [(91, 95), (300, 310)], 100) == (0, 0, -1)
    # near: the overlap with the tail is removed at |d| = near - 1 and not at near
    assert a([hello, the], [the], [plain], [(199, 210), (300, 310)], 100) == (1, 1, -1)
    assert a([hello, the], [the], [plain], [(200, 210), (300, 310)], 100) == (0, 0, -1)
    assert a([hello, the], [the], [plain], [(150, 160), (300, 310)], 100, max_ngram=1, near_cs=51, late_cs=0) == (1, 1, -1)
    assert a([hello, the], [the], [plain], [(150, 160), (300, 310)], 100, max_ngram=1, near_cs=50, late_cs=0) == (0, 0, -1)
    dot = [i[b" the"], i[b"."]]
    assert a([hello, dot, hello], [plain, dot, sp], [], [(300, 310), (320, 330), (340, 350)], 100) == (0, 2, 1)
    assert a([hello, dot + [i[b"\""]]], [plain, dot + [i[b"\""]]], [], [(300, 310), (320, 330)], 100) == (0, 2, -1)


# ---- the kernel's arithmetic, built for the host --------------------------------------------------------------------------------------------------------
def test_host_build_of_the_kernels_arithmetic_equals_the_restatement_under_sanitizers(tmp_path):
    """csrc/wm_stream.h is plain C++: the functions k_stream_agree runs per session, compiled by the host compiler into a stand-alone program
    (tests/stream_host.cpp) with -fsanitize=address,undefined, on one lane and as the shares of 256 lanes reduced the way the block reduces."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "stream_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "whisper-medusa_amd", "csrc"), os.path.join(ROOT, "tests", "stream_host.cpp"), "-o", exe], check=True)
    SR.pack_cases(TOKEN_BYTES, CASES).tofile(str(tmp_path / "in.bin"))
    for lanes in (1, 256, 64):
        subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.txt"), str(lanes)], check=True)
        got = [tuple(int(x) for x in line.split()) for line in open(tmp_path / "out.txt").read().splitlines()]
        assert len(got) == len(CASES)
        for n, (g, r) in enumerate(zip(got, REF)):
            assert g == r, (lanes, n, g, r)
    assert {len(c["new"]) for c in CASES} >= set(SR.EDGES)


# ---- the session layer over a double ----------------------------------------------------------------------------------------------------------------------
WORD_CS = 20                                                # every spoken word lasts 20 cs = 3200 samples
WORD_N = WORD_CS * SR.HOP
F = 192                                                     # the micro shape's window: 1.92 s
WIN = F * SR.HOP
VOCAB = [b"<%d>" % t for t in range(400)]
for _k in range(100):
    VOCAB[100 + _k] = b" w%d" % _k + (b"." if _k % 5 == 4 else b"")              # every fifth word ends a sentence
    VOCAB[200 + _k] = b" ~%d" % _k                                               # a word heard in part: unstable
VOCAB[300] = b"s"


def recording(seed, n_words=60):
    """A recording in which word k is 3200 samples of the value (k + 1) / 1000 (+ the recording's own 0.1 * seed): the scripted generate() reads
    the words, and their times, back from the audio it is handed."""
    x = np.repeat((np.arange(n_words) + 1) / 1000.0 + 0.1 * seed, WORD_N).astype(np.float32)
    return x


class _Eng:
    def __init__(self):
        self.calls = []

    def stream_agree(self, new, prev, tail, times, last_cs, late_cs=10, near_cs=100, max_ngram=5):
        self.calls.append(dict(new=new, prev=prev, tail=tail, times=times, last_cs=list(last_cs), late_cs=late_cs, near_cs=near_cs))
        self.last_stream_ms = 0.5
        r = [SR.agree_ref(VOCAB, new[s], prev[s], tail[s], times[s], last_cs[s], late_cs, near_cs, max_ngram) for s in range(len(new))]
        return tuple(np.asarray([x[k] for x in r], dtype=np.int32) for k in range(3))


class _Model:
    """The five things the layer touches.  extract_features hands the audio through; generate() finds the runs of equal samples in every row."""

    def __init__(self):
        self.config = types.SimpleNamespace(n_mel_frames=F, eos_token_id=399)
        self.device = torch.device("cpu")
        self.engine = _Eng()
        self.gen_calls, self.feat_calls = [], []

    def extract_features(self, wav):
        wav = torch.as_tensor(np.asarray(wav)) if not isinstance(wav, torch.Tensor) else wav
        self.feat_calls.append(wav.clone())
        return wav.clone()

    def generate(self, feats, **kw):
        self.gen_calls.append((int(feats.shape[0]), dict(kw)))
        assert kw.get("return_word_timestamps") is True and feats.shape[1] == WIN
        rows, words = [], []
        for x in feats.numpy():
            row, ws = [1, 2, 3], []
            cut = np.flatnonzero(np.diff(x) != 0) + 1
            for a, z in zip(np.concatenate([[0], cut]), np.concatenate([cut, [len(x)]])):
                if x[a] == 0:
                    continue
                k = int(round((float(x[a]) % 0.1) * 1000)) - 1
                ids = [100 + k % 100] + ([300] if k % 3 == 0 else []) if z - a == WORD_N else [200 + ((z - a) // SR.HOP) % 100]
                w = {"text": b"".join(VOCAB[t] for t in ids).decode(), "timestamp": (round(a / 16000, 2), round(z / 16000, 2)), "tokens": (len(row), len(row) + len(ids))}
                if kw.get("return_token_logprobs"):
                    w["probability"] = 0.5
                row += ids
                ws.append(w)
            rows.append(row + [399])
            words.append(ws)
        T = max(len(r) for r in rows)
        return {"sequences": torch.tensor([r + [399] * (T - len(r)) for r in rows]), "words": words}


def _sessions(n, model=None, **kw):
    m = model or _Model()
    kw.setdefault("word_table", object())
    return m, ST.StreamSessions(m, n, **kw)


def _truth(k, seed=0):
    ids = [100 + k % 100] + ([300] if k % 3 == 0 else [])
    return {"text": b"".join(VOCAB[t] for t in ids).decode(), "timestamp": (k * WORD_CS / 100.0, (k + 1) * WORD_CS / 100.0), "ids": ids}


def test_committed_words_are_append_only_and_on_the_recordings_clock_across_trims():
    m, ss = _sessions(1, min_chunk_s=0.3)
    rec = recording(0)
    assert ss.trim_cs == 96 and ss.hard_trim_cs == 160 and ss.window == WIN
    got, offsets, text = [], [0.0], ""
    for t in range(0, 40 * WORD_N, 4800):
        r = ss.feed([rec[t: t + 4800]])[0]
        assert r["decoded"] and len(m.gen_calls) == t // 4800 + 1
        got += r["committed"]
        assert got == [_truth(k) for k in range(len(got))]                         # in order, each with its true time on the recording's clock
        assert ss.transcript(0).startswith(text) and ss.committed_words(0) == got
        text = ss.transcript(0)
        if r["offset_s"] != offsets[-1]:
            offsets.append(r["offset_s"])
        # whole centiseconds, the buffer is the recording from the offset on, and everything behind it is exactly zero
        s = ss.s[0]
        assert r["offset_s"] == s.offset_cs / 100.0 and r["buffer_s"] == s.length / 16000.0 and r["lost_s"] == 0.0
        o = s.offset_cs * SR.HOP
        assert o + s.length == t + 4800 and np.array_equal(ss.buf[0, : s.length].numpy(), rec[o: o + s.length])
        assert not ss.buf[0, s.length:].any()
        assert all(w["timestamp"][0] >= got[-1]["timestamp"][1] for w in r["pending"]) if got else True
    print(f"{len(got)} words committed, offsets {offsets}")
    assert len(got) >= 30 and len(offsets) >= 3                                    # at least two trims
    # every cut is at the end of a committed word, in whole centiseconds: 1.0 behind " w4." (a sentence end); " w9.s" is none, so the buffer grows
    # past hard_trim_s and is cut behind the last committed word, at 2.4
    assert all(round(o * 100) % WORD_CS == 0 for o in offsets) and offsets[:3] == [0.0, 1.0, 2.4]
    assert m.engine.calls[-1]["late_cs"] == 10 and m.engine.calls[-1]["near_cs"] == 100
    assert ss.last_stats["n_due"] == 1 and ss.last_stats["batches"] == 1 and ss.last_stats["ms_agree"] == 0.5
    assert ss.last_stats["ms_feed"] >= ss.last_stats["ms_generate"] > 0


def test_the_tail_holds_only_committed_words_still_in_the_buffer():
    m, ss = _sessions(1, min_chunk_s=0.3)
    rec = recording(0)
    shorter = off = 0
    for t in range(0, 40 * WORD_N, 4800):
        before = ss.committed_words(0)
        r = ss.feed([rec[t: t + 4800]])[0]
        want = [w["ids"] for w in before[-5:] if round(w["timestamp"][1] * 100) > off]       # off: where the buffer began when it was decoded
        assert m.engine.calls[-1]["tail"][0] == want, (t, m.engine.calls[-1]["tail"][0], want)
        shorter += len(want) < min(5, len(before))
        off = round(r["offset_s"] * 100)
    assert shorter > 0


def test_feed_equals_the_one_session_reference_driver_under_trims_and_overflow():
    """Three sessions at different rates — one of them with chunks so large that the window overflows before anything is committed — against
    stream_ref.drive_ref, one session and one one-clip generate() at a time."""
    kw = dict(min_chunk_s=0.25, trim_s=1.0, hard_trim_s=1.5)
    m, ss = _sessions(3, **kw)
    recs = [recording(s) for s in range(3)]
    steps = [[4000] * 40, [1600, 0, 7000, 0, 0] * 8, [20000, 17000, 30000, 30720, 500, 9000] * 2]
    sched = []
    for s in range(3):
        pos, out = 0, []
        for n in steps[s]:
            out.append(recs[s][pos: pos + n] if n else None)
            pos += n
        sched.append(out)
    T = max(len(x) for x in sched)
    sched = [x + [None] * (T - len(x)) for x in sched]
    got = [[] for _ in range(3)]
    for t in range(T):
        calls = len(m.gen_calls)
        res = ss.feed([sched[s][t] for s in range(3)])
        assert len(m.gen_calls) - calls == (1 if any(r["decoded"] for r in res) else 0)
        for s in range(3):
            got[s].append(res[s])
    lost = trims = 0
    for s in range(3):
        want = SR.drive_ref(_Model(), VOCAB, sched[s], word_table=object(), **kw)
        assert got[s] == want, s
        lost += want[-1]["lost_s"] > 0
        trims += len({r["offset_s"] for r in want}) - 1
        assert sum(len(r["committed"]) for r in want) > 0
        for r in want:                                                              # and on the true clock, whatever was cut
            for w in r["committed"]:
                k = round(w["timestamp"][0] * 100) // WORD_CS
                assert w["ids"][0] >= 200 or w == _truth(k), w                      # (a word the cut left in part is not a word of the recording)
    print(f"lost in {lost} sessions, {trims} cuts")
    assert lost >= 1 and trims >= 4
    # the overflow rule by hand: nothing committed, 36000 samples into a window of 30720: the cut is at ceil(5280 / 160) = 33 cs, all of it lost
    m, ss = _sessions(1, min_chunk_s=100.0)
    for t in range(3):
        r = ss.feed([recs[0][12000 * t: 12000 * (t + 1)]])[0]
    assert not r["decoded"] and r["lost_s"] == 0.33 and r["offset_s"] == 0.33 and r["buffer_s"] == 1.92 and not m.gen_calls
    assert np.array_equal(ss.buf[0].numpy(), recs[0][5280: 36000])


def test_due_rule_and_one_generate_call_per_tick():
    m, ss = _sessions(4, min_chunk_s=0.5, max_batch=8)
    recs = [recording(s) for s in range(4)]
    res = ss.feed([recs[0][:4000], None, recs[2][:7999], np.zeros(0, np.float32)])
    assert not m.gen_calls and not m.engine.calls and [r["decoded"] for r in res] == [False] * 4 and ss.last_stats["n_due"] == 0
    assert [r["buffer_s"] for r in res] == [0.25, 0.0, 7999 / 16000, 0.0] and ss.last_stats["batches"] == 0 and ss.last_stats["ms_agree"] == 0.0
    res = ss.feed([recs[0][4000:8000], None, recs[2][7999:8000], None])            # both reach 8000 samples: one batch of two
    assert [r["decoded"] for r in res] == [True, False, True, False] and [c[0] for c in m.gen_calls] == [2] and len(m.engine.calls) == 1
    assert len(m.engine.calls[0]["new"]) == 2 and ss.last_stats["n_due"] == 2 and ss.last_stats["batches"] == 1
    res = ss.feed([recs[0][8000:9000], recs[1][:8000], None, None])                # session 0 is not due again yet
    assert [r["decoded"] for r in res] == [False, True, False, False] and [c[0] for c in m.gen_calls] == [2, 1]
    res = ss.feed([recs[s][16000:24000] for s in range(4)])                        # all four at once: still one call
    assert all(r["decoded"] for r in res) and [c[0] for c in m.gen_calls] == [2, 1, 4] and len(m.engine.calls) == 3
    # the keywords reach every generate() call unchanged
    m, ss = _sessions(3, min_chunk_s=0.5, max_batch=2, language="en", max_new_tokens=12, vanilla=True, no_repeat_ngram_size=1, hotwords=["x"], prompt_ids=[7])
    res = ss.feed([recs[s][:8000] for s in range(3)])                              # more than max_batch: two calls, one agreement call
    assert [c[0] for c in m.gen_calls] == [2, 1] and len(m.engine.calls) == 1 and len(m.engine.calls[0]["new"]) == 3 and ss.last_stats["batches"] == 2
    for _, kw in m.gen_calls:
        assert kw == dict(language="en", max_new_tokens=12, vanilla=True, no_repeat_ngram_size=1, hotwords=["x"], prompt_ids=[7], return_word_timestamps=True,
                          word_table=kw["word_table"])
    a = ss.feed([recs[s][8000:16000] for s in range(3)])
    one = _sessions(1, min_chunk_s=0.5)[1]
    one.feed([recs[2][:8000]])
    assert a[2] == one.feed([recs[2][8000:16000]])[0] and len(a[2]["committed"]) > 0       # the group a session falls into changes nothing
    # probabilities ride along
    m, ss = _sessions(1, min_chunk_s=0.5, return_token_logprobs=True)
    ss.feed([recs[0][:8000]])
    r = ss.feed([recs[0][8000:16000]])[0]
    assert r["committed"] and all(w["probability"] == 0.5 for w in r["committed"] + r["pending"])


def test_finish_and_reset():
    m, ss = _sessions(2, min_chunk_s=0.5)
    recs = [recording(s) for s in range(2)]
    for t in range(2):
        res = ss.feed([recs[s][8000 * t: 8000 * (t + 1)] for s in range(2)])
    assert all(r["committed"] and r["pending"] for r in res)
    text, calls = ss.transcript(1), len(m.gen_calls)
    assert text == "".join(w["text"] for w in ss.committed_words(1)).strip() and text == "w0s w1"
    out = ss.finish(1)
    assert out == [res[1]["pending"]] and len(m.gen_calls) == calls                # as they stand, no decode
    assert ss.transcript(1) == "" and ss.s[1].length == 0 and ss.s[1].offset_cs == 0 and not ss.buf[1].any() and ss.buf[0].any()
    assert ss.transcript(0) != "" and ss.s[0].pending
    r = ss.feed([None, recs[1][:8000]])[1]                                         # a fresh session: its clock starts again
    assert r["decoded"] and r["offset_s"] == 0.0 and not r["committed"] and r["pending"][0]["timestamp"] == (0.0, 0.2)
    ss.reset([0])
    assert ss.transcript(0) == "" and not ss.s[0].pending and not ss.buf[0].any() and ss.s[1].pending
    assert ss.finish() == [[], [w for w in r["pending"]]] and not ss.buf.any()
    with pytest.raises(IndexError):
        ss.reset(2)


def test_refusals_name_their_keyword():
    for kw, word in ((dict(streamer=object()), "streamer"), (dict(num_beams=2), "num_beams"), (dict(num_return_sequences=2), "num_return_sequences"),
                     (dict(return_timestamps=True), "return_timestamps"), (dict(sequential_longform=True), "sequential_longform"),
                     (dict(chunk_longform=True), "chunk_longform"), (dict(vad_longform=True), "vad_longform")):
        with pytest.raises(NotImplementedError, match="stream_sessions: " + word):
            _sessions(1, **kw)
    _sessions(1, num_beams=1, num_return_sequences=1, return_timestamps=False, chunk_longform=False)       # not requests
    with pytest.raises(ValueError, match=re.escape("return_word_timestamps=True needs the bytes of the vocabulary: pass tokenizer= (or word_table=)")):
        ST.StreamSessions(_Model(), 1)
    with pytest.raises(ValueError, match="n must be at least 1"):
        _sessions(0)
    m, ss = _sessions(2)
    x = np.zeros(100, np.float32)
    with pytest.raises(ValueError, match="sampling_rate=8000"):
        ss.feed([x, x], sampling_rate=8000)
    with pytest.raises(ValueError, match="1-D"):
        ss.feed([x, np.zeros((2, 100), np.float32)])
    with pytest.raises(ValueError, match="feed it in pieces"):
        ss.feed([x, np.zeros(WIN + 1, np.float32)])
    with pytest.raises(ValueError, match="1 chunks for 2 sessions"):
        ss.feed([x])
    assert all(s.length == 0 for s in ss.s)                                        # a refused call changed no session
    ss.feed([x, np.zeros(WIN, np.float32)])                                        # a whole window is fine
    assert [s.length for s in ss.s] == [100, WIN]


def test_the_models_door_passes_max_batch_and_the_same_refusals():
    from test_merge_cpu import _cfg
    from test_topk_cpu import _model
    cfg = _cfg()
    m = _model(cfg, _Eng(), 8)
    ss = m.stream_sessions(3, word_table=object(), min_chunk_s=0.2, max_new_tokens=12)
    assert isinstance(ss, ST.StreamSessions) and ss.max_batch == 8 and ss.n == 3 and ss.window == 160 * cfg.n_mel_frames and ss.min_chunk == 3200
    assert ss.buf.shape == (3, ss.window) and ss.buf.dtype == torch.float32 and ss.kw["max_new_tokens"] == 12
    assert (ss.trim_cs, ss.hard_trim_cs) == (ss.window // 320, 5 * (ss.window // 160) // 6)
    with pytest.raises(NotImplementedError, match="streamer"):
        m.stream_sessions(1, word_table=object(), streamer=object())
    with pytest.raises(ValueError, match="tokenizer="):
        m.stream_sessions(1)


# ---- surface ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_export_sources_and_abi(built_lib):
    import build as wm_build
    from whisper_medusa import engine
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert "int wm_stream_agree(wm_ctx* ctx, int S, const wm_stream_list* new_list" in hdr and "typedef struct wm_stream_list {" in hdr
    assert "#define WM_STREAM_TAIL          5" in hdr and "#define WM_STREAM_SESSIONS_MAX  4096" in hdr and "#define WM_ABI_VERSION 9" in hdr
    assert "#define WM_STREAM_WORDS_MAX     (1 << 20)" in hdr and "#define WM_STREAM_IDS_MAX       (4 << 20)" in hdr and "LocalAgreement-2" in hdr
    assert "wm_stream.hip" in wm_build.SOURCES and "wm_stream_agree" in engine.EXPORTS
    assert (engine.STREAM_TAIL, engine.STREAM_SESSIONS_MAX, engine.STREAM_WORDS_MAX, engine.STREAM_IDS_MAX) == (5, 4096, 1 << 20, 4 << 20)
    assert (engine.STREAM_LATE_CS, engine.STREAM_NEAR_CS) == (SR.LATE_CS, SR.NEAR_CS) == (10, 100) and ST.TAIL == SR.TAIL == engine.STREAM_TAIL
    assert engine.WM_ABI_VERSION == 9
    for f16 in (False, True):
        lib = engine.load_library(act_fp16=f16)
        assert lib.wm_abi_version() == 9 and lib.wm_stream_agree.argtypes is not None and len(lib.wm_stream_agree.argtypes) == 12
    assert callable(engine.Engine.stream_agree)
    src = open(os.path.join(ROOT, "whisper-medusa_amd", "csrc", "wm_stream.hip")).read()
    assert "atomic" not in src.lower().replace("no atomics", "") and "k_stream_agree<<<dim3(S), dim3(256)" in src
    h = open(os.path.join(ROOT, "whisper-medusa_amd", "csrc", "wm_stream.h")).read()
    assert "__host__ __device__" in h and "hip" not in h.lower().replace("__hipcc__", "").replace("wm_stream.hip", "")
    # the packing of Engine.stream_agree, without a context
    w, t, i = engine.Engine._stream_list("new", [[[1, 2], [3]], [], [[4]]])
    assert w.tolist() == [0, 2, 2, 3] and t.tolist() == [0, 2, 3, 4] and i.tolist() == [1, 2, 3, 4] and w.dtype == t.dtype == i.dtype == np.int32
    with pytest.raises(ValueError, match="at least one id"):
        engine.Engine._stream_list("prev", [[[1], []]])
