"""Word timestamps (return_word_timestamps) without a GPU: the restated contract of tests/words_ref.py against transformers'
_combine_tokens_into_words on the seeded list in both modes, the classes that list has to hold, the pinned whitespace set, the off-domain rule, the
vocabulary table, the route through generate() over an engine double whose word_spans IS the restatement, and the surface (header, export, ABI)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import words_ref as W
from test_merge_cpu import EN, SCRIPT, STRIDE_S, _cfg, _padded, _prompt, _StrideEng, _strided, _ts
from test_topk_cpu import _feats, _model
from whisper_medusa import words as WD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOK, TOKEN_BYTES, N_TEXT = W.byte_level_whisper_tokenizer()
CASES = W.seeded_cases(TOKEN_BYTES)
MODES = ((W.SPACES, "english"), (W.UNICODE, "chinese"))


# ---- the restatement against transformers -------------------------------------------------------------------------------------------------------
def test_every_case_is_inside_the_domain():
    for ids in CASES:
        b = b"".join(TOKEN_BYTES[t] for t in ids)
        assert "�" not in b.decode("utf-8")            # strict: raises on invalid UTF-8


def test_restatement_equals_transformers_on_every_case_in_both_modes():
    words = multi = 0
    for n, ids in enumerate(CASES):
        for mode, lang in MODES:
            wf = W.word_first_ref(TOKEN_BYTES, ids, mode)
            texts, idx = W.hf_words(TOK, ids, lang)
            assert [i[0] for i in idx] + [len(ids)] == wf and [t for i in idx for t in i] == list(range(len(ids))), (n, mode)
            assert texts == W.word_texts(TOKEN_BYTES, ids, wf), (n, mode)
            words += len(idx)
            multi += sum(len(i) > 1 for i in idx)
    print(f"{len(CASES)} rows x 2 modes: {words} words, {multi} of several tokens")
    assert multi > 1000


def test_case_list_holds_every_class():
    """On transformers alone: at least 5 rows of every class the issue names."""
    total = {}
    for ids in CASES:
        for _, lang in MODES:
            for k in W.case_classes(TOK, ids, lang):
                total[k] = total.get(k, 0) + 1
    print("classes:", total)
    assert all(total.get(k, 0) >= 5 for k in W.CLASSES), total


def test_times_and_logprobs_of_the_restatement_against_collate_word_timestamps():
    rng = np.random.default_rng(3)
    for ids in CASES[::40]:
        t = np.cumsum(rng.random(len(ids) + 1)).astype(np.float32)
        pairs = [(float(t[k]), float(t[k + 1])) for k in range(len(ids))]
        lp = -rng.random(len(ids)).astype(np.float32)
        for mode, lang in MODES:
            wf, wt, wl = W.word_spans_ref(TOKEN_BYTES, ids, mode, pairs, lp)
            hf = W.hf_words(TOK, ids, lang, pairs)
            assert [tuple(float(x) for x in row) for row in wt] == [w["timestamp"] for w in hf]
            assert wl.dtype == np.float32 and all(abs(float(wl[w]) - float(np.mean(lp[wf[w]: wf[w + 1]], dtype=np.float64))) < 1e-5 for w in range(len(wf) - 1))


# ---- strip() and the off-domain rule ----------------------------------------------------------------------------------------------------------------
def test_isspace_set_is_pythons():
    assert list(W.ISSPACE) == [c for c in range(0x110000) if chr(c).isspace()]
    for s in (" a　", " \t", " x  ", "", " .  ", "a b"):
        assert W.strip_bytes(s.encode()) == s.strip().encode()
    assert str(list(W.PUNCT.decode())) and W.PUNCT.decode() == "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"


def test_off_domain_rows_follow_the_restatement():
    i = {b: t for t, b in reversed(list(enumerate(TOKEN_BYTES)))}
    the, dot, sp = i[b" the"], i[b"."], i[b" "]
    e3, x80, x82 = i[b"\xe3"], i[b"\x80"], i[b"\x82"]
    # a truncated character at the very end: the tokens left over are a last piece of their own (appended to " the": no space, no punctuation)
    assert W.word_first_ref(TOKEN_BYTES, [the, dot, the, e3, x80], W.SPACES) == [0, 2, 5]
    # on characters the truncated "。" (E3 80) is a word of its own, and as a substring of the append set, on bytes, it joins " the" all the same;
    # a truncated emoji (F0 9F) is in no set and stays apart
    assert W.word_first_ref(TOKEN_BYTES, [the, dot, the, e3, x80], W.UNICODE) == [0, 2, 5]
    assert W.word_first_ref(TOKEN_BYTES, [the, dot, the, i[b"\xf0"], i[b"\x9f"]], W.UNICODE) == [0, 2, 3, 5]
    assert W.word_first_ref(TOKEN_BYTES, [the, dot, the, i[b"\xf0"], i[b"\x9f"]], W.SPACES) == [0, 2, 5]
    assert W.word_texts(TOKEN_BYTES, [the, e3, x80], [0, 3]) == [" the�"]
    # the same bytes closed: "。" joins the word in front of it
    assert W.word_first_ref(TOKEN_BYTES, [the, e3, x80, x82], W.SPACES) == [0, 4]
    # a lone continuation byte: no piece closes behind it, everything that follows is one piece
    assert W.word_first_ref(TOKEN_BYTES, [the, x80, sp, the, dot], W.SPACES) == [0, 5]
    assert W.word_first_ref(TOKEN_BYTES, [x80, the], W.UNICODE) == [0, 2]
    # a truncated prefix of "“" (E2 80) behind a space is still a substring of the prepend set, on bytes; as the last word it is never tested
    assert W.word_first_ref(TOKEN_BYTES, [the, sp, i[b"\xe2"], x80], W.SPACES) == [0, 1, 4]


# ---- the kernel's arithmetic, built for the host ------------------------------------------------------------------------------------------------------
def test_host_build_of_the_kernels_walk_equals_the_restatement_on_and_off_the_domain(tmp_path):
    """csrc/wm_words.h is plain C++: the walk k_word_spans runs per row, compiled by the host compiler (tests/words_host.cpp), against the
    restatement on the seeded list in both modes and on rows outside the domain (random ids over the whole table, random bytes)."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "words_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "whisper-medusa_amd", "csrc"), os.path.join(ROOT, "tests", "words_host.cpp"), "-o", exe],
                   check=True)
    rows = [(ids, m) for ids in CASES for m in (W.SPACES, W.UNICODE)]
    rng = np.random.default_rng(5)
    hot = [0x20, 0xC2, 0xA0, 0xE2, 0x80, 0x9C, 0xE3, 0x82, 0x81, 0x9F, 0x2E, 0x61, 0x28, 0xF0, 0x9F, 0x98, 0x85, 0xE1, 0x9A, 0x22, 0xEF, 0xBC, 0x8C, 300, 270, 280]
    for k in range(3000):
        n = int(rng.integers(0, 30))
        rows.append(([int(x) for x in (rng.integers(0, N_TEXT, n) if k % 2 else rng.choice(hot, n))], int(k % 3 == 0)))
    rows.append(([int(x) for x in rng.integers(0, N_TEXT, 3000)], W.SPACES))
    off = np.cumsum([0] + [len(b) for b in TOKEN_BYTES])
    blob = b"".join(TOKEN_BYTES)
    first = np.cumsum([0] + [len(r[0]) for r in rows])
    data = [N_TEXT, len(blob)] + list(off) + list(blob) + [len(rows)] + list(first) + [m for _, m in rows] + [t for r, _ in rows for t in r]
    np.asarray(data, dtype=np.int32).tofile(str(tmp_path / "in.bin"))
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.txt")], check=True)
    lines = open(tmp_path / "out.txt").read().splitlines()
    assert len(lines) == len(rows)
    for n, ((ids, mode), line) in enumerate(zip(rows, lines)):
        assert [int(x) for x in line.split()] == W.word_first_ref(TOKEN_BYTES, ids, mode), (n, mode, [TOKEN_BYTES[t] for t in ids][:20])


# ---- the vocabulary table -----------------------------------------------------------------------------------------------------------------------------
def test_word_table_from_tokenizer_is_the_tokenizers_decode():
    t = WD.WordTable.from_tokenizer(TOK, N_TEXT)
    assert t.n_text == N_TEXT == TOK.eos_token_id and t.token_bytes == TOKEN_BYTES
    assert WD.WordTable.from_tokenizer(TOK).token_bytes == TOKEN_BYTES            # n_text defaults to eos_token_id
    for i in range(N_TEXT):
        assert t.token_bytes[i].decode("utf-8", "replace") == TOK.decode([i]), i
    assert t.offsets.dtype == np.int32 and t.offsets[0] == 0 and t.offsets[-1] == len(t.blob) and t.blob.dtype == np.uint8
    assert bytes(t.blob[t.offsets[300]: t.offsets[301]]) == TOKEN_BYTES[300]
    assert WD.bytes_to_unicode() == W.bytes_to_unicode()
    with pytest.raises(ValueError, match="at least one byte"):
        WD.WordTable([b"a", b""])
    with pytest.raises(ValueError, match="byte-level"):
        WD.WordTable.from_tokenizer(type("T", (), {"eos_token_id": 1, "convert_ids_to_tokens": lambda self, ids: ["a b"]})())      # a raw space is no byte-level character
    assert [WD.language_mode(l) for l in ("en", "<|zh|>", "japanese", "yue", None, "<|de|>", "Thai")] == [0, 1, 1, 1, 0, 0, 1]


# ---- the route: an engine double whose word_spans is the restatement ------------------------------------------------------------------------------------
VOCAB = {101: b" The", 102: b" qu", 103: b"ick", 104: b" (", 105: b"fox", 106: b")", 107: b",", 108: b" \xe4\xbd\xa0", 109: b"\xe5\xa5\xbd",
         201: b" a", 202: b".", 300: b" x", 301: b"y", 400: b" one", 401: b" \"", 402: b"two"}


def _table(cfg):
    return WD.WordTable([VOCAB.get(t, b"<%d>" % t) for t in range(cfg.eos_token_id)])


class _WordEng(_StrideEng):
    def set_word_table(self, blob, offsets):
        self.calls.append(("set_word_table", len(offsets) - 1))
        self.token_bytes = [bytes(blob[offsets[t]: offsets[t + 1]]) for t in range(len(offsets) - 1)]

    def word_spans(self, rows, modes, times=None, logprobs=None):
        self.calls.append(("word_spans", [list(r) for r in rows], list(modes), times, logprobs))
        self.last_words_ms = 0.25
        return [W.word_spans_ref(self.token_bytes, r, modes[k], None if times is None else times[k], None if logprobs is None else logprobs[k])
                for k, r in enumerate(rows)]


def _expect(cfg, row, tt, mode=W.SPACES, lp=None):
    """The words of one output row from the restatement, shaped by hand as the issue states them."""
    tb = _table(cfg).token_bytes
    P = len(_prompt(cfg, EN))
    out = []
    for a, z in WD.text_rows(row, P, cfg.eos_token_id):
        wf = W.word_first_ref(tb, row[a:z], mode)
        for f, s in zip(wf[:-1], wf[1:]):
            w = {"text": b"".join(tb[t] for t in row[a + f: a + s]).decode("utf-8", "replace"),
                 "timestamp": (round(float(np.float32(tt[a + f - 1])), 2), round(float(np.float32(tt[a + s - 1])), 2)), "tokens": (a + f, a + s)}
            if lp is not None:
                acc = np.float32(0)
                for k in range(a + f, a + s):
                    acc = np.float32(acc + np.float32(lp[k]))
                w["probability"] = math.exp(float(np.float32(acc / np.float32(s - f))))
            out.append(w)
    return out


def test_short_form_words_pairing_rounding_and_stats():
    cfg = _cfg()
    eng = _WordEng(cfg)
    m = _model(cfg, eng, 8)
    tab = _table(cfg)
    out = m.generate(_feats(cfg, [0, 1]), language="en", return_word_timestamps=True, word_table=tab)
    rows = out["sequences"].tolist()
    P = len(_prompt(cfg, EN))
    assert rows[0][P:] == SCRIPT[0] + [cfg.eos_token_id] and out["token_timestamps"].shape == out["sequences"].shape
    call = [c for c in eng.calls if c[0] == "word_spans"]
    assert len(call) == 1 and call[0][1] == [SCRIPT[0], SCRIPT[1]] and call[0][2] == [0, 0] and call[0][4] is None
    # the pipeline's pairing: the token at position p runs from token_timestamps[p - 1] to token_timestamps[p]
    tt = out["token_timestamps"][0].tolist()
    assert call[0][3][0].tolist() == [[np.float32(tt[p - 1]), np.float32(tt[p])] for p in range(P, P + 5)]
    for b in range(2):
        assert out["words"][b] == _expect(cfg, rows[b], out["token_timestamps"][b].tolist())
    # " The" | " quick" | " (fox": 101 | 102 103 | 104 105
    assert [w["text"] for w in out["words"][0]] == [" The", " quick", " (fox"] and [w["tokens"] for w in out["words"][0]] == [(P, P + 1), (P + 1, P + 3), (P + 3, P + 5)]
    assert out["words"][0][1]["timestamp"] == (round(_ts(0, P), 2), round(_ts(0, P + 2), 2)) and "probability" not in out["words"][0][0]
    assert m.last_stats["ms_words"] == 0.25 and [c for c in eng.calls if c[0] == "set_word_table"] == [("set_word_table", cfg.eos_token_id)]
    # the table is uploaded once per engine; with log-probabilities every word carries exp(mean)
    out = m.generate(_feats(cfg, [1]), language="en", return_word_timestamps=True, word_table=tab, return_token_logprobs=True)
    assert len([c for c in eng.calls if c[0] == "set_word_table"]) == 1
    assert out["words"][0] == _expect(cfg, out["sequences"][0].tolist(), out["token_timestamps"][0].tolist(), lp=out["token_logprobs"][0].tolist())
    assert all(0.0 < w["probability"] <= 1.0 for w in out["words"][0])


def test_without_the_keyword_nothing_changes():
    cfg = _cfg()
    eng = _WordEng(cfg)
    m = _model(cfg, eng, 8)
    out = m.generate(_feats(cfg, [0]), language="en", return_token_timestamps=True)
    assert "words" not in out and "ms_words" not in m.last_stats and not [c for c in eng.calls if c[0] in ("word_spans", "set_word_table")]
    t = m.generate(_feats(cfg, [0]), language="en", return_word_timestamps=False)
    assert isinstance(t, torch.Tensor)
    out = m.generate(_feats(cfg, [0]), language="en", return_timestamps="word", return_dict_in_generate=True)      # truthy, as before
    assert "words" not in out


def test_unicode_mode_follows_the_clips_language_and_segments_carry_their_words():
    cfg = _cfg()
    cfg.lang_to_id = {"<|en|>": 20, "<|zh|>": 22}
    eng = _WordEng(cfg)
    m = _model(cfg, eng, 8)
    out = m.generate(_feats(cfg, [2, 2]), language=["zh", "en"], return_word_timestamps=True, word_table=_table(cfg), return_segments=True)
    call = [c for c in eng.calls if c[0] == "word_spans"][0]
    assert call[2] == [W.UNICODE, W.SPACES]
    for b, mode in enumerate((W.UNICODE, W.SPACES)):
        assert out["words"][b] == _expect(cfg, out["sequences"][b].tolist(), out["token_timestamps"][b].tolist(), mode)
        assert [w for sg in out["segments"][b] for w in sg["words"]] == out["words"][b]
    # "," then " 你" "好": one word on spaces, two on characters ("好" is a piece of its own)
    assert [w["text"] for w in out["words"][1]][-1] == " 你好" and [w["text"] for w in out["words"][0]][-2:] == [" 你", "好"]


def test_strided_route_is_one_row_per_clip_with_absolute_times():
    cfg = _cfg()
    eng = _WordEng(cfg)
    m = _model(cfg, eng, 8)
    out = m.generate(_strided(cfg, [[0, 1, 2], [9, 9, 9]]), chunk_longform=True, stride_length_s=STRIDE_S, language="en",
                     return_word_timestamps=True, word_table=_table(cfg))
    call = [c for c in eng.calls if c[0] == "word_spans"]
    assert len(call) == 1 and call[0][1][0] == list(range(101, 110))
    for b in range(2):
        assert out["words"][b] == _expect(cfg, out["sequences"][b].tolist(), out["token_timestamps"][b].tolist())
    assert "window_keep" in out and m.last_stats["ms_words"] == 0.25 and "ms_merge" in m.last_stats
    # the unstrided chunked route: the windows' texts back to back are one row
    eng.calls.clear()
    f = torch.zeros(1, cfg.num_mel_bins, 2 * 192)
    f[:, :, 192:] = 2.0
    out = m.generate(f, chunk_longform=True, language="en", return_word_timestamps=True, word_table=_table(cfg))
    assert [c for c in eng.calls if c[0] == "word_spans"][0][1] == [SCRIPT[0] + SCRIPT[2]]
    assert out["words"][0] == _expect(cfg, out["sequences"][0].tolist(), out["token_timestamps"][0].tolist())


def test_refusals():
    cfg = _cfg()
    m = _model(cfg, _WordEng(cfg), 8)
    f = _feats(cfg, [0])
    with pytest.raises(ValueError, match="tokenizer="):
        m.generate(f, language="en", return_word_timestamps=True)
    with pytest.raises(ValueError, match="return_token_timestamps=False"):
        m.generate(f, language="en", return_word_timestamps=True, word_table=_table(cfg), return_token_timestamps=False)
    # what return_token_timestamps refuses stays refused, under the same messages
    with pytest.raises(NotImplementedError, match="return_token_timestamps is not supported together with sequential_longform"):
        m.generate(f, language="en", return_word_timestamps=True, word_table=_table(cfg), sequential_longform=True, return_timestamps=True)
    with pytest.raises(NotImplementedError, match="return_token_timestamps is not supported together with logits_processor="):
        m.generate(f, language="en", return_word_timestamps=True, word_table=_table(cfg), logits_processor=[lambda i, s: s])
    cfg2 = _cfg()
    cfg2.alignment_heads = None
    m2 = _model(cfg2, _WordEng(cfg2), 8)
    with pytest.raises(Exception) as e1:
        m2.generate(f, language="en", return_token_timestamps=True)
    with pytest.raises(type(e1.value), match=re.escape(str(e1.value))):
        m2.generate(f, language="en", return_word_timestamps=True, word_table=_table(cfg2))


# ---- surface ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_export_and_abi(built_lib):
    import build as wm_build
    from whisper_medusa import engine
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert "int wm_set_word_table(wm_ctx* ctx, const uint8_t* bytes" in hdr and "int wm_word_spans(wm_ctx* ctx, int R, const int32_t* first /* HOST [R+1] */" in hdr
    assert "#define WM_WORDS_ROWS_MAX    65536" in hdr and "#define WM_WORDS_IDS_MAX     (4 << 20)" in hdr and "#define WM_ABI_VERSION 9" in hdr
    assert "_combine_tokens_into_words" in hdr and "_merge_punctuations" in hdr
    assert "wm_words.hip" in wm_build.SOURCES and "wm_set_word_table" in engine.EXPORTS and "wm_word_spans" in engine.EXPORTS
    assert (engine.WORDS_SPACES, engine.WORDS_UNICODE) == (W.SPACES, W.UNICODE) == (WD.SPACES, WD.UNICODE) == (0, 1)
    assert (engine.WORDS_ROWS_MAX, engine.WORDS_IDS_MAX) == (65536, 4 << 20) and engine.WM_ABI_VERSION == 9
    for f16 in (False, True):
        lib = engine.load_library(act_fp16=f16)
        assert lib.wm_abi_version() == 9 and lib.wm_word_spans.restype is not None and lib.wm_set_word_table.restype is not None
    assert callable(engine.Engine.word_spans) and callable(engine.Engine.set_word_table)
    src = open(os.path.join(ROOT, "whisper-medusa_amd", "csrc", "wm_words.hip")).read()
    assert "atomic" not in src.lower().replace("no atomics", "") and "k_word_spans<<<dim3(R), dim3(256)" in src
