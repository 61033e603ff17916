"""Word grouping (include/wm.h wm_word_spans) in plain Python: transformers' `_combine_tokens_into_words` itself (`hf_words`),
its restatement on bytes (`word_spans_ref`: the contract the kernel is held to), a byte-level `WhisperTokenizer` built from a vocabulary made
here, and the seeded case list both test files share."""
import numpy as np

SPACES, UNICODE = 0, 1
UNICODE_LANGUAGES = ("chinese", "japanese", "thai", "lao", "myanmar", "cantonese")
PUNCT = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~".encode()
PREPEND = "\"'“¡¿([{-".encode()
APPEND = "\"'.。,，!！?？:：”)]}、".encode()
# the code points for which str.isspace() is true (tests/test_words_cpu.py pins the set against chr(c).isspace())
ISSPACE = tuple(list(range(0x09, 0x0E)) + list(range(0x1C, 0x21)) + [0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B))
                + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
_WS = tuple(chr(c).encode() for c in ISSPACE)


def strip_bytes(b: bytes) -> bytes:
    """Python's str.strip() on UTF-8 bytes: the encodings of the ISSPACE code points leave at both ends, one at a time."""
    again = True
    while again:
        again = False
        for w in _WS:
            if b.startswith(w):
                b, again = b[len(w):], True
    again = True
    while again:
        again = False
        for w in _WS:
            if b.endswith(w):
                b, again = b[: len(b) - len(w)], True
    return b


def _valid(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def word_first_ref(token_bytes, ids, mode):
    """The start indices [n_words + 1] of the words of one row, as the issue states them: pieces, words, the prepend pass, the append pass."""
    pieces, cur = [], []                                   # pieces: lists of positions
    for p, t in enumerate(ids):
        cur.append(p)
        if _valid(b"".join(token_bytes[ids[q]] for q in cur)):
            pieces.append(cur); cur = []
    if cur:
        pieces.append(cur)
    text = lambda idx: b"".join(token_bytes[ids[q]] for q in idx)
    words = []
    for pc in pieces:
        b = text(pc)
        if mode == UNICODE or b[:1] == b" " or strip_bytes(b) in PUNCT or not words:
            words.append(list(pc))
        else:
            words[-1].extend(pc)
    wt = [text(w) for w in words]
    n = len(words)
    i, j = n - 2, n - 1
    while i >= 0:
        if wt[i][:1] == b" " and strip_bytes(wt[i]) in PREPEND:
            wt[j] = wt[i] + wt[j]; words[j] = words[i] + words[j]
            wt[i] = b""; words[i] = []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < n:
        if wt[i][-1:] != b" " and wt[j] in APPEND:
            wt[i] += wt[j]; words[i] += words[j]
            wt[j] = b""; words[j] = []
        else:
            i = j
        j += 1
    words = [w for w in words if w]
    flat = [p for w in words for p in w]
    assert flat == list(range(len(ids)))
    return [w[0] for w in words] + [len(ids)]


def word_spans_ref(token_bytes, ids, mode, times=None, logprobs=None):
    """(word_first, word_times or None, word_logprobs or None) of one row; float32 throughout: a word's time is (start of its first token, end of
    its last), its log-probability the float32 sum in ascending token order divided by the count in float32."""
    wf = word_first_ref(token_bytes, [int(t) for t in ids], mode)
    nw = len(wf) - 1
    wt = wl = None
    if times is not None:
        tm = np.asarray(times, dtype=np.float32).reshape(-1, 2)
        wt = np.zeros((nw, 2), dtype=np.float32)
        for w in range(nw):
            wt[w] = (tm[wf[w], 0], tm[wf[w + 1] - 1, 1])
    if logprobs is not None:
        lp = np.asarray(logprobs, dtype=np.float32)
        wl = np.zeros(nw, dtype=np.float32)
        for w in range(nw):
            s = np.float32(0)
            for k in range(wf[w], wf[w + 1]):
                s = np.float32(s + lp[k])
            wl[w] = np.float32(s / np.float32(wf[w + 1] - wf[w]))
    return np.asarray(wf, dtype=np.int32), wt, wl


def word_texts(token_bytes, ids, word_first):
    return [b"".join(token_bytes[int(t)] for t in ids[a:b]).decode("utf-8", "replace") for a, b in zip(word_first[:-1], word_first[1:])]


def hf_words(tok, ids, language=None, token_timestamps=None):
    """transformers' own grouping: (texts, token index lists) — with `token_timestamps` [(start, end), ..] the list of `_collate_word_timestamps`."""
    from transformers.models.whisper import tokenization_whisper as tw
    ids = [int(t) for t in ids]
    if token_timestamps is not None:
        return tw._collate_word_timestamps(tok, ids, token_timestamps, language or "english", False)
    words, _, idx = tw._combine_tokens_into_words(tok, ids, language or "english")
    return words, idx


def bytes_to_unicode():
    """GPT-2's byte -> printable code point map."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b); cs.append(256 + n); n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


# multi-byte vocabulary entries beyond the 256 single bytes (a token is any byte string: decoding needs no merges)
EXTRA_TOKENS = [" the", "th", "e", "in", "ing", " a", "or", " w", " hello", " world", "  ", " (", " \"", ".\"", "。", "，", "、", "“", "”", " “", "¿", " ¡",
                "!", "?!", "...", " -", " [", "]", "你好", "世界", "。”", "　", " ", "  ", "😀", "ly", " 'n", "'s", "),", " \t", "\n", " internationalisation", "。。。！？……", ", ", "\t ", "e "]
SPECIALS = ["<|endoftext|>", "<|startoftranscript|>", "<|en|>", "<|zh|>", "<|transcribe|>", "<|notimestamps|>"]


def byte_level_whisper_tokenizer():
    """(WhisperTokenizer, token_bytes [n_text], n_text = eos_token_id): the recipe of tests/test_metrics_cpu.py with more entries."""
    from transformers import WhisperTokenizer
    b2u = bytes_to_unicode()
    vocab = {b2u[b]: b for b in range(256)}
    token_bytes = [bytes([b]) for b in range(256)]
    merges = []
    for s in EXTRA_TOKENS:
        u = "".join(b2u[b] for b in s.encode())
        for k in range(2, len(u) + 1):
            if u[:k] not in vocab:
                vocab[u[:k]] = len(vocab)
                token_bytes.append(bytes(next(b for b, c in b2u.items() if c == ch) for ch in u[:k]))
                merges.append((u[: k - 1], u[k - 1]))
    n_text = len(vocab)
    for t in SPECIALS:
        vocab[t] = len(vocab)
    tok = WhisperTokenizer(vocab=vocab, merges=merges)
    tok.add_special_tokens({"additional_special_tokens": SPECIALS[1:]})
    assert tok.eos_token_id == n_text
    return tok, token_bytes, n_text


# ---- the seeded case list -------------------------------------------------------------------------------------------------------------------------
ATOMS = ["a", "b", "e", "th", "ing", " the", " a", " w", " hello", " world", "or", "ly", " ", "  ", " \t", "\n", " ", "　", "  ", "😀",
         ".", ",", "!", "?", ":", "。", "，", "、", "！", "？", "”", "“", " “", " (", " [", " \"", " '", " -", " ¡", " ¿", "¿", ")", "]", "}", "),",
         ".\"", "。”", "'s", " 'n", "...", "你好", "世界", "é", "ß", "-", "(", "\"", "'", " internationalisation", "。。。！？……", ", ", "\t ", "e "]
CASE_SEED, N_CASES = 20261, 1200


def seeded_cases(token_bytes):
    """[ids]: rows (each is checked in both modes) drawn from ATOMS, every atom either as its longest vocabulary entries or byte by byte (so multi-byte
    characters are split across tokens); always inside the domain of equality with transformers (valid UTF-8, no U+FFFD)."""
    index = {}
    for i, b in enumerate(token_bytes):
        index.setdefault(b, i)
    longest = max(len(b) for b in token_bytes)

    def greedy(b):
        out, p = [], 0
        while p < len(b):
            for n in range(min(longest, len(b) - p), 0, -1):
                if b[p: p + n] in index:
                    out.append(index[b[p: p + n]]); p += n
                    break
        return out

    rng = np.random.default_rng(CASE_SEED)
    cases = [[] for _ in range(6)]
    for c in range(N_CASES):
        n = int(rng.choice([0, 1, 1, 2, 3, 5, 8, 13, 21, 34]))
        ids = []
        for _ in range(n):
            a = ATOMS[int(rng.integers(len(ATOMS)))].encode()
            ids += greedy(a) if rng.random() < 0.6 else [index[bytes([x])] for x in a]
        cases.append(ids)
    return cases


CLASSES = ("multi_token_word", "whitespace_piece", "prepend_run", "prepend_last", "append_refused_space", "append_into_emptied", "multi_piece_append",
           "empty_row", "one_token_row")


def case_classes(tok, ids, language="english"):
    """Which classes of the census one row holds, from transformers' own functions and string tests alone (its two passes replayed on its words)."""
    from transformers.models.whisper import tokenization_whisper as tw
    ids = [int(t) for t in ids]
    got = set()
    if len(ids) == 0:
        return {"empty_row"}
    if len(ids) == 1:
        got.add("one_token_row")
    prepended, appended = "\"'“¡¿([{-", "\"'.。,，!！?？:：”)]}、"
    pieces, _, _ = tw._split_tokens_on_unicode(tok, ids)
    split = tw._split_tokens_on_unicode if language in UNICODE_LANGUAGES else tw._split_tokens_on_spaces
    words, _, idx = split(tok, ids)
    _, final = hf_words(tok, ids, language)
    if any(len(i) > 1 for i in final):
        got.add("multi_token_word")
    if any(p.strip() == "" for p in pieces):
        got.add("whitespace_piece")
    n = len(words)
    P = [w.startswith(" ") and w.strip() in prepended for w in words]
    if any(P[i] and P[i + 1] for i in range(n - 2)):
        got.add("prepend_run")
    if n >= 2 and P[n - 1]:
        got.add("prepend_last")
    _, _, pidx = tw._split_tokens_on_unicode(tok, ids)
    starts = {i[0] for i in pidx}                          # first token index of every piece
    if any(w in appended and sum(1 for t in i if t in starts) > 1 for w, i in zip(words, idx)):
        got.add("multi_piece_append")
    ws = list(words)
    i, j = n - 2, n - 1
    while i >= 0:
        if ws[i].startswith(" ") and ws[i].strip() in prepended:
            ws[j] = ws[i] + ws[j]; ws[i] = ""
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < n:
        if not ws[i].endswith(" ") and ws[j] in appended:
            if ws[i] == "":
                got.add("append_into_emptied")
            ws[i] += ws[j]; ws[j] = ""
        else:
            if ws[i].endswith(" ") and ws[j] and ws[j] in appended:
                got.add("append_refused_space")
            i = j
        j += 1
    return got


WHOLE_CHARS = list("abcdefghijklmnopqrstuvwxyzABCDEéß") + [" "] * 6 + list(".,!?:;'\"()[]{}-") + list("。，！？：”“、¿¡你好世界")


def whole_char_tokenizer(n_text, seed=7):
    """(WhisperTokenizer, token_bytes) with ``n_text`` text ids made of whole characters — letters, spaces, ASCII and CJK punctuation, quotes —, so
    that ANY id list is inside the domain of equality; the specials follow from ``n_text`` (= eos_token_id) on."""
    from transformers import WhisperTokenizer
    rng = np.random.default_rng(seed)
    seen, toks = set(), []
    for c in WHOLE_CHARS + [" " + c for c in WHOLE_CHARS if c != " "]:
        if c not in seen:
            seen.add(c); toks.append(c)
    while len(toks) < n_text:
        s = "".join(WHOLE_CHARS[int(k)] for k in rng.integers(0, 33, int(rng.integers(2, 6))))
        s = (" " if rng.random() < 0.5 else "") + s
        if s not in seen:
            seen.add(s); toks.append(s)
    toks = toks[:n_text]
    b2u = bytes_to_unicode()
    vocab = {"".join(b2u[b] for b in s.encode()): i for i, s in enumerate(toks)}
    assert len(vocab) == n_text
    for t in SPECIALS:
        vocab[t] = len(vocab)
    tok = WhisperTokenizer(vocab=vocab, merges=[])
    tok.add_special_tokens({"additional_special_tokens": SPECIALS[1:]})
    assert tok.eos_token_id == n_text
    return tok, [s.encode() for s in toks]
