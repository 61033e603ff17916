"""Live transcription (include/wm.h wm_stream_agree) in plain Python, stated twice and independently: `agree_ref`, written from the
four steps of the contract, and `HypothesisBufferRef`, the list-popping formulation of the LocalAgreement-2 policy (Macháček et al. 2023); the
whole session loop for ONE session with one one-clip generate() per tick (`drive_ref`); and the seeded case list with its class census that both
test files share."""
import math

import numpy as np

LATE_CS, NEAR_CS, MAX_NGRAM, TAIL = 10, 100, 5, 5
ENDERS = (b".", b"?", b"!", "。".encode(), "？".encode(), "！".encode())
HOP = 160


def key(token_bytes, word) -> bytes:
    """The key of a word (a list of ids): its bytes with every leading and trailing 0x20 removed, nothing else."""
    return b"".join(token_bytes[int(t)] for t in word).strip(b" ")


# ---- (a) the four steps ---------------------------------------------------------------------------------------------------------------------------
def agree_ref(token_bytes, new, prev, tail, times, last_cs, late_cs=LATE_CS, near_cs=NEAR_CS, max_ngram=MAX_NGRAM):
    """(skip, commit, ender) of one session.  new / prev / tail: lists of words (lists of ids); times: (start, end) centiseconds per word of new."""
    K = lambda w: key(token_bytes, w)                       # noqa: E731
    n, P, C = len(new), len(prev), len(tail)
    assert C <= TAIL and len(times) == n
    k0 = n                                                  # 1. late words: a prefix
    for w in range(n):
        if int(times[w][0]) > last_cs - late_cs:
            k0 = w
            break
    if k0 < n and C > 0 and abs(int(times[k0][0]) - last_cs) < near_cs:            # 2. overlap with what is committed
        for i in range(1, min(C, n - k0, max_ngram) + 1):
            if all(K(tail[C - i + j]) == K(new[k0 + j]) for j in range(i)):
                k0 += i
                break
    m = 0                                                   # 3. agreement
    while m < min(n - k0, P) and K(new[k0 + m]) == K(prev[m]):
        m += 1
    ender = -1                                              # 4. sentence end
    for w in range(k0, k0 + m):
        if K(new[w]).endswith(ENDERS):
            ender = w
    return k0, m, ender


# ---- (b) the list-popping formulation ---------------------------------------------------------------------------------------------------------------
class HypothesisBufferRef:
    """Three lists of (start, end, word): `committed_in_buffer`, `buffer` (the last hypothesis' uncommitted rest) and `new`."""

    def __init__(self, token_bytes, late_cs=LATE_CS, near_cs=NEAR_CS, max_ngram=MAX_NGRAM):
        self.tb, self.late, self.near, self.max_ngram = token_bytes, late_cs, near_cs, max_ngram
        self.committed_in_buffer, self.buffer, self.new = [], [], []
        self.last = 0

    def _same(self, a, b):
        return key(self.tb, a) == key(self.tb, b)

    def insert(self, words, times, offset=0):
        shifted = [(int(a) + offset, int(b) + offset, w) for (a, b), w in zip(times, words)]
        self.new = [x for x in shifted if x[0] > self.last - self.late]
        if self.new and abs(self.new[0][0] - self.last) < self.near and self.committed_in_buffer:
            C, n = len(self.committed_in_buffer), len(self.new)
            for i in range(1, min(C, n, self.max_ngram) + 1):
                if all(self._same(self.committed_in_buffer[C - i + j][2], self.new[j][2]) for j in range(i)):
                    for _ in range(i):
                        self.new.pop(0)
                    break

    def flush(self):
        commit = []
        while self.new and self.buffer and self._same(self.new[0][2], self.buffer[0][2]):
            commit.append(self.new[0])
            self.last = self.new[0][1]
            self.new.pop(0)
            self.buffer.pop(0)
        self.buffer, self.new = self.new, []
        self.committed_in_buffer += commit
        return commit

    def pop_committed(self, t):
        while self.committed_in_buffer and self.committed_in_buffer[0][1] <= t:
            self.committed_in_buffer.pop(0)


def buffer_ref(token_bytes, case):
    """(skip, commit) of one case through HypothesisBufferRef (equal to agree_ref's on non-decreasing starts: its late rule is a filter)."""
    h = HypothesisBufferRef(token_bytes, case.get("late_cs", LATE_CS), case.get("near_cs", NEAR_CS), case.get("max_ngram", MAX_NGRAM))
    h.committed_in_buffer = [(0, 0, w) for w in case["tail"]]
    h.buffer = [(0, 0, w) for w in case["prev"]]
    h.last = case["last_cs"]
    h.insert(case["new"], case["times"])
    skip = len(case["new"]) - len(h.new)
    return skip, len(h.flush())


# ---- the seeded case list -----------------------------------------------------------------------------------------------------------------------------
CASE_SEED = 20263
EDGES = (63, 64, 65, 255, 256, 257, 600)
WORDS = ["hello", "world", "the", "a", "Hello", "world,", "there", "end.", "ok?", "wow!", "好。", "吗？", "啊！", "said.\"", "你好", "hel", "x", "and", "internationalisation",
         "e e", "...", "ing", "or"]


def _coders(token_bytes):
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

    def bytewise(b):
        return [index[bytes([x])] for x in b]
    return greedy, bytewise


def _case(new, prev, tail, starts, last_cs, ends=None):
    ends = ends if ends is not None else [s + 7 for s in starts]
    return dict(new=[list(w) for w in new], prev=[list(w) for w in prev], tail=[list(w) for w in tail], times=[(int(a), int(b)) for a, b in zip(starts, ends)],
                last_cs=int(last_cs))


def seeded_cases(token_bytes):
    """[case]: dicts of new / prev / tail (lists of words as id lists), times [(start, end)] and last_cs, all under the default parameters: the
    classes of `CLASSES` by construction, the long hypotheses of EDGES with the first mismatch at every edge, then seeded random cases."""
    greedy, bytewise = _coders(token_bytes)
    g = lambda s: greedy(s.encode() if isinstance(s, str) else s)           # noqa: E731
    bw = lambda s: bytewise(s.encode() if isinstance(s, str) else s)        # noqa: E731
    cases = []
    L = 1000                                                # last_cs of the hand-made cases
    far = [L + 300 + 20 * k for k in range(700)]            # starts far behind last_cs: no late words, no overlap test
    # late prefix: start == last - late is dropped, one centisecond later is kept
    cases.append(_case([g(" a"), g(" hello"), g(" world")], [g(" world")], [], [L - LATE_CS - 5, L - LATE_CS, L + 400], L))
    cases.append(_case([g(" a"), g(" hello"), g(" world")], [g(" hello")], [], [L - LATE_CS - 5, L - LATE_CS + 1, L + 400], L))
    cases.append(_case([g(" a"), g(" hello")], [g(" hello")], [], [L - 50, L - LATE_CS], L))                     # all late: k0 = n
    # the overlap test applies below near, not at near
    cases.append(_case([g(" hello"), g(" world")], [g(" world")], [g(" hello")], [L + NEAR_CS - 1, L + NEAR_CS + 30], L))
    cases.append(_case([g(" hello"), g(" world")], [g(" world")], [g(" hello")], [L + NEAR_CS, L + NEAR_CS + 30], L))
    cases.append(_case([g(" hello"), g(" world")], [g(" world")], [g(" hello")], [L - 9, L + 30], L))             # in front of last_cs, inside late
    # overlaps of 1..5 words, and six committed words of which the tail holds five: not removed
    six = [g(" x"), g(" hello"), g(" world"), g(" the"), g(" a"), g(" there")]
    rest = [g(" and"), g(" end.")]
    for i in range(1, 6):
        cases.append(_case(six[6 - i:] + rest, rest, six[1:], [L + 5 * k for k in range(i + 2)], L))
        cases.append(_case(six[6 - i:] + rest, rest, six[6 - i:], [L + 5 * k for k in range(i + 2)], L))          # the tail is exactly the overlap
    cases.append(_case(six + rest, rest, six[1:], [L + 5 * k for k in range(8)], L))
    cases.append(_case(six + rest, six, six[1:], [L + 5 * k for k in range(8)], L))
    # an empty tail next to last_cs; a mismatch at word 0; P < n - k0 and P > n - k0
    cases.append(_case([g(" hello"), g(" world")], [g(" hello")], [], [L + 1, L + 30], L))
    cases.append(_case([g(" hello"), g(" world")], [g(" world"), g(" hello")], [], far[:2], L))
    cases.append(_case([g(" hello"), g(" world"), g(" the")], [g(" hello")], [], far[:3], L))
    cases.append(_case([g(" hello")], [g(" hello"), g(" world"), g(" the")], [], far[:1], L))
    cases.append(_case([g(" hello"), g(" world")], [], [], far[:2], L))
    # equal keys under different tokenisations; a leading space; case; a trailing comma; a strict prefix, both ways; all-space words
    cases.append(_case([g(" hel") + g("lo"), bw(" world")], [g(" hello"), g(" world")], [], far[:2], L))
    cases.append(_case([bw(" internationalisation"), g(" a")], [g(" internationalisation"), bw(" a")], [], far[:2], L))
    cases.append(_case([g(" hello"), g("world")], [g("hello"), g(" world")], [], far[:2], L))
    cases.append(_case([g(" hello"), g(" the")], [g("  hello  "), g(" the")], [], far[:2], L))                   # several spaces at both ends
    cases.append(_case([g(" a"), g(" hello")], [g(" a"), g(" Hello")], [], far[:2], L))
    cases.append(_case([g(" a"), g(" world")], [g(" a"), g(" world,")], [], far[:2], L))
    cases.append(_case([g(" a"), g(" hel")], [g(" a"), g(" hello")], [], far[:2], L))
    cases.append(_case([g(" a"), g(" hello")], [g(" a"), g(" hel")], [], far[:2], L))
    cases.append(_case([g(" a"), g(" e e")], [g(" a"), g(" e  e")], [], far[:2], L))                               # inner bytes are kept
    cases.append(_case([g(" a"), g(" e e"), g(" x")], [g(" a"), bw(" e e "), g(" x")], [], far[:3], L))
    cases.append(_case([g(" "), g(" a")], [g("   "), g(" a")], [], far[:2], L))
    cases.append(_case([g(" a"), g("  ")], [g(" a"), g(" ")], [g(" ")], far[:2], L))
    cases.append(_case([g(" a"), g(" \t")], [g(" a"), g(" ")], [], far[:2], L))                                    # a tab is no 0x20
    cases.append(_case([g(" "), g(" a")], [g(" a")], [g("  ")], [L + 1, L + 9], L))                                # an empty key in the overlap
    # every ender, `."` is none; the last one in the agreed range counts, one behind it does not
    for e in ("end.", "ok?", "wow!", "好。", "吗？", "啊！", "said.\""):
        cases.append(_case([g(" a"), g(" " + e), g(" the")], [g(" a"), g(" " + e), g(" the")], [], far[:3], L))
        cases.append(_case([g(" a"), bw(" " + e + "  ")], [g(" a"), g(" " + e)], [], far[:2], L))                 # spaces behind the ender, byte by byte
        cases.append(_case([g(" a"), g(" " + e)], [g(" a")], [], far[:2], L))                                      # the ender is not agreed
    cases.append(_case([g(" end."), g(" ok?"), g(" a"), g(" wow!")], [g(" end."), g(" ok?"), g(" a")], [], far[:4], L))
    cases.append(_case([g("."), g("。"), g(" 。")], [g(" ."), bw("。"), g("。")], [], far[:3], L))
    cases.append(_case([g(" end."), g(" a")], [g(" a")], [g(" end.")], [L + 1, L + 9], L))                         # an ender inside the overlap is skipped, not agreed
    # n = 0, with and without the other lists
    cases.append(_case([], [], [], [], 0))
    cases.append(_case([], [g(" a")], [g(" the")], [], L))
    # long hypotheses: the first mismatch at every edge, and none
    rng = np.random.default_rng(CASE_SEED)
    pool = [g(" " + w) for w in WORDS] + [bw(" " + w) for w in WORDS]
    for n in EDGES:
        words = [pool[int(k)] for k in rng.integers(len(pool), size=n)]
        cases.append(_case(words, words, [], far[:n], L))
        for e in EDGES:
            if e < n:
                prev = list(words)
                prev[e] = g(" DIFF")
                cases.append(_case(words, prev, [], far[:n], L))
        cases.append(_case(words + [g(" x")], words, [], far[:n + 1], L))
        cases.append(_case(words, words + [g(" x")], [], far[:n], L))
    # seeded random cases
    alt = lambda w: bw(b"".join(token_bytes[t] for t in w)) if rng.random() < 0.5 else list(w)          # noqa: E731
    while len(cases) < 420:
        n = int(rng.choice([0, 1, 2, 3, 5, 8, 13, 30]))
        words = [pool[int(k)] for k in rng.integers(len(pool), size=n)]
        starts = list(np.cumsum(rng.integers(0, 60, size=n)) + 500) if n else []
        ends = [int(s + rng.integers(1, 50)) for s in starts]
        if n and rng.random() < 0.15:                        # out of order: the late rule as a prefix, not a filter
            j = int(rng.integers(n))
            starts[j] = int(starts[j] - rng.integers(0, 200))
        last = int(rng.choice([0, 500, starts[int(rng.integers(n))] + int(rng.integers(-15, 15)) if n else 0, 480 + int(rng.integers(0, 200))]))
        k0 = next((w for w in range(n) if starts[w] > last - LATE_CS), n)
        ov = int(rng.integers(0, 6))
        tail = [pool[int(k)] for k in rng.integers(len(pool), size=int(rng.integers(0, 6)))]
        if ov and k0 + ov <= n and rng.random() < 0.6:
            tail = (tail + [alt(w) for w in words[k0: k0 + ov]])[-TAIL:]
        else:
            ov = 0
        agreed = int(rng.integers(0, 8))
        prev = [alt(w) for w in words[k0 + ov: k0 + ov + agreed]]
        prev += [pool[int(k)] for k in rng.integers(len(pool), size=int(rng.integers(0, 4)))]
        cases.append(_case(words, prev, tail, starts, last, ends))
    return cases


CLASSES = ("late_at_bound_dropped", "late_one_after_kept", "all_late", "near_minus_1", "near_exact", "overlap_1", "overlap_2", "overlap_3", "overlap_4",
           "overlap_5", "overlap_6_kept", "empty_tail", "mismatch_at_0", "prev_shorter", "prev_longer", "retokenised_equal", "leading_space_equal",
           "case_differs", "trailing_comma_differs", "strict_prefix_new", "strict_prefix_prev", "all_space_pair", "ender_quote_is_none", "n_zero",
           "unordered_starts") + tuple("ender_" + e.hex() for e in ENDERS) + tuple(f"len_{n}" for n in EDGES) + tuple(f"mismatch_at_{n}" for n in EDGES[:-1])


def case_classes(token_bytes, case):
    """Which classes of the census one case holds, from its own data and the keys alone."""
    K = lambda w: key(token_bytes, w)                       # noqa: E731
    raw = lambda w: b"".join(token_bytes[t] for t in w)     # noqa: E731
    new, prev, tail, last = case["new"], case["prev"], case["tail"], case["last_cs"]
    st = [t[0] for t in case["times"]]
    n, P, C = len(new), len(prev), len(tail)
    got = set()
    if n == 0:
        return {"n_zero"}
    if any(b < a for a, b in zip(st, st[1:])):
        got.add("unordered_starts")
    k0 = next((w for w in range(n) if st[w] > last - LATE_CS), n)
    if k0 == n:
        got.add("all_late")
    if k0 > 0 and st[k0 - 1] == last - LATE_CS:
        got.add("late_at_bound_dropped")
    if k0 < n and st[k0] == last - LATE_CS + 1:
        got.add("late_one_after_kept")
    ov = 0
    if k0 < n:
        d = abs(st[k0] - last)
        match = [i for i in range(1, min(C, n - k0) + 1) if [K(w) for w in tail[C - i:]] == [K(w) for w in new[k0: k0 + i]]]
        if C == 0 and d < NEAR_CS:
            got.add("empty_tail")
        if match and d == NEAR_CS - 1:
            got.add("near_minus_1")
        if match and d == NEAR_CS:
            got.add("near_exact")
        if match and d < NEAR_CS:
            ov = match[0]
            got.add(f"overlap_{ov}")
        if not match and d < NEAR_CS and C == 5 and n - k0 >= 6 and [K(w) for w in new[k0 + 1: k0 + 6]] == [K(w) for w in tail]:
            got.add("overlap_6_kept")
    k0 += ov
    lim = min(n - k0, P)
    m = next((j for j in range(lim) if K(new[k0 + j]) != K(prev[j])), lim)
    if P < n - k0:
        got.add("prev_shorter")
    if P > n - k0:
        got.add("prev_longer")
    if n in EDGES:
        got.add(f"len_{n}")
    if m < lim:
        a, b = K(new[k0 + m]), K(prev[m])
        if m == 0:
            got.add("mismatch_at_0")
        if m in EDGES:
            got.add(f"mismatch_at_{m}")
        if a != b and a.lower() == b.lower():
            got.add("case_differs")
        if b == a + b"," or a == b + b",":
            got.add("trailing_comma_differs")
        if b.startswith(a) and a != b and b != a + b",":
            got.add("strict_prefix_new")
        if a.startswith(b) and a != b and a != b + b",":
            got.add("strict_prefix_prev")
    for j in range(m):
        a, b = new[k0 + j], prev[j]
        if a != b:
            got.add("retokenised_equal")
        if raw(a) != raw(b) and raw(a).lstrip(b" ") == raw(b).lstrip(b" "):
            got.add("leading_space_equal")
        if K(a) == b"" and K(b) == b"":
            got.add("all_space_pair")
        for e in ENDERS:
            if K(a).endswith(e):
                got.add("ender_" + e.hex())
        if K(a).endswith(b".\""):
            got.add("ender_quote_is_none")
    return got


def pack_cases(token_bytes, cases) -> np.ndarray:
    """The case list as the int32 words tests/stream_host.cpp reads: [n_tokens, n_bytes, offsets, bytes (one per word), S, late, near, max_ngram,
    then per list words S+1 | n_tok | tok | n_ids | ids, then times 2 per new word, last_cs S]."""
    off = np.cumsum([0] + [len(b) for b in token_bytes])
    blob = b"".join(token_bytes)
    data = [len(token_bytes), len(blob)] + list(off) + list(blob) + [len(cases), LATE_CS, NEAR_CS, MAX_NGRAM]
    for name in ("new", "prev", "tail"):
        words = np.cumsum([0] + [len(c[name]) for c in cases])
        tok = np.cumsum([0] + [len(w) for c in cases for w in c[name]])
        ids = [t for c in cases for w in c[name] for t in w]
        data += list(words) + [len(tok)] + list(tok) + [len(ids)] + ids
    data += [x for c in cases for t in c["times"] for x in t] + [c["last_cs"] for c in cases]
    return np.asarray(data, dtype=np.int32)


# ---- the session loop, one session at a time ----------------------------------------------------------------------------------------------------------
def drive_ref(model, token_bytes, schedule, *, min_chunk_s=1.0, trim_s=None, hard_trim_s=None, late_s=0.1, near_s=1.0, **kw):
    """One session fed the chunks of ``schedule`` (arrays or None) in order: per tick the result dict of StreamSessions.feed, from ONE one-clip
    ``model.generate`` per due tick, `agree_ref` as the agreement and the overflow / due / trim rules restated on a numpy buffer."""
    cfg = model.config
    W = HOP * cfg.n_mel_frames
    wcs = W // HOP
    trim = wcs // 2 if trim_s is None else int(round(trim_s * 100))
    hard = 5 * wcs // 6 if hard_trim_s is None else int(round(hard_trim_s * 100))
    late, near = int(round(late_s * 100)), int(round(near_s * 100))
    need = int(round(min_chunk_s * 16000))
    buf = np.zeros(0, dtype=np.float32)                     # the audio itself, no padding
    off = last = sentence = lost = since = 0
    committed, pending, out = [], [], []

    def word(w):
        d = {"text": w["text"], "timestamp": (w["cs"][0] / 100.0, w["cs"][1] / 100.0), "ids": w["ids"]}
        if "probability" in w:
            d["probability"] = w["probability"]
        return d

    for chunk in schedule:
        x = np.zeros(0, dtype=np.float32) if chunk is None else np.asarray(chunk, dtype=np.float32)
        if len(x):
            excess = len(buf) + len(x) - W
            if excess > 0:
                c = max(min(last, off + len(buf) // HOP), off + math.ceil(excess / HOP))
                lost += max(0, c - max(last, off))
                buf = np.concatenate([buf, x])[(c - off) * HOP:]
                off = c
            else:
                buf = np.concatenate([buf, x])
            since += len(x)
        done, decoded = [], False
        if len(buf) and since and since >= need:
            decoded = True
            clip = np.zeros(W, dtype=np.float32)
            clip[: len(buf)] = buf
            o = model.generate(model.extract_features([clip]), return_word_timestamps=True, **kw)
            row = o["sequences"][0].tolist()
            new = []
            for w in o["words"][0]:
                a, z = w["tokens"]
                d = {"text": w["text"], "ids": [int(t) for t in row[a:z]], "cs": (round(w["timestamp"][0] * 100) + off, round(w["timestamp"][1] * 100) + off)}
                if "probability" in w:
                    d["probability"] = w["probability"]
                new.append(d)
            tail = [w for w in committed[-TAIL:] if w["cs"][1] > off]
            k0, m, e = agree_ref(token_bytes, [w["ids"] for w in new], [w["ids"] for w in pending], [w["ids"] for w in tail], [w["cs"] for w in new], last,
                                 late, near)
            done, pending = new[k0: k0 + m], new[k0 + m:]
            committed += done
            if m:
                last = done[-1]["cs"][1]
            if e >= 0:
                sentence = new[e]["cs"][1]
            since = 0
            d = len(buf) // HOP
            if d > trim:
                c = sentence if sentence > off else last if (d > hard and last > off) else None
                if c is not None:
                    c = min(c, off + d)
                    buf, off = buf[(c - off) * HOP:], c
        out.append(dict(committed=[word(w) for w in done], pending=[word(w) for w in pending], offset_s=off / 100.0, buffer_s=len(buf) / 16000.0,
                        decoded=decoded, lost_s=lost / 100.0))
    return out
