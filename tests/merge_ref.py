"""References and cases of the overlapping-window merge (include/wm.h wm_merge_windows): transformers' own
``_find_longest_common_sequence`` (hf_merge), the contract of k_merge_windows restated in plain Python as one slice per window (keep_slices),
what one boundary looks like under that contract (boundary_info: what the class guard of tests/test_merge_cpu.py reads), and the case lists
both the CPU and the GPU tests run.  tests/test_merge_cpu.py holds, from these references alone, that the two agree on every case."""
from fractions import Fraction

import numpy as np

LEN_MAX, WINDOWS_MAX = 512, 4096                # WM_MERGE_LEN_MAX, WM_MERGE_WINDOWS_MAX (include/wm.h)


# ---- the two references ----------------------------------------------------------------------------------------------------------------------
def hf_merge(windows, times=None):
    """transformers' function on the NON-EMPTY windows of one clip (the pipeline never appends an empty one): the merged ids, and with ``times``
    (one float per id) the merged times next to them."""
    from transformers.models.whisper.tokenization_whisper import _find_longest_common_sequence
    idx = [j for j, w in enumerate(windows) if len(w)]
    if not idx:
        return [] if times is None else ([], [])
    seqs = [list(windows[j]) for j in idx]
    if times is None:
        return [int(t) for t in _find_longest_common_sequence(seqs)]
    ids, ts = _find_longest_common_sequence(seqs, [[float(np.float32(v)) for v in times[j]] for j in idx])
    return [int(t) for t in ids], [float(v) for v in ts]


def shift_table(left, right, tl=None, tr=None):
    """Every shift i in 1 .. L + R - 1 of one boundary: (i, left_start, left_stop, right_start, right_stop, matches, score)."""
    L, R = len(left), len(right)
    out = []
    for i in range(1, L + R):
        ls, le, rs, re = max(0, L - i), min(L, L + R - i), max(0, i - L), min(R, i)
        m = 0
        for k in range(le - ls):
            if left[ls + k] == right[rs + k] and (tl is None or np.float32(tl[ls + k]) <= np.float32(tr[rs + k])):
                m += 1
        out.append((i, ls, le, rs, re, m, m / i + i / 10000.0))
    return out


def best_shift(table):
    """The winner of a boundary: the best score among the shifts with matches > 1, among equal scores the smallest i; None: no shift counts."""
    best = None
    for row in table:
        if row[5] > 1 and (best is None or row[6] > best[6]):
            best = row
    return best


def _walk(windows, times=None, skip_empty=True):
    """The chain of one clip: yields (prev window, this window, left ids, right ids, left times, right times, a) per boundary and returns the
    slices through ``keep`` (a list the caller passes in)."""
    keep = [(0, 0)] * len(windows)
    prev, a, left, tl = None, 0, None, None
    info = []
    for w, ids in enumerate(windows):
        if skip_empty and len(ids) == 0:
            continue
        ids = [int(t) for t in ids]
        tw = None if times is None else [float(np.float32(v)) for v in times[w]]
        if prev is None:
            prev, a, left, tl = w, 0, ids, tw
            continue
        table = shift_table(left, ids, tl, tw)
        win = best_shift(table)
        L = len(left)
        ls, le, rs, re = (L, L, 0, 0) if win is None else win[1:5]
        left_mid, right_mid = (ls + le) // 2, (rs + re) // 2
        keep[prev] = (a, a + left_mid)
        info.append(dict(prev=prev, w=w, L=L, R=len(ids), table=table, win=win))
        prev, a, left, tl = w, right_mid, ids[right_mid:], None if tw is None else tw[right_mid:]
    if prev is not None:
        keep[prev] = (a, len(windows[prev]))
    return keep, info


def keep_slices(windows, times=None):
    """The contract of wm_merge_windows for one clip: window w contributes windows[w][a:b]; [(a, b)] per window, (0, 0) for an empty one."""
    return _walk(windows, times)[0]


def boundary_info(windows, times=None):
    """Per boundary of the clip's chain: L, R, the shift table and the winner (None: plain concatenation)."""
    return _walk(windows, times)[1]


def assemble(windows, keep, field=None):
    src = windows if field is None else field
    return [v for w, (a, b) in enumerate(keep) for v in src[w][a:b]]


def merged_with_empty_links(windows):
    """What comes out when an empty window stays a link of the chain (NOT the contract): transformers' function over all windows."""
    from transformers.models.whisper.tokenization_whisper import _find_longest_common_sequence
    return [int(t) for t in _find_longest_common_sequence([list(w) for w in windows])]


# ---- the classes the case list has to hold -----------------------------------------------------------------------------------------------------
CLASSES = ("concat", "i<L", "i==L", "i>L", "fault_tolerant", "eps_decides", "one_match_rule", "times_change", "empty_middle")


def boundary_classes(b):
    """The classes one boundary (boundary_info entry) falls into."""
    out = set()
    win, L = b["win"], b["L"]
    if win is None:
        out.add("concat")
        return out
    i, ls, le, _, _, m, score = win
    out.add("i<L" if i < L else "i==L" if i == L else "i>L")
    if m < le - ls:
        out.add("fault_tolerant")           # the winning overlap holds a damaged position (so matches / i < 1 as well)
    if any(r[5] > 1 and r[0] != i and Fraction(r[5], r[0]) == Fraction(m, i) for r in b["table"]):
        out.add("eps_decides")
    if any(r[5] == 1 and r[6] > score for r in b["table"]):
        out.add("one_match_rule")
    return out


def case_classes(case):
    """(class -> count) of one case: boundaries for the boundary classes, 1 per case for the two case-level ones."""
    n = {}
    for b in boundary_info(case["windows"], case.get("times")):
        for c in boundary_classes(b):
            n[c] = n.get(c, 0) + 1
    if case.get("times") is not None and keep_slices(case["windows"], case["times"]) != keep_slices(case["windows"]):
        n["times_change"] = 1
    ws = case["windows"]
    if case.get("times") is None and any(len(w) == 0 for w in ws[1:-1]) and len(ws[0]) and len(ws[-1]):
        if assemble(ws, keep_slices(ws)) != merged_with_empty_links(ws):
            n["empty_middle"] = 1
    return n


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 7, 16, 33, 65)


def _pair(rng, L, R, vocab, plant, damage):
    """Two windows; ``plant``: 0 none, 1 a suffix of left is the prefix of right, 2 the whole left opens right, 3 left sits inside right behind
    a prefix of other ids; ``damage``: one id of the planted copy changed."""
    left = [int(t) for t in rng.integers(0, vocab, L)]
    right = [int(t) for t in rng.integers(0, vocab, R)]
    if plant == 1:
        k = int(rng.integers(1, min(L, R) + 1))
        right[:k] = left[L - k:]
        lo, n = 0, k
    elif plant == 2 and L <= R:
        right[:L] = left
        lo, n = 0, L
    elif plant == 3 and L < R:
        p = int(rng.integers(1, R - L + 1))
        right[p: p + L] = left
        lo, n = p, L
    else:
        return left, right
    if damage and n > 2:
        q = lo + int(rng.integers(0, n))
        right[q] = (right[q] + 1 + int(rng.integers(0, max(vocab - 1, 1)))) % vocab if vocab > 1 else right[q]
    return left, right


def _times_for(rng, windows, step=20.0):
    """Ascending float32 times per window, window j offset by j * step; inside a window's first ids a coin decides whether the times run ahead of
    the previous window's (in order: a match counts) or behind them (out of order: it does not)."""
    out = []
    for j, w in enumerate(windows):
        t = np.sort(rng.uniform(0.0, 30.0, len(w))).astype(np.float32) + np.float32(j * step)
        if j and rng.integers(0, 2):
            t = t - np.float32(15.0)        # this window's clock runs early: its overlap lies BEFORE the left window's times
        out.append([float(v) for v in t.astype(np.float32)])
    return out


def cpu_cases():
    """The seeded list both suites run: pairs, chains of 3 and of up to 9 windows, with and without times, and chains with empty windows."""
    rng = np.random.default_rng(20240611)
    cases = []
    for n in range(260):
        vocab = int(rng.integers(2, 51))
        L, R = (int(v) for v in rng.choice(LENGTHS, 2))
        plant = int(rng.integers(1, 4)) if n % 2 else 0
        left, right = _pair(rng, L, R, vocab, plant, damage=(n % 4 == 3))
        cases.append(dict(windows=[left, right]))
    for n in range(60):                     # two or three ids: equal match ratios at several shifts are common, the i / 10000 term decides
        L, R = (int(v) for v in rng.choice(LENGTHS[2:], 2))
        left, right = _pair(rng, L, R, 2 + n % 2, n % 3, damage=False)
        cases.append(dict(windows=[left, right]))
    for n in range(60):                     # with times
        vocab = int(rng.integers(2, 51))
        L, R = (int(v) for v in rng.choice(LENGTHS, 2))
        left, right = _pair(rng, L, R, vocab, 1 + n % 3 if n % 4 else 0, damage=(n % 3 == 0))
        ws = [left, right]
        cases.append(dict(windows=ws, times=_times_for(rng, ws)))
    for n in range(40):                     # chains: 3 .. 9 windows, every boundary planted on what the previous one leaves
        vocab = int(rng.integers(5, 51))
        k = (3, 3, 4, 9)[n % 4]
        ws = [[int(t) for t in rng.integers(0, vocab, int(rng.choice(LENGTHS[2:])))]]
        for _ in range(k - 1):
            R = int(rng.choice(LENGTHS[2:]))
            w = [int(t) for t in rng.integers(0, vocab, R)]
            ov = int(rng.integers(0, min(len(ws[-1]), R) + 1))
            if ov:
                w[:ov] = ws[-1][len(ws[-1]) - ov:]
            ws.append(w)
        cases.append(dict(windows=ws, times=_times_for(rng, ws) if n % 5 == 4 else None))
    for n in range(40):                     # an empty window in the middle: the outer two overlap, so skipping it matters
        vocab = int(rng.integers(10, 51))
        L, R = (int(v) for v in rng.choice(LENGTHS[3:], 2))
        left, right = _pair(rng, L, R, vocab, 1, damage=False)
        ws = [left, [], right] if n % 2 else [left, [], [], right, []]
        cases.append(dict(windows=ws))
    cases.append(dict(windows=[[], [], []]))
    cases.append(dict(windows=[[5, 6, 7]]))
    cases.append(dict(windows=[[], [5, 6, 7, 8], [7, 8, 9]]))
    for c in cases:
        c.setdefault("times", None)
    return cases


GPU_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512)
# (L, R): L + R - 1 shifts on both sides of 256, 512 and 768, the thread count's multiples; and the edges 0 / 1 / LEN_MAX
GPU_PAIRS = ((0, 3), (3, 0), (1, 1), (2, 1), (1, 255), (2, 255), (255, 2), (3, 255), (63, 64), (64, 65), (65, 63), (255, 257), (256, 257), (257, 256),
             (257, 257), (1, 512), (512, 1), (255, 512), (256, 512), (512, 257), (257, 511), (511, 512), (512, 512), (512, 0), (0, 512), (63, 3))


def gpu_length_cases():
    """Pairs over GPU_PAIRS (vocabularies of 3 and 40 ids, suffix overlaps of a random length, every third with a damaged id), with times on every
    second; then clips of 1, 2, 3 and 9 windows with lengths from GPU_LENGTHS."""
    rng = np.random.default_rng(977)
    cases = []
    for n, (L, R) in enumerate(GPU_PAIRS):
        assert L in GPU_LENGTHS and R in GPU_LENGTHS
        for vocab in (3, 40):
            left, right = _pair(rng, L, R, vocab, 1 if min(L, R) else 0, damage=(n % 3 == 0))
            ws = [left, right]
            cases.append(dict(windows=ws, times=_times_for(rng, ws) if n % 2 else None))
    for k in (1, 2, 3, 9):
        for rep in range(3):
            lens = [int(v) for v in rng.choice(GPU_LENGTHS if rep else GPU_LENGTHS[:9], k)]
            ws = [[int(t) for t in rng.integers(0, 6 if rep == 1 else 60, n)] for n in lens]
            for j in range(1, k):
                ov = int(rng.integers(0, min(len(ws[j - 1]), len(ws[j])) + 1))
                if ov:
                    ws[j][:ov] = ws[j - 1][len(ws[j - 1]) - ov:]
            cases.append(dict(windows=ws, times=_times_for(rng, ws) if rep == 2 else None))
    return cases


def five_clips():
    """One call's worth: 5 clips of 1, 4, 2, 9 and 3 windows (block indexing), from the lists above."""
    rng = np.random.default_rng(5)
    clips = []
    for k in (1, 4, 2, 9, 3):
        ws = [[int(t) for t in rng.integers(0, 12, int(rng.choice((0, 3, 17, 64, 130))))] for _ in range(k)]
        for j in range(1, k):
            ov = int(rng.integers(0, min(len(ws[j - 1]), len(ws[j])) + 1))
            if ov:
                ws[j][:ov] = ws[j - 1][len(ws[j - 1]) - ov:]
        clips.append(ws)
    return clips


# ---- the window plan ---------------------------------------------------------------------------------------------------------------------------------
def hf_chunk_plan(T, F, left, right):
    """transformers' chunk_iter over T units with a stub feature extractor: [(start, stop)] of every chunk it yields."""
    from transformers.pipelines.automatic_speech_recognition import chunk_iter

    class _Stub:
        sampling_rate = 16000

        def __call__(self, chunk, sampling_rate=None, return_tensors=None, return_attention_mask=None):
            return {"start": int(chunk[0]), "stop": int(chunk[-1]) + 1}

    return [(c["start"], c["stop"]) for c in chunk_iter(np.arange(T), _Stub(), F, left, right)]
