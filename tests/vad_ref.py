"""The contract of wm_vad_windows (include/wm.h), restated in numpy and plain Python loops, and the seeded cases the CPU and GPU
suites share.  This file is the yardstick: it is written from the contract's seven steps, one obvious loop each — not from the kernels' scan
formulation — and nothing in it is fitted to a kernel's output."""
import numpy as np

HOP = 160
f32 = np.float32


def frame_energy(x, n):
    """Step 1, the vectorised part: E[t] for the T = ceil(n / 160) frames of x[:n], samples behind n count as 0.  Sixteen partial sums
    p_j = sum_i x[160 t + 16 i + j]^2 (i ascending, a rounded multiply and a rounded add per term), then the fold 8, 4, 2, 1."""
    T = -(-int(n) // HOP)
    buf = np.zeros(T * HOP, dtype=f32)
    buf[:n] = np.asarray(x, dtype=f32)[:n]
    X = buf.reshape(T, HOP // 16, 16)
    p = np.zeros((T, 16), dtype=f32)
    for i in range(HOP // 16):
        sq = X[:, i, :] * X[:, i, :]
        p = p + sq
    for o in (8, 4, 2, 1):
        p = p[:, :o] + p[:, o: 2 * o]
    return np.ascontiguousarray(p[:, 0])


def loud_level(E, q_permille):
    """Step 2: the order statistic of rank (q (T - 1)) // 1000 among E, ordered by bit pattern."""
    rank = (int(q_permille) * (len(E) - 1)) // 1000
    return np.sort(E.view(np.uint32))[rank: rank + 1].view(f32)[0]


def thresholds(R, P):
    """Step 3: one float32 multiply each, then fmaxf."""
    on = max(f32(R) * f32(P["k_on"]), f32(P["abs_on"]))
    off = max(f32(R) * f32(P["k_off"]), f32(P["abs_off"]))
    return f32(on), f32(off)


def vad_numpy_parts(x, n, P):
    """What of the contract is vectorised numpy (the microbenchmark times this): energy, loud level, thresholds, the two comparisons."""
    E = frame_energy(x, n)
    R = loud_level(E, P["q_permille"])
    on, off = thresholds(R, P)
    return E, R, on, off, E >= on, E < off


def vad_windows_ref(x, n, P):
    """All seven steps for one recording.  Returns a dict: E, R, thr_on, thr_off, s, runs, merged, kept, regions (padded, step 5), pieces
    (step 6), windows (step 7), and what the class guard of the CPU suite counts: ties (splits whose smallest E occurs more than once in the
    search range), absorbed (pieces each window took in behind its first) and refused (stop - u of every piece that opened a new window)."""
    E, R, on, off, hi, lo = vad_numpy_parts(x, n, P)
    T = len(E)
    # 4. hysteresis
    s = np.zeros(T, dtype=np.int8)
    prev = 0
    for t in range(T):
        if hi[t]:
            prev = 1
        elif lo[t]:
            prev = 0
        s[t] = prev
    # 5. regions: runs, merge, drop, pad
    runs = []
    t = 0
    while t < T:
        if s[t]:
            a = t
            while t < T and s[t]:
                t += 1
            runs.append((a, t))
        else:
            t += 1
    merged = []
    for a, b in runs:
        if merged and a - merged[-1][1] < P["min_silence"]:
            merged[-1] = (merged[-1][0], b)
        else:
            merged.append((a, b))
    kept = [(a, b) for a, b in merged if b - a >= P["min_speech"]]
    pad = P["pad"]
    starts, stops = [a for a, _ in kept], [b for _, b in kept]
    new_starts, new_stops = list(starts), list(stops)
    for i in range(len(kept) - 1):
        g = starts[i + 1] - stops[i]
        if g >= 2 * pad:
            new_stops[i] = stops[i] + pad
            new_starts[i + 1] = starts[i + 1] - pad
        else:
            new_stops[i] = stops[i] + g // 2
            new_starts[i + 1] = stops[i] + g // 2
    if kept:
        new_starts[0] = max(0, starts[0] - pad)
        new_stops[-1] = min(T, stops[-1] + pad)
    regions = list(zip(new_starts, new_stops))
    # 6. split
    F = P["F"]
    bits = E.view(np.uint32)
    pieces, ties = [], 0
    for a, b in regions:
        while b - a > F:
            lo_t, hi_t = a + F // 2, a + F
            best = lo_t
            for t in range(lo_t, hi_t + 1):
                if bits[t] < bits[best]:
                    best = t
            ties += int(np.sum(bits[lo_t: hi_t + 1] == bits[best]) > 1)
            pieces.append((a, best))
            a = best
        pieces.append((a, b))
    # 7. pack
    windows, absorbed, refused = [], [], []
    for a, b in pieces:
        if windows and b - windows[-1][0] <= F:
            windows[-1] = (windows[-1][0], b)
            absorbed[-1] += 1
        else:
            if windows:
                refused.append(b - windows[-1][0])
            windows.append((a, b))
            absorbed.append(0)
    return dict(E=E, R=R, thr_on=on, thr_off=off, s=s, runs=runs, merged=merged, kept=kept, regions=regions, pieces=pieces, windows=windows,
                ties=ties, absorbed=absorbed, refused=refused, T=T)


# ---- the seeded cases ----------------------------------------------------------------------------------------------------------------------
LOUD, QUIET = 0.1, 1e-4
DEAD = LOUD * 10.0 ** (-31.5 / 20.0)            # noise 32 dB below loud noise, 33.3 dB below a loud tone: inside the default -30 / -35 dB dead band
GARBAGE = 7.0                                   # what lies behind n_samples in a case's buffer: not audio, never to be read as such


def default_params(**kw):
    k_on, k_off = f32(10.0 ** (-30.0 / 10.0)), f32(10.0 ** (-35.0 / 10.0))
    abs_on = f32(160.0 * 10.0 ** (-60.0 / 10.0))
    P = dict(k_on=k_on, k_off=k_off, abs_on=abs_on, abs_off=f32(abs_on * k_off / k_on), q_permille=950, min_silence=5, min_speech=4, pad=3, F=40)
    P.update(kw)
    return P


def render(rng, plan, cut=0, tail=64):
    """plan: [(kind, frames)..], kind 'L' loud noise, 'T' loud tone (period 16: every frame the same samples, so the same E to the bit), 'D'
    noise in the dead band, 'Q' quiet noise, 'Z' digital silence.  cut: samples taken off the last frame (n no multiple of 160).  Returns
    (buffer, n): the buffer is `tail` samples longer than n and holds GARBAGE there."""
    parts = []
    for kind, frames in plan:
        m = frames * HOP
        if kind == "Z":
            parts.append(np.zeros(m, dtype=f32))
        elif kind == "T":
            parts.append((LOUD * np.sin(2.0 * np.pi * np.arange(m) / 16.0 + 0.3)).astype(f32))
        else:
            amp = {"L": LOUD, "D": DEAD, "Q": QUIET}[kind]
            parts.append((amp * rng.uniform(-1.0, 1.0, m)).astype(f32))
    x = np.concatenate(parts) if parts else np.zeros(0, dtype=f32)
    n = len(x) - cut
    buf = np.full(n + tail, GARBAGE, dtype=f32)
    buf[:n] = x[:n]
    return buf, n


def seeded_cases(seeds=range(6)):
    """[(name, buffer, n, params)..]: every case class of the issue, each under several seeds (the seed moves the noise, the loud kind, lengths
    that do not matter to the class, and the ragged tail)."""
    out = []
    for seed in seeds:
        rng = np.random.default_rng(1000 + seed)

        def add(name, plan, P=None, cut=None):
            P = default_params() if P is None else P
            if cut is None:
                cut = int(rng.integers(0, HOP)) if seed % 2 else 0
            buf, n = render(rng, plan, cut)
            out.append((f"{name}-{seed}", buf, n, P))

        L = "LT"[seed % 2]
        q = lambda lo, hi: ("Q", int(rng.integers(lo, hi)))          # noqa: E731  a quiet stretch of a length that does not matter
        P = default_params()
        ms, sp, pad, F = P["min_silence"], P["min_speech"], P["pad"], P["F"]
        add("gaps", [q(8, 12), (L, 8), ("Q", ms - 1), (L, 8), ("Q", ms), (L, 8), ("Q", ms + 1), (L, 8), q(8, 12)])
        add("speech-lengths", [q(8, 12), (L, sp - 1), ("Q", 8), (L, sp), ("Q", 8), (L, 10), q(8, 12)])
        P4 = default_params(pad=4)
        add("pad-gaps", [q(9, 12), (L, 8), ("Q", 7), (L, 8), ("Q", 8), (L, 8), ("Q", 9), (L, 8), q(9, 12)], P4)
        add("pad-clipped", [("Q", 1 + seed % 2), (L, 8), ("Q", 10), (L, 8), ("Q", 2)], cut=0 if seed % 2 == 0 else 7)
        add("region-lengths", [q(10, 14), (L, F - 2 * pad), ("Q", 12), (L, F + 1 - 2 * pad), ("Q", 12), ("L", 2 * F + 5 + seed), q(10, 14)])
        add("tie", [q(8, 12), ("T", 2 * F + 7 + seed), q(8, 12)])
        add("dead-band", [q(6, 9), (L, 8), ("D", 4), ("Q", 6), ("D", 4), (L, 8), ("D", 3), (L, 6), q(6, 9)])
        add("abs-no-speech", [("Q", int(rng.integers(20, 90)))])
        add("abs-speech", [("Q", 60), ("L", 4), ("Q", 60)])
        add("digital-silence", [("Z", int(rng.integers(1, 120)))])
        add("all-speech", [(L, int(rng.integers(30, 130)))])
        add("one-frame", [("LZQ"[seed % 3], 1)], cut=int(rng.integers(0, HOP)))
        add("pack-absorb", [q(6, 9), (L, 5), ("Q", 7), (L, 5), ("Q", 7), (L, 5), ("Q", 7), (L, 5), q(6, 9)])
        g = 8 + seed
        add("pack-refuse", [("Q", 6), (L, 5), ("Q", g), (L, 30 - g), q(8, 12)])          # the second piece stops at u + F + 1
        add("pack-fits", [("Q", 6), (L, 5), ("Q", g), (L, 29 - g), q(8, 12)])            # .. at u + F
        add("quantile-0", [q(6, 9), (L, 12), q(6, 9)], default_params(q_permille=0))
        add("quantile-1000", [q(6, 9), (L, 12), q(6, 9)], default_params(q_permille=1000))
        add("F-2", [q(6, 9), (L, 9), q(6, 9)], default_params(F=2, pad=0, min_speech=1, min_silence=1))
        # a random plan
        kinds = "LTDQZ"
        plan = [(kinds[int(rng.integers(0, 5))], int(rng.integers(1, 30))) for _ in range(int(rng.integers(3, 14)))]
        add("random", plan, default_params(min_silence=int(rng.integers(1, 9)), min_speech=int(rng.integers(1, 9)), pad=int(rng.integers(0, 6)),
                                           F=int(rng.integers(2, 60)), q_permille=int(rng.integers(0, 1001))))
    return out


def random_case(rng):
    """One small random recording and parameter set (the host program's random list)."""
    kinds = "LTDQZ"
    plan = [(kinds[int(rng.integers(0, 5))], int(rng.integers(1, 24))) for _ in range(int(rng.integers(1, 10)))]
    P = default_params(min_silence=int(rng.integers(1, 9)), min_speech=int(rng.integers(1, 9)), pad=int(rng.integers(0, 6)),
                       F=int(rng.integers(2, 50)), q_permille=int(rng.integers(0, 1001)))
    buf, n = render(rng, plan, int(rng.integers(0, HOP)))
    return buf, n, P


def long_case(tile=1024, tiles=39, F=1500):
    """One recording of about 40 000 frames whose events straddle the edges of `tile`-frame blocks: a dead-band run after speech and one after
    silence across an edge, a region across an edge, and an all-speech stretch of several F so that split searches cross edges."""
    rng = np.random.default_rng(77)
    plan, t = [], 0

    def upto(target, kind):
        nonlocal t
        assert target > t
        plan.append((kind, target - t))
        t = target

    upto(1 * tile - 20, "Q"); upto(1 * tile - 6, "L"); upto(1 * tile + 9, "D"); upto(2 * tile - 30, "Q")     # dead band after speech over edge 1
    upto(2 * tile - 5, "D"); upto(2 * tile + 5, "D"); upto(2 * tile + 40, "L")                                # dead band after silence over edge 2
    upto(3 * tile - 50, "Q"); upto(3 * tile + 50, "L")                                                        # a region over edge 3
    upto(5 * tile - 300, "Q"); upto(5 * tile - 10, "T"); upto(5 * tile + 10, "Q"); upto(5 * tile + 400, "T")
    upto(8 * tile + 100, "Q")
    upto(8 * tile + 100 + 6 * F + 333, "L")                                                                   # splits: searches of F / 2 + 1 frames
    upto(20 * tile, "Q")
    while t < tiles * tile - 700:                                                                             # short bursts to the end
        upto(t + int(rng.integers(20, 400)), "LT"[int(rng.integers(0, 2))])
        upto(t + int(rng.integers(10, 200)), "QD"[int(rng.integers(0, 4)) == 0])
    upto(tiles * tile - 3, "L")                                                                               # speech up to the very end: the last run closes at T
    buf, n = render(rng, plan, cut=77)
    return buf, n, default_params(min_silence=50, min_speech=25, pad=20, F=F)
