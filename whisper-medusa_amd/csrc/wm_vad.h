// wm_vad.h — the arithmetic of the speech-window detector that is plain C++ (include/wm.h wm_vad_windows): the energy of one frame,
// the per-region stage (merge, drop, pad) and the split-and-pack loop.  k_vad_* in wm_vad.hip run these functions; tests/vad_host.cpp compiles
// them with the host compiler and holds them against tests/vad_ref.py without a GPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VAD_HD __host__ __device__ __forceinline__
#else
#define VAD_HD inline
#endif

#define VAD_HOP 160                 // samples per frame: the log-mel's hop, a frame index is a mel frame index
#define VAD_LANES 16                // partial sums per frame: sixteen neighbouring lanes read sixteen neighbouring floats

// p_j = sum over i = 0..9 of x[16 i + j]^2, i ascending, every term a rounded multiply followed by a rounded add (no fused multiply-add).
// x: the frame's first sample; n_rem: the samples of the recording from there on, samples behind them count as 0 and are not read.
VAD_HD float vad_energy_partial(const float* x, int j, long long n_rem)
{
#pragma clang fp contract(off)
    float p = 0.f;
    for (int i = 0; i < VAD_HOP / VAD_LANES; ++i) {
        const int k = VAD_LANES * i + j;
        const float v = k < n_rem ? x[k] : 0.f;
        const float sq = v * v;
        p = p + sq;
    }
    return p;
}

// the fold of the sixteen partial sums: p_j += p_{j+8}, p_j += p_{j+4}, p_j += p_{j+2}, p_0 += p_1 (the kernel does the same with lane shuffles)
VAD_HD float vad_energy_fold(float* p)
{
#pragma clang fp contract(off)
    for (int o = VAD_LANES / 2; o > 0; o >>= 1)
        for (int j = 0; j < o; ++j) p[j] = p[j] + p[j + o];
    return p[0];
}

VAD_HD float vad_energy_frame(const float* x, long long n_rem)
{
    float p[VAD_LANES];
    for (int j = 0; j < VAD_LANES; ++j) p[j] = vad_energy_partial(x, j, n_rem);
    return vad_energy_fold(p);
}

// The per-region stage.  bnd: the n_bnd (even) ascending positions at which s changes, s[-1] = s[T] = 0: runs [bnd[2i], bnd[2i+1]).  Merge
// neighbours with a gap below min_silence, drop merged regions shorter than min_speech, pad (neighbours with gap g: pad each if g >= 2 pad, else
// both meet at b + g / 2; the first start max(0, a - pad), the last stop min(T, b + pad)).  One forward walk: a merged region is final when the
// next run does not join it, a kept region's stop is final when the next kept region is known.  Writes at most cap pairs to out (may alias bnd:
// pair k is written after run k was read), returns the count, which may exceed cap.
VAD_HD int vad_regions(const int* bnd, int n_bnd, int T, int min_silence, int min_speech, int pad, int* out, int cap)
{
    int n = 0;
    bool have_cur = false, have_prev = false;
    int ca = 0, cb = 0, pa = 0, pb = 0;             // the merged region being grown; the kept region whose stop is not padded yet
    for (int i = 0; i <= n_bnd / 2; ++i) {
        const bool last = i == n_bnd / 2;
        int a = 0, b = 0;
        if (!last) { a = bnd[2 * i]; b = bnd[2 * i + 1]; }
        if (!last && have_cur && a - cb < min_silence) { cb = b; continue; }
        if (have_cur && cb - ca >= min_speech) {    // the merged region [ca, cb) is kept
            int na = ca;
            if (have_prev) {
                const int g = ca - pb;
                if (g >= 2 * pad) { pb += pad; na = ca - pad; }
                else { pb += g / 2; na = pb; }
                if (n < cap) { out[2 * n] = pa; out[2 * n + 1] = pb; }
                ++n;
            } else
                na = ca - pad > 0 ? ca - pad : 0;
            pa = na; pb = cb; have_prev = true;
        }
        if (!last) { ca = a; cb = b; have_cur = true; }
    }
    if (have_prev) {
        pb = pb + pad < T ? pb + pad : T;
        if (n < cap) { out[2 * n] = pa; out[2 * n + 1] = pb; }
        ++n;
    }
    return n;
}

// The split-and-pack loop over the padded regions.  A region longer than F is cut at c = argmin(lo, hi): the frame of smallest E (bit-pattern
// order, smallest t among equals) in [a + F/2, a + F], ends inclusive.  The pieces are packed greedily: a window opens at a piece's start u and
// absorbs following pieces while stop - u <= F.  Every caller runs the loop with the same values (on the device argmin is a block-wide reduction
// that every thread enters); only `writer` stores.  Writes at most cap pairs, returns the count, which may exceed cap.
template <class ArgMin>
VAD_HD int vad_split_pack(const int* regions, int n_regions, int F, ArgMin argmin, bool writer, int* out, int cap)
{
    int n = 0, u = 0, v = 0;
    bool open = false;
    for (int r = 0; r < n_regions; ++r) {
        int a = regions[2 * r];
        const int b = regions[2 * r + 1];
        for (;;) {
            int stop = b;
            if (b - a > F) stop = argmin(a + F / 2, a + F);
            if (open && stop - u <= F) v = stop;
            else {
                if (open) {
                    if (writer && n < cap) { out[2 * n] = u; out[2 * n + 1] = v; }
                    ++n;
                }
                u = a; v = stop; open = true;
            }
            if (stop == b) break;
            a = stop;
        }
    }
    if (open) {
        if (writer && n < cap) { out[2 * n] = u; out[2 * n + 1] = v; }
        ++n;
    }
    return n;
}
