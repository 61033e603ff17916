// wm_vad.hip — speech windows of long recordings on the device (include/wm.h wm_vad_windows): an energy detector with hysteresis,
// regions merged, dropped and padded, long regions cut at their quietest frame, the pieces packed into windows of at most F frames.  All
// per-frame work is parallel over frames; a recording owns T / VAD_TILE + 1 tiles of VAD_TILE frame positions (0 .. T inclusive: position T is
// where a last run closes), a block works on one tile and finds its recording by a binary search over the tile offsets.  Scan state crosses
// blocks by chained launches (tile summaries, a scan of the summaries, apply); no block waits on another inside a kernel.
//   k_vad_energy    grid (tiles, 4) x 256: 16 lanes per frame (csrc/wm_vad.h), E as float32; the first radix digit's histogram
//   k_vad_hist      grid (tiles) x 256, passes 1..3 of the radix select over E's bit patterns: LDS histogram, merged with integer atomics
//   k_vad_keys      R and the thresholds from the four histograms; per tile the largest "2 t + on" over its decisive frames
//   k_vad_scan      one block per recording: exclusive scan of the tile summaries (maximum, or sum)
//   k_vad_state     s[t] from the running maximum, one byte per position; per tile the count of positions with s[t] != s[t-1]
//   k_vad_compact   those positions, ascending, per recording
//   k_vad_regions   one block per recording: one lane walks the runs (merge, drop, pad) and the packing; the search for the quietest frame of a
//                   split is a reduction over all 256 threads
// Integers and bit patterns only, integer atomics only, plain vector stores: two runs give the same bytes.
#include <climits>
#include <cmath>
#include "wm_internal.h"
#include "wm_vad.h"

#define VAD_TILE 1024               // frame positions per tile: 256 threads x 4 consecutive positions

struct wm_vad_state {
    DevBuf<int> meta;                   // [tile0 C+1 | T C | nsamp (2 words each) C | reg0 C+1 | win0 C+1]
    DevBuf<float> E;                    // [tiles * VAD_TILE]
    DevBuf<unsigned char> s;            // [tiles * VAD_TILE]
    DevBuf<int> bnd;                    // [tiles * VAD_TILE]
    DevBuf<unsigned> hist;              // [C][4][256]
    DevBuf<float> thr;                  // [C][4]: R, thr_on, thr_off
    DevBuf<int> tsum, tpre;             // [tiles] a tile's summary and the scan over the tiles in front of it
    DevBuf<int> tot;                    // [C] boundary positions per recording
    DevBuf<int> reg, win;               // [region slots][2], [window slots][2]
    DevBuf<int> cnt;                    // [C][2] regions, windows
    std::vector<int32_t> host, back;    // the upload (meta, then the region and window slots of every recording); the counts
    hipEvent_t ev0 = nullptr, ev1 = nullptr;     // (its own pair: the context's may belong to a decode in progress)
    ~wm_vad_state() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); }
};

void wm_vad_free(wm_ctx* ctx) { delete ctx->vad_state; ctx->vad_state = nullptr; }

// the recording of tile b: the last c with tile0[c] <= b (tile0 ascends strictly, tile0[C] = the number of tiles)
__device__ __forceinline__ int vad_clip_of(const int* __restrict__ tile0, int C, int b)
{
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile0[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// exclusive scan over the block's 256 threads (maximum with identity -1, or sum with identity 0) and the block's total; w4: 4 ints of LDS
template <bool MAX>
__device__ __forceinline__ int vad_block_scan(int v, int* w4, int& total)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v = MAX ? max(v, u) : v + u;
    }
    int ex = __shfl_up(v, 1, 64);
    if (lane == 0) ex = MAX ? -1 : 0;
    __syncthreads();                                          // (w4 may still be read from an earlier scan)
    if (lane == 63) w4[w] = v;
    __syncthreads();
    int pre = MAX ? -1 : 0, all = MAX ? -1 : 0;
    for (int q = 0; q < 4; ++q) {
        const int x = w4[q];
        if (q < w) pre = MAX ? max(pre, x) : pre + x;
        all = MAX ? max(all, x) : all + x;
    }
    total = all;
    return MAX ? max(pre, ex) : pre + ex;
}

__global__ void __launch_bounds__(256)
k_vad_energy(const float* __restrict__ x, long long n_max, const int* __restrict__ tile0, const int* __restrict__ Ts, const long long* __restrict__ nsamp,
             int C, float* __restrict__ E, unsigned* hist)
{
    __shared__ unsigned h[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int c = vad_clip_of(tile0, C, b);
    const int T = Ts[c];
    const long long n = nsamp[c];
    const float* xc = x + (size_t)c * (size_t)n_max;
    h[tid] = 0;
    __syncthreads();
    const int t_base = (b - tile0[c]) * VAD_TILE + blockIdx.y * (VAD_TILE / 4);
    const int j = tid & 15;
    for (int k = tid >> 4; k < VAD_TILE / 4; k += 16) {       // (uniform trip count: the shuffles below see all 16 lanes of a frame)
        const int t = t_base + k;
        const bool live = t < T;
        float p = 0.f;
        if (live) p = vad_energy_partial(xc + (size_t)t * VAD_HOP, j, n - (long long)t * VAD_HOP);
        {
#pragma clang fp contract(off)
            p = p + __shfl_down(p, 8, 16);
            p = p + __shfl_down(p, 4, 16);
            p = p + __shfl_down(p, 2, 16);
            p = p + __shfl_down(p, 1, 16);
        }
        if (live && j == 0) {
            E[(size_t)b * VAD_TILE + blockIdx.y * (VAD_TILE / 4) + k] = p;
            atomicAdd(&h[__float_as_uint(p) >> 24], 1u);
        }
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&hist[((size_t)c * 4 + 0) * 256 + tid], h[tid]);
}

// The radix select's state in front of pass `npass`: the digits chosen by passes 0 .. npass-1 as the prefix, the rank left among the values under
// that prefix.  Every thread of the block enters; lds: 4 + 2 ints.
__device__ __forceinline__ void vad_select(const unsigned* __restrict__ hist_c, int npass, int rank, int* lds, unsigned& prefix, int& rank_left)
{
    const int tid = threadIdx.x;
    unsigned pre = 0;
    int rk = rank;
    for (int p = 0; p < npass; ++p) {
        const int cnt = (int)hist_c[p * 256 + tid];
        int total;
        const int ex = vad_block_scan<false>(cnt, lds, total);
        if (ex <= rk && rk < ex + cnt) { lds[4] = tid; lds[5] = rk - ex; }   // exactly one bin holds the rank
        __syncthreads();
        pre = (pre << 8) | (unsigned)lds[4];
        rk = lds[5];
        __syncthreads();
    }
    prefix = pre; rank_left = rk;
}

__device__ __forceinline__ int vad_rank(int q_permille, int T) { return (int)(((long long)q_permille * (long long)(T - 1)) / 1000); }

__global__ void __launch_bounds__(256)
k_vad_hist(const float* __restrict__ E, const int* __restrict__ tile0, const int* __restrict__ Ts, int C, int q_permille, int pass, unsigned* hist)
{
    __shared__ unsigned h[256];
    __shared__ int lds[6];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int c = vad_clip_of(tile0, C, b);
    const int T = Ts[c];
    unsigned prefix; int rk;
    vad_select(hist + (size_t)c * 4 * 256, pass, vad_rank(q_permille, T), lds, prefix, rk);
    h[tid] = 0;
    __syncthreads();
    const int t0 = (b - tile0[c]) * VAD_TILE;
    const int sh = 32 - 8 * pass;                             // pass 1..3: the bits above the digit must equal the prefix
    for (int k = tid; k < VAD_TILE; k += 256)
        if (t0 + k < T) {
            const unsigned u = __float_as_uint(E[(size_t)b * VAD_TILE + k]);
            if ((u >> sh) == prefix) atomicAdd(&h[(u >> (sh - 8)) & 255u], 1u);
        }
    __syncthreads();
    if (h[tid]) atomicAdd(&hist[((size_t)c * 4 + pass) * 256 + tid], h[tid]);
}

// the key of frame t: 2 t + 1 at or above thr_on, 2 t below thr_off, -1 in the dead band: s[t] is bit 0 of the running maximum (0 if none)
__device__ __forceinline__ int vad_key(float e, int t, float thr_on, float thr_off)
{
    return e >= thr_on ? 2 * t + 1 : (e < thr_off ? 2 * t : -1);
}

__global__ void __launch_bounds__(256)
k_vad_keys(const float* __restrict__ E, const int* __restrict__ tile0, const int* __restrict__ Ts, int C, int q_permille,
           float k_on, float k_off, float abs_on, float abs_off, const unsigned* __restrict__ hist, float* thr, int* __restrict__ tsum)
{
    __shared__ int lds[6];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int c = vad_clip_of(tile0, C, b);
    const int T = Ts[c];
    unsigned bits; int rk;
    vad_select(hist + (size_t)c * 4 * 256, 4, vad_rank(q_permille, T), lds, bits, rk);
    const float R = __uint_as_float(bits);
    const float thr_on = fmaxf(R * k_on, abs_on), thr_off = fmaxf(R * k_off, abs_off);
    if (b == tile0[c] && tid == 0) { thr[4 * c] = R; thr[4 * c + 1] = thr_on; thr[4 * c + 2] = thr_off; thr[4 * c + 3] = 0.f; }
    const int t0 = (b - tile0[c]) * VAD_TILE + 4 * tid;
    int m = -1;
    for (int i = 0; i < 4; ++i)
        if (t0 + i < T) m = max(m, vad_key(E[(size_t)b * VAD_TILE + 4 * tid + i], t0 + i, thr_on, thr_off));
    int total;
    (void)vad_block_scan<true>(m, lds, total);
    if (tid == 0) tsum[b] = total;
}

// exclusive scan of a recording's tile summaries, in rounds of 256 tiles under a carried value; tot (may be null): the recording's total
template <bool MAX>
__global__ void __launch_bounds__(256)
k_vad_scan(const int* __restrict__ tile0, const int* __restrict__ tsum, int* __restrict__ tpre, int* __restrict__ tot)
{
    __shared__ int lds[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int b0 = tile0[c], b1 = tile0[c + 1];
    int carry = MAX ? -1 : 0;
    for (int r = b0; r < b1; r += 256) {                      // (uniform over the block)
        const int b = r + tid;
        const int v = b < b1 ? tsum[b] : (MAX ? -1 : 0);
        int total;
        const int ex = vad_block_scan<MAX>(v, lds, total);
        if (b < b1) tpre[b] = MAX ? max(carry, ex) : carry + ex;
        carry = MAX ? max(carry, total) : carry + total;
    }
    if (tot && tid == 0) tot[c] = carry;
}

__global__ void __launch_bounds__(256)
k_vad_state(const float* __restrict__ E, const int* __restrict__ tile0, const int* __restrict__ Ts, int C, const float* __restrict__ thr,
            const int* __restrict__ tpre, unsigned char* __restrict__ s, int* __restrict__ tsum)
{
    __shared__ int lds[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int c = vad_clip_of(tile0, C, b);
    const int T = Ts[c];
    const float thr_on = thr[4 * c + 1], thr_off = thr[4 * c + 2];
    const int t0 = (b - tile0[c]) * VAD_TILE + 4 * tid;
    int key[4], m = -1;
    for (int i = 0; i < 4; ++i) {
        key[i] = t0 + i < T ? vad_key(E[(size_t)b * VAD_TILE + 4 * tid + i], t0 + i, thr_on, thr_off) : -1;
        m = max(m, key[i]);
    }
    int total;
    int run = max(tpre[b], vad_block_scan<true>(m, lds, total));      // the running maximum in front of this thread's first position
    int prev = (t0 <= T && run >= 0) ? (run & 1) : 0, n = 0;         // s[t0 - 1]; positions from T on are 0
    unsigned packed = 0;
    for (int i = 0; i < 4; ++i) {
        run = max(run, key[i]);
        const int si = (t0 + i < T && run >= 0) ? (run & 1) : 0;      // positions from T on are 0: a last run closes at T
        packed |= (unsigned)si << (8 * i);
        n += si != prev;
        prev = si;
    }
    *reinterpret_cast<unsigned*>(s + (size_t)b * VAD_TILE + 4 * tid) = packed;
    int ex = vad_block_scan<false>(n, lds, total);
    (void)ex;
    if (tid == 0) tsum[b] = total;
}

__global__ void __launch_bounds__(256)
k_vad_compact(const unsigned char* __restrict__ s, const int* __restrict__ tile0, int C, const int* __restrict__ tpre, int* __restrict__ bnd)
{
    __shared__ int lds[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int c = vad_clip_of(tile0, C, b);
    const int t0 = (b - tile0[c]) * VAD_TILE + 4 * tid;
    const size_t at = (size_t)b * VAD_TILE + 4 * tid;
    const unsigned packed = *reinterpret_cast<const unsigned*>(s + at);
    // the recording's tiles are contiguous: the position in front of a tile's first is the last of the tile before
    int prev = t0 > 0 ? s[at - 1] : 0, n = 0;
    int si[4];
    for (int i = 0; i < 4; ++i) si[i] = (packed >> (8 * i)) & 1;
    int p = prev;
    for (int i = 0; i < 4; ++i) { n += si[i] != p; p = si[i]; }
    int total;
    int o = tpre[b] + vad_block_scan<false>(n, lds, total);
    int* out = bnd + (size_t)tile0[c] * VAD_TILE;
    p = prev;
    for (int i = 0; i < 4; ++i) {
        if (si[i] != p) out[o++] = t0 + i;
        p = si[i];
    }
}

// the frame of smallest E in [lo, hi], bit-pattern order, the smallest t among equals: every thread of the block enters, every thread returns it
struct VadArgMin {
    const float* E;                 // the recording's first frame
    unsigned long long* w4;         // 4 words of LDS
    __device__ int operator()(int lo, int hi) const
    {
        const int tid = threadIdx.x;
        unsigned long long best = ~0ull;
        for (int t = lo + tid; t <= hi; t += 256) {
            const unsigned long long k = ((unsigned long long)__float_as_uint(E[t]) << 32) | (unsigned)t;
            best = k < best ? k : best;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long u = __shfl_xor(best, o, 64);
            best = u < best ? u : best;
        }
        __syncthreads();                                      // (w4 may still be read from the search before)
        if ((tid & 63) == 0) w4[tid >> 6] = best;
        __syncthreads();
        for (int q = 0; q < 4; ++q) best = w4[q] < best ? w4[q] : best;
        return (int)(unsigned)best;
    }
};

__global__ void __launch_bounds__(256)
k_vad_regions(const float* __restrict__ E, const int* __restrict__ tile0, const int* __restrict__ Ts, const int* __restrict__ bnd,
              const int* __restrict__ n_bnd, int min_silence, int min_speech, int pad, int F,
              const int* __restrict__ reg0, const int* __restrict__ win0, int* reg, int* __restrict__ win, int* __restrict__ cnt)
{
    __shared__ unsigned long long w4[4];
    __shared__ int s_nr;
    const int c = blockIdx.x, tid = threadIdx.x;
    const size_t f0 = (size_t)tile0[c] * VAD_TILE;
    int* rc = reg + 2 * (size_t)reg0[c];
    const int rcap = reg0[c + 1] - reg0[c], wcap = win0[c + 1] - win0[c];
    if (tid == 0) s_nr = vad_regions(bnd + f0, n_bnd[c], Ts[c], min_silence, min_speech, pad, rc, rcap);
    __syncthreads();                                          // thread 0's regions are visible to the block
    const int nr = s_nr;                                      // (never above rcap: a region needs a run, rcap counts the runs T frames can hold)
    const int nw = vad_split_pack(rc, min(nr, rcap), F, VadArgMin{E + f0, w4}, tid == 0, win + 2 * (size_t)win0[c], wcap);
    if (tid == 0) { cnt[2 * c] = nr; cnt[2 * c + 1] = nw; }
}

extern "C" int wm_vad_windows(wm_ctx* ctx, int C, const float* samples, int64_t n_max, const int64_t* n_samples, const wm_vad_params* prm,
                              int32_t* n_regions, int32_t* regions, int cap_regions, int32_t* n_windows, int32_t* windows, int cap_windows,
                              float* E, float* R, float* thr_on, float* thr_off, float* ms)
{
    if (!ctx) return WM_ERR_ARG;
    if (ms) *ms = 0.f;
    if (!samples || !n_samples || !prm || !n_regions || !regions || !n_windows || !windows) {
        ctx->err = "wm_vad_windows: null pointer (samples, n_samples, params, n_regions, regions, n_windows, windows)";
        return WM_ERR_ARG;
    }
    if (C < 1 || C > WM_VAD_CLIPS_MAX) { ctx->err = "wm_vad_windows: C must be in [1, " + std::to_string(WM_VAD_CLIPS_MAX) + "] recordings"; return WM_ERR_ARG; }
    if (cap_regions < 0 || cap_windows < 0) { ctx->err = "wm_vad_windows: cap_regions and cap_windows must not be negative"; return WM_ERR_ARG; }
    const wm_vad_params& P = *prm;
    if (!(P.k_off > 0.f && P.k_off <= P.k_on) || !std::isfinite(P.k_on)) { ctx->err = "wm_vad_windows: 0 < k_off <= k_on (finite) required"; return WM_ERR_ARG; }
    if (!(P.abs_off >= 0.f && P.abs_off <= P.abs_on) || !std::isfinite(P.abs_on)) { ctx->err = "wm_vad_windows: 0 <= abs_off <= abs_on (finite) required"; return WM_ERR_ARG; }
    if (P.q_permille < 0 || P.q_permille > 1000) { ctx->err = "wm_vad_windows: q_permille must be in [0, 1000]"; return WM_ERR_ARG; }
    if (P.min_silence < 1) { ctx->err = "wm_vad_windows: min_silence must be at least 1 frame"; return WM_ERR_ARG; }
    if (P.min_speech < 1) { ctx->err = "wm_vad_windows: min_speech must be at least 1 frame"; return WM_ERR_ARG; }
    if (P.pad < 0 || P.pad > WM_VAD_FRAMES_MAX) { ctx->err = "wm_vad_windows: pad must be in [0, WM_VAD_FRAMES_MAX] frames"; return WM_ERR_ARG; }
    if (P.F < 2) { ctx->err = "wm_vad_windows: F must be at least 2 frames"; return WM_ERR_ARG; }
    if (P.min_silence > WM_VAD_FRAMES_MAX || P.min_speech > WM_VAD_FRAMES_MAX || P.F > WM_VAD_FRAMES_MAX) {
        ctx->err = "wm_vad_windows: min_silence, min_speech and F must not exceed WM_VAD_FRAMES_MAX = " + std::to_string(WM_VAD_FRAMES_MAX);
        return WM_ERR_ARG;
    }
    if (n_max < 1) { ctx->err = "wm_vad_windows: n_max must be at least 1"; return WM_ERR_ARG; }
    if (!ctx->vad_state) ctx->vad_state = new wm_vad_state();
    wm_vad_state& S = *ctx->vad_state;
    // meta: tile0 [C+1] | T [C] | (pad to an even word) n_samples [C] as 64-bit;  slot: reg0 [C+1] | win0 [C+1]
    const size_t o_tile0 = 0, o_T = (size_t)C + 1, o_ns = (2 * (size_t)C + 1 + 1) & ~(size_t)1, n_meta = o_ns + 2 * (size_t)C;
    S.host.assign(n_meta + 2 * ((size_t)C + 1), 0);
    int32_t* tile0 = S.host.data() + o_tile0;
    int32_t* Ts = S.host.data() + o_T;
    int32_t* reg0 = S.host.data() + n_meta;
    int32_t* win0 = reg0 + C + 1;
    long long frames = 0, tiles = 0, rslots = 0, wslots = 0;
    for (int c = 0; c < C; ++c) {
        const int64_t n = n_samples[c];
        if (n < 1 || n > n_max) { ctx->err = "wm_vad_windows: n_samples[" + std::to_string(c) + "] = " + std::to_string(n) + " outside [1, n_max = " + std::to_string(n_max) + "]"; return WM_ERR_ARG; }
        const int64_t T = (n + VAD_HOP - 1) / VAD_HOP;
        if (T > WM_VAD_FRAMES_MAX) { ctx->err = "wm_vad_windows: recording " + std::to_string(c) + " has " + std::to_string(T) + " frames, more than WM_VAD_FRAMES_MAX = " + std::to_string(WM_VAD_FRAMES_MAX); return WM_ERR_ARG; }
        frames += T;
        if (frames > WM_VAD_TOTAL_FRAMES_MAX) { ctx->err = "wm_vad_windows: more than WM_VAD_TOTAL_FRAMES_MAX = " + std::to_string(WM_VAD_TOTAL_FRAMES_MAX) + " frames in one call"; return WM_ERR_ARG; }
        tile0[c] = (int32_t)tiles; Ts[c] = (int32_t)T;
        std::memcpy(S.host.data() + o_ns + 2 * (size_t)c, &n, 8);
        tiles += T / VAD_TILE + 1;
        // T frames hold at most T / 2 + 1 runs, so as many regions; a window holds at least one piece, a piece is a region's rest or a cut of
        // at least F / 2 frames
        reg0[c] = (int32_t)rslots; win0[c] = (int32_t)wslots;
        rslots += T / 2 + 1;
        wslots += T / 2 + 1 + T / (P.F / 2);
    }
    tile0[C] = (int32_t)tiles; reg0[C] = (int32_t)rslots; win0[C] = (int32_t)wslots;
    WM_HIP(hipSetDevice(ctx->device));
    if (!S.ev0) WM_HIP(hipEventCreate(&S.ev0));
    if (!S.ev1) WM_HIP(hipEventCreate(&S.ev1));
    hipStream_t st = ctx->stream;
    WM_HIP(hipStreamSynchronize(st));                         // (the workspace may grow: nothing of an earlier call is in flight)
    const size_t nfr = (size_t)tiles * VAD_TILE;
    WM_HIP(S.meta.reserve(S.host.size()));
    WM_HIP(S.E.reserve(nfr));
    WM_HIP(S.s.reserve(nfr));
    WM_HIP(S.bnd.reserve(nfr));
    WM_HIP(S.hist.reserve((size_t)C * 4 * 256));
    WM_HIP(S.thr.reserve((size_t)C * 4));
    WM_HIP(S.tsum.reserve((size_t)tiles));
    WM_HIP(S.tpre.reserve((size_t)tiles));
    WM_HIP(S.tot.reserve((size_t)C));
    WM_HIP(S.reg.reserve(2 * (size_t)rslots));
    WM_HIP(S.win.reserve(2 * (size_t)wslots));
    WM_HIP(S.cnt.reserve(2 * (size_t)C));
    const int* d_tile0 = S.meta + o_tile0;
    const int* d_T = S.meta + o_T;
    const long long* d_ns = reinterpret_cast<const long long*>(S.meta + o_ns);
    const int* d_reg0 = S.meta + n_meta;
    const int* d_win0 = d_reg0 + C + 1;
    const dim3 grid((unsigned)tiles), blk(256);
    WM_HIP(hipEventRecord(S.ev0, st));
    WM_HIP(hipMemcpyAsync(S.meta, S.host.data(), S.host.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemsetAsync(S.hist, 0, (size_t)C * 4 * 256 * sizeof(unsigned), st));
    k_vad_energy<<<dim3((unsigned)tiles, 4), blk, 0, st>>>(samples, (long long)n_max, d_tile0, d_T, d_ns, C, S.E, S.hist);
    for (int pass = 1; pass < 4; ++pass) k_vad_hist<<<grid, blk, 0, st>>>(S.E, d_tile0, d_T, C, P.q_permille, pass, S.hist);
    k_vad_keys<<<grid, blk, 0, st>>>(S.E, d_tile0, d_T, C, P.q_permille, P.k_on, P.k_off, P.abs_on, P.abs_off, S.hist, S.thr, S.tsum);
    k_vad_scan<true><<<dim3(C), blk, 0, st>>>(d_tile0, S.tsum, S.tpre, nullptr);
    k_vad_state<<<grid, blk, 0, st>>>(S.E, d_tile0, d_T, C, S.thr, S.tpre, S.s, S.tsum);
    k_vad_scan<false><<<dim3(C), blk, 0, st>>>(d_tile0, S.tsum, S.tpre, S.tot);
    k_vad_compact<<<grid, blk, 0, st>>>(S.s, d_tile0, C, S.tpre, S.bnd);
    k_vad_regions<<<dim3(C), blk, 0, st>>>(S.E, d_tile0, d_T, S.bnd, S.tot, P.min_silence, P.min_speech, P.pad, P.F, d_reg0, d_win0, S.reg, S.win, S.cnt);
    WM_HIP(hipGetLastError());
    // the counts first: the outputs are written only when all of them fit
    S.back.assign(2 * (size_t)C, 0);
    WM_HIP(hipMemcpyAsync(S.back.data(), S.cnt, 2 * (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    WM_HIP(hipStreamSynchronize(st));
    long long need_r = 0, need_w = 0;
    for (int c = 0; c < C; ++c) { need_r += S.back[2 * c]; need_w += S.back[2 * c + 1]; }
    if (need_w > WM_VAD_WINDOWS_MAX) {
        ctx->err = "wm_vad_windows: " + std::to_string(need_w) + " windows exceed WM_VAD_WINDOWS_MAX = " + std::to_string(WM_VAD_WINDOWS_MAX) + " per call: split the call";
        return WM_ERR_ARG;
    }
    if (need_r > cap_regions || need_w > cap_windows) {
        ctx->err = "wm_vad_windows: the result needs " + std::to_string(need_r) + " regions and " + std::to_string(need_w) + " windows, the capacities are " +
                   std::to_string(cap_regions) + " and " + std::to_string(cap_windows);
        return WM_ERR_ARG;
    }
    size_t ar = 0, aw = 0, ae = 0;
    for (int c = 0; c < C; ++c) {
        const int nr = S.back[2 * c], nw = S.back[2 * c + 1];
        n_regions[c] = nr; n_windows[c] = nw;
        if (nr) WM_HIP(hipMemcpyAsync(regions + 2 * ar, S.reg + 2 * (size_t)reg0[c], 2 * (size_t)nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (nw) WM_HIP(hipMemcpyAsync(windows + 2 * aw, S.win + 2 * (size_t)win0[c], 2 * (size_t)nw * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (E) WM_HIP(hipMemcpyAsync(E + ae, S.E + (size_t)tile0[c] * VAD_TILE, (size_t)Ts[c] * sizeof(float), hipMemcpyDeviceToHost, st));
        ar += nr; aw += nw; ae += Ts[c];
    }
    std::vector<float> th;
    if (R || thr_on || thr_off) {
        th.resize(4 * (size_t)C);
        WM_HIP(hipMemcpyAsync(th.data(), S.thr, th.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    WM_HIP(hipEventRecord(S.ev1, st));
    WM_HIP(hipEventSynchronize(S.ev1));
    WM_HIP(hipStreamSynchronize(st));
    if (ms) WM_HIP(hipEventElapsedTime(ms, S.ev0, S.ev1));
    for (int c = 0; c < C && !th.empty(); ++c) {
        if (R) R[c] = th[4 * c];
        if (thr_on) thr_on[c] = th[4 * c + 1];
        if (thr_off) thr_off[c] = th[4 * c + 2];
    }
    return WM_OK;
}
