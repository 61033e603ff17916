// wm_align.hip — token-level timestamps (include/wm.h wm_token_timestamps): what HF WhisperGenerationMixin._extract_token_timestamps
// computes from the cross-attentions of an autoregressive decode (transformers generation_whisper.py: _extract_token_timestamps,
// _median_filter, _dynamic_time_warping), for an engine whose Medusa loop never materialises attention weights.
//
//   replay        the final ids of every stream go through the decoder once more, teacher-forced, in 16-row tiles (the shared driver
//                 wm_dec_replay: wm_internal.h / wm_decoder.hip), up to the highest alignment layer; no heads, no vocabulary projection
//   k_align_probs behind every layer that owns alignment heads: softmax(q K^T) of those heads over the n_ctx encoder frames, from the
//                 layer's fp32 cross-attention query rows (ctx->qbuf) and the bf16 cross-K -> workspace [stream][A][N][n_ctx] fp32
//   k_align_stats mean / population std over the N rows per (head, frame)
//   k_align_norm  z-score, median filter along the frames (reflect padding), mean over the heads -> M [stream][N][F] fp32
//   k_dtw         dynamic time warping on -M, one workgroup per stream: anti-diagonal wavefront, then the back-trace by one wave
//
// Row r of a stream is the query at input position r; rows P .. T-2 are kept (N = T - P - 1: HF has no weights for the last token).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "wm_internal.h"

struct AlignStream {            // one stream of the resident group (device copy: si)
    int P, N, F, pad_;
    long long poff;             // floats into probs: [A][N][S]
    long long soff;             // floats into stats: [A][2][F] (mean, std)
    long long moff;             // floats into M: [N][F]
    long long toff;             // bytes into trace: [(N + 1)][(F + 1)]
    long long foff;             // ints into first: [N]
};

struct wm_align_state {
    DevBuf<float> probs, stats, M;
    DevBuf<unsigned char> trace;
    DevBuf<int> first;
    DevBuf<AlignStream> si;
    DevBuf<int2> heads;             // [A] (layer, head)
    DevBuf<int> lay_list;           // [A] head indices a grouped by layer
    // the group of the last call that is still resident (parity taps)
    int g0 = 0, g1 = 0, A = 0, B = 0;
    std::vector<AlignStream> host;  // [B] of the last call (offsets valid for streams in [g0, g1))
};

void wm_align_free(wm_ctx* ctx)
{
    delete ctx->align;
    ctx->align = nullptr;
}

// ---------------------------------------------------------------------------------------------
// k_align_probs: block (alignment head of this layer, stream of the group), 256 threads.  The 16 query rows of the tile against the
// head's bf16 cross-K: thread t takes frames t, t + 256, .. (one 128-byte K row each, 16 dot products against the q rows in LDS:
// fp32 FMAs, q as the bf16 hi + lo sum the decode contract feeds its cross-attention), scores to LDS [16][Spad]; then each wave
// normalises 4 rows (max, sum of exp, division) over the n_ctx valid frames and writes the kept rows.  Pad frames never leave the block.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_align_probs(const float* __restrict__ qbuf, const bf16_t* __restrict__ kx, const int* __restrict__ lay_list, const int2* __restrict__ heads,
              const AlignStream* __restrict__ si, float* __restrict__ probs, int pos0, int Mper, int d, int H, int S, int Spad)
{
    extern __shared__ float lds[];
    float* qs = lds;                    // [16][64]
    float* sc = lds + 16 * 64;          // [16][Spad]
    const int a = lay_list[blockIdx.x], s = blockIdx.y, tid = threadIdx.x;
    const AlignStream st = si[s];
    // rows of this tile that are kept: n = pos0 + r - P in [0, N)
    const int r_lo = max(0, st.P - pos0), r_hi = min(Mper, st.P + st.N - pos0);
    if (r_lo >= r_hi) return;
    const int h = heads[a].y;
    for (int i = tid; i < 16 * 64; i += 256) {
        const int r = i >> 6, j = i & 63;
        float q = 0.f;
        if (r < Mper) {
            q = qbuf[((size_t)s * Mper + r) * d + h * 64 + j];
            const float hi = bf2f(f2bf(q));
            q = hi + bf2f(f2bf(q - hi));
        }
        qs[i] = q;
    }
    __syncthreads();
    const bf16_t* K = kx + ((size_t)s * H + h) * Spad * 64;
    for (int f = tid; f < Spad; f += 256) {
        if (f < S) {
            float kf[64];
            const uint4* kr = reinterpret_cast<const uint4*>(K + (size_t)f * 64);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint4 u = kr[c];
                kf[c * 8 + 0] = __uint_as_float(u.x << 16); kf[c * 8 + 1] = __uint_as_float(u.x & 0xffff0000u);
                kf[c * 8 + 2] = __uint_as_float(u.y << 16); kf[c * 8 + 3] = __uint_as_float(u.y & 0xffff0000u);
                kf[c * 8 + 4] = __uint_as_float(u.z << 16); kf[c * 8 + 5] = __uint_as_float(u.z & 0xffff0000u);
                kf[c * 8 + 6] = __uint_as_float(u.w << 16); kf[c * 8 + 7] = __uint_as_float(u.w & 0xffff0000u);
            }
            for (int r = 0; r < 16; ++r) {
                const float4* q4 = reinterpret_cast<const float4*>(qs + r * 64);
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const float4 q = q4[c];
                    acc = fmaf(q.x, kf[c * 4 + 0], acc); acc = fmaf(q.y, kf[c * 4 + 1], acc);
                    acc = fmaf(q.z, kf[c * 4 + 2], acc); acc = fmaf(q.w, kf[c * 4 + 3], acc);
                }
                sc[r * Spad + f] = acc;
            }
        } else {
            for (int r = 0; r < 16; ++r) sc[r * Spad + f] = -INFINITY;
        }
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int r = wave * 4; r < wave * 4 + 4; ++r) {
        if (r < r_lo || r >= r_hi) continue;          // (wave-uniform)
        float* row = sc + r * Spad;
        float mx = -INFINITY;
        for (int f = lane; f < S; f += 64) mx = fmaxf(mx, row[f]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float sum = 0.f;
        for (int f = lane; f < S; f += 64) { const float e = expf(row[f] - mx); row[f] = e; sum += e; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        float* out = probs + st.poff + ((size_t)a * st.N + (pos0 + r - st.P)) * S;
        for (int f = lane; f < S; f += 64) out[f] = row[f] / sum;
    }
}

// ---------------------------------------------------------------------------------------------
// k_align_stats: per (stream, head, frame < F): mean and population standard deviation over the N rows (torch.mean / torch.std(unbiased=False)
// of _extract_token_timestamps), two passes with fp64 sums, rounded once to fp32.  grid (ceil(F / 256), A, streams)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_align_stats(const float* __restrict__ probs, const AlignStream* __restrict__ si, float* __restrict__ stats, int S)
{
    const AlignStream st = si[blockIdx.z];
    const int f = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y;
    if (st.N < 2 || f >= st.F) return;
    const float* p = probs + st.poff + (size_t)a * st.N * S + f;
    double sum = 0.0;
    for (int n = 0; n < st.N; ++n) sum += (double)p[(size_t)n * S];
    const double mean = sum / (double)st.N;
    double q = 0.0;
    for (int n = 0; n < st.N; ++n) { const double dlt = (double)p[(size_t)n * S] - mean; q += dlt * dlt; }
    float* o = stats + st.soff + (size_t)a * 2 * st.F;
    o[f] = (float)mean;
    o[st.F + f] = (float)sqrt(q / (double)st.N);
}

// NaN sorts last, as torch.sort does (a frame whose std is 0 gives 0 / 0 = NaN for every row, as in torch)
__device__ __forceinline__ void cswap(float& x, float& y)
{
    const bool sw = (x > y) || (x != x && y == y);
    const float lo = sw ? y : x, hi = sw ? x : y;
    x = lo; y = hi;
}

// ---------------------------------------------------------------------------------------------
// k_align_norm<W>: block (256 frames, row n, stream).  Per head, in the caller's order: z = (w - mean) / std of the block's frames and a halo
// of W / 2 on each side (reflected at the ends by index) to LDS, every thread sorts its W values in registers (odd-even transposition
// network) and takes the middle one; the medians are summed over the heads and divided by A.  F <= W / 2: no filter (_median_filter returns
// its input).
// ---------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256)
k_align_norm(const float* __restrict__ probs, const float* __restrict__ stats, const AlignStream* __restrict__ si, float* __restrict__ M, int A, int S)
{
    constexpr int HW = W / 2;
    __shared__ float z[256 + 2 * HW + 1];
    const AlignStream st = si[blockIdx.z];
    const int n = blockIdx.y, f0 = blockIdx.x * 256, tid = threadIdx.x, F = st.F;
    if (st.N < 2 || n >= st.N || f0 >= F) return;        // (block-uniform)
    const bool filt = F > HW;
    const int f = f0 + tid;
    float acc = 0.f;
    for (int a = 0; a < A; ++a) {
        const float* p = probs + st.poff + ((size_t)a * st.N + n) * S;
        const float* mu = stats + st.soff + (size_t)a * 2 * F;
        for (int i = tid; i < 256 + 2 * HW; i += 256) {
            int j = f0 + i - HW;
            float v = 0.f;
            if (filt) {
                if (j < 0) j = -j;
                if (j >= F) j = 2 * (F - 1) - j;
                if (j >= 0 && j < F) v = (p[j] - mu[j]) / mu[F + j];        // (outside only for halo slots no kept frame reads)
            } else if (j >= 0 && j < F) v = (p[j] - mu[j]) / mu[F + j];
            z[i] = v;
        }
        __syncthreads();
        if (f < F) {
            float med;
            if (filt) {
                float v[W];
#pragma unroll
                for (int t = 0; t < W; ++t) v[t] = z[tid + t];
#pragma unroll
                for (int pass = 0; pass < W; ++pass) {
#pragma unroll
                    for (int t = pass & 1; t + 1 < W; t += 2) cswap(v[t], v[t + 1]);
                }
                med = v[HW];
            } else med = z[tid + HW];
            acc += med;
        }
        __syncthreads();
    }
    if (f < F) M[st.moff + (size_t)n * F + f] = acc / (float)A;
}

// ---------------------------------------------------------------------------------------------
// k_dtw: _dynamic_time_warping(-M) of one stream per workgroup.  Cell (i, j), 1 <= i <= N, 1 <= j <= F, lies on anti-diagonal k = i + j and
// needs (i-1, j-1) of diagonal k - 2 and (i-1, j), (i, j-1) of diagonal k - 1: the diagonals are walked in order with one barrier each, their
// costs in a rolling window of three LDS rows indexed by i.  numpy's column-major double loop is only an iteration order: every cell gets
// the same three inputs.  Arithmetic as numpy's: cost float32, comparisons on float32, the sum double(-m) + double(c) rounded to float32.
// One trace byte per cell, row-major [(N + 1)][(F + 1)] in global memory.  Back-trace by wave 0: the 64 cells to the left of (i, j) in one
// load, the run of "left" moves found with a ballot; first[r] = time index of the first path element of text row r.  path_* (wm_dtw tap,
// may be null): the path in back-trace order.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float dtw_cost(const float* buf, int N1, int i, int j)       // cost[i][j] incl. the borders
{
    if (i == 0) return j == 0 ? 0.f : INFINITY;
    if (j == 0) return INFINITY;
    return buf[((i + j) % 3) * N1 + i];
}

__global__ void __launch_bounds__(512)
k_dtw(const float* __restrict__ M, const AlignStream* __restrict__ si, unsigned char* __restrict__ trace, int* __restrict__ first,
      int* __restrict__ path_text, int* __restrict__ path_time, int* __restrict__ path_len)
{
    extern __shared__ float buf[];      // [3][N + 1]
    const AlignStream st = si[blockIdx.x];
    const int N = st.N, F = st.F, N1 = N + 1, tid = threadIdx.x;
    if (N < 2 && !path_len) return;     // (nothing to align: the host writes zeros; the tap accepts N = 1)
    if (N < 1 || F < 1) return;
    const float* m = M + st.moff;
    unsigned char* tr = trace + st.toff;
    const size_t F1 = (size_t)F + 1;
    for (int k = 2; k <= N + F; ++k) {
        const int ilo = max(1, k - F), ihi = min(N, k - 1);
        float* cur = buf + (k % 3) * N1;
        for (int i = ilo + tid; i <= ihi; i += blockDim.x) {
            const int j = k - i;
            const float c0 = dtw_cost(buf, N1, i - 1, j - 1), c1 = dtw_cost(buf, N1, i - 1, j), c2 = dtw_cost(buf, N1, i, j - 1);
            float c; unsigned char t;
            if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
            else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
            else { c = c2; t = 2; }
            cur[i] = (float)(-(double)m[(size_t)(i - 1) * F + (j - 1)] + (double)c);
            tr[(size_t)i * F1 + j] = t;
        }
        __syncthreads();
    }
    if (tid >= 64) return;
    const int lane = tid;
    int* fr = first + st.foff;
    int i = N, j = F, len = 0;
    while (i > 0 || j > 0) {
        if (i == 0) {                   // trace[0, :] = 2: left to (0, 0); elements (-1, j - 1 - t)
            if (path_text) for (int t = lane; t < j; t += 64) { path_text[len + t] = -1; path_time[len + t] = j - 1 - t; }
            len += j; j = 0;
            continue;
        }
        if (j == 0) {                   // trace[:, 0] = 1: up
            if (lane == 0) { fr[i - 1] = -1; if (path_text) { path_text[len] = i - 1; path_time[len] = -1; } }
            len += 1; i -= 1;
            continue;
        }
        const int jj = j - lane;
        const int t = jj >= 1 ? (int)tr[(size_t)i * F1 + jj] : 3;
        const unsigned long long stop = __ballot(t != 2);
        const int run = stop ? __builtin_ctzll(stop) : 64;          // cells (i, j) .. (i, j - run + 1) move left
        if (path_text && lane < run) { path_text[len + lane] = i - 1; path_time[len + lane] = jj - 1; }
        len += run;
        if (run == 64) { j -= 64; continue; }
        const int tm = __shfl(t, run, 64);
        j -= run;
        if (tm == 3) continue;          // reached column 0 (j == 0 now)
        if (lane == 0) { fr[i - 1] = j - 1; if (path_text) { path_text[len] = i - 1; path_time[len] = j - 1; } }
        len += 1;
        i -= 1;
        if (tm == 0) j -= 1;
    }
    if (path_len && lane == 0) *path_len = len;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct ReplayHook {
    wm_align_state* al;
    const std::vector<int>* lay_off;    // [dec_layers + 1] into lay_list
    int g0, nb;
    size_t lds;
};

static int after_layer(wm_ctx* ctx, int l, int pos0, int Mper, void* arg)
{
    const ReplayHook* hk = static_cast<const ReplayHook*>(arg);
    const int o0 = (*hk->lay_off)[l], cnt = (*hk->lay_off)[l + 1] - o0;
    if (cnt == 0) return WM_OK;
    const bf16_t* kx = ctx->kx + ((size_t)l * ctx->Benc + hk->g0) * ctx->H * ctx->Spad * 64;       // the bf16 projection (also on a cross_kv_fp8 context)
    hipLaunchKernelGGL(k_align_probs, dim3(cnt, hk->nb), dim3(256), hk->lds, ctx->stream, ctx->qbuf, kx, hk->al->lay_list + o0, hk->al->heads,
                       hk->al->si, hk->al->probs, pos0, Mper, ctx->d, ctx->H, ctx->S, ctx->Spad);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

static int launch_norm(wm_ctx* ctx, wm_align_state* al, int width, int Fmax, int Nmax, int nb, int A)
{
    const dim3 grid((Fmax + 255) / 256, Nmax, nb), blk(256);
#define WM_NORM(Wv) case Wv: hipLaunchKernelGGL(k_align_norm<Wv>, grid, blk, 0, ctx->stream, al->probs, al->stats, al->si, al->M, A, ctx->S); break
    switch (width) { WM_NORM(1); WM_NORM(3); WM_NORM(5); WM_NORM(7); WM_NORM(9); WM_NORM(11); WM_NORM(13); WM_NORM(15); default: return WM_ERR_ARG; }
#undef WM_NORM
    WM_HIP(hipGetLastError());
    return WM_OK;
}

// the decimal a float time_precision was written from (0.02f -> 0.02): HF multiplies the frame index by the Python float
static double precision_decimal(float tp)
{
    char s[32];
    std::snprintf(s, sizeof(s), "%.7g", (double)tp);
    return std::strtod(s, nullptr);
}

static wm_align_state* align_state(wm_ctx* ctx)
{
    if (!ctx->align) ctx->align = new wm_align_state();
    return ctx->align;
}

extern "C" int wm_token_timestamps(wm_ctx* ctx, const wm_align_params* ap, int B, const int32_t* tokens, int Tmax, const int32_t* lens,
                                   const int32_t* n_prompt, const int32_t* num_frames, float* out, float* ms)
{
    if (!ctx) return WM_ERR_ARG;
    if (!ap || !ap->heads || !tokens || !lens || !n_prompt || !out || B < 1 || Tmax < 1) { ctx->err = "wm_token_timestamps: bad arguments"; return WM_ERR_ARG; }
    if (int rc = wm_replay_check(ctx, "wm_token_timestamps", B, Tmax, lens, n_prompt, 0)) return rc;
    const int A = ap->n_heads, W = ap->median_filter_width, S = ctx->S;
    if (A < 1 || A > 64) { ctx->err = "wm_token_timestamps: n_heads must be in 1..64"; return WM_ERR_ARG; }
    if (W < 1 || W > 15 || W % 2 == 0) { ctx->err = "wm_token_timestamps: median_filter_width must be odd, 1..15"; return WM_ERR_ARG; }
    if (!(ap->time_precision > 0.f)) { ctx->err = "wm_token_timestamps: time_precision must be positive"; return WM_ERR_ARG; }
    int lmax = -1;
    for (int a = 0; a < A; ++a) {
        const int l = ap->heads[2 * a], h = ap->heads[2 * a + 1];
        if (l < 0 || l >= ctx->cfg.dec_layers || h < 0 || h >= ctx->H) {
            ctx->err = "wm_token_timestamps: alignment head (" + std::to_string(l) + ", " + std::to_string(h) + ") out of range"; return WM_ERR_ARG; }
        lmax = std::max(lmax, l);
    }
    for (int b = 0; num_frames && b < B; ++b)
        if (num_frames[b] / 2 < 1) { ctx->err = "wm_token_timestamps: num_frames must be at least 2"; return WM_ERR_ARG; }
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    wm_align_state* al = align_state(ctx);
    const double tp = precision_decimal(ap->time_precision);

    // the replay overwrites the decode state (ids, kvlen, self K/V): begin again afterwards.  Its launches read only the shape fields of
    // the scalars; the rest stays what the last decode left.
    wm_decode_invalidate(ctx);
    GenDev g = ctx->gp;
    g.K = ctx->K; g.V = ctx->V; g.Vpad = ctx->Vpad; g.Tids = ctx->Tal;
    wm_scalars_swap swap(ctx, g, ctx->ts);

    std::vector<AlignStream>& hs = al->host;
    hs.assign(B, AlignStream{});
    for (int b = 0; b < B; ++b) {
        hs[b].P = n_prompt[b];
        hs[b].N = std::max(lens[b] - n_prompt[b] - 1, 0);
        hs[b].F = num_frames ? std::min(num_frames[b] / 2, S) : S;
        for (int t = 0; t < Tmax; ++t) out[(size_t)b * Tmax + t] = 0.f;
    }
    al->A = A; al->B = B; al->g0 = al->g1 = 0;
    // alignment heads grouped by layer, the caller's order kept inside a layer (k_align_norm sums the heads in the caller's order)
    std::vector<int> lay_off(ctx->cfg.dec_layers + 1, 0), lay_list(A);
    std::vector<int2> heads(A);
    for (int a = 0; a < A; ++a) { heads[a] = make_int2(ap->heads[2 * a], ap->heads[2 * a + 1]); lay_off[heads[a].x + 1]++; }
    for (int l = 0; l < ctx->cfg.dec_layers; ++l) lay_off[l + 1] += lay_off[l];
    { std::vector<int> fill(lay_off.begin(), lay_off.end() - 1); for (int a = 0; a < A; ++a) lay_list[fill[heads[a].x]++] = a; }
    WM_HIP(al->heads.reserve(A)); WM_HIP(al->lay_list.reserve(A));
    WM_HIP(hipMemcpyAsync(al->heads, heads.data(), A * sizeof(int2), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(al->lay_list, lay_list.data(), A * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(al->si.reserve(ctx->maxB));

    const size_t lds = (size_t)(16 * 64 + 16 * ctx->Spad) * sizeof(float);
    WM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_align_probs), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    static const size_t cap_bytes = [] { const char* v = std::getenv("WM_ALIGN_WS_MB"); return (size_t)(v ? std::max(1, std::atoi(v)) : 512) << 20; }();

    WM_HIP(hipEventRecord(ctx->ev0, st));
    std::vector<int> fr;
    for (int g0 = 0; g0 < B;) {
        // streams [g0, g1) whose probabilities fit the workspace cap (at least one)
        int g1 = g0;
        size_t np = 0, ns = 0, nm = 0, nt = 0, nf = 0;
        int maxlen = 1, Nmax = 0, Fmax = 1;
        while (g1 < B) {
            AlignStream& s = hs[g1];
            const size_t add = (size_t)A * s.N * S;
            if (g1 > g0 && (np + add) * sizeof(float) > cap_bytes) break;
            s.poff = (long long)np; s.soff = (long long)ns; s.moff = (long long)nm; s.toff = (long long)nt; s.foff = (long long)nf;
            np += add; ns += (size_t)A * 2 * s.F; nm += (size_t)s.N * s.F; nt += (size_t)(s.N + 1) * (s.F + 1); nf += (size_t)s.N;
            if (s.N >= 2) { maxlen = std::max(maxlen, lens[g1]); Nmax = std::max(Nmax, s.N); Fmax = std::max(Fmax, s.F); }
            ++g1;
        }
        const int nb = g1 - g0;
        if (Nmax >= 2) {
            WM_HIP(al->probs.reserve(np)); WM_HIP(al->stats.reserve(ns)); WM_HIP(al->M.reserve(nm));
            WM_HIP(al->trace.reserve(nt)); WM_HIP(al->first.reserve(nf));
            WM_HIP(hipMemcpyAsync(al->si, hs.data() + g0, nb * sizeof(AlignStream), hipMemcpyHostToDevice, st));
            // teacher-forced replay of the group's input positions 0 .. maxlen - 2
            ReplayHook hk{al, &lay_off, g0, nb, lds};
            wm_replay_hooks hooks; hooks.layer = after_layer; hooks.arg = &hk;
            if (int rc = wm_dec_replay(ctx, g0, nb, tokens, Tmax, lens, maxlen - 1, lmax + 1, hooks)) return rc;
            hipLaunchKernelGGL(k_align_stats, dim3((Fmax + 255) / 256, A, nb), dim3(256), 0, st, al->probs, al->si, al->stats, S);
            WM_HIP(hipGetLastError());
            if (int rc = launch_norm(ctx, al, W, Fmax, Nmax, nb, A)) return rc;
            hipLaunchKernelGGL(k_dtw, dim3(nb), dim3(512), (size_t)3 * (Nmax + 1) * sizeof(float), st, al->M, al->si, al->trace, al->first,
                               (int*)nullptr, (int*)nullptr, (int*)nullptr);
            WM_HIP(hipGetLastError());
            fr.assign(nf, 0);
            WM_HIP(hipMemcpyAsync(fr.data(), al->first, nf * sizeof(int), hipMemcpyDeviceToHost, st));
            WM_HIP(hipStreamSynchronize(st));
            for (int b = g0; b < g1; ++b) {
                const AlignStream& s = hs[b];
                if (s.N < 2) continue;      // N == 0: zeros; N == 1: HF's 0 / 0 matrix warps to 0.0 everywhere
                float* o = out + (size_t)b * Tmax;
                float last = 0.f;
                for (int n = 0; n < s.N; ++n) { last = (float)((double)fr[s.foff + n] * tp); o[s.P + n] = last; }
                for (int t = s.P + s.N; t < Tmax; ++t) o[t] = last;     // the last token repeats it; so do the positions after the stream's end
            }
        }
        al->g0 = g0; al->g1 = g1;
        g0 = g1;
    }
    WM_HIP(hipEventRecord(ctx->ev1, st));
    WM_HIP(hipEventSynchronize(ctx->ev1));
    if (ms) WM_HIP(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return WM_OK;
}

static int tap_stream(wm_ctx* ctx, int stream, const AlignStream** s)
{
    wm_align_state* al = ctx->align;
    if (!al || al->B < 1) { ctx->err = "alignment tap: call wm_token_timestamps first"; return WM_ERR_STATE; }
    if (stream < 0 || stream >= al->B) { ctx->err = "alignment tap: stream out of range"; return WM_ERR_ARG; }
    if (stream < al->g0 || stream >= al->g1) { ctx->err = "alignment tap: the stream's workspace group is no longer resident"; return WM_ERR_STATE; }
    *s = &al->host[stream];
    if ((*s)->N < 2) { ctx->err = "alignment tap: the stream has fewer than 2 aligned rows (nothing was computed)"; return WM_ERR_STATE; }
    return WM_OK;
}

extern "C" int wm_get_align_probs(wm_ctx* ctx, int stream, int a, float* out)
{
    if (!ctx || !out) return WM_ERR_ARG;
    const AlignStream* s = nullptr;
    if (int rc = tap_stream(ctx, stream, &s)) return rc;
    if (a < 0 || a >= ctx->align->A) { ctx->err = "wm_get_align_probs: head index out of range"; return WM_ERR_ARG; }
    WM_HIP(hipSetDevice(ctx->device));
    WM_HIP(hipMemcpyAsync(out, ctx->align->probs + s->poff + (size_t)a * s->N * ctx->S, (size_t)s->N * ctx->S * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

extern "C" int wm_get_align_matrix(wm_ctx* ctx, int stream, float* out)
{
    if (!ctx || !out) return WM_ERR_ARG;
    const AlignStream* s = nullptr;
    if (int rc = tap_stream(ctx, stream, &s)) return rc;
    WM_HIP(hipSetDevice(ctx->device));
    WM_HIP(hipMemcpyAsync(out, ctx->align->M + s->moff, (size_t)s->N * s->F * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

extern "C" int wm_dtw(wm_ctx* ctx, const float* matrix, int N, int F, int32_t* first_frame, int32_t* path_text, int32_t* path_time, int* path_len)
{
    if (!ctx) return WM_ERR_ARG;
    if (!matrix || N < 1 || F < 1 || N > 4096 || F > 8192 || !first_frame || !path_text || !path_time || !path_len) {
        ctx->err = "wm_dtw: bad arguments (N in 1..4096, F in 1..8192)"; return WM_ERR_ARG; }
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // buffers of its own: the workspace of the last wm_token_timestamps call stays as it is
    float* m = nullptr; unsigned char* tr = nullptr; int* iv = nullptr; AlignStream* si = nullptr;
    const size_t nm = (size_t)N * F, nt = (size_t)(N + 1) * (F + 1), ni = (size_t)N + 2 * (size_t)(N + F) + 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m), nm * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&tr), nt);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&iv), ni * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&si), sizeof(AlignStream));
    AlignStream s{}; s.N = N; s.F = F;
    int len = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(m, matrix, nm * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(si, &s, sizeof(s), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(iv, 0, ni * sizeof(int), st);
    if (e == hipSuccess) {
        int *pt = iv + N, *pm = pt + (N + F), *pl = pm + (N + F);
        hipLaunchKernelGGL(k_dtw, dim3(1), dim3(512), (size_t)3 * (N + 1) * sizeof(float), st, m, si, tr, iv, pt, pm, pl);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&len, pl, sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(first_frame, iv, N * sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess && len >= 0 && len <= N + F) {
            std::vector<int> t(len), u(len);
            e = hipMemcpyAsync(t.data(), pt, len * sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(u.data(), pm, len * sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            for (int i = 0; i < len; ++i) { path_text[i] = t[len - 1 - i]; path_time[i] = u[len - 1 - i]; }     // forward order, as numpy's [::-1]
            *path_len = len;
        }
    }
    (void)hipStreamSynchronize(st);
    if (m) (void)hipFree(m);
    if (tr) (void)hipFree(tr);
    if (iv) (void)hipFree(iv);
    if (si) (void)hipFree(si);
    if (e != hipSuccess) { ctx->err = std::string("wm_dtw: ") + hipGetErrorString(e); return WM_ERR_HIP; }
    return WM_OK;
}
