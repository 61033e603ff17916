// wm_merge.hip — stitching the token lists of overlapping long-form windows on the device (include/wm.h wm_merge_windows): what
// transformers' _find_longest_common_sequence (models/whisper/tokenization_whisper.py) does per recording with one numpy compare per shift — a
// fault-tolerant sliding match of the carried left sequence against the next window, cut at the mid-point of the best overlap — stated as one
// slice [a, b) per window.
//   k_merge_windows: grid (clips) x 256.  A clip's boundaries are serial (each starts from the previous one's right_mid), its shifts are not: the
//                    carried left sequence and the right window sit in LDS (ids and times, 8 KB), thread t counts the matches of shifts t + 1,
//                    t + 257, ..  Neighbouring threads read neighbouring left words and largely the same right words.  The counts are integers;
//                    the best (score, i) is reduced by wave64 shuffles, then one LDS round across the four waves, under the total order "score
//                    descending, i ascending" (HF scans i upward with a strict >).  No atomics.
#include <climits>
#include "wm_internal.h"

struct wm_merge_state {
    DevBuf<int> dev;                    // [first C+1 | lens W | tokens W*Tp | times W*Tp | keep 2W], 4-byte words
    std::vector<int32_t> host;          // the upload, packed in the same order
    hipEvent_t ev0 = nullptr, ev1 = nullptr;     // (its own pair: the context's may belong to a decode in progress)
    ~wm_merge_state() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); }
};

void wm_merge_free(wm_ctx* ctx) { delete ctx->merge_state; ctx->merge_state = nullptr; }

// (s, i) <- the better of (s, i) and (os, oi): the larger score, among equal scores the smaller shift
__device__ __forceinline__ void merge_better(double& s, int& i, double os, int oi)
{
    if (os > s || (os == s && oi < i)) { s = os; i = oi; }
}

// HF's `matches / i + eps`, eps = i / 10000.0, in Python floats: two correctly rounded divisions and one addition
__device__ __forceinline__ double merge_score(int matches, int i)
{
#pragma clang fp contract(off)
    const double q = (double)matches / (double)i;
    const double eps = (double)i / 10000.0;
    return q + eps;
}

template <bool TIMES>
__device__ __forceinline__ int merge_count(const int* lid, const int* rid, const float* lt, const float* rt, int ls, int rs, int n)
{
    int m = 0;
    for (int k = 0; k < n; ++k) {
        bool eq = lid[ls + k] == rid[rs + k];
        if (TIMES) eq = eq && lt[ls + k] <= rt[rs + k];
        m += eq ? 1 : 0;
    }
    return m;
}

__global__ void __launch_bounds__(256)
k_merge_windows(const int* __restrict__ first, const int* __restrict__ tokens, int Tp, const int* __restrict__ lens,
                const float* __restrict__ times /* null: ids alone */, int* __restrict__ keep)
{
    __shared__ int lid[WM_MERGE_LEN_MAX], rid[WM_MERGE_LEN_MAX];
    __shared__ float lt[WM_MERGE_LEN_MAX], rt[WM_MERGE_LEN_MAX];
    __shared__ double ws[4];
    __shared__ int wi[4];
    __shared__ int best_i;
    const int c = blockIdx.x, tid = threadIdx.x;
    const int w0 = first[c], w1 = first[c + 1];
    // every branch on R, prev, L below is uniform over the block: the barriers are reached by all threads or by none
    int L = 0, a = 0, prev = -1;            // the carried left sequence lid[0 .. L) is window prev from a on
    for (int w = w0; w < w1; ++w) {
        const int R = lens[w];
        if (R == 0) {                       // an empty window is no link of the chain (the pipeline never appends it)
            if (tid == 0) { keep[2 * w] = 0; keep[2 * w + 1] = 0; }
            continue;
        }
        if (prev < 0) {
            for (int k = tid; k < R; k += 256) { lid[k] = tokens[(size_t)w * Tp + k]; lt[k] = times ? times[(size_t)w * Tp + k] : 0.f; }
            L = R; a = 0; prev = w;
            __syncthreads();
            continue;
        }
        for (int k = tid; k < R; k += 256) { rid[k] = tokens[(size_t)w * Tp + k]; rt[k] = times ? times[(size_t)w * Tp + k] : 0.f; }
        __syncthreads();
        double bs = -1.0; int bi = INT_MAX;                   // (a thread without a counting shift loses every comparison)
        for (int i = tid + 1; i < L + R; i += 256) {
            const int ls = max(0, L - i), rs = max(0, i - L), n = min(L, L + R - i) - ls;
            const int m = times ? merge_count<true>(lid, rid, lt, rt, ls, rs, n) : merge_count<false>(lid, rid, lt, rt, ls, rs, n);
            if (m > 1) merge_better(bs, bi, merge_score(m, i), i);
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double os = __shfl_xor(bs, o, 64); const int oi = __shfl_xor(bi, o, 64);
            merge_better(bs, bi, os, oi);
        }
        if ((tid & 63) == 0) { ws[tid >> 6] = bs; wi[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < 4; ++q) merge_better(bs, bi, ws[q], wi[q]);
            best_i = bi;
        }
        __syncthreads();
        const int i = best_i;
        int left_mid = L, right_mid = 0;                      // no counting shift: HF's default (L, L, 0, 0), a plain concatenation
        if (i != INT_MAX) {
            left_mid = (max(0, L - i) + min(L, L + R - i)) / 2;
            right_mid = (max(0, i - L) + min(R, i)) / 2;
        }
        if (tid == 0) { keep[2 * prev] = a; keep[2 * prev + 1] = a + left_mid; }
        // the next left sequence: right[right_mid ..).  Every read of lid / lt of this boundary lies two barriers back
        const int nL = R - right_mid;
        for (int k = tid; k < nL; k += 256) { lid[k] = rid[right_mid + k]; lt[k] = rt[right_mid + k]; }
        __syncthreads();
        L = nL; a = right_mid; prev = w;
    }
    if (prev >= 0 && tid == 0) { keep[2 * prev] = a; keep[2 * prev + 1] = lens[prev]; }
}

extern "C" int wm_merge_windows(wm_ctx* ctx, int C, const int32_t* first, const int32_t* tokens, int Tmax, const int32_t* lens, const float* times,
                                int32_t* keep, float* ms)
{
    if (!ctx) return WM_ERR_ARG;
    if (ms) *ms = 0.f;
    if (!first || !tokens || !lens || !keep) { ctx->err = "wm_merge_windows: null pointer (first, tokens, lens, keep)"; return WM_ERR_ARG; }
    if (C < 1 || C > WM_MERGE_WINDOWS_MAX) { ctx->err = "wm_merge_windows: C must be in [1, " + std::to_string(WM_MERGE_WINDOWS_MAX) + "] clips"; return WM_ERR_ARG; }
    if (Tmax < 1) { ctx->err = "wm_merge_windows: Tmax must be at least 1"; return WM_ERR_ARG; }
    if (first[0] != 0) { ctx->err = "wm_merge_windows: first[0] must be 0"; return WM_ERR_ARG; }
    for (int c = 0; c < C; ++c)
        if (first[c + 1] < first[c]) { ctx->err = "wm_merge_windows: first must ascend (first[" + std::to_string(c + 1) + "] < first[" + std::to_string(c) + "])"; return WM_ERR_ARG; }
    const int W = first[C];
    if (W > WM_MERGE_WINDOWS_MAX) { ctx->err = "wm_merge_windows: " + std::to_string(W) + " windows exceed WM_MERGE_WINDOWS_MAX = " + std::to_string(WM_MERGE_WINDOWS_MAX); return WM_ERR_ARG; }
    const int cap = std::min(Tmax, WM_MERGE_LEN_MAX);
    int Tp = 1;                                               // the packed row stride: the longest window of the call
    for (int w = 0; w < W; ++w) {
        if (lens[w] < 0 || lens[w] > cap) {
            ctx->err = "wm_merge_windows: lens[" + std::to_string(w) + "] = " + std::to_string(lens[w]) + " outside [0, min(Tmax, WM_MERGE_LEN_MAX) = " + std::to_string(cap) + "]";
            return WM_ERR_ARG;
        }
        Tp = std::max(Tp, (int)lens[w]);
    }
    if (W == 0) return WM_OK;
    if (!ctx->merge_state) ctx->merge_state = new wm_merge_state();
    wm_merge_state& S = *ctx->merge_state;
    WM_HIP(hipSetDevice(ctx->device));
    if (!S.ev0) WM_HIP(hipEventCreate(&S.ev0));
    if (!S.ev1) WM_HIP(hipEventCreate(&S.ev1));
    const size_t o_first = 0, o_lens = o_first + C + 1, o_tok = o_lens + W, o_time = o_tok + (size_t)W * Tp,
                 o_keep = o_time + (times ? (size_t)W * Tp : 0), n_up = o_keep, n_all = o_keep + 2 * (size_t)W;
    S.host.assign(n_up, 0);
    std::memcpy(S.host.data() + o_first, first, (C + 1) * sizeof(int32_t));
    std::memcpy(S.host.data() + o_lens, lens, W * sizeof(int32_t));
    for (int w = 0; w < W; ++w) {
        std::memcpy(S.host.data() + o_tok + (size_t)w * Tp, tokens + (size_t)w * Tmax, lens[w] * sizeof(int32_t));
        if (times) std::memcpy(S.host.data() + o_time + (size_t)w * Tp, times + (size_t)w * Tmax, lens[w] * sizeof(float));
    }
    hipStream_t st = ctx->stream;
    WM_HIP(hipStreamSynchronize(st));                         // (the workspace may grow: nothing of an earlier call is in flight)
    WM_HIP(S.dev.reserve(n_all));
    int* d = S.dev;
    WM_HIP(hipEventRecord(S.ev0, st));
    WM_HIP(hipMemcpyAsync(d, S.host.data(), n_up * sizeof(int32_t), hipMemcpyHostToDevice, st));
    k_merge_windows<<<dim3(C), dim3(256), 0, st>>>(d + o_first, d + o_tok, Tp, d + o_lens,
                                                  times ? reinterpret_cast<const float*>(d + o_time) : nullptr, d + o_keep);
    WM_HIP(hipGetLastError());
    WM_HIP(hipMemcpyAsync(keep, d + o_keep, 2 * (size_t)W * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    WM_HIP(hipEventRecord(S.ev1, st));
    WM_HIP(hipEventSynchronize(S.ev1));
    WM_HIP(hipStreamSynchronize(st));
    if (ms) WM_HIP(hipEventElapsedTime(ms, S.ev0, S.ev1));
    return WM_OK;
}
