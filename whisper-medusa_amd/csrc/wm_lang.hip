// wm_lang.hip — language detection that stays on the device (include/wm.h wm_detect_language / wm_lang_pick_rows): what HF's
// WhisperGenerationMixin.detect_language does with the logits row behind <|startoftranscript|> — every id that is no language token masked to -inf,
// then argmax — as a pick among the candidate ids alone.
//   k_lang_pick: grid (rows) x 256.  Thread t < n gathers candidate t's value from the Vpad-strided fp32 row; the (value, id) pairs are reduced by
//                wave64 shuffles, then one LDS round across the four waves.  Order: value descending, then id ascending — a total order on distinct
//                ids, so the winner does not depend on which lane or wave a candidate lands in.  No atomics, no vocabulary sweep.
#include <climits>
#include <cmath>
#include <set>
#include "wm_internal.h"

// (v, i) <- the better of (v, i) and (ov, oi): the larger value, among equal values the smaller id
__device__ __forceinline__ void lang_better(float& v, int& i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ void __launch_bounds__(256)
k_lang_pick(const float* __restrict__ logits, int Vpad, const int* __restrict__ lang_ids, int n, int* __restrict__ out)
{
    __shared__ float wv[4];
    __shared__ int wi[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    float v = -INFINITY; int id = INT_MAX;                    // (a lane without a candidate loses every comparison, ties included)
    if (tid < n) {
        id = lang_ids[tid];
        v = logits[(size_t)row * Vpad + id];
        if (!(v == v)) v = -INFINITY;                         // NaN counts as -inf
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(id, o, 64);
        lang_better(v, id, ov, oi);
    }
    if ((tid & 63) == 0) { wv[tid >> 6] = v; wi[tid >> 6] = id; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) lang_better(v, id, wv[w], wi[w]);
        out[row] = id;
    }
}

// checks of the candidate list (errors under `who`), then its upload to ctx->lang_ids; returns with the stream idle
static int lang_ids_upload(wm_ctx* ctx, const char* who, const int32_t* lang_ids, int n)
{
    const std::string w = std::string(who) + ": ";
    if (!lang_ids) { ctx->err = w + "null lang_ids"; return WM_ERR_ARG; }
    if (n < 1 || n > WM_LANG_MAX) { ctx->err = w + "n must be in [1, " + std::to_string(WM_LANG_MAX) + "] language ids"; return WM_ERR_ARG; }
    std::set<int> seen;
    for (int i = 0; i < n; ++i) {
        if (lang_ids[i] < 0 || lang_ids[i] >= ctx->V) { ctx->err = w + "language id " + std::to_string(lang_ids[i]) + " outside the vocabulary"; return WM_ERR_ARG; }
        if (!seen.insert(lang_ids[i]).second) { ctx->err = w + "language id " + std::to_string(lang_ids[i]) + " given twice (ids must be distinct)"; return WM_ERR_ARG; }
    }
    WM_HIP(hipSetDevice(ctx->device));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    WM_HIP(hipMemcpyAsync(ctx->lang_ids, lang_ids, n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

// k_lang_pick over the first `rows` rows of ctx->logits -> ctx->lang_out[0 .. rows)
static int lang_pick_launch(wm_ctx* ctx, int rows, int n)
{
    k_lang_pick<<<dim3(rows), dim3(256), 0, ctx->stream>>>(ctx->logits, ctx->Vpad, ctx->lang_ids, n, ctx->lang_out);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

// HF detect_language: one base pass over the start token for the B resident clips, then the pick; B ints come back
extern "C" int wm_detect_language(wm_ctx* ctx, int B, const int32_t* lang_ids, int n, int32_t start_token, int32_t* out, float* ms)
{
    if (!ctx) return WM_ERR_ARG;
    if (!out) { ctx->err = "wm_detect_language: null out"; return WM_ERR_ARG; }
    if (start_token < 0 || start_token >= ctx->V) { ctx->err = "wm_detect_language: start_token outside the vocabulary"; return WM_ERR_ARG; }
    if (ctx->beam_expanded) { if (int rc = wm_beam_compact(ctx)) return rc; }      // (a beam decode that was never run to its end)
    if (ctx->Benc < 1 || B != ctx->Benc) { ctx->err = "wm_detect_language: call wm_encode with the same B first"; return WM_ERR_STATE; }
    if (B > ctx->maxB || B > ctx->Rcap) { ctx->err = "wm_detect_language: B exceeds max_batch"; return WM_ERR_ARG; }
    if (int rc = lang_ids_upload(ctx, "wm_detect_language", lang_ids, n)) return rc;
    hipStream_t st = ctx->stream;
    wm_decode_invalidate(ctx);
    // the scalars a plain base pass reads (wm_forward_logits sets the same ones); the decode's come back on every exit path
    GenDev g = ctx->gp;
    g.K = ctx->K; g.V = ctx->V; g.Vpad = ctx->Vpad; g.Tids = ctx->Tal; g.vanilla = 1; g.sib = 0; g.fuse = 0;
    wm_scalars_swap swap(ctx, g, ctx->ts);
    const int Tids = ctx->Tal;
    std::vector<int> tok(B, start_token), zero(B, 0), one(B, 1);
    WM_HIP(hipEventRecord(ctx->ev0, st));
    WM_HIP(hipMemcpy2DAsync(ctx->ids, (size_t)Tids * sizeof(int), tok.data(), sizeof(int), sizeof(int), B, hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(ctx->kvlen, zero.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(ctx->L, one.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipStreamSynchronize(st));       // (pageable host vectors)
    if (int rc = wm_dec_pass(ctx, 0, B, 1, 0, 0, 0)) return rc;     // row b of ctx->logits = stream b's base logits at position 0
    if (int rc = lang_pick_launch(ctx, B, n)) return rc;
    WM_HIP(hipMemcpyAsync(out, ctx->lang_out, B * sizeof(int), hipMemcpyDeviceToHost, st));
    WM_HIP(hipEventRecord(ctx->ev1, st));
    WM_HIP(hipEventSynchronize(ctx->ev1));
    WM_HIP(hipStreamSynchronize(st));
    if (ms) WM_HIP(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return WM_OK;
}

// Language-pick parity tap: caller-given rows through k_lang_pick alone (include/wm.h)
extern "C" int wm_lang_pick_rows(wm_ctx* ctx, int R, const float* logits, const int32_t* lang_ids, int n, int32_t* out)
{
    if (!ctx) return WM_ERR_ARG;
    if (R < 1 || !logits || !out) { ctx->err = "wm_lang_pick_rows: bad arguments"; return WM_ERR_ARG; }
    if (int rc = lang_ids_upload(ctx, "wm_lang_pick_rows", lang_ids, n)) return rc;
    hipStream_t st = ctx->stream;
    wm_decode_invalidate(ctx);
    const wm_tap_stage s{ctx, "wm_lang_pick_rows", 0, WM_TAP_ROWS};       // rows alone: no prefixes, no lengths
    return wm_tap_groups(s, R, logits, nullptr, nullptr, [&](int r0, int nr) {
        if (int rc = lang_pick_launch(ctx, nr, n)) return rc;
        WM_TAP_HIP(s, hipMemcpyAsync(out + r0, ctx->lang_out, nr * sizeof(int), hipMemcpyDeviceToHost, st));
        return WM_OK;
    });
}
