// wm_select.h — the pieces of the select stage that more than one translation unit uses: the logits processors of one element
// (proc_logit), the per-token masks of the Whisper timestamp rules (ts_mask), the finish of a row from its slice partials (ts_finish) and
// the block reductions.  wm_decoder.hip holds the select kernels of the decode loop, wm_score.hip the scoring kernels of wm_score_tokens.
#pragma once
#include "wm_internal.h"

#define SEL_SP 16

__device__ __forceinline__ float proc_logit(float x, int n, int cur_len, const GenDev& gp, const unsigned char* mask,
                                            const float* exppen)
{
    if (n == gp.eos && gp.exp_start >= 0 && cur_len > gp.exp_start) x += fabsf(x) * exppen[cur_len];
    const unsigned char mk = mask[n];
    if ((mk & 1) || ((mk & 2) && cur_len == gp.begin)) x = -INFINITY;
    return x;
}

// ---- Whisper timestamp rules (wm_decode_begin_ts; HF WhisperTimeStampLogitsProcessor.__call__, applied after the processors above) ----
// A row's per-token masks come from its prefix ids[:len] through a compact state (TsDev); the row-global log-softmax decision
// (logsumexp of the timestamps > the best text token -> all text masked) is finished by every consumer from the slice partials of the
// two regions [0, tb) and [tb, V).
__device__ __forceinline__ float ts_mask(float v, int n, int4 rec, const GenDev& gp, const TsDev& ts)
{
    if (n == ts.nots) return -INFINITY;
    if (n >= ts.tb) return (n < rec.x || n > rec.y) ? -INFINITY : v;
    return ((rec.z & 2) || ((rec.z & 1) && n < gp.eos)) ? -INFINITY : v;
}
// the row's record: base / head rows of stream s from the committed state at L; verify row i from k_cand_fin's fold
__device__ __forceinline__ int4 ts_row_record(const GenDev& gp, const TsDev& ts, int ts_verify, int s, int i, int cur_len)
{
    return ts_verify ? ts.ver[s * WM_CAND_STRIDE + i] : ts_record(ts.st[s], cur_len, gp.begin, ts.tb, gp.V, ts.mit);
}
struct TsSel { float mx; int mi; float z; int forced; };
// finish a row from its SEL_SP x 2 slice partials: the decision, then (arg-max, max, softmax denominator at 1/T) of what it leaves
__device__ __forceinline__ TsSel ts_finish(const float* p1, const float* p1t, float inv_temp)
{
    float mt = -INFINITY, ms = -INFINITY; int it = 0x7fffffff, is = 0x7fffffff;
    for (int k = 0; k < SEL_SP; ++k) {
        const float v = p1[4 * k]; const int idx = __float_as_int(p1[4 * k + 1]);
        if (v > mt || (v == mt && idx < it)) { mt = v; it = idx; }
        const float u = p1t[4 * k]; const int iu = __float_as_int(p1t[4 * k + 1]);
        if (u > ms || (u == ms && iu < is)) { ms = u; is = iu; }
    }
    float zt = 0.f, zs = 0.f, zs1 = 0.f;
    for (int k = 0; k < SEL_SP; ++k) {
        const float v = p1[4 * k], u = p1t[4 * k];
        if (v != -INFINITY) zt += p1[4 * k + 2] * expf((v - mt) * inv_temp);
        if (u != -INFINITY) { zs += p1t[4 * k + 2] * expf((u - ms) * inv_temp); zs1 += p1t[4 * k + 3] * expf(u - ms); }
    }
    TsSel r;
    r.forced = (ms != -INFINITY && ms + logf(zs1) > mt) ? 1 : 0;     // logsumexp(ts) > max(text), both shifted by the same log Z
    if (r.forced) { r.mx = ms; r.mi = is; r.z = zs; }
    else if (ms > mt) { r.mx = ms; r.mi = is; r.z = zs + (mt == -INFINITY ? 0.f : zt * expf((mt - ms) * inv_temp)); }
    else { r.mx = mt; r.mi = it; r.z = zt + (ms == -INFINITY ? 0.f : zs * expf((ms - mt) * inv_temp)); }
    return r;
}
__device__ __forceinline__ void block_argmax(float& mx, int& mi, float* sv, int* si, int tid)
{
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mx, o, 64); const int oi = __shfl_xor(mi, o, 64);
        if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
    }
    __syncthreads();
    if (lane == 0) { sv[w] = mx; si[w] = mi; }
    __syncthreads();
    mx = sv[0]; mi = si[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) if (sv[k] > mx || (sv[k] == mx && si[k] < mi)) { mx = sv[k]; mi = si[k]; }
}
__device__ __forceinline__ float block_sum(float z, float* sz, int tid)
{
    z = wave_sum(z);
    __syncthreads();
    if ((tid & 63) == 0) sz[tid >> 6] = z;
    __syncthreads();
    return (sz[0] + sz[1]) + (sz[2] + sz[3]);
}
