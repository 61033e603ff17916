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
    if (!ts.on) return make_int4(0, 0, 0, 0);          // (repetition rules alone: no timestamp mask; tb = V, nots = -1)
    return ts_verify ? ts.ver[s * WM_CAND_STRIDE + i] : ts_record(ts.st[s], cur_len, gp.begin, ts.tb, gp.V, ts.mit);
}

// ---- repetition rules (wm_set_repeat_rules; HF RepetitionPenaltyLogitsProcessor, then NoRepeatNGramLogitsProcessor, both BEFORE the
// processors above) ----
// A block that sweeps tokens [n0, n1) of a row builds, in dynamic LDS, two bitmaps over that range from the row's prefix ids (`pre`, then
// `ext`: the candidates a verify row follows): the tokens of the prefix (penalised) and the tokens that followed an earlier occurrence of
// its last g - 1 ids (banned).  The prefix is walked once per block, 256 ids at a time — never once per vocabulary element — and the
// element test is two LDS bit reads.  sh[0] collects the same two bits for one token outside the range (the probe / target).
struct RpPre { const int* pre; int len; const int* ext; int next; };
__host__ __device__ __forceinline__ int rp_words(int V) { return V / (32 * SEL_SP) + 3; }      // covers ceil(V / SEL_SP) + 4 tokens (k_score1's float4 slices)
static inline size_t rp_lds_bytes(const TsDev& ts, int V) { return ts.rp ? (size_t)(4 + 2 * rp_words(V)) * sizeof(unsigned) : 0; }
__device__ __forceinline__ int rp_tok(const RpPre& p, int j) { return j < p.len ? p.pre[j] : p.ext[j - p.len]; }
__device__ __forceinline__ void rp_build(const TsDev& ts, const RpPre& p, int n0, int n1, int probe, int V, unsigned* sh, int tid, int nthr)
{
    const int W = rp_words(V);
    for (int k = tid; k < 4 + 2 * W; k += nthr) sh[k] = 0u;
    __syncthreads();
    const int T = p.len + p.next, g = ts.rp_g;
    for (int j = tid; j < T; j += nthr) {
        const int tok = rp_tok(p, j);
        const bool in = tok >= n0 && tok < n1;
        unsigned fl = 0u;
        if (ts.rp & 1) {
            fl |= 1u;
            if (in) atomicOr(&sh[4 + ((tok - n0) >> 5)], 1u << ((tok - n0) & 31));
        }
        if ((ts.rp & 2) && T >= g && j >= g - 1) {          // the n-gram ending at j: pre[j-g+1 .. j-1] against the last g - 1 ids
            bool same = true;
            for (int k = 1; k < g && same; ++k) same = rp_tok(p, j - k) == rp_tok(p, T - k);
            if (same) {
                fl |= 2u;
                if (in) atomicOr(&sh[4 + W + ((tok - n0) >> 5)], 1u << ((tok - n0) & 31));
            }
        }
        if (tok == probe && fl) atomicOr(&sh[0], fl);
    }
    __syncthreads();
}
__device__ __forceinline__ float rp_penalise(float x, float p) { return x < 0.f ? x * p : __fdiv_rn(x, p); }
// step 1 on the raw logit of token n in [n0, n1)
__device__ __forceinline__ float rp_pen(float x, int n, int n0, const TsDev& ts, const unsigned* sh)
{
    return ((sh[4 + ((n - n0) >> 5)] >> ((n - n0) & 31)) & 1u) ? rp_penalise(x, ts.rp_pen) : x;
}
__device__ __forceinline__ bool rp_banned(int n, int n0, int V, const unsigned* sh)
{
    return (sh[4 + rp_words(V) + ((n - n0) >> 5)] >> ((n - n0) & 31)) & 1u;
}
// the prefix of a select row: the tap's own, else the stream's committed ids (+ the candidates c_0 .. c_i of verify row i)
__device__ __forceinline__ RpPre rp_row_prefix(const TsDev& ts, int verify, int s, int i, int cur_len)
{
    if (ts.rp_len) return RpPre{ts.rp_ids + (size_t)i * ts.rp_stride, ts.rp_len[i], ts.rp_ids, 0};
    return RpPre{ts.rp_ids + (size_t)s * ts.rp_stride, min(cur_len, ts.rp_stride), ts.rp_cand + s * WM_CAND_STRIDE, verify ? i + 1 : 0};
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
