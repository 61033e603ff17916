// wm_score.hip — token log-probabilities and the no-speech probability (include/wm.h wm_score_tokens / wm_score_rows): what
// HF's greedy decode hands out as `scores[i]` (GenerationMixin with output_scores: the processed logits of step i, log-softmaxed by
// WhisperGenerationMixin._retrieve_avg_logprobs) and what WhisperNoSpeechDetection reads off the raw <|startoftranscript|> row, for an
// engine whose Medusa loop emits several tokens per iteration under one shared length and never keeps a logits row.
//
//   replay         the final ids of every stream go through ALL decoder layers once more, teacher-forced, in 16-row tiles (the shared driver
//                  wm_dec_replay: wm_internal.h / wm_decoder.hip); behind every tile (score_tile) the final LayerNorm and the packed
//                  vocabulary projection of the base head for the tile's rows (no Medusa heads, no Medusa-Block extra layer)
//   k_score_build  one thread per stream: the tile's row descriptors — row of input position t - 1 scores s[t] under cur_len = t, its OWN
//                  length — and, with the timestamp rules on, the row's record from the fold of its own prefix (carried from tile to tile)
//   k_score1       SEL_SP slice blocks per row: running (max, sum of exp) at temperature 1 of the processed row, text region [0, tb) and
//                  timestamp region [tb, V) apart (the partials ts_finish takes); 16-byte loads, wave64 shuffles, one LDS round
//   k_score2       one thread per row: merges the slices (ts_finish: the log-softmax decision of the timestamp rules), gathers the processed
//                  logit of the target and writes logit - max - log Z, or -inf where the target is masked
//   k_topk1        (wm_score_tokens_topk / wm_topk_rows only) behind k_score1 on the same rows, SEL_SP slice blocks per row: the
//                  slice's WM_TOPK_MAX best (value, id) pairs of the processed row AFTER the decision, and how many of its elements beat the target
//   k_topk2        one wave per row: merges the slice candidates into the row's best k, writes ids, logit - max - log Z (k_score2's expression
//                  on k_score2's max and Z) and the target's rank
// The raw <|startoftranscript|> row rides in the launches of the tile that holds it as one extra row per stream: no mask, target = the
// no-speech token.  Only [B][Tmax] + [B] floats go back to the host.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "wm_select.h"

struct wm_score_state {
    DevBuf<int4> desc, rec, sst;    // [rows] {logits row, cur_len (< 0: raw row), target (< 0: skip), out index}, records; [maxB] fold state
    DevBuf<float> p1, p1t, out;     // [rows][SEL_SP][4] text / timestamp partials; outputs
    DevBuf<int> lens, npr;          // [maxB] each
    DevBuf<int> rpf;                // [rows] repetition rules: the target's bits (k_score1 -> k_score2)
    DevBuf<float> cv, tlp;          // alternatives: [rows][SEL_SP][WM_TOPK_MAX] slice candidates' values; [outputs][k] log-probabilities
    DevBuf<int> ci, cn, tid, trk;   // their ids, [rows][SEL_SP] counts of elements ahead of the target; [outputs][k] ids, [outputs] ranks
};

void wm_score_free(wm_ctx* ctx)
{
    delete ctx->score;
    ctx->score = nullptr;
}

static int score_reserve(wm_ctx* ctx, size_t rows, size_t nout, size_t nb)
{
    if (!ctx->score) ctx->score = new wm_score_state();
    wm_score_state* sc = ctx->score;
    WM_HIP(sc->desc.reserve(rows)); WM_HIP(sc->rec.reserve(rows));
    WM_HIP(sc->p1.reserve(rows * SEL_SP * 4)); WM_HIP(sc->p1t.reserve(rows * SEL_SP * 4));
    WM_HIP(sc->out.reserve(nout)); WM_HIP(sc->rpf.reserve(rows));
    WM_HIP(sc->lens.reserve(nb)); WM_HIP(sc->npr.reserve(nb)); WM_HIP(sc->sst.reserve(nb));
    return WM_OK;
}
static int topk_reserve(wm_ctx* ctx, size_t rows, size_t nout)
{
    wm_score_state* sc = ctx->score;
    WM_HIP(sc->cv.reserve(rows * SEL_SP * WM_TOPK_MAX)); WM_HIP(sc->ci.reserve(rows * SEL_SP * WM_TOPK_MAX)); WM_HIP(sc->cn.reserve(rows * SEL_SP));
    WM_HIP(sc->tlp.reserve(nout * WM_TOPK_MAX)); WM_HIP(sc->tid.reserve(nout * WM_TOPK_MAX)); WM_HIP(sc->trk.reserve(nout));
    return WM_OK;
}

// ---------------------------------------------------------------------------------------------
// k_score_build: thread b = stream b of the call.  Tile rows i = 0 .. Mper - 1 are input positions pos0 + i; row i scores s[t], t = pos0 + i + 1,
// when n_prompt <= t < len.  The timestamp state of ids[begin : t) is carried across the tiles in sst (reset by the first tile).
// Row nb * Mper + b is the stream's raw <|startoftranscript|> row when position `sot` lies in this tile.
// ---------------------------------------------------------------------------------------------
__global__ void k_score_build(const int* __restrict__ ids, int Tids, const int* __restrict__ lens, const int* __restrict__ npr, int nb, int pos0,
                              int Mper, GenDev gp, TsDev ts, int sot, int ns_id, int Tout, int ns_out0, int4* __restrict__ sst,
                              int4* __restrict__ desc, int4* __restrict__ rec)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    int4 st = pos0 == 0 ? make_int4(0, 0, -1, 0) : sst[b];
    const int* id = ids + (size_t)b * Tids;
    const int T = lens[b], P = npr[b];
    for (int i = 0; i < Mper; ++i) {
        const int pos = pos0 + i, t = pos + 1;
        if (ts.on && pos >= gp.begin && pos < T) st = ts_fold(st, id[pos], ts.tb);          // st: ids[begin : t)
        const bool scored = t >= P && t < T;
        desc[b * Mper + i] = make_int4(b * Mper + i, t, scored ? id[t] : -1, b * Tout + t);
        int4 rc = ts.on ? ts_record(st, t, gp.begin, ts.tb, gp.V, ts.mit) : make_int4(0, 0, 0, 0);
        rc.w = b * Tids;                // repetition rules: where the row's prefix ids[0 : t) start
        rec[b * Mper + i] = rc;
    }
    sst[b] = st;
    const bool here = ns_id >= 0 && sot >= pos0 && sot < pos0 + Mper && sot < T;
    desc[nb * Mper + b] = make_int4(here ? b * Mper + (sot - pos0) : 0, -1, here ? ns_id : -1, ns_out0 + b);
    rec[nb * Mper + b] = make_int4(0, 0, 0, 0);
}

// parity tap: row r = caller-given logits row r under prefix pre[r][0 .. len[r]) (the fold k_ts_tap_build does for wm_select_rows), its own length
__global__ void k_score_tap_build(const int* __restrict__ pre, const int* __restrict__ len, const int* __restrict__ tgt, int R, int Tmax, GenDev gp,
                                  TsDev ts, int4* __restrict__ desc, int4* __restrict__ rec)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    int4 st = make_int4(0, 0, -1, 0);
    const int n = len[r];
    if (ts.on) for (int t = max(gp.begin, 0); t < n; ++t) st = ts_fold(st, pre[(size_t)r * Tmax + t], ts.tb);
    desc[r] = make_int4(r, n, tgt[r], r);
    int4 rc = ts.on ? ts_record(st, n, gp.begin, ts.tb, gp.V, ts.mit) : make_int4(0, 0, 0, 0);
    rc.w = r * Tmax;
    rec[r] = rc;
}

// running (max, sum of exp(v - max)) of one more value / of two partial results; -inf never enters
__device__ __forceinline__ void lse_push(float& m, float& z, float v)
{
    if (v > m) { z = z * expf(m - v) + 1.0f; m = v; }
    else z += expf(v - m);
}
__device__ __forceinline__ void lse_merge(float& m, float& z, float om, float oz)
{
    const float M = fmaxf(m, om);
    z = (M == -INFINITY) ? 0.f : z * expf(m - M) + oz * expf(om - M);
    m = M;
}

// ---------------------------------------------------------------------------------------------
// k_score1: grid (SEL_SP, rows), 256 threads.  Slice sp of a row is float4s [sp * per4, (sp + 1) * per4) of its Vpad-strided logits row (16-byte
// aligned: Vpad is a multiple of 16).  Sibling of k_select1_ts<true> with the row's own cur_len and record, one sweep, temperature 1.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_score1(const float* __restrict__ logits, GenDev gp, const unsigned char* __restrict__ mask, const float* __restrict__ exppen, TsDev ts,
         const int4* __restrict__ desc, const int4* __restrict__ recs, float* __restrict__ p1, float* __restrict__ p1t)
{
    __shared__ float sm[4][4];
    const int row = blockIdx.y, sp = blockIdx.x;
    const int4 dsc = desc[row];
    if (dsc.z < 0) return;
    const bool raw = dsc.y < 0;
    const int cur_len = dsc.y;
    const int4 rec = recs[row];
    const bool tson = ts.on && !raw;
    const int tb = tson ? ts.tb : gp.V;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float4* x4 = reinterpret_cast<const float4*>(logits + (size_t)dsc.x * gp.Vpad);
    const int n4 = (gp.V + 3) / 4, per4 = (n4 + SEL_SP - 1) / SEL_SP, q0 = sp * per4, q1 = min(n4, q0 + per4);
    float mt = -INFINITY, zt = 0.f, ms = -INFINITY, zs = 0.f;
    // repetition rules (not on the raw row): the slice's token sets from the row's own prefix ids[0 : cur_len), the target's bits for k_score2
    extern __shared__ unsigned rp_sh[];
    const bool rp = ts.rp != 0 && !raw;
    const int n0 = 4 * q0;
    if (rp) {
        rp_build(ts, RpPre{ts.rp_ids + rec.w, cur_len, ts.rp_ids, 0}, n0, min(gp.V, 4 * q1), dsc.z, gp.V, rp_sh, tid, 256);
        if (sp == 0 && tid == 0) ts.rp_flags[row] = (int)rp_sh[0];
    }
    for (int q = q0 + tid; q < q1; q += 256) {
        const float4 v4 = x4[q];
        const float vals[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = 4 * q + j;
            if (n >= gp.V) continue;
            float v = vals[j];
            if (!raw) {
                if (rp) v = rp_pen(v, n, n0, ts, rp_sh);
                v = proc_logit(v, n, cur_len, gp, mask, exppen);
                if (tson) v = ts_mask(v, n, rec, gp, ts);
                if (rp && rp_banned(n, n0, gp.V, rp_sh)) v = -INFINITY;
            }
            if (v == -INFINITY) continue;
            if (n < tb) lse_push(mt, zt, v); else lse_push(ms, zs, v);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lse_merge(mt, zt, __shfl_xor(mt, o, 64), __shfl_xor(zt, o, 64));
        lse_merge(ms, zs, __shfl_xor(ms, o, 64), __shfl_xor(zs, o, 64));
    }
    if (lane == 0) { sm[w][0] = mt; sm[w][1] = zt; sm[w][2] = ms; sm[w][3] = zs; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < 4; ++k) { lse_merge(mt, zt, sm[k][0], sm[k][1]); lse_merge(ms, zs, sm[k][2], sm[k][3]); }
        float* o = p1 + ((size_t)row * SEL_SP + sp) * 4;
        o[0] = mt; o[1] = __int_as_float(0); o[2] = zt; o[3] = 0.f;
        float* q = p1t + ((size_t)row * SEL_SP + sp) * 4;
        q[0] = ms; q[1] = __int_as_float(0); q[2] = zs; q[3] = zs;      // temperature 1: both sums of the timestamp region are the same
    }
}

// k_score2: one thread per row (the shape of k_select_argmax_ts): the decision and the row's (max, Z) from the slices, then the target's score
__global__ void k_score2(const float* __restrict__ logits, GenDev gp, const unsigned char* __restrict__ mask, const float* __restrict__ exppen,
                         TsDev ts, const int4* __restrict__ desc, const int4* __restrict__ recs, const float* __restrict__ p1,
                         const float* __restrict__ p1t, int nrows, float* __restrict__ out)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows) return;
    const int4 dsc = desc[row];
    if (dsc.z < 0) return;
    const TsSel f = ts_finish(p1 + (size_t)row * SEL_SP * 4, p1t + (size_t)row * SEL_SP * 4, 1.0f);
    const int n = dsc.z;
    float v = logits[(size_t)dsc.x * gp.Vpad + n];
    if (dsc.y >= 0) {
        const int fl = ts.rp ? ts.rp_flags[row] : 0;
        if (fl & 1) v = rp_penalise(v, ts.rp_pen);
        v = proc_logit(v, n, dsc.y, gp, mask, exppen);
        if (ts.on) {
            v = ts_mask(v, n, recs[row], gp, ts);
            if (f.forced && n < ts.tb) v = -INFINITY;
        }
        if (fl & 2) v = -INFINITY;
    }
    out[dsc.w] = (v == -INFINITY) ? -INFINITY : (v - f.mx) - logf(f.z);
}

// ---------------------------------------------------------------------------------------------
// token alternatives: the k best tokens of every scored row and the rank of its target.  Order everywhere: value descending, then
// id ascending (k_select_argmax's convention).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool tk_before(float v, int n, float ov, int on) { return v > ov || (v == ov && n < on); }

// the target's processed value as k_score2 obtains it: one element, the repetition bits k_score1 left in rp_flags
__device__ __forceinline__ float tk_target(const float* __restrict__ logits, const GenDev& gp, const unsigned char* __restrict__ mask,
                                           const float* __restrict__ exppen, const TsDev& ts, const int4 dsc, const int4 rec, int row, int forced)
{
    const int n = dsc.z;
    float v = logits[(size_t)dsc.x * gp.Vpad + n];
    const int fl = ts.rp ? ts.rp_flags[row] : 0;
    if (fl & 1) v = rp_penalise(v, ts.rp_pen);
    v = proc_logit(v, n, dsc.y, gp, mask, exppen);
    if (ts.on) {
        v = ts_mask(v, n, rec, gp, ts);
        if (forced && n < ts.tb) v = -INFINITY;
    }
    if (fl & 2) v = -INFINITY;
    return v;
}

// A thread's WM_TOPK_MAX best in named slots: every access below is compile-time indexed once the loops are unrolled, so the list lives in
// registers (a runtime-indexed per-thread array would go to scratch; the code object's private segment size is 0).
struct TkList {
    float v[WM_TOPK_MAX]; int n[WM_TOPK_MAX];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < WM_TOPK_MAX; ++j) { v[j] = -INFINITY; n[j] = 0x7fffffff; }
    }
    __device__ __forceinline__ void push(float x, int id)
    {
        if (!tk_before(x, id, v[WM_TOPK_MAX - 1], n[WM_TOPK_MAX - 1])) return;
        v[WM_TOPK_MAX - 1] = x; n[WM_TOPK_MAX - 1] = id;
#pragma unroll
        for (int j = WM_TOPK_MAX - 1; j > 0; --j) {
            const bool up = tk_before(v[j], n[j], v[j - 1], n[j - 1]);
            const float a = v[j], b = v[j - 1]; const int c = n[j], d = n[j - 1];
            v[j - 1] = up ? a : b; v[j] = up ? b : a;
            n[j - 1] = up ? c : d; n[j] = up ? d : c;
        }
    }
    __device__ __forceinline__ void pop()
    {
#pragma unroll
        for (int j = 0; j < WM_TOPK_MAX - 1; ++j) { v[j] = v[j + 1]; n[j] = n[j + 1]; }
        v[WM_TOPK_MAX - 1] = -INFINITY; n[WM_TOPK_MAX - 1] = 0x7fffffff;
    }
};

// k_topk1: grid (SEL_SP, rows), 256 threads, the float4 slice of k_score1 and its processing chain — plus the decision: text is -inf on a forced
// row, as k_score2 has it for the target.  Per (row, slice): the best `topk` (value, id) pairs — (-inf, -1) once the slice has no finite element
// left — and the number of elements ahead of the target in the order.
__global__ void __launch_bounds__(256)
k_topk1(const float* __restrict__ logits, GenDev gp, const unsigned char* __restrict__ mask, const float* __restrict__ exppen, TsDev ts,
        const int4* __restrict__ desc, const int4* __restrict__ recs, const float* __restrict__ p1, const float* __restrict__ p1t, int topk,
        float* __restrict__ cv, int* __restrict__ ci, int* __restrict__ cn)
{
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int sc[4];
    const int row = blockIdx.y, sp = blockIdx.x;
    const int4 dsc = desc[row];
    if (dsc.z < 0 || dsc.y < 0) return;             // nothing scored / the raw <|startoftranscript|> row
    const int cur_len = dsc.y;
    const int4 rec = recs[row];
    const TsSel f = ts_finish(p1 + (size_t)row * SEL_SP * 4, p1t + (size_t)row * SEL_SP * 4, 1.0f);
    const bool forced = ts.on && f.forced;
    const float vt = tk_target(logits, gp, mask, exppen, ts, dsc, rec, row, f.forced);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float4* x4 = reinterpret_cast<const float4*>(logits + (size_t)dsc.x * gp.Vpad);
    const int n4 = (gp.V + 3) / 4, per4 = (n4 + SEL_SP - 1) / SEL_SP, q0 = sp * per4, q1 = min(n4, q0 + per4);
    extern __shared__ unsigned rp_sh[];
    const bool rp = ts.rp != 0;
    const int n0 = 4 * q0;
    if (rp) rp_build(ts, RpPre{ts.rp_ids + rec.w, cur_len, ts.rp_ids, 0}, n0, min(gp.V, 4 * q1), dsc.z, gp.V, rp_sh, tid, 256);
    TkList best;
    best.clear();
    int ahead = 0;
    for (int q = q0 + tid; q < q1; q += 256) {
        const float4 v4 = x4[q];
        const float vals[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = 4 * q + j;
            if (n >= gp.V) continue;
            float v = vals[j];
            if (rp) v = rp_pen(v, n, n0, ts, rp_sh);
            v = proc_logit(v, n, cur_len, gp, mask, exppen);
            if (ts.on) v = ts_mask(v, n, rec, gp, ts);
            if (forced && n < ts.tb) v = -INFINITY;
            if (rp && rp_banned(n, n0, gp.V, rp_sh)) v = -INFINITY;
            if (v == -INFINITY) continue;
            best.push(v, n);
            ahead += (vt != -INFINITY && tk_before(v, n, vt, dsc.z)) ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ahead += __shfl_xor(ahead, o, 64);
    if (lane == 0) sc[w] = ahead;
    const size_t o0 = ((size_t)row * SEL_SP + sp) * WM_TOPK_MAX;
    for (int r = 0; r < topk; ++r) {
        float mx = best.v[0]; int mi = best.n[0];
        block_argmax(mx, mi, sv, si, tid);           // (its barriers also publish sc[] before the read below)
        if (mx != -INFINITY && best.n[0] == mi) best.pop();          // ids are unique: one owner
        if (tid == 0) { cv[o0 + r] = mx; ci[o0 + r] = mx == -INFINITY ? -1 : mi; }
    }
    if (tid == 0) cn[(size_t)row * SEL_SP + sp] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
}

// k_topk2: one wave per row.  Lane l holds slice candidates l and l + 64 of the row's SEL_SP x WM_TOPK_MAX (slots >= topk were not written:
// empty); k rounds of a wave arg-max, the winner's owner drops it.  out index desc.w, as for the log-probability.
__global__ void __launch_bounds__(256)
k_topk2(const float* __restrict__ logits, GenDev gp, const unsigned char* __restrict__ mask, const float* __restrict__ exppen, TsDev ts,
        const int4* __restrict__ desc, const int4* __restrict__ recs, const float* __restrict__ p1, const float* __restrict__ p1t, int nrows,
        int topk, const float* __restrict__ cv, const int* __restrict__ ci, const int* __restrict__ cn, int* __restrict__ out_id,
        float* __restrict__ out_lp, int* __restrict__ out_rank)
{
    static_assert(SEL_SP * WM_TOPK_MAX == 128 && SEL_SP <= 64, "k_topk2: two candidates per lane");
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    const int4 dsc = desc[row];
    if (dsc.z < 0 || dsc.y < 0) return;
    const TsSel f = ts_finish(p1 + (size_t)row * SEL_SP * 4, p1t + (size_t)row * SEL_SP * 4, 1.0f);
    const float vt = tk_target(logits, gp, mask, exppen, ts, dsc, recs[row], row, f.forced);
    const size_t c0 = (size_t)row * SEL_SP * WM_TOPK_MAX;
    const bool ha = (lane & (WM_TOPK_MAX - 1)) < topk;         // (l + 64 sits in the same slot of another slice)
    float va = ha ? cv[c0 + lane] : -INFINITY, vb = ha ? cv[c0 + 64 + lane] : -INFINITY;
    int na = ha ? ci[c0 + lane] : -1, nb = ha ? ci[c0 + 64 + lane] : -1;
    if (va == -INFINITY) na = 0x7fffffff;
    if (vb == -INFINITY) nb = 0x7fffffff;
    int ahead = lane < SEL_SP ? cn[(size_t)row * SEL_SP + lane] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ahead += __shfl_xor(ahead, o, 64);
    const float lz = logf(f.z);
    for (int r = 0; r < topk; ++r) {
        const bool first = tk_before(va, na, vb, nb);
        float mx = first ? va : vb; int mi = first ? na : nb;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(mx, o, 64); const int oi = __shfl_xor(mi, o, 64);
            if (tk_before(ov, oi, mx, mi)) { mx = ov; mi = oi; }
        }
        if (mx != -INFINITY) {
            if (na == mi) { va = -INFINITY; na = 0x7fffffff; }
            else if (nb == mi) { vb = -INFINITY; nb = 0x7fffffff; }
        }
        if (lane == 0) {
            out_id[(size_t)dsc.w * topk + r] = mx == -INFINITY ? -1 : mi;
            out_lp[(size_t)dsc.w * topk + r] = mx == -INFINITY ? -INFINITY : (mx - f.mx) - lz;
        }
    }
    if (lane == 0) out_rank[dsc.w] = vt == -INFINITY ? 0 : 1 + ahead;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// the processors of a scoring call: the decode's own (wm_proc_setup) as a plain greedy step sees them — temperature 1, typical mode, no
// length limit below n_tgt; vanilla: the final stage stops at the LayerNorm (no Medusa-Block extra layer)
static int score_setup(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, const char* who, GenDev* g, TsDev* ts)
{
    if (int rc = wm_proc_setup(ctx, who, gp, tsp, g, ts)) return rc;
    g->max_length = g->hard_max_length = ctx->Tmax;
    g->inv_temp = 1.0f; g->force_accept = -1;
    g->accept_mode = WM_ACCEPT_TYPICAL; g->vanilla = 1;
    return WM_OK;
}

// topk > 0 (wm_score_tokens_topk / wm_topk_rows): the two top-k kernels behind the scores of the same rows; 0: no launch is added
static int score_launch(wm_ctx* ctx, const GenDev& g, const TsDev& ts_in, int nrows, int topk = 0)
{
    wm_score_state* sc = ctx->score;
    TsDev ts = ts_in; ts.rp_flags = sc->rpf;
    hipLaunchKernelGGL(k_score1, dim3(SEL_SP, nrows), dim3(256), rp_lds_bytes(ts, g.V), ctx->stream, ctx->logits, g, ctx->supmask, ctx->exppen, ts, sc->desc, sc->rec,
                       sc->p1, sc->p1t);
    WM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_score2, dim3((nrows + 63) / 64), dim3(64), 0, ctx->stream, ctx->logits, g, ctx->supmask, ctx->exppen, ts, sc->desc, sc->rec,
                       sc->p1, sc->p1t, nrows, sc->out);
    WM_HIP(hipGetLastError());
    if (topk < 1) return WM_OK;
    hipLaunchKernelGGL(k_topk1, dim3(SEL_SP, nrows), dim3(256), rp_lds_bytes(ts, g.V), ctx->stream, ctx->logits, g, ctx->supmask, ctx->exppen, ts, sc->desc, sc->rec,
                       sc->p1, sc->p1t, topk, sc->cv, sc->ci, sc->cn);
    WM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_topk2, dim3((nrows + 3) / 4), dim3(256), 0, ctx->stream, ctx->logits, g, ctx->supmask, ctx->exppen, ts, sc->desc, sc->rec, sc->p1, sc->p1t,
                       nrows, topk, sc->cv, sc->ci, sc->cn, sc->tid, sc->tlp, sc->trk);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

struct ScoreCall {
    GenDev g; TsDev ts;
    int ns_id, sot, B, Tmax;
    const int32_t *lens, *n_prompt;
    int topk;       // > 0: alternatives
};

// behind the layers of a tile: its row descriptors, then — for a tile that holds a scored row — final LayerNorm, base head, scores
static int score_tile(wm_ctx* ctx, int pos0, int Mper, void* arg)
{
    const ScoreCall& c = *static_cast<const ScoreCall*>(arg);
    wm_score_state* sc = ctx->score;
    const int B = c.B;
    // EVERY tile folds its tokens into the streams' timestamp state (k_score_build resets it at pos0 == 0 and carries it in sst): a long
    // prompt's tokens — prompt_ids may hold timestamps of previous text — reach the records of the later tiles as they reach the decode's
    hipLaunchKernelGGL(k_score_build, dim3((B + 63) / 64), dim3(64), 0, ctx->stream, ctx->ids, ctx->Tal, sc->lens, sc->npr, B, pos0, Mper, c.g, c.ts,
                       c.sot, c.ns_id, c.Tmax, B * c.Tmax, sc->sst, sc->desc, sc->rec);
    WM_HIP(hipGetLastError());
    // logits only for a tile that holds a scored row (a long prompt's leading tiles are wanted for their K/V and their fold alone)
    bool need = c.ns_id >= 0 && c.sot >= pos0 && c.sot < pos0 + Mper;
    for (int b = 0; b < B && !need; ++b) need = std::max(c.n_prompt[b], pos0 + 1) < std::min(c.lens[b], pos0 + Mper + 1);
    if (!need) return WM_OK;
    if (int rc = wm_dec_stage_final(ctx, 0, B, Mper, 0, 0)) return rc;
    if (int rc = wm_dec_stage_heads(ctx, B * Mper, 1, 0, 0)) return rc;
    return score_launch(ctx, c.g, c.ts, B * Mper + B, c.topk);
}

static bool topk_ok(wm_ctx* ctx, const char* who, int topk)
{
    if (topk >= 1 && topk <= WM_TOPK_MAX) return true;
    ctx->err = std::string(who) + ": topk must be in [1, " + std::to_string(WM_TOPK_MAX) + "] (WM_TOPK_MAX), got " + std::to_string(topk);
    return false;
}

// wm_score_tokens (topk == 0) and wm_score_tokens_topk: one body, the same launches for the scores
static int score_tokens(wm_ctx* ctx, const char* who_c, const wm_gen_params* gp, const wm_timestamp_params* tsp, const wm_score_params* sp, int B,
                        const int32_t* tokens, int Tmax, const int32_t* lens, const int32_t* n_prompt, float* logprobs, float* no_speech_prob, float* ms,
                        int topk, int32_t* top_ids, float* top_logprobs, int32_t* ranks)
{
    const std::string who(who_c);
    if (!gp || !tokens || !lens || !n_prompt || !logprobs || B < 1 || Tmax < 1) { ctx->err = who + ": bad arguments"; return WM_ERR_ARG; }
    if (int rc = wm_replay_check(ctx, who_c, B, Tmax, lens, n_prompt, 1)) return rc;
    ScoreCall c{};
    c.ns_id = (sp && no_speech_prob) ? sp->no_speech_token_id : -1;
    c.sot = (sp && sp->sot_index >= 0) ? sp->sot_index : 0;
    c.B = B; c.Tmax = Tmax; c.lens = lens; c.n_prompt = n_prompt; c.topk = topk;
    if (c.ns_id >= ctx->V) { ctx->err = who + ": no_speech_token_id outside the vocabulary"; return WM_ERR_ARG; }
    int npos = 0;
    for (int b = 0; b < B; ++b) {
        if (c.ns_id >= 0 && c.sot >= n_prompt[b]) { ctx->err = who + ": sot_index must lie inside the prompt"; return WM_ERR_ARG; }
        for (int t = 0; t < lens[b]; ++t)
            if (tokens[(size_t)b * Tmax + t] < 0 || tokens[(size_t)b * Tmax + t] >= ctx->V) {
                ctx->err = who + ": target outside the vocabulary (stream " + std::to_string(b) + ", position " + std::to_string(t) + ")";
                return WM_ERR_ARG;
            }
        npos = std::max(npos, std::max(lens[b] - 1, c.ns_id >= 0 ? c.sot + 1 : 0));
    }
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = score_setup(ctx, gp, tsp, who_c, &c.g, &c.ts)) return rc;
    if (int rc = score_reserve(ctx, (size_t)B * 17, (size_t)B * Tmax + B, (size_t)B)) return rc;
    if (topk > 0) if (int rc = topk_reserve(ctx, (size_t)B * 17, (size_t)B * Tmax)) return rc;
    wm_score_state* sc = ctx->score;
    // the replay overwrites the decode state (ids, kvlen, self K/V, the processors' tables): begin again afterwards
    wm_decode_invalidate(ctx);
    wm_scalars_swap swap(ctx, c.g, c.ts);
    for (size_t i = 0; i < (size_t)B * Tmax; ++i) logprobs[i] = 0.f;
    WM_HIP(hipEventRecord(ctx->ev0, st));
    WM_HIP(hipMemcpyAsync(sc->lens, lens, B * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(sc->npr, n_prompt, B * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemsetAsync(sc->out, 0, ((size_t)B * Tmax + B) * sizeof(float), st));
    wm_replay_hooks hk; hk.tile = score_tile; hk.arg = &c;
    if (int rc = wm_dec_replay(ctx, 0, B, tokens, Tmax, lens, npos, ctx->cfg.dec_layers, hk)) return rc;
    std::vector<float> ns(B, 0.f);
    WM_HIP(hipMemcpyAsync(logprobs, sc->out, (size_t)B * Tmax * sizeof(float), hipMemcpyDeviceToHost, st));
    WM_HIP(hipMemcpyAsync(ns.data(), sc->out + (size_t)B * Tmax, B * sizeof(float), hipMemcpyDeviceToHost, st));
    if (topk > 0) {
        WM_HIP(hipMemcpyAsync(top_ids, sc->tid, (size_t)B * Tmax * topk * sizeof(int), hipMemcpyDeviceToHost, st));
        WM_HIP(hipMemcpyAsync(top_logprobs, sc->tlp, (size_t)B * Tmax * topk * sizeof(float), hipMemcpyDeviceToHost, st));
        WM_HIP(hipMemcpyAsync(ranks, sc->trk, (size_t)B * Tmax * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    WM_HIP(hipStreamSynchronize(st));
    WM_HIP(hipEventRecord(ctx->ev1, st));
    WM_HIP(hipEventSynchronize(ctx->ev1));
    if (no_speech_prob) for (int b = 0; b < B; ++b) no_speech_prob[b] = c.ns_id >= 0 ? (float)std::exp((double)ns[b]) : 0.f;
    if (ms) WM_HIP(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    // unscored positions (the prompt, behind a stream's end): the device rows there were never written
    for (int b = 0; topk > 0 && b < B; ++b)
        for (int t = 0; t < Tmax; ++t) {
            if (t >= n_prompt[b] && t < lens[b]) continue;
            const size_t i = (size_t)b * Tmax + t;
            for (int k = 0; k < topk; ++k) { top_ids[i * topk + k] = -1; top_logprobs[i * topk + k] = -INFINITY; }
            ranks[i] = 0;
        }
    return WM_OK;
}

extern "C" int wm_score_tokens(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, const wm_score_params* sp, int B,
                               const int32_t* tokens, int Tmax, const int32_t* lens, const int32_t* n_prompt, float* logprobs,
                               float* no_speech_prob, float* ms)
{
    if (!ctx) return WM_ERR_ARG;
    return score_tokens(ctx, "wm_score_tokens", gp, tsp, sp, B, tokens, Tmax, lens, n_prompt, logprobs, no_speech_prob, ms, 0, nullptr, nullptr, nullptr);
}

extern "C" int wm_score_tokens_topk(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, const wm_score_params* sp, int B,
                                    const int32_t* tokens, int Tmax, const int32_t* lens, const int32_t* n_prompt, int topk, float* logprobs,
                                    float* no_speech_prob, int32_t* top_ids, float* top_logprobs, int32_t* ranks, float* ms)
{
    if (!ctx) return WM_ERR_ARG;
    if (!top_ids || !top_logprobs || !ranks) { ctx->err = "wm_score_tokens_topk: bad arguments"; return WM_ERR_ARG; }
    if (!topk_ok(ctx, "wm_score_tokens_topk", topk)) return WM_ERR_ARG;
    return score_tokens(ctx, "wm_score_tokens_topk", gp, tsp, sp, B, tokens, Tmax, lens, n_prompt, logprobs, no_speech_prob, ms, topk, top_ids,
                        top_logprobs, ranks);
}

// wm_score_rows (topk == 0, out_logprob) and wm_topk_rows (topk > 0, the three other outputs): one body
static int score_rows(wm_ctx* ctx, const char* who_c, const wm_gen_params* gp, const wm_timestamp_params* tsp, int R, const float* logits,
                      const int32_t* prefixes, int Tmax, const int32_t* lens, const int32_t* targets, float* out_logprob, int topk, int32_t* top_ids,
                      float* top_logprobs, int32_t* ranks)
{
    const std::string who(who_c);
    if (!gp || R < 1 || !logits || !prefixes || Tmax < 1 || !lens || !targets || (topk ? !top_ids || !top_logprobs || !ranks : !out_logprob)) {
        ctx->err = who + ": bad arguments"; return WM_ERR_ARG;
    }
    if (int rc = wm_tap_check_lens(ctx, who_c, lens, R, Tmax, true)) return rc;
    for (int r = 0; r < R; ++r)
        if (targets[r] < 0 || targets[r] >= ctx->V) { ctx->err = who + ": target outside the vocabulary (row " + std::to_string(r) + ")"; return WM_ERR_ARG; }
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    GenDev g{}; TsDev ts{};
    if (int rc = score_setup(ctx, gp, tsp, who_c, &g, &ts)) return rc;
    wm_decode_invalidate(ctx);       // (the processors' tables are the tap's now)
    const int G = ctx->Rcap;                   // rows per group: what the logits scratch holds (not WM_TAP_ROWS)
    if (int rc = score_reserve(ctx, (size_t)G, (size_t)G, 0)) return rc;
    if (topk > 0) if (int rc = topk_reserve(ctx, (size_t)G, (size_t)G)) return rc;
    wm_score_state* sc = ctx->score;
    wm_tap_stage s{ctx, who_c, Tmax, G};
    if (int rc = s.reserve(G)) return rc;           // extra: the group's targets
    ts.rp_ids = s.pre; ts.rp_stride = Tmax;         // repetition rules: the rows' own prefixes
    return wm_tap_groups(s, R, logits, prefixes, lens, [&](int r0, int n) {
        WM_TAP_HIP(s, hipMemcpyAsync(s.extra, targets + r0, n * sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_score_tap_build, dim3((n + 63) / 64), dim3(64), 0, st, s.pre, s.len, s.extra, n, Tmax, g, ts, sc->desc, sc->rec);
        WM_TAP_HIP(s, hipGetLastError());
        if (int rc = score_launch(ctx, g, ts, n, topk)) return rc;
        if (topk > 0) {
            WM_TAP_HIP(s, hipMemcpyAsync(top_ids + (size_t)r0 * topk, sc->tid, (size_t)n * topk * sizeof(int), hipMemcpyDeviceToHost, st));
            WM_TAP_HIP(s, hipMemcpyAsync(top_logprobs + (size_t)r0 * topk, sc->tlp, (size_t)n * topk * sizeof(float), hipMemcpyDeviceToHost, st));
            WM_TAP_HIP(s, hipMemcpyAsync(ranks + r0, sc->trk, n * sizeof(int), hipMemcpyDeviceToHost, st));
        } else
            WM_TAP_HIP(s, hipMemcpyAsync(out_logprob + r0, sc->out, n * sizeof(float), hipMemcpyDeviceToHost, st));
        return WM_OK;
    });
}

extern "C" int wm_score_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, int R, const float* logits,
                             const int32_t* prefixes, int Tmax, const int32_t* lens, const int32_t* targets, float* out_logprob)
{
    if (!ctx) return WM_ERR_ARG;
    return score_rows(ctx, "wm_score_rows", gp, tsp, R, logits, prefixes, Tmax, lens, targets, out_logprob, 0, nullptr, nullptr, nullptr);
}

extern "C" int wm_topk_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, int R, const float* logits, const int32_t* prefixes,
                            int Tmax, const int32_t* lens, const int32_t* targets, int topk, int32_t* top_ids, float* top_logprobs, int32_t* ranks)
{
    if (!ctx) return WM_ERR_ARG;
    if (!topk_ok(ctx, "wm_topk_rows", topk)) return WM_ERR_ARG;
    return score_rows(ctx, "wm_topk_rows", gp, tsp, R, logits, prefixes, Tmax, lens, targets, nullptr, topk, top_ids, top_logprobs, ranks);
}
