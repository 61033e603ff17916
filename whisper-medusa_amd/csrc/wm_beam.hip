// wm_beam.hip — beam search on the plain decode path (include/wm.h wm_set_beam / wm_beam_rows / wm_beam_reorder_kv): what HF's
// GenerationMixin._beam_search does behind the model call of every step, on the device, with no logits row going to the host.  Beam j of clip g is
// stream g * n + j of a plain decode; all streams sit at one length.
//   select       k_beam_lse:     grid (SEL_SP, rows) x 256: slice partials {max, sum exp} of the raw row (log_softmax FIRST)
//                k_beam_region:  timestamp rules on: slice partials of the processed row w for the rules' own log-softmax decision
//                k_beam_slice:   w = processors(x - lse) under the row's own prefix, a = running score + w, the slice's best 2n (a, token)
//                k_beam_merge:   one block per clip: the ordered 2n candidates (value descending, then (beam, token) ascending)
//   bookkeeping  k_beam_book:    one block per clip: hits, next running beams, finished-table merge, heuristic flag, clip done; next token and
//                                beam_idx of every stream; L / kvlen; ctx->done when every clip is done
//   reorder      k_beam_ids_gather / _scatter, k_beam_kv_gather / _scatter: ids row, timestamp state and self K/V rows [0, L) follow beam_idx
//                through a shadow buffer (a slot may be source and destination): gather what moves, then write it back
//   expand / compact   k_beam_slot_copy: the cross K/V of a clip to its n streams before the first step and back after the last
// The processed row is k_sample1's pl(n) on x - lse: repetition rules, proc_logit, timestamp masks (wm_select.h).
#include <cmath>
#include <cstring>
#include "wm_select.h"

#define BEAM_C (2 * WM_BEAM_MAX)        // candidate slots per (row, slice)
#define BEAM_NEG (-1.0e9f)              // HF's "never chosen" score

struct wm_beam_state {
    DevBuf<float> run, cval, fscore, lse, reg, sval, den;
    DevBuf<int> cbeam, ctok, fset, flen, fids, heur, cdone, bidx, ntok, stok, sh_ids;
    DevBuf<int4> sh_st;
    DevBuf<bf16_t> sh_kv;
};

void wm_beam_free(wm_ctx* ctx)
{
    ctx->graphs_beam.drop();                // its graph names the shadow K/V freed below
    delete ctx->beam_state;
    ctx->beam_state = nullptr;
}

// ---- select ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float beam_row_lse(const float* p)       // p: [SEL_SP][2], merged in slice order by every consumer alike
{
    float M = -INFINITY;
    for (int k = 0; k < SEL_SP; ++k) M = fmaxf(M, p[2 * k]);
    float Z = 0.f;
    for (int k = 0; k < SEL_SP; ++k) if (p[2 * k] != -INFINITY) Z += p[2 * k + 1] * expf(p[2 * k] - M);
    return M + logf(Z);
}
// WhisperTimeStampLogitsProcessor's decision on the processed row: logsumexp(w[tb:]) > max(w[:tb]) (both sides carry the same log Z)
__device__ __forceinline__ int beam_row_forced(const float* p)      // p: [SEL_SP][4]
{
    float mt = -INFINITY, ms = -INFINITY;
    for (int k = 0; k < SEL_SP; ++k) { mt = fmaxf(mt, p[4 * k]); ms = fmaxf(ms, p[4 * k + 1]); }
    float zs = 0.f;
    for (int k = 0; k < SEL_SP; ++k) if (p[4 * k + 1] != -INFINITY) zs += p[4 * k + 2] * expf(p[4 * k + 1] - ms);
    return (ms != -INFINITY && ms + logf(zs) > mt) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
k_beam_lse(const float* __restrict__ logits, GenDev gp, BeamDev bd, const int* __restrict__ done)
{
    __shared__ float sv[4]; __shared__ int si[4]; __shared__ float sz[4];
    if (done[0]) return;
    const int row = blockIdx.y, sp = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (size_t)row * gp.Vpad;
    const int per = (gp.V + SEL_SP - 1) / SEL_SP, n0 = sp * per, n1 = min(gp.V, n0 + per);
    float m = -INFINITY;
    for (int n = n0 + tid; n < n1; n += 256) m = fmaxf(m, x[n]);
    int dummy = 0;
    block_argmax(m, dummy, sv, si, tid);
    float z = 0.f;
    for (int n = n0 + tid; n < n1; n += 256) z += expf(x[n] - m);
    z = block_sum(z, sz, tid);
    if (tid == 0) { float* o = bd.lse + ((size_t)row * SEL_SP + sp) * 2; o[0] = m; o[1] = z; }
}

// the processed log-probability of token n of row `row` (stream `row`): what HF's processors leave of log_softmax(raw row)[n]
#define BEAM_ROW_SETUP                                                                                                              \
    const int row = blockIdx.y, sp = blockIdx.x, tid = threadIdx.x;                                                                 \
    const int cur_len = pos[row];                                                                                                   \
    const float* x = logits + (size_t)row * gp.Vpad;                                                                                \
    const int per = (gp.V + SEL_SP - 1) / SEL_SP, n0 = sp * per, n1 = min(gp.V, n0 + per);                                          \
    const float lse = beam_row_lse(bd.lse + (size_t)row * SEL_SP * 2);                                                              \
    int4 rec = make_int4(0, 0, 0, 0);                                                                                               \
    if (TS) rec = ts_row_record(gp, ts, 0, row, 0, cur_len);                                                                        \
    extern __shared__ unsigned rp_sh[];                                                                                             \
    const bool rp = TS && ts.rp != 0;                                                                                               \
    if (rp) rp_build(ts, rp_row_prefix(ts, 0, row, row, cur_len), n0, n1, -1, gp.V, rp_sh, tid, 256);                               \
    auto pw = [&](int n) {                                                                                                          \
        float v = x[n] - lse;                                                                                                       \
        if (rp) v = rp_pen(v, n, n0, ts, rp_sh);                                                                                    \
        v = proc_logit(v, n, cur_len, gp, mask, exppen);                                                                            \
        if (TS) v = ts_mask(v, n, rec, gp, ts);                                                                                     \
        if (rp && rp_banned(n, n0, gp.V, rp_sh)) v = -INFINITY;                                                                     \
        return v;                                                                                                                   \
    }

__global__ void __launch_bounds__(256)
k_beam_region(const float* __restrict__ logits, GenDev gp, const unsigned char* __restrict__ mask, const float* __restrict__ exppen,
              const int* __restrict__ pos, TsDev ts, BeamDev bd, const int* __restrict__ done)
{
    constexpr bool TS = true;
    __shared__ float sv[4]; __shared__ int si[4]; __shared__ float sz[4];
    if (done[0]) return;
    BEAM_ROW_SETUP;
    float mt = -INFINITY, ms = -INFINITY;
    for (int n = n0 + tid; n < n1; n += 256) {
        const float v = pw(n);
        if (n < ts.tb) mt = fmaxf(mt, v); else ms = fmaxf(ms, v);
    }
    int dummy = 0;
    block_argmax(mt, dummy, sv, si, tid);
    dummy = 0;
    block_argmax(ms, dummy, sv, si, tid);
    float zs = 0.f;
    for (int n = max(n0, ts.tb) + tid; n < n1; n += 256) {
        const float v = pw(n);
        if (v != -INFINITY) zs += expf(v - ms);
    }
    zs = block_sum(zs, sz, tid);
    if (tid == 0) { float* o = bd.reg + ((size_t)row * SEL_SP + sp) * 4; o[0] = mt; o[1] = ms; o[2] = zs; o[3] = 0.f; }
}

// dynamic LDS: the repetition rules' bitmaps (rp_lds_bytes), then the slice's accumulated values [per]
template <bool TS>
__global__ void __launch_bounds__(256)
k_beam_slice(const float* __restrict__ logits, GenDev gp, const unsigned char* __restrict__ mask, const float* __restrict__ exppen,
             const int* __restrict__ pos, TsDev ts, BeamDev bd, int rp_words_lds, const int* __restrict__ done)
{
    __shared__ float sv[4]; __shared__ int si[4];
    if (done[0]) return;
    BEAM_ROW_SETUP;
    float* acc = reinterpret_cast<float*>(rp_sh + rp_words_lds);
    const int forced = (TS && ts.on) ? beam_row_forced(bd.reg + (size_t)row * SEL_SP * 4) : 0;
    const float base = bd.run[row];
    const int cnt = max(n1 - n0, 0);
    for (int i = tid; i < cnt; i += 256) {
        const int n = n0 + i;
        float v = pw(n);
        if (forced && n < ts.tb) v = -INFINITY;
        acc[i] = base + v;
    }
    __syncthreads();
    // the slice's best 2n by (value descending, token ascending): round r takes the best element behind round r - 1's
    float pv = INFINITY; int pt = -1;
    const int want = 2 * bd.n;
    float* ov = bd.sval + ((size_t)row * SEL_SP + sp) * BEAM_C;
    int* ot = bd.stok + ((size_t)row * SEL_SP + sp) * BEAM_C;
    for (int r = 0; r < want; ++r) {
        float mx = -INFINITY; int mi = 0x7fffffff;
        for (int i = tid; i < cnt; i += 256) {
            const float v = acc[i]; const int n = n0 + i;
            const bool behind = v < pv || (v == pv && n > pt);
            if (behind && (v > mx || (v == mx && n < mi))) { mx = v; mi = n; }
        }
        block_argmax(mx, mi, sv, si, tid);
        if (tid == 0) { ov[r] = mx; ot[r] = (mi == 0x7fffffff) ? -1 : mi; }
        if (mi == 0x7fffffff) { pv = -INFINITY; pt = 0x7fffffff; } else { pv = mx; pt = mi; }
    }
}

// the clip's ordered 2n candidates from its n rows' slice candidates: value descending, then (beam, token) ascending
__global__ void __launch_bounds__(256)
k_beam_merge(GenDev gp, BeamDev bd, const int* __restrict__ done)
{
    __shared__ float sv[4]; __shared__ int si[4];
    if (done[0]) return;
    const int g = blockIdx.x, tid = threadIdx.x, n = bd.n, want = 2 * n;
    const int E = n * SEL_SP * want;                    // <= 8 * 16 * 16 = 2048 = 8 per thread
    float v[8]; int f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int e = tid + 256 * i;
        v[i] = -INFINITY; f[i] = -1;
        if (e < E) {
            const int j = e / (SEL_SP * want), k = (e / want) % SEL_SP, c = e % want;
            const size_t o = ((size_t)(g * n + j) * SEL_SP + k) * BEAM_C + c;
            const int tok = bd.stok[o];
            if (tok >= 0) { v[i] = bd.sval[o]; f[i] = j * gp.V + tok; }
        }
    }
    float pv = INFINITY; int pf = -1;
    for (int r = 0; r < want; ++r) {
        float mx = -INFINITY; int mi = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool behind = f[i] >= 0 && (v[i] < pv || (v[i] == pv && f[i] > pf));
            if (behind && (v[i] > mx || (v[i] == mx && f[i] < mi))) { mx = v[i]; mi = f[i]; }
        }
        block_argmax(mx, mi, sv, si, tid);
        if (tid == 0) {
            const bool none = mi == 0x7fffffff;
            bd.cval[g * want + r] = mx; bd.cbeam[g * want + r] = none ? 0 : mi / gp.V; bd.ctok[g * want + r] = none ? 0 : mi % gp.V;
        }
        if (mi == 0x7fffffff) { pv = -INFINITY; pf = 0x7fffffff; } else { pv = mx; pf = mi; }
    }
}

// ---- bookkeeping: steps d to g of HF's loop for one clip (include/wm.h, points 2 to 4) ------------------------------------------------
__global__ void __launch_bounds__(64)
k_beam_book(GenDev gp, BeamDev bd, const int* __restrict__ ids, int* __restrict__ L, int* __restrict__ kvlen, int* __restrict__ finished,
            int* __restrict__ niter, long long* __restrict__ hist, int* __restrict__ done)
{
    __shared__ int plan[WM_BEAM_MAX];           // finished-table entry p comes from: old entry i (i), new candidate k (100 + k)
    __shared__ float pscore[WM_BEAM_MAX]; __shared__ int pset[WM_BEAM_MAX];
    __shared__ int s_cur;
    const int g = blockIdx.x, tid = threadIdx.x, n = bd.n, n2 = 2 * n;
    if (done[0] || bd.cdone[g]) {               // the clip's streams step as no-ops
        if (tid < n) { bd.bidx[g * n + tid] = g * n + tid; bd.ntok[g * n + tid] = -1; }
        return;
    }
    // (the decisions are a few dozen scalar steps: thread 0 takes them on arrays in LDS, ordered by counting — the rank of an entry is the number of
    // entries ahead of it —, so that no private array is indexed by a value computed at run time)
    __shared__ float c_val[BEAM_C], c_rv[BEAM_C], c_ns[BEAM_C], o_fs[WM_BEAM_MAX];
    __shared__ int c_beam[BEAM_C], c_tok[BEAM_C], c_hit[BEAM_C], o_set[WM_BEAM_MAX];
    if (tid == 0) {
        const int cur = L[g * n], P = gp.P;
        s_cur = cur;
        bool allhit = true;
        for (int k = 0; k < n2; ++k) {
            c_val[k] = bd.cval[g * n2 + k]; c_beam[k] = bd.cbeam[g * n2 + k]; c_tok[k] = bd.ctok[g * n2 + k];
            c_hit[k] = (c_tok[k] == gp.eos || cur + 1 >= gp.max_length) ? 1 : 0;
            c_rv[k] = c_hit[k] ? c_val[k] + BEAM_NEG : c_val[k];
            allhit = allhit && c_hit[k];
        }
        // e. the next running beams: the best n of rv (value descending, then (beam, token) ascending)
        float run0 = 0.f;
        for (int k = 0; k < n2; ++k) {
            int rank = 0;
            for (int q = 0; q < n2; ++q) {
                const bool ahead = c_rv[q] > c_rv[k] || (c_rv[q] == c_rv[k] && (c_beam[q] < c_beam[k] || (c_beam[q] == c_beam[k] && c_tok[q] < c_tok[k])));
                rank += (q != k && ahead) ? 1 : 0;
            }
            if (rank < n) { bd.run[g * n + rank] = c_rv[k]; bd.bidx[g * n + rank] = g * n + c_beam[k]; bd.ntok[g * n + rank] = c_tok[k]; }
            if (rank == 0) run0 = c_rv[k];
        }
        // f. the finished table: old entries (in table order) before the candidates of the first n ranks that hit
        bool full = true;
        for (int i = 0; i < n; ++i) { o_fs[i] = bd.fscore[g * n + i]; o_set[i] = bd.fset[g * n + i]; full = full && o_set[i]; }
        const int heur = bd.heur[g];
        const float den = bd.den[min(max(cur + 1 - P, 0), gp.Tids + 1)];
        for (int k = 0; k < n2; ++k) {
            float sc = __fdiv_rn(c_val[k], den);
            if (full && bd.es == 1) sc += BEAM_NEG;
            if (!heur) sc += BEAM_NEG;
            if (!(c_hit[k] && k < n)) sc += BEAM_NEG;
            c_ns[k] = sc;
        }
        for (int i = 0; i < n; ++i) {           // an old entry: behind the old ones before it that are not worse, and behind every better new one
            int rank = 0;
            for (int q = 0; q < n; ++q) rank += (q != i && (o_fs[q] > o_fs[i] || (o_fs[q] == o_fs[i] && q < i))) ? 1 : 0;
            for (int q = 0; q < n2; ++q) rank += (c_ns[q] > o_fs[i]) ? 1 : 0;
            if (rank < n) { plan[rank] = i; pscore[rank] = o_fs[i]; pset[rank] = o_set[i]; }
        }
        for (int k = 0; k < n2; ++k) {          // a new one: behind every old one that is not worse; two new ones that tie: (beam, token) ascending
            int rank = 0;
            for (int q = 0; q < n; ++q) rank += (o_fs[q] >= c_ns[k]) ? 1 : 0;
            for (int q = 0; q < n2; ++q) {
                const bool ahead = c_ns[q] > c_ns[k] || (c_ns[q] == c_ns[k] && (c_beam[q] < c_beam[k] || (c_beam[q] == c_beam[k] && c_tok[q] < c_tok[k])));
                rank += (q != k && ahead) ? 1 : 0;
            }
            if (rank < n) { plan[rank] = 100 + k; pscore[rank] = c_ns[k]; pset[rank] = (c_hit[k] && k < n) ? 1 : 0; }
        }
        // g. the heuristic flag and the clip's stop
        float minfs = pscore[0]; bool allset = true;
        for (int p = 0; p < n; ++p) { minfs = fminf(minfs, pscore[p]); allset = allset && pset[p]; }
        const int curn = cur + 1;
        const int bl = min(max((bd.es == 2 && bd.lp_pos) ? gp.max_length - P : curn - P, 0), gp.Tids + 1);
        const float bestrun = __fdiv_rn(run0, bd.den[bl]);
        bool any = false;
        for (int p = 0; p < n; ++p) any = any || bestrun > (pset[p] ? minfs : BEAM_NEG);
        const int h = (heur && any) ? 1 : 0;
        bd.heur[g] = h;
        const bool cont = h && !(allset && bd.es == 1) && !allhit;
        if (!cont) {
            bd.cdone[g] = 1;
            for (int j = 0; j < n; ++j) finished[g * n + j] = 1;
            if (atomicAdd(done + 1, 1) == bd.G - 1) done[0] = 1;
        }
        atomicAdd(reinterpret_cast<unsigned long long*>(hist + 16), (unsigned long long)n);
    }
    __syncthreads();
    const int cur = s_cur;
    // the table moves in place from its last entry down: an old entry never moves up (the order is stable), so its source is still intact
    for (int p = n - 1; p >= 0; --p) {
        const int src = plan[p];
        int* dst = bd.fids + (size_t)(g * n + p) * gp.Tids;
        if (src >= 100) {
            const int k = src - 100;
            const int* from = ids + (size_t)(g * n + bd.cbeam[g * n2 + k]) * gp.Tids;
            for (int t = tid; t < cur && t < gp.Tids; t += 64) dst[t] = from[t];
            if (tid == 0) { if (cur < gp.Tids) dst[cur] = bd.ctok[g * n2 + k]; bd.flen[g * n + p] = min(cur + 1, gp.Tids); }
        } else if (src != p) {
            const int* from = bd.fids + (size_t)(g * n + src) * gp.Tids;
            const int len = bd.flen[g * n + src];
            for (int t = tid; t < len; t += 64) dst[t] = from[t];
            __syncthreads();
            if (tid == 0) bd.flen[g * n + p] = len;
        }
        if (tid == 0) { bd.fscore[g * n + p] = pscore[p]; bd.fset[g * n + p] = pset[p]; }
        __syncthreads();
    }
    if (tid < n) { const int s = g * n + tid; L[s] = cur + 1; kvlen[s] = cur; niter[s] += 1; }
}

// ---- reorder ---------------------------------------------------------------------------------------------------------------------------
// A stream that steps (ntok >= 0) has kvlen[s] rows behind it: ids[0, kvlen), self K/V rows [0, kvlen).  Gather reads the sources, scatter writes the
// destinations; a stream whose source is itself moves nothing.
__global__ void __launch_bounds__(64)
k_beam_ids_gather(BeamDev bd, const int* __restrict__ ids, const int* __restrict__ kvlen, int Tids, TsDev ts)
{
    const int s = blockIdx.x, tid = threadIdx.x;
    if (bd.ntok[s] < 0) return;
    const int src = bd.bidx[s], rows = min(kvlen[s], Tids);
    if (tid == 0 && ts.on) bd.sh_st[s] = ts.st[src];
    if (src == s) return;
    for (int t = tid; t < rows; t += 64) bd.sh_ids[(size_t)s * Tids + t] = ids[(size_t)src * Tids + t];
}
__global__ void __launch_bounds__(64)
k_beam_ids_scatter(BeamDev bd, int* __restrict__ ids, const int* __restrict__ kvlen, int Tids, TsDev ts)
{
    const int s = blockIdx.x, tid = threadIdx.x;
    const int tok = bd.ntok[s];
    if (tok < 0) return;
    const int src = bd.bidx[s], rows = min(kvlen[s], Tids);
    if (src != s)
        for (int t = tid; t < rows; t += 64) ids[(size_t)s * Tids + t] = bd.sh_ids[(size_t)s * Tids + t];
    if (tid == 0) {
        if (rows < Tids) ids[(size_t)s * Tids + rows] = tok;
        if (ts.on) ts.st[s] = ts_fold(bd.sh_st[s], tok, ts.tb);
    }
}
// Self K/V: per (kv layer, stream, head) K is [Tal][64] bf16 row-major and V is V^T fragments of 32 keys (vfrag_index), so rows [0, 32 u) of either
// are the first u units of 4 KiB: a block moves one unit per iteration, 16 B per lane.  grid (H, streams, nkv); the loop bound comes from kvlen on
// the device, so the launch does not depend on the length.
__global__ void __launch_bounds__(256)
k_beam_kv_gather(BeamDev bd, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc, const int* __restrict__ kvlen, int H, int Tal, int maxB,
                 int nstreams)
{
    const int hd = blockIdx.x, s = blockIdx.y, slot = blockIdx.z, tid = threadIdx.x;
    if (bd.ntok[s] < 0) return;
    const int src = bd.bidx[s];
    if (src == s) return;
    const int units = (min(kvlen[s], bd.rows_cap) + 31) >> 5;
    const size_t from = (((size_t)slot * maxB + src) * H + hd) * (size_t)Tal * 64;
    const size_t to = (((size_t)slot * nstreams + s) * H + hd) * (size_t)bd.rows_cap * 64;
    const size_t vhalf = (size_t)gridDim.z * nstreams * H * (size_t)bd.rows_cap * 64;
    for (int u = 0; u < units; ++u) {
        const size_t o = (size_t)u * 2048 + tid * 8;
        const uint4 a = *reinterpret_cast<const uint4*>(kc + from + o);
        const uint4 b = *reinterpret_cast<const uint4*>(vc + from + o);
        *reinterpret_cast<uint4*>(bd.sh_kv + to + o) = a;
        *reinterpret_cast<uint4*>(bd.sh_kv + vhalf + to + o) = b;
    }
}
__global__ void __launch_bounds__(256)
k_beam_kv_scatter(BeamDev bd, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc, const int* __restrict__ kvlen, int H, int Tal, int maxB, int nstreams)
{
    const int hd = blockIdx.x, s = blockIdx.y, slot = blockIdx.z, tid = threadIdx.x;
    if (bd.ntok[s] < 0) return;
    if (bd.bidx[s] == s) return;
    const int units = (min(kvlen[s], bd.rows_cap) + 31) >> 5;
    const size_t to = (((size_t)slot * maxB + s) * H + hd) * (size_t)Tal * 64;
    const size_t from = (((size_t)slot * nstreams + s) * H + hd) * (size_t)bd.rows_cap * 64;
    const size_t vhalf = (size_t)gridDim.z * nstreams * H * (size_t)bd.rows_cap * 64;
    for (int u = 0; u < units; ++u) {
        const size_t o = (size_t)u * 2048 + tid * 8;
        const uint4 a = *reinterpret_cast<const uint4*>(bd.sh_kv + from + o);
        const uint4 b = *reinterpret_cast<const uint4*>(bd.sh_kv + vhalf + from + o);
        *reinterpret_cast<uint4*>(kc + to + o) = a;
        *reinterpret_cast<uint4*>(vc + to + o) = b;
    }
}

// ---- expand / compact: slot `src` of an array of equal slots to slots dst0 .. dst0 + ncopy - 1 (a destination equal to the source is skipped) ----
template <class T>
__global__ void __launch_bounds__(256)
k_beam_slot_copy(T* __restrict__ base, size_t per, size_t src, size_t dst0, int ncopy)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (size_t)gridDim.x * 256) {
        const T v = base[src * per + i];
        for (int c = 0; c < ncopy; ++c)
            if (dst0 + c != src) base[(dst0 + c) * per + i] = v;
    }
}
template <class T>
static hipError_t slot_copy(hipStream_t st, T* base, size_t per, size_t src, size_t dst0, int ncopy)
{
    const unsigned blocks = (unsigned)std::min<size_t>((per + 255) / 256, 2048);
    k_beam_slot_copy<T><<<dim3(blocks), dim3(256), 0, st>>>(base, per, src, dst0, ncopy);
    return hipGetLastError();
}
// every cross-K/V array is [nkv][Benc] equal slots: one launch per (kv layer, clip) and array, ordered so that no launch reads a slot an earlier one
// has written — expanding from the last (layer, clip) down (a destination index n (l G + g) + j is never below its source l G + g), compacting
// from the first up
static int cross_move(wm_ctx* ctx, int G, int n, bool expand)
{
    hipStream_t st = ctx->stream;
    const size_t per16 = (size_t)ctx->H * ctx->Spad * 64 * sizeof(bf16_t) / 16, per8 = (size_t)ctx->H * ctx->Spad * 64 / 16, perS = ctx->H;
    const int total = ctx->nkv * G;
    for (int q = 0; q < total; ++q) {
        const int x = expand ? total - 1 - q : q;           // x = l * G + g
        const size_t src = expand ? (size_t)x : (size_t)x * n, dst = expand ? (size_t)x * n : (size_t)x;
        const int nc = expand ? n : 1;
        WM_HIP(slot_copy(st, reinterpret_cast<uint4*>(ctx->kx), per16, src, dst, nc));
        WM_HIP(slot_copy(st, reinterpret_cast<uint4*>(ctx->vx), per16, src, dst, nc));
        if (ctx->xkv8) {
            WM_HIP(slot_copy(st, reinterpret_cast<uint4*>(ctx->kx8), per8, src, dst, nc));
            WM_HIP(slot_copy(st, reinterpret_cast<uint4*>(ctx->vx8), per8, src, dst, nc));
            WM_HIP(slot_copy(st, ctx->kxs, perS, src, dst, nc));
            WM_HIP(slot_copy(st, ctx->vxs, perS, src, dst, nc));
        }
    }
    WM_HIP(hipStreamSynchronize(st));
    return WM_OK;
}
int wm_beam_expand(wm_ctx* ctx, int G, int n)
{
    if (ctx->beam_expanded) return WM_OK;
    if (int rc = cross_move(ctx, G, n, true)) return rc;
    ctx->beam_expanded = true; ctx->Benc = G * n;
    return WM_OK;
}
int wm_beam_compact(wm_ctx* ctx)
{
    if (!ctx->beam_expanded) return WM_OK;
    const int n = ctx->beam.n, G = ctx->beam_clips;
    ctx->beam_expanded = false; ctx->Benc = G;
    return cross_move(ctx, G, n, false);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
int wm_beam_check(wm_ctx* ctx, const char* who, const wm_beam_params* bp)
{
    if (bp->num_beams < 2 || bp->num_beams > WM_BEAM_MAX) {
        ctx->err = std::string(who) + ": num_beams must be in [2, " + std::to_string(WM_BEAM_MAX) + "]"; return WM_ERR_ARG; }
    if (!std::isfinite(bp->length_penalty)) { ctx->err = std::string(who) + ": length_penalty must be finite"; return WM_ERR_ARG; }
    if (bp->early_stopping < 0 || bp->early_stopping > 2) { ctx->err = std::string(who) + ": early_stopping must be 0 (False), 1 (True) or 2 (\"never\")"; return WM_ERR_ARG; }
    return WM_OK;
}

int wm_beam_begin(wm_ctx* ctx, const wm_beam_params& bp, int G, const GenDev& g, bool kv, const float* init_scores, int len0, BeamDev* out)
{
    hipStream_t st = ctx->stream;
    if (!ctx->beam_state) ctx->beam_state = new wm_beam_state();
    wm_beam_state& S = *ctx->beam_state;
    const size_t MB = ctx->maxB, Tids = ctx->Tal;
    const int n = bp.num_beams, Bs = G * n;
    WM_HIP(S.run.reserve(MB)); WM_HIP(S.cval.reserve(2 * MB)); WM_HIP(S.cbeam.reserve(2 * MB)); WM_HIP(S.ctok.reserve(2 * MB));
    WM_HIP(S.fscore.reserve(MB)); WM_HIP(S.fset.reserve(MB)); WM_HIP(S.flen.reserve(MB)); WM_HIP(S.fids.reserve(MB * Tids));
    WM_HIP(S.heur.reserve(MB)); WM_HIP(S.cdone.reserve(MB)); WM_HIP(S.bidx.reserve(MB)); WM_HIP(S.ntok.reserve(MB));
    WM_HIP(S.lse.reserve(MB * SEL_SP * 2)); WM_HIP(S.reg.reserve(MB * SEL_SP * 4));
    WM_HIP(S.sval.reserve(MB * SEL_SP * BEAM_C)); WM_HIP(S.stok.reserve(MB * SEL_SP * BEAM_C));
    WM_HIP(S.den.reserve(Tids + 2)); WM_HIP(S.sh_ids.reserve(MB * Tids)); WM_HIP(S.sh_st.reserve(MB));
    ctx->beam_done = false;                 // (the tables of an earlier beam decode are overwritten)
    BeamDev b{};
    b.on = 1; b.n = n; b.G = G; b.es = bp.early_stopping; b.lp_pos = bp.length_penalty > 0.f ? 1 : 0;
    // the shadow holds what one step can move: rows [0, max_length) of every stream of this call, in units of 32 rows
    b.rows_cap = std::min(ctx->Tal, (std::max(g.max_length, 1) + 31) / 32 * 32);
    if (kv) WM_HIP(S.sh_kv.reserve((size_t)2 * ctx->nkv * Bs * ctx->H * (size_t)b.rows_cap * 64));
    b.run = S.run; b.cval = S.cval; b.cbeam = S.cbeam; b.ctok = S.ctok; b.fscore = S.fscore; b.fset = S.fset; b.flen = S.flen; b.fids = S.fids;
    b.heur = S.heur; b.cdone = S.cdone; b.bidx = S.bidx; b.ntok = S.ntok; b.lse = S.lse; b.reg = S.reg; b.sval = S.sval; b.stok = S.stok;
    b.den = S.den; b.sh_ids = S.sh_ids; b.sh_st = S.sh_st; b.sh_kv = S.sh_kv;
    // fl(t ** length_penalty): the power in double like the Python scalar, rounded to the fp32 the tensor division reads
    std::vector<float> den(Tids + 2);
    for (size_t t = 0; t < den.size(); ++t) den[t] = (float)std::pow((double)t, (double)bp.length_penalty);
    std::vector<float> run(Bs), fs(Bs, BEAM_NEG);
    for (int s = 0; s < Bs; ++s) run[s] = init_scores ? init_scores[s] : (s % n == 0 ? 0.f : BEAM_NEG);
    std::vector<int> zero(Bs, 0), one(G, 1), plen(Bs, std::min(len0, (int)Tids));
    WM_HIP(hipMemcpyAsync(S.den, den.data(), den.size() * sizeof(float), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.run, run.data(), Bs * sizeof(float), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.fscore, fs.data(), Bs * sizeof(float), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.fset, zero.data(), Bs * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.flen, plen.data(), Bs * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.heur, one.data(), G * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.cdone, zero.data(), G * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipStreamSynchronize(st));          // host vectors go out of scope
    *out = b;
    return WM_OK;
}

// HF: `sequences = running_sequences.clone()`: an entry of the finished table that is never set keeps its beam's starting ids (ctx->ids, uploaded by the caller)
int wm_beam_seed_table(wm_ctx* ctx, const BeamDev& bd)
{
    WM_HIP(hipMemcpyAsync(bd.fids, ctx->ids, (size_t)bd.G * bd.n * ctx->Tal * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    return WM_OK;
}

int wm_beam_step(wm_ctx* ctx, const GenDev& gp, const TsDev& ts, const BeamDev& bd, bool kv)
{
    hipStream_t st = ctx->stream;
    const int rows = bd.G * bd.n;
    const bool rules = wm_rules_on(ts);
    const size_t rp_bytes = rp_lds_bytes(ts, gp.V);
    const int per = (gp.V + SEL_SP - 1) / SEL_SP;
    k_beam_lse<<<dim3(SEL_SP, rows), dim3(256), 0, st>>>(ctx->logits, gp, bd, ctx->done);
    WM_HIP(hipGetLastError());
    // sequence bias (wm_set_sequence_bias): HF runs its processors on log_softmax(raw), so the normaliser above is the unbiased row's; the rows
    // are edited in place before the kernels below subtract it.  (The taps run with the context's scalars swapped: ctx->sbias is a decode's.)
    if (kv && ctx->sbias.on) { if (int rc = wm_seq_bias_launch(ctx, ctx->sbias, ctx->ids, gp.Tids, ctx->L, gp.Tids, rows)) return rc; }
    if (kv && ctx->cons.on) { if (int rc = wm_constraint_launch(ctx, ctx->cons, gp, ctx->ids, gp.Tids, ctx->L, gp.Tids, rows)) return rc; }     // (wm_set_constraint: the same place)
    if (ts.on) {
        k_beam_region<<<dim3(SEL_SP, rows), dim3(256), rp_bytes, st>>>(ctx->logits, gp, ctx->supmask, ctx->exppen, ctx->L, ts, bd, ctx->done);
        WM_HIP(hipGetLastError());
    }
    const size_t lds = rp_bytes + (size_t)per * sizeof(float);
    if (rules)
        k_beam_slice<true><<<dim3(SEL_SP, rows), dim3(256), lds, st>>>(ctx->logits, gp, ctx->supmask, ctx->exppen, ctx->L, ts, bd, (int)(rp_bytes / 4), ctx->done);
    else
        k_beam_slice<false><<<dim3(SEL_SP, rows), dim3(256), lds, st>>>(ctx->logits, gp, ctx->supmask, ctx->exppen, ctx->L, ts, bd, 0, ctx->done);
    WM_HIP(hipGetLastError());
    k_beam_merge<<<dim3(bd.G), dim3(256), 0, st>>>(gp, bd, ctx->done);
    WM_HIP(hipGetLastError());
    k_beam_book<<<dim3(bd.G), dim3(64), 0, st>>>(gp, bd, ctx->ids, ctx->L, ctx->kvlen, ctx->finished, ctx->niter, ctx->hist, ctx->done);
    WM_HIP(hipGetLastError());
    k_beam_ids_gather<<<dim3(rows), dim3(64), 0, st>>>(bd, ctx->ids, ctx->kvlen, gp.Tids, ts);
    WM_HIP(hipGetLastError());
    if (kv) {
        k_beam_kv_gather<<<dim3(ctx->H, rows, ctx->nkv), dim3(256), 0, st>>>(bd, ctx->kc, ctx->vc, ctx->kvlen, ctx->H, ctx->Tal, ctx->maxB, rows);
        WM_HIP(hipGetLastError());
    }
    k_beam_ids_scatter<<<dim3(rows), dim3(64), 0, st>>>(bd, ctx->ids, ctx->kvlen, gp.Tids, ts);
    WM_HIP(hipGetLastError());
    if (kv) {
        k_beam_kv_scatter<<<dim3(ctx->H, rows, ctx->nkv), dim3(256), 0, st>>>(bd, ctx->kc, ctx->vc, ctx->kvlen, ctx->H, ctx->Tal, ctx->maxB, rows);
        WM_HIP(hipGetLastError());
    }
    return WM_OK;
}

// ---- C-ABI -----------------------------------------------------------------------------------------------------------------------------
// HF generate(num_beams=n, length_penalty=, early_stopping=) -> GenerationMixin._beam_search: kept on the context, read by wm_decode_begin*
extern "C" int wm_set_beam(wm_ctx* ctx, const wm_beam_params* bp)
{
    if (!ctx) return WM_ERR_ARG;
    if (!bp) { ctx->beam_set_on = false; return WM_OK; }
    if (int rc = wm_beam_check(ctx, "wm_set_beam", bp)) return rc;
    ctx->beam_set_on = true; ctx->beam_set = *bp;
    return WM_OK;
}

// HF _beam_search's return: row clip * num_return_sequences + rank of `sequences` / `sequences_scores`
extern "C" int wm_get_beam_result(wm_ctx* ctx, int clip, int rank, int32_t* out_ids, int cap, int* n, float* score)
{
    if (!ctx || !out_ids || !n || !score) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    if (!ctx->beam_done || !ctx->beam_state) { ctx->err = "wm_get_beam_result: no finished beam decode on this context"; return WM_ERR_STATE; }
    if (clip < 0 || clip >= ctx->beam_clips || rank < 0 || rank >= ctx->beam.n) { ctx->err = "wm_get_beam_result: clip / rank out of range"; return WM_ERR_ARG; }
    const int e = clip * ctx->beam.n + rank, Tids = ctx->Tal;
    int len = 0; float sc = 0.f;
    WM_HIP(hipMemcpyAsync(&len, ctx->beam.flen + e, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipMemcpyAsync(&sc, ctx->beam.fscore + e, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    len = std::max(0, std::min(len, Tids));
    std::vector<int> ids(std::max(len, 1));
    WM_HIP(hipMemcpyAsync(ids.data(), ctx->beam.fids + (size_t)e * Tids, len * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(out_ids, ids.data(), std::min(len, cap) * sizeof(int));
    *n = len; *score = sc;
    return WM_OK;
}

// HF Cache.reorder_cache(beam_idx) (GenerationMixin._beam_search step g) alone
extern "C" int wm_beam_reorder_kv(wm_ctx* ctx, int B_streams, const int32_t* beam_idx, int len)
{
    if (!ctx) return WM_ERR_ARG;
    if (!beam_idx || B_streams < 1 || B_streams > ctx->maxB || len < 1 || len > ctx->Tmax) { ctx->err = "wm_beam_reorder_kv: B_streams must be in [1, max_batch], len in [1, n_tgt]"; return WM_ERR_ARG; }
    for (int s = 0; s < B_streams; ++s)
        if (beam_idx[s] < 0 || beam_idx[s] >= B_streams) { ctx->err = "wm_beam_reorder_kv: beam_idx out of range"; return WM_ERR_ARG; }
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    wm_decode_invalidate(ctx);
    GenDev g{}; g.max_length = len; g.P = 1;
    // B_streams single-beam "clips": only the shadow buffer and the two index arrays of the state are used
    BeamDev bd{};
    if (int rc = wm_beam_begin(ctx, wm_beam_params{1, 1.0f, 0}, B_streams, g, true, nullptr, 1, &bd)) return rc;
    std::vector<int> zero(B_streams, 0), kv(B_streams, len);
    WM_HIP(hipMemcpyAsync(bd.bidx, beam_idx, B_streams * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(bd.ntok, zero.data(), B_streams * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(ctx->kvlen, kv.data(), B_streams * sizeof(int), hipMemcpyHostToDevice, st));
    k_beam_kv_gather<<<dim3(ctx->H, B_streams, ctx->nkv), dim3(256), 0, st>>>(bd, ctx->kc, ctx->vc, ctx->kvlen, ctx->H, ctx->Tal, ctx->maxB, B_streams);
    WM_HIP(hipGetLastError());
    k_beam_kv_scatter<<<dim3(ctx->H, B_streams, ctx->nkv), dim3(256), 0, st>>>(bd, ctx->kc, ctx->vc, ctx->kvlen, ctx->H, ctx->Tal, ctx->maxB, B_streams);
    WM_HIP(hipGetLastError());
    WM_HIP(hipStreamSynchronize(st));
    return WM_OK;
}

// Beam-search parity tap: caller-given rows through the select, bookkeeping and ids-reorder kernels (include/wm.h)
extern "C" int wm_beam_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, const wm_beam_params* bp, int G, int S,
                            const float* logits, const int32_t* prefixes, int Tmax, int prefix_len, const float* init_scores,
                            float* cand_val, int32_t* cand_beam, int32_t* cand_tok, int32_t* beam_idx, int32_t* out_steps,
                            int32_t* fin_ids, int32_t* fin_len, float* fin_score, int32_t* fin_set, int32_t* run_ids, int32_t* run_len, float* run_score)
{
    if (!ctx) return WM_ERR_ARG;
    if (!gp || !bp || G < 1 || S < 1 || !logits || !prefixes || Tmax < 1 || !cand_val || !cand_beam || !cand_tok || !beam_idx || !out_steps || !fin_ids ||
        !fin_len || !fin_score || !fin_set || !run_ids || !run_len || !run_score) { ctx->err = "wm_beam_rows: bad arguments"; return WM_ERR_ARG; }
    if (int rc = wm_beam_check(ctx, "wm_beam_rows", bp)) return rc;
    const int n = bp->num_beams, Bs = G * n, Tids = ctx->Tal;
    if (Bs > ctx->maxB) { ctx->err = "wm_beam_rows: G * num_beams exceeds max_batch"; return WM_ERR_ARG; }
    if (prefix_len < std::max(gp->prompt_len, 1) || prefix_len > Tmax || prefix_len + S > std::min(Tmax, ctx->Tmax)) {
        ctx->err = "wm_beam_rows: prefix_len must be in [max(prompt_len, 1), Tmax] with prefix_len + S <= min(Tmax, n_tgt)"; return WM_ERR_ARG; }
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    GenDev g{}; TsDev ts{};
    if (int rc = wm_proc_setup(ctx, "wm_beam_rows", gp, tsp, &g, &ts)) return rc;
    g.max_length = g.hard_max_length = std::min(gp->max_length, ctx->Tmax);
    g.inv_temp = 1.0f; g.force_accept = -1; g.accept_mode = WM_ACCEPT_GREEDY; g.vanilla = 1;
    wm_decode_invalidate(ctx);
    wm_scalars_swap swap(ctx, g, ts);
    BeamDev bd{};
    if (int rc = wm_beam_begin(ctx, *bp, G, g, false, init_scores, prefix_len, &bd)) return rc;
    std::vector<int> ids((size_t)Bs * Tids, gp->pad_token_id), L(Bs, prefix_len), kvl(Bs, prefix_len - 1), zero(Bs, 0);
    std::vector<int4> tst(Bs, make_int4(0, 0, -1, 0));
    for (int s = 0; s < Bs; ++s) {
        for (int t = 0; t < prefix_len; ++t) ids[(size_t)s * Tids + t] = prefixes[(size_t)s * Tmax + t];
        if (ts.on) tst[s] = ts_fold_ids(tst[s], prefixes + (size_t)s * Tmax, g.begin, prefix_len, ts.tb);
    }
    WM_HIP(hipMemcpyAsync(ctx->ids, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (int rc = wm_beam_seed_table(ctx, bd)) return rc;
    WM_HIP(hipMemcpyAsync(ctx->L, L.data(), Bs * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(ctx->kvlen, kvl.data(), Bs * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(ctx->finished, zero.data(), Bs * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(ctx->niter, zero.data(), Bs * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemsetAsync(ctx->done, 0, 4 * sizeof(int), st));
    WM_HIP(hipMemsetAsync(ctx->hist, 0, 32 * sizeof(long long), st));
    if (ts.on) WM_HIP(hipMemcpyAsync(ts.st, tst.data(), Bs * sizeof(int4), hipMemcpyHostToDevice, st));
    WM_HIP(hipStreamSynchronize(st));
    std::vector<int> cd(G, 0), cd_prev(G, 0);
    for (int g0 = 0; g0 < G; ++g0) out_steps[g0] = S;
    const int n2 = 2 * n;
    for (int step = 0; step < S; ++step) {
        WM_HIP(wm_tap_upload_logits(ctx, logits + (size_t)step * Bs * ctx->V, Bs));        // (step-shaped, not group-shaped: the taps' logits upload alone)
        if (int rc = wm_beam_step(ctx, g, ts, bd, false)) return rc;
        WM_HIP(hipMemcpyAsync(cand_val + (size_t)step * G * n2, bd.cval, (size_t)G * n2 * sizeof(float), hipMemcpyDeviceToHost, st));
        WM_HIP(hipMemcpyAsync(cand_beam + (size_t)step * G * n2, bd.cbeam, (size_t)G * n2 * sizeof(int), hipMemcpyDeviceToHost, st));
        WM_HIP(hipMemcpyAsync(cand_tok + (size_t)step * G * n2, bd.ctok, (size_t)G * n2 * sizeof(int), hipMemcpyDeviceToHost, st));
        WM_HIP(hipMemcpyAsync(beam_idx + (size_t)step * Bs, bd.bidx, Bs * sizeof(int), hipMemcpyDeviceToHost, st));
        WM_HIP(hipMemcpyAsync(cd.data(), bd.cdone, G * sizeof(int), hipMemcpyDeviceToHost, st));
        WM_HIP(hipStreamSynchronize(st));
        for (int g0 = 0; g0 < G; ++g0) if (cd[g0] && !cd_prev[g0]) { out_steps[g0] = step + 1; cd_prev[g0] = 1; }
    }
    std::vector<int> fbuf((size_t)Bs * Tids), rbuf((size_t)Bs * Tids);
    WM_HIP(hipMemcpyAsync(fbuf.data(), bd.fids, fbuf.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    WM_HIP(hipMemcpyAsync(rbuf.data(), ctx->ids, rbuf.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    WM_HIP(hipMemcpyAsync(fin_len, bd.flen, Bs * sizeof(int), hipMemcpyDeviceToHost, st));
    WM_HIP(hipMemcpyAsync(fin_score, bd.fscore, Bs * sizeof(float), hipMemcpyDeviceToHost, st));
    WM_HIP(hipMemcpyAsync(fin_set, bd.fset, Bs * sizeof(int), hipMemcpyDeviceToHost, st));
    WM_HIP(hipMemcpyAsync(run_len, ctx->L, Bs * sizeof(int), hipMemcpyDeviceToHost, st));
    WM_HIP(hipMemcpyAsync(run_score, bd.run, Bs * sizeof(float), hipMemcpyDeviceToHost, st));
    WM_HIP(hipStreamSynchronize(st));
    for (int s = 0; s < Bs; ++s)
        for (int t = 0; t < Tmax; ++t) {
            fin_ids[(size_t)s * Tmax + t] = t < Tids ? fbuf[(size_t)s * Tids + t] : gp->pad_token_id;
            run_ids[(size_t)s * Tmax + t] = t < Tids ? rbuf[(size_t)s * Tids + t] : gp->pad_token_id;
        }
    return WM_OK;
}
