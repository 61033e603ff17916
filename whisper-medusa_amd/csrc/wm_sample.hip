// wm_sample.hip — seeded sampling on the plain decode path (include/wm.h wm_set_sampling / wm_sample_rows): what HF's
// generate(do_sample=True, temperature=T) does behind its processors — warp the processed row by 1 / T and draw from its softmax — as a
// Gumbel-max over counter-based noise, so that a token's draw depends on (seed, stream key, position, token id) alone.
//   k_sample1:    grid (SEL_SP, rows) x 256: per vocabulary slice and region ([0, tb) text, [tb, V) timestamps) the unperturbed maximum (and the
//                 timestamp region's sum of exp at temperature 1: the log-softmax decision is taken before the temperature), and the maximum
//                 and arg-max of v / T + g.
//   k_sample_fin: one thread per row: merges the slices, takes the decision, writes the token where k_select_argmax* writes its arg-max.
//   k_filter_prep / k_filter_row (below; wm_set_sampling_filter): with a top-k / top-p / min-p filter on they stand in for k_sample_fin.
// The processed row v is select1_body's pl(n): repetition rules, proc_logit, timestamp masks, each under the row's own prefix.
#include "wm_select.h"

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11; the Random123 constants)
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c;
}
// u = (2 (x >> 9) + 1) 2^-24: odd multiples of 2^-24 in [2^-24, 1 - 2^-24], each exact in fp32 — never 0 or 1, so g is finite
__device__ __forceinline__ float gumbel_of(unsigned x)
{
    const float u = (float)(2u * (x >> 9) + 1u) * 5.9604644775390625e-08f;
    return -logf(-logf(u));
}

// The processed row v of one block's slice [n0, n1) of a sampled row — the ONE definition k_sample1 and k_filter_prep share: the set-up (tb, the
// row's timestamp record, the repetition bitmaps of the slice in dynamic LDS, built by the block's 256 threads) and pl(n): the repetition penalty,
// proc_logit, the timestamp masks, the n-gram ban (wm_select.h), each under the row's own prefix.  A macro over the kernel's own names (TS, gp, ts,
// tap, row, cur_len, x, mask, exppen, n0, n1, tid), like wm_beam.hip's row prologue: the expansion is the text k_sample1 always had, so its code
// object does not move (a struct or a function holding the same lines reorders instructions of k_sample1<true>).
#define SAMP_ROW_PL                                                                                                                 \
    const int tb = TS ? ts.tb : gp.V;                                                                                               \
    int4 rec = make_int4(0, 0, 0, 0);                                                                                               \
    if (TS) rec = ts_row_record(gp, ts, tap, tap ? 0 : row, tap ? row : 0, cur_len);                                                \
    extern __shared__ unsigned rp_sh[];                                                                                             \
    const bool rp = TS && ts.rp != 0;                                                                                               \
    if (rp) rp_build(ts, rp_row_prefix(ts, 0, row, row, cur_len), n0, n1, -1, gp.V, rp_sh, tid, 256);                               \
    auto pl = [&](int n) {                                                                                                          \
        float v = x[n];                                                                                                             \
        if (rp) v = rp_pen(v, n, n0, ts, rp_sh);                                                                                    \
        v = proc_logit(v, n, cur_len, gp, mask, exppen);                                                                            \
        if (TS) v = ts_mask(v, n, rec, gp, ts);                                                                                     \
        if (rp && rp_banned(n, n0, gp.V, rp_sh)) v = -INFINITY;                                                                     \
        return v;                                                                                                                   \
    }

template <bool TS>
__global__ void __launch_bounds__(256)
k_sample1(const float* __restrict__ logits, GenDev gp, const unsigned char* __restrict__ mask, const float* __restrict__ exppen,
          const int* __restrict__ pos, TsDev ts, SampDev sd, int tap)
{
    __shared__ float sv[4]; __shared__ int si[4]; __shared__ float sz[4];
    const int row = blockIdx.y, sp = blockIdx.x, tid = threadIdx.x;
    const int cur_len = pos[row];
    const float* x = logits + (size_t)row * gp.Vpad;
    const int per = (gp.V + SEL_SP - 1) / SEL_SP, n0 = sp * per, n1 = min(gp.V, n0 + per);
    SAMP_ROW_PL;
    const unsigned long long key = sd.keys[row];
    const unsigned key_lo = (unsigned)key, key_hi = (unsigned)(key >> 32);
    float mt = -INFINITY, ms = -INFINITY;                           // unperturbed maxima of the two regions
    float pt = -INFINITY, ps = -INFINITY; int it = 0x7fffffff, is = 0x7fffffff;     // perturbed maxima and their ids
    auto take = [&](int n, unsigned xw) {
        if (n < n0 || n >= n1) return;
        const float v = pl(n);
        // a masked token keeps -inf (and its id: a row with nothing left yields the lowest id, as the arg-max kernels do)
        const float p = (v == -INFINITY) ? -INFINITY : __fmaf_rn(v, sd.inv_t, gumbel_of(xw));
        // (both regions' updates as selects on values: an `if (n < tb) .. else ..` over the captured references becomes a runtime-indexed
        // private array {text, timestamps} — scratch traffic per token)
        const bool txt = n < tb;
        mt = fmaxf(mt, txt ? v : -INFINITY); ms = fmaxf(ms, txt ? -INFINITY : v);
        const bool wt = txt && (p > pt || (p == pt && n < it)), ws = !txt && (p > ps || (p == ps && n < is));
        pt = wt ? p : pt; it = wt ? n : it;
        ps = ws ? p : ps; is = ws ? n : is;
    };
    // one Philox block serves the four ids 4 q .. 4 q + 3: the slice is swept in aligned groups, its ragged ends tested per id
    for (int q = (n0 >> 2) + tid; 4 * q < n1; q += 256) {
        const uint4 xw = philox4x32_10(make_uint4((unsigned)q, (unsigned)cur_len, key_lo, key_hi), sd.seed_lo, sd.seed_hi);
        take(4 * q, xw.x); take(4 * q + 1, xw.y); take(4 * q + 2, xw.z); take(4 * q + 3, xw.w);
    }
    int dummy = 0;
    block_argmax(mt, dummy, sv, si, tid);
    block_argmax(pt, it, sv, si, tid);
    float zs1 = 0.f;
    if (TS) {
        dummy = 0;
        block_argmax(ms, dummy, sv, si, tid);
        block_argmax(ps, is, sv, si, tid);
        for (int n = max(n0, tb) + tid; n < n1; n += 256) {
            const float v = pl(n);
            if (v != -INFINITY) zs1 += expf(v - ms);
        }
        zs1 = block_sum(zs1, sz, tid);
    }
    if (tid == 0) {
        float* o = sd.part + ((size_t)row * SEL_SP + sp) * 8;
        o[0] = mt; o[1] = pt; o[2] = __int_as_float(it);
        o[3] = ms; o[4] = zs1; o[5] = ps; o[6] = __int_as_float(is); o[7] = 0.f;
    }
}

__global__ void k_sample_fin(SampDev sd, int nrows, int out_row0, int* __restrict__ amax, int* __restrict__ forced_out)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows) return;
    const float* p = sd.part + (size_t)row * SEL_SP * 8;
    float mt = -INFINITY, ms = -INFINITY;
    for (int k = 0; k < SEL_SP; ++k) { mt = fmaxf(mt, p[8 * k]); ms = fmaxf(ms, p[8 * k + 3]); }
    float zs1 = 0.f;
    for (int k = 0; k < SEL_SP; ++k) if (p[8 * k + 3] != -INFINITY) zs1 += p[8 * k + 4] * expf(p[8 * k + 3] - ms);
    const int forced = (ms != -INFINITY && ms + logf(zs1) > mt) ? 1 : 0;        // ts_finish's decision: at temperature 1, before the noise
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int k = 0; k < SEL_SP; ++k) {
        const float u = p[8 * k + 5]; const int iu = __float_as_int(p[8 * k + 6]);
        if (u > best || (u == best && iu < bi)) { best = u; bi = iu; }
        if (forced) continue;
        const float v = p[8 * k + 1]; const int iv = __float_as_int(p[8 * k + 2]);
        if (v > best || (v == best && iv < bi)) { best = v; bi = iv; }
    }
    amax[out_row0 + row] = (bi == 0x7fffffff) ? 0 : bi;
    if (forced_out) forced_out[out_row0 + row] = forced;
    sd.val[out_row0 + row] = best;
}

// ---- top-k / top-p / min-p filters (include/wm.h wm_set_sampling_filter) ----------------------------------------------------------
// All three filters are one fp32 value threshold tau per row, applied between the decision and the perturbed arg-max.  With a filter on, a row runs
//   k_sample1:     as above: its slice partials carry the region maxima and the timestamp region's sum of exp, i.e. the decision;
//   k_filter_prep: grid (SEL_SP, rows) x 256: the processed row pl(n) after the decision (text masked where the row is forced), written once as fp32;
//   k_filter_row:  one block of 1024 threads per row: tau by selects over integer LDS histograms — a coarse digit (1/128-logit steps below the row's
//                  maximum), then MSB-first radix passes (12 + 10 + 10 bits) over the order-preserving key inside the selected bin; counts for
//                  top-k, 2^40 fixed-point masses of exp((v - m) / T) for top-p —, the min-p threshold as a minimum over the values that pass
//                  its test, then the perturbed arg-max of k_sample1 restricted to v >= tau and the outputs.
// Nothing here adds floats in an order that depends on the grid: counts and masses are 64-bit integers, maxima and minima are order-free.
#define FLT_NT 1024
#define FLT_BINS 4096
#define FLT_ONE 1099511627776.0f        // 2^40: exp(a) in (0, 1] in fixed point

// order-preserving key of a finite or infinite fp32 value; -0.0 and +0.0 share one key (v >= tau is a float comparison)
__device__ __forceinline__ unsigned flt_key(float v)
{
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float flt_val(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
// a_n = fl(fl(v - m) * fl(1 / T)), two roundings (never contracted); the mass is round-to-nearest of expf(a) * 2^40
__device__ __forceinline__ float flt_arg(float v, float m, float inv_t) { return __fmul_rn(__fsub_rn(v, m), inv_t); }
__device__ __forceinline__ unsigned long long flt_mass(float v, float m, float inv_t)
{
    return __float2ull_rn(__fmul_rn(expf(flt_arg(v, m, inv_t)), FLT_ONE));
}
// k_sample_fin's decision from a row's slice partials (the same operations in the same order): forced, and the maximum of what the decision leaves
__device__ __forceinline__ int flt_decision(const float* p, float& m)
{
    float mt = -INFINITY, ms = -INFINITY;
    for (int k = 0; k < SEL_SP; ++k) { mt = fmaxf(mt, p[8 * k]); ms = fmaxf(ms, p[8 * k + 3]); }
    float zs1 = 0.f;
    for (int k = 0; k < SEL_SP; ++k) if (p[8 * k + 3] != -INFINITY) zs1 += p[8 * k + 4] * expf(p[8 * k + 3] - ms);
    const int forced = (ms != -INFINITY && ms + logf(zs1) > mt) ? 1 : 0;
    m = forced ? ms : fmaxf(mt, ms);
    return forced;
}

template <bool TS>
__global__ void __launch_bounds__(256)
k_filter_prep(const float* __restrict__ logits, GenDev gp, const unsigned char* __restrict__ mask, const float* __restrict__ exppen,
              const int* __restrict__ pos, TsDev ts, SampDev sd, int tap)
{
    __shared__ int s_forced;
    const int row = blockIdx.y, sp = blockIdx.x, tid = threadIdx.x;
    const int cur_len = pos[row];
    const float* x = logits + (size_t)row * gp.Vpad;
    const int per = (gp.V + SEL_SP - 1) / SEL_SP, n0 = sp * per, n1 = min(gp.V, n0 + per);
    SAMP_ROW_PL;
    if (tid == 0) { float m; s_forced = flt_decision(sd.part + (size_t)row * SEL_SP * 8, m); }
    __syncthreads();
    const bool forced = s_forced != 0;
    float* o = sd.fv + (size_t)row * gp.Vpad;
    for (int n = n0 + tid; n < n1; n += 256) o[n] = (forced && n < tb) ? -INFINITY : pl(n);
}

// exclusive prefix sum over the block's FLT_NT threads in thread order (integers: the grouping does not matter); total: the block's sum
__device__ __forceinline__ unsigned long long flt_scan(unsigned long long v, unsigned long long* sw, int tid, unsigned long long& total)
{
    const int lane = tid & 63, w = tid >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) sw[w] = inc;
    __syncthreads();
    unsigned long long base = 0; total = 0;
    for (int k = 0; k < FLT_NT / 64; ++k) { const unsigned long long t = sw[k]; if (k < w) base += t; total += t; }
    return base + inc - v;
}
// one sweep of the row by the block: thread t visits ids 4 q .. 4 q + 3, q = t, t + FLT_NT, .. (one 16-byte load; the row's stride is a multiple
// of 128 floats, ids >= V read as -inf, which every visitor skips)
template <class Fn>
__device__ __forceinline__ void flt_sweep(const float* __restrict__ x, int V, int tid, Fn&& fn)
{
    for (int q = tid; 4 * q < V; q += FLT_NT) {
        const int n = 4 * q;
        const float4 v = *reinterpret_cast<const float4*>(x + n);
        fn(n, v.x); fn(n + 1, n + 1 < V ? v.y : -INFINITY); fn(n + 2, n + 2 < V ? v.z : -INFINITY); fn(n + 3, n + 3 < V ? v.w : -INFINITY);
    }
}
// the coarse first digit: 1/128-logit steps below the row's maximum m, clamped to FLT_BINS - 1 steps, stored top down (a larger index never holds
// a smaller value: one fp32 subtraction, an exact scaling and a truncation are all monotone).  The leading bits of an fp32 key do not spread a row
// of logits — a few exponents hold everything, and every lane of a wave would hit the same LDS word —; equal steps below the maximum do.
__device__ __forceinline__ int flt_lin(float v, float m)
{
    const float t = __fsub_rn(m, v) * 128.0f;
    return t >= (float)(FLT_BINS - 1) ? 0 : FLT_BINS - 1 - (int)t;
}
// Select over the keys >= lo of the row x[0, V): the key at which the sum of weights, taken from the largest key down, first reaches `target` —
// weights 1 (MASS = false, target = k: the k-th largest value) or the fixed-point masses (MASS = true, target = ceil(top_p * total): the last
// value whose strictly greater values hold less than top_p of the mass).  Four sweeps: the coarse digit flt_lin, then, inside the bin it selects,
// an MSB-first radix select over the 32-bit key (12 + 10 + 10 bits).  Returns false when the total weight is below the target (fewer than k
// values) and, for counts, when it equals it (the k-th largest is the smallest: nothing to cut).
// A thread adds a run of equal digits in registers and flushes it with one LDS atomic: a row of equal values costs no contention.
template <bool MASS>
__device__ bool flt_select(const float* __restrict__ x, int V, unsigned lo, float m, float inv_t, unsigned long long target, float top_p,
                           unsigned long long* hist, unsigned long long* sw, unsigned long long* sres, int tid, unsigned& out_key)
{
    unsigned prefix = 0u, pmask = 0u;
    int lin = 0;
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = pass == 1 ? 20 : (pass == 2 ? 10 : 0), nb = pass < 2 ? FLT_BINS : 1024;
        for (int k = tid; k < nb; k += FLT_NT) hist[k] = 0ull;
        if (tid == 0) sres[0] = ~0ull;
        __syncthreads();
        int cd = -1; unsigned long long cw = 0ull;
        flt_sweep(x, V, tid, [&](int, float v) {
            const unsigned key = flt_key(v);
            if (v == -INFINITY || key < lo) return;
            const int dl = flt_lin(v, m);
            if (pass > 0 && (dl != lin || (key & pmask) != prefix)) return;
            const int d = pass == 0 ? dl : (int)((key >> shift) & (unsigned)(nb - 1));
            const unsigned long long w = MASS ? flt_mass(v, m, inv_t) : 1ull;
            if (d != cd) { if (cw) atomicAdd(&hist[cd], cw); cd = d; cw = 0ull; }
            cw += w;
        });
        if (cw) atomicAdd(&hist[cd], cw);
        __syncthreads();
        // thread t owns the `per` bins below nb - t * per, walked downwards: thread order is descending key order
        const int per = nb / FLT_NT, top = nb - 1 - tid * per;
        unsigned long long local = 0ull;
        for (int j = 0; j < per; ++j) local += hist[top - j];
        unsigned long long total;
        const unsigned long long excl = flt_scan(local, sw, tid, total);
        if (pass == 0) {
            if (MASS) target = (unsigned long long)ceil((double)top_p * (double)total);
            if (target < 1ull) target = 1ull;
            if (total < target || (!MASS && total == target)) return false;
        }
        if (excl < target && target <= excl + local) {
            unsigned long long c = excl;
            for (int j = 0; j < per; ++j) {
                const unsigned long long h = hist[top - j];
                if (c + h >= target) { sres[0] = (unsigned long long)(top - j); sres[1] = target - c; break; }
                c += h;
            }
        }
        __syncthreads();
        if (pass == 0) lin = (int)sres[0];
        else { prefix |= (unsigned)sres[0] << shift; pmask |= (unsigned)(nb - 1) << shift; }
        target = sres[1];
        __syncthreads();
    }
    out_key = prefix;
    return true;
}

__global__ void __launch_bounds__(FLT_NT)
k_filter_row(GenDev gp, const int* __restrict__ pos, SampDev sd, int out_row0, int* __restrict__ amax, int* __restrict__ forced_out)
{
    __shared__ unsigned long long hist[FLT_BINS];
    __shared__ unsigned long long sw[FLT_NT / 64], sres[2];
    __shared__ float s_m; __shared__ int s_forced;
    __shared__ float rv[FLT_NT / 64]; __shared__ int ri[FLT_NT / 64]; __shared__ unsigned rk[FLT_NT / 64]; __shared__ int rc[FLT_NT / 64];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, V = gp.V;
    const float* x = sd.fv + (size_t)row * gp.Vpad;
    if (tid == 0) { float m; s_forced = flt_decision(sd.part + (size_t)row * SEL_SP * 8, m); s_m = m; }
    __syncthreads();
    const float m = s_m;
    unsigned tau = flt_key(-INFINITY);                                      // keeps every finite value
    if (m != -INFINITY) {                                                   // (a row with nothing left: no threshold, token 0 below)
        unsigned key;
        if (sd.top_k > 0 && flt_select<false>(x, V, 0u, m, sd.inv_t, (unsigned long long)sd.top_k, 1.0f, hist, sw, sres, tid, key)) tau = max(tau, key);
        if (sd.top_p < 1.0f && flt_select<true>(x, V, tau, m, sd.inv_t, 0ull, sd.top_p, hist, sw, sres, tid, key)) tau = max(tau, key);
        if (sd.min_p > 0.0f) {                                              // the smallest value that passes expf(a) >= min_p (the maximum always does)
            unsigned lk = 0xffffffffu;
            flt_sweep(x, V, tid, [&](int, float v) {
                if (v != -INFINITY && expf(flt_arg(v, m, sd.inv_t)) >= sd.min_p) lk = min(lk, flt_key(v));
            });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) lk = min(lk, (unsigned)__shfl_xor((int)lk, o, 64));
            __syncthreads();
            if (lane == 0) rk[wv] = lk;
            __syncthreads();
            for (int k = 0; k < FLT_NT / 64; ++k) lk = min(lk, rk[k]);
            tau = max(tau, lk);
        }
    }
    const float thr = flt_val(tau);
    // k_sample1's draw over {v > -inf, v >= thr}: the same Philox blocks, the same fused multiply-add, ties to the lower id
    const int cur_len = pos[row];
    const unsigned long long skey = sd.keys[row];
    const unsigned key_lo = (unsigned)skey, key_hi = (unsigned)(skey >> 32);
    float best = -INFINITY; int bi = 0x7fffffff, cnt = 0;
    for (int q = tid; 4 * q < V; q += FLT_NT) {
        const float4 ld = *reinterpret_cast<const float4*>(x + 4 * q);
        float v4[4] = {ld.x, ld.y, ld.z, ld.w}; bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * q + j >= V || v4[j] == -INFINITY || !(v4[j] >= thr)) v4[j] = -INFINITY;
            any = any || v4[j] != -INFINITY;
        }
        if (!any) continue;
        const uint4 xw = philox4x32_10(make_uint4((unsigned)q, (unsigned)cur_len, key_lo, key_hi), sd.seed_lo, sd.seed_hi);
        const unsigned xs[4] = {xw.x, xw.y, xw.z, xw.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (v4[j] == -INFINITY) continue;
            const int n = 4 * q + j;
            const float p = __fmaf_rn(v4[j], sd.inv_t, gumbel_of(xs[j]));
            ++cnt;
            if (p > best || (p == best && n < bi)) { best = p; bi = n; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        cnt += __shfl_xor(cnt, o, 64);
    }
    __syncthreads();
    if (lane == 0) { rv[wv] = best; ri[wv] = bi; rc[wv] = cnt; }
    __syncthreads();
    if (tid == 0) {
        best = rv[0]; bi = ri[0]; cnt = rc[0];
        for (int k = 1; k < FLT_NT / 64; ++k) {
            if (rv[k] > best || (rv[k] == best && ri[k] < bi)) { best = rv[k]; bi = ri[k]; }
            cnt += rc[k];
        }
        amax[out_row0 + row] = (bi == 0x7fffffff) ? 0 : bi;
        if (forced_out) forced_out[out_row0 + row] = s_forced;
        sd.val[out_row0 + row] = best;
        sd.thr[out_row0 + row] = thr;
        sd.kept[out_row0 + row] = cnt;
    }
}

int wm_sample_launch(wm_ctx* ctx, const GenDev& gp, const TsDev& ts, const SampDev& sd, const int* pos, int nrows, int out_row0, int tap)
{
    hipStream_t st = ctx->stream;
    if (wm_rules_on(ts))
        k_sample1<true><<<dim3(SEL_SP, nrows), dim3(256), rp_lds_bytes(ts, gp.V), st>>>(ctx->logits, gp, ctx->supmask, ctx->exppen, pos, ts, sd, tap);
    else
        k_sample1<false><<<dim3(SEL_SP, nrows), dim3(256), 0, st>>>(ctx->logits, gp, ctx->supmask, ctx->exppen, pos, ts, sd, tap);
    WM_HIP(hipGetLastError());
    if (wm_filter_on(sd)) {     // the filters: the row after the decision, then threshold, draw and outputs (k_sample_fin's) in one block per row
        if (wm_rules_on(ts))
            k_filter_prep<true><<<dim3(SEL_SP, nrows), dim3(256), rp_lds_bytes(ts, gp.V), st>>>(ctx->logits, gp, ctx->supmask, ctx->exppen, pos, ts, sd, tap);
        else
            k_filter_prep<false><<<dim3(SEL_SP, nrows), dim3(256), 0, st>>>(ctx->logits, gp, ctx->supmask, ctx->exppen, pos, ts, sd, tap);
        WM_HIP(hipGetLastError());
        k_filter_row<<<dim3(nrows), dim3(FLT_NT), 0, st>>>(gp, pos, sd, out_row0, ctx->amax, wm_rules_on(ts) ? ts.forced : nullptr);
        WM_HIP(hipGetLastError());
        return WM_OK;
    }
    k_sample_fin<<<dim3((nrows + 63) / 64), dim3(64), 0, st>>>(sd, nrows, out_row0, ctx->amax, wm_rules_on(ts) ? ts.forced : nullptr);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
