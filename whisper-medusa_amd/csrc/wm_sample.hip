// wm_sample.hip — seeded sampling on the plain decode path (include/wm.h wm_set_sampling / wm_sample_rows): what HF's
// generate(do_sample=True, temperature=T) does behind its processors — warp the processed row by 1 / T and draw from its softmax — as a
// Gumbel-max over counter-based noise, so that a token's draw depends on (seed, stream key, position, token id) alone.
//   k_sample1:    grid (SEL_SP, rows) x 256: per vocabulary slice and region ([0, tb) text, [tb, V) timestamps) the unperturbed maximum (and the
//                 timestamp region's sum of exp at temperature 1: the log-softmax decision is taken before the temperature), and the maximum
//                 and arg-max of v / T + g.
//   k_sample_fin: one thread per row: merges the slices, takes the decision, writes the token where k_select_argmax* writes its arg-max.
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
    const int tb = TS ? ts.tb : gp.V;
    int4 rec = make_int4(0, 0, 0, 0);
    if (TS) rec = ts_row_record(gp, ts, tap, tap ? 0 : row, tap ? row : 0, cur_len);
    extern __shared__ unsigned rp_sh[];
    const bool rp = TS && ts.rp != 0;
    if (rp) rp_build(ts, rp_row_prefix(ts, 0, row, row, cur_len), n0, n1, -1, gp.V, rp_sh, tid, 256);
    auto pl = [&](int n) {
        float v = x[n];
        if (rp) v = rp_pen(v, n, n0, ts, rp_sh);
        v = proc_logit(v, n, cur_len, gp, mask, exppen);
        if (TS) v = ts_mask(v, n, rec, gp, ts);
        if (rp && rp_banned(n, n0, gp.V, rp_sh)) v = -INFINITY;
        return v;
    };
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

int wm_sample_launch(wm_ctx* ctx, const GenDev& gp, const TsDev& ts, const SampDev& sd, const int* pos, int nrows, int out_row0, int tap)
{
    hipStream_t st = ctx->stream;
    if (wm_rules_on(ts))
        k_sample1<true><<<dim3(SEL_SP, nrows), dim3(256), rp_lds_bytes(ts, gp.V), st>>>(ctx->logits, gp, ctx->supmask, ctx->exppen, pos, ts, sd, tap);
    else
        k_sample1<false><<<dim3(SEL_SP, nrows), dim3(256), 0, st>>>(ctx->logits, gp, ctx->supmask, ctx->exppen, pos, ts, sd, tap);
    WM_HIP(hipGetLastError());
    k_sample_fin<<<dim3((nrows + 63) / 64), dim3(64), 0, st>>>(sd, nrows, out_row0, ctx->amax, wm_rules_on(ts) ? ts.forced : nullptr);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
