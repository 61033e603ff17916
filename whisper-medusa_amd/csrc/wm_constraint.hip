// wm_constraint.hip — constrained decoding on the plain decode path (include/wm.h wm_set_constraint / wm_constraint_rows): what HF's
// PrefixConstrainedLogitsProcessor does to a row when its callback walks a fixed list of token sequences — scores + mask, the mask 0 on the allowed
// ids and -inf elsewhere — as an in-place edit of the fp32 logits row before any select kernel reads it.
//   The host sorts the sequences (each closed by CONS_CLOSE, padded with CONS_PAD to W = WM_CONSTRAINT_MAX_LEN + 1 ids) and uploads them twice:
//   row-major [n][W] for comparing, column-major [W][n] for reading one column.  The sequences that start with g = ids[P:len] are a contiguous range.
//   k_constraint: grid (CONS_SLICES, rows) x 256.  Lane j of every wave holds g[j]; two binary searches, side by side, find the range: a step loads
//               one table row per search (lane j its id j: one coalesced load), a ballot of the mismatches and its first set bit give the order —
//               ceil(log2(n + 1)) dependent rounds whatever t = len - P is.  The block clears the bitmap of ITS slice of the vocabulary in LDS, reads
//               column t over the range (coalesced) and ors the bits of the ids that fall in the slice (CONS_CLOSE stands for eos); an empty range
//               sets eos alone.  Then the slice is swept: -inf wherever the bit is clear, nothing read back, allowed elements untouched.
#include <cmath>
#include <cstring>
#include <numeric>
#include "wm_internal.h"

constexpr int CONS_W = WM_CONSTRAINT_MAX_LEN + 1;
constexpr int CONS_PAD = -1, CONS_CLOSE = -2;      // behind a sequence's end / its closing eos (eos itself is a decode's: the table does not depend on it)
constexpr int CONS_SLICES = 8;                     // vocabulary slices (blocks) per row

// words of a slice's bitmap: the vocabulary's ceil(V / 32) words dealt out evenly
__host__ __device__ static inline int cons_slice_words(int V) { return ((V + 31) / 32 + CONS_SLICES - 1) / CONS_SLICES; }

// order of table row `r` against the prefix g (lane j < t holds g[j]): -1 the row's first t ids are less, 0 they equal g, +1 greater
__device__ __forceinline__ int cons_cmp(const int* __restrict__ rowmaj, int r, int lane, int t, int gj)
{
    const bool act = lane < t;
    const int v = act ? rowmaj[(size_t)r * CONS_W + lane] : 0;
    const unsigned long long ne = __ballot(act && v != gj), lt = __ballot(act && v < gj);
    if (ne == 0ull) return 0;
    const int f = __ffsll((long long)ne) - 1;
    return ((lt >> f) & 1ull) ? -1 : 1;
}

__global__ void __launch_bounds__(256)
k_constraint(float* __restrict__ logits, int V, int Vpad, const int* __restrict__ ids, int ids_stride, const int* __restrict__ lens, int len_cap,
             int P, int eos, ConstraintDev cd, int* __restrict__ n_allowed /* [rows][CONS_SLICES] or NULL */)
{
    extern __shared__ unsigned bits[];             // cons_slice_words(V) words, then one counter
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int words = cons_slice_words(V);
    const int v0 = blockIdx.x * words * 32, v1 = min(v0 + words * 32, V);       // this block's ids [v0, v1)
    for (int w = tid; w <= words; w += 256) bits[w] = 0u;
    const int len = min(max(lens[row], 0), len_cap);
    const int t = max(len - P, 0);
    // the range [lo, hi) of the sequences that start with g; every wave searches (the same loads, no hand-over through LDS)
    int lo = 0, hi = 0;
    if (t < CONS_W) {
        const int gj = lane < t ? ids[(size_t)row * ids_stride + P + lane] : 0;
        int a0 = 0, a1 = cd.n, b0 = 0, b1 = cd.n;  // lower bound: first row >= g; upper bound: first row > g
        while (a0 < a1 || b0 < b1) {
            const int ma = a0 + ((a1 - a0) >> 1), mb = b0 + ((b1 - b0) >> 1);
            const int ca = a0 < a1 ? cons_cmp(cd.rowmaj, ma, lane, t, gj) : 0;
            const int cb = b0 < b1 ? cons_cmp(cd.rowmaj, mb, lane, t, gj) : 0;
            if (a0 < a1) { if (ca < 0) a0 = ma + 1; else a1 = ma; }
            if (b0 < b1) { if (cb <= 0) b0 = mb + 1; else b1 = mb; }
        }
        lo = a0; hi = b0;
    }
    __syncthreads();
    const int* col = cd.colmaj + (size_t)min(t, CONS_W - 1) * cd.n;
    for (int i = lo + tid; i < hi; i += 256) {
        int v = col[i];
        if (v == CONS_CLOSE) v = eos;
        if (v >= v0 && v < v1) atomicOr(&bits[(v - v0) >> 5], 1u << ((v - v0) & 31));
    }
    if (lo >= hi && tid == 0 && eos >= v0 && eos < v1) bits[(eos - v0) >> 5] = 1u << ((eos - v0) & 31);
    __syncthreads();
    float* x = logits + (size_t)row * Vpad;
    const float ninf = -INFINITY;
    for (int v = v0 + tid * 4; v < v1; v += 256 * 4) {         // four ids per thread and round: one 16-byte store where none of them is allowed
        const unsigned nib = (bits[(v - v0) >> 5] >> ((v - v0) & 31)) & 15u;
        if (nib == 0u && v + 3 < v1) { *reinterpret_cast<float4*>(x + v) = make_float4(ninf, ninf, ninf, ninf); continue; }
        for (int k = 0; k < 4 && v + k < v1; ++k) if (!((nib >> k) & 1u)) x[v + k] = ninf;
    }
    if (n_allowed) {
        int c = 0;
        for (int w = tid; w < words; w += 256) c += __popc(bits[w]);
        if (c) atomicAdd(&bits[words], (unsigned)c);
        __syncthreads();
        if (tid == 0) n_allowed[row * CONS_SLICES + blockIdx.x] = (int)bits[words];
    }
}

// the sorted form of a table (host) and its device copy.  The device buffers are allocated once, at the maximum size
struct ConstraintTable {
    int n = 0;
    std::vector<int> rowmaj, colmaj;                 // [n][CONS_W] / [CONS_W][n]
    std::vector<int> used, first;                    // the distinct ids of the sequences / of their first places, ascending
};
struct wm_constraint_state {
    DevBuf<int> rowmaj, colmaj, cnt;                 // cnt: [WM_TAP_ROWS][CONS_SLICES] (the tap's n_allowed partials)
    bool set = false;
    ConstraintTable table;                           // what wm_set_constraint was given (set == true)
};

// checks of wm_set_constraint, then the sorted table
static int constraint_lower(wm_ctx* ctx, const char* who, const wm_constraint_params* c, ConstraintTable* out)
{
    const std::string w = std::string(who) + ": ";
    if (!c->tokens || !c->lens) { ctx->err = w + "null tokens / lens"; return WM_ERR_ARG; }
    if (c->n < 1 || c->n > WM_CONSTRAINT_MAX) { ctx->err = w + "n must be in [1, " + std::to_string(WM_CONSTRAINT_MAX) + "] sequences"; return WM_ERR_ARG; }
    const int n = c->n;
    std::vector<int> rows((size_t)n * CONS_W, CONS_PAD);
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        const int m = c->lens[i];
        if (m < 1 || m > WM_CONSTRAINT_MAX_LEN) {
            ctx->err = w + "sequence " + std::to_string(i) + ": length must be in [1, " + std::to_string(WM_CONSTRAINT_MAX_LEN) + "] tokens"; return WM_ERR_ARG; }
        for (int j = 0; j < m; ++j) {
            const int t = c->tokens[off + j];
            if (t < 0 || t >= ctx->V) { ctx->err = w + "sequence " + std::to_string(i) + ": token id " + std::to_string(t) + " outside the vocabulary"; return WM_ERR_ARG; }
            rows[(size_t)i * CONS_W + j] = t;
        }
        rows[(size_t)i * CONS_W + m] = CONS_CLOSE;
        off += m;
    }
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        return std::lexicographical_compare(&rows[(size_t)a * CONS_W], &rows[(size_t)a * CONS_W] + CONS_W, &rows[(size_t)b * CONS_W], &rows[(size_t)b * CONS_W] + CONS_W); });
    for (int i = 1; i < n; ++i)
        if (std::equal(&rows[(size_t)order[i - 1] * CONS_W], &rows[(size_t)order[i - 1] * CONS_W] + CONS_W, &rows[(size_t)order[i] * CONS_W])) {
            const int a = std::min(order[i - 1], order[i]), b = std::max(order[i - 1], order[i]);
            ctx->err = w + "sequences " + std::to_string(a) + " and " + std::to_string(b) + " are identical (duplicate sequence)"; return WM_ERR_ARG;
        }
    ConstraintTable t;
    t.n = n; t.rowmaj.resize((size_t)n * CONS_W); t.colmaj.resize((size_t)n * CONS_W);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < CONS_W; ++j) {
            const int v = rows[(size_t)order[i] * CONS_W + j];
            t.rowmaj[(size_t)i * CONS_W + j] = v; t.colmaj[(size_t)j * n + i] = v;
            if (v >= 0) { t.used.push_back(v); if (j == 0) t.first.push_back(v); }
        }
    for (std::vector<int>* u : {&t.used, &t.first}) { std::sort(u->begin(), u->end()); u->erase(std::unique(u->begin(), u->end()), u->end()); }
    *out = std::move(t);
    return WM_OK;
}

static int constraint_state(wm_ctx* ctx, wm_constraint_state** out)
{
    if (!ctx->cons_state) ctx->cons_state = new wm_constraint_state();
    wm_constraint_state& S = *ctx->cons_state;
    const size_t N = (size_t)WM_CONSTRAINT_MAX * CONS_W;
    WM_HIP(S.rowmaj.reserve(N)); WM_HIP(S.colmaj.reserve(N)); WM_HIP(S.cnt.reserve((size_t)WM_TAP_ROWS * CONS_SLICES));
    *out = &S;
    return WM_OK;
}

// a table into the device buffers; returns with the stream idle (nothing in flight reads the buffers while they change, the host vectors may go)
static int constraint_upload(wm_ctx* ctx, wm_constraint_state& S, const ConstraintTable& t)
{
    hipStream_t st = ctx->stream;
    WM_HIP(hipStreamSynchronize(st));
    WM_HIP(hipMemcpyAsync(S.rowmaj, t.rowmaj.data(), t.rowmaj.size() * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.colmaj, t.colmaj.data(), t.colmaj.size() * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipStreamSynchronize(st));
    return WM_OK;
}

static ConstraintDev constraint_dev(const wm_constraint_state& S, int n)
{
    ConstraintDev d{};
    d.on = 1; d.n = n; d.rowmaj = S.rowmaj; d.colmaj = S.colmaj;
    return d;
}

// eos must not stand inside a sequence (it closes every one)
static int constraint_check_eos(wm_ctx* ctx, const std::string& w, const ConstraintTable& t, int eos)
{
    if (!std::binary_search(t.used.begin(), t.used.end(), eos)) return WM_OK;
    ctx->err = w + "eos (" + std::to_string(eos) + ") stands inside an allowed sequence: every sequence is closed by eos implicitly";
    return WM_ERR_ARG;
}

void wm_constraint_free(wm_ctx* ctx) { delete ctx->cons_state; ctx->cons_state = nullptr; }

static int constraint_launch_cnt(wm_ctx* ctx, const ConstraintDev& cd, const int* ids, int ids_stride, const int* lens, int len_cap, int P, int eos,
                                 int nrows, int* cnt)
{
    if (!cd.on || cd.n < 1 || nrows < 1) return WM_OK;
    const size_t lds = ((size_t)cons_slice_words(ctx->V) + 1) * sizeof(unsigned);
    k_constraint<<<dim3(CONS_SLICES, nrows), dim3(256), lds, ctx->stream>>>(ctx->logits, ctx->V, ctx->Vpad, ids, ids_stride, lens, len_cap, P, eos, cd, cnt);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
int wm_constraint_launch(wm_ctx* ctx, const ConstraintDev& cd, const GenDev& gp, const int* ids, int ids_stride, const int* lens, int len_cap, int nrows)
{
    return constraint_launch_cnt(ctx, cd, ids, ids_stride, lens, len_cap, gp.P, gp.eos, nrows, nullptr);
}

int wm_constraint_begin(wm_ctx* ctx, const char* who, const wm_gen_params* gp, const wm_timestamp_params* tsp, ConstraintDev* out)
{
    ConstraintDev d{};
    *out = d;
    if (!ctx->cons_state || !ctx->cons_state->set) return WM_OK;
    const std::string w = std::string(who) + ": ";
    if (!gp->vanilla) { ctx->err = w + "the constraint runs on the plain decode path only (wm_gen_params.vanilla = 1)"; return WM_ERR_ARG; }
    if (ctx->tn) { ctx->err = w + "the constraint is not supported with a candidate tree (medusa_choices with top-k > 1)"; return WM_ERR_ARG; }
    if (tsp) { ctx->err = w + "the constraint is not supported with the timestamp rules: a timestamp is never in the allowed set, the rules would force a row of -inf"; return WM_ERR_ARG; }
    if (gp->exp_decay_start >= 0) { ctx->err = w + "the constraint is not supported with the exponential decay: its x + |x| p turns a masked eos into NaN"; return WM_ERR_ARG; }
    const wm_constraint_state& S = *ctx->cons_state;
    const ConstraintTable& t = S.table;
    if (int rc = constraint_check_eos(ctx, w + "constraint: ", t, gp->eos_token_id)) return rc;
    for (int i = 0; i < gp->n_suppress; ++i)
        if (std::binary_search(t.used.begin(), t.used.end(), gp->suppress[i])) {
            ctx->err = w + "constraint: token id " + std::to_string(gp->suppress[i]) + " of an allowed sequence is in the suppress list"; return WM_ERR_ARG; }
    for (int i = 0; i < gp->n_begin_suppress; ++i)
        if (std::binary_search(t.first.begin(), t.first.end(), gp->begin_suppress[i])) {
            ctx->err = w + "constraint: token id " + std::to_string(gp->begin_suppress[i]) + ", the first of an allowed sequence, is in the begin-suppress list"; return WM_ERR_ARG; }
    *out = constraint_dev(S, t.n);
    return WM_OK;
}

// HF generate(prefix_allowed_tokens_fn=) over a fixed list of sequences: kept on the context, read by wm_decode_begin*
extern "C" int wm_set_constraint(wm_ctx* ctx, const wm_constraint_params* c)
{
    if (!ctx) return WM_ERR_ARG;
    if (!c) { if (ctx->cons_state) ctx->cons_state->set = false; return WM_OK; }
    ConstraintTable t;
    if (int rc = constraint_lower(ctx, "wm_set_constraint", c, &t)) return rc;
    WM_HIP(hipSetDevice(ctx->device));
    wm_constraint_state* S = nullptr;
    if (int rc = constraint_state(ctx, &S)) return rc;
    if (int rc = constraint_upload(ctx, *S, t)) return rc;
    S->table = std::move(t); S->set = true;
    return WM_OK;
}

// Constraint parity tap: caller-given rows through k_constraint alone (include/wm.h)
extern "C" int wm_constraint_rows(wm_ctx* ctx, const wm_constraint_params* c, int eos, int prompt_len, int R, const float* logits,
                                  const int32_t* prefixes, int Tmax, const int32_t* lens, float* out, int32_t* n_allowed)
{
    if (!ctx) return WM_ERR_ARG;
    if (!c || R < 1 || !logits || !prefixes || Tmax < 1 || !lens || !out) { ctx->err = "wm_constraint_rows: bad arguments"; return WM_ERR_ARG; }
    if (eos < 0 || eos >= ctx->V) { ctx->err = "wm_constraint_rows: eos out of range"; return WM_ERR_ARG; }
    bool ok = prompt_len >= 0;
    for (int r = 0; r < R; ++r) ok = ok && lens[r] >= prompt_len;
    if (int rc = wm_tap_check_lens(ctx, "wm_constraint_rows", lens, R, Tmax, false, ok, " and >= prompt_len >= 0")) return rc;
    ConstraintTable t;
    if (int rc = constraint_lower(ctx, "wm_constraint_rows", c, &t)) return rc;
    if (int rc = constraint_check_eos(ctx, "wm_constraint_rows: ", t, eos)) return rc;
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    wm_constraint_state* S = nullptr;
    if (int rc = constraint_state(ctx, &S)) return rc;
    wm_decode_invalidate(ctx);
    wm_tap_stage s{ctx, "wm_constraint_rows", Tmax, WM_TAP_ROWS};
    if (int rc = s.reserve()) return rc;
    if (int rc = constraint_upload(ctx, *S, t)) return rc;
    const ConstraintDev d = constraint_dev(*S, t.n);
    std::vector<int> cnt((size_t)WM_TAP_ROWS * CONS_SLICES);
    const int rc = wm_tap_groups(s, R, logits, prefixes, lens, [&](int r0, int n) {
        if (int rc = constraint_launch_cnt(ctx, d, s.pre, Tmax, s.len, Tmax, prompt_len, eos, n, n_allowed ? (int*)S->cnt : nullptr)) return rc;
        WM_TAP_HIP(s, hipMemcpy2DAsync(out + (size_t)r0 * ctx->V, (size_t)ctx->V * sizeof(float), ctx->logits, (size_t)ctx->Vpad * sizeof(float),
                                       (size_t)ctx->V * sizeof(float), n, hipMemcpyDeviceToHost, st));
        if (n_allowed) {
            WM_TAP_HIP(s, hipMemcpyAsync(cnt.data(), S->cnt, (size_t)n * CONS_SLICES * sizeof(int), hipMemcpyDeviceToHost, st));
            WM_TAP_HIP(s, hipStreamSynchronize(st));
            for (int r = 0; r < n; ++r) n_allowed[r0 + r] = std::accumulate(&cnt[(size_t)r * CONS_SLICES], &cnt[(size_t)r * CONS_SLICES] + CONS_SLICES, 0);
        }
        return WM_OK;
    });
    // the tap borrowed the device tables, so the context's own sticky table goes back in place — on the error path too
    if (S->set) { if (int rc2 = constraint_upload(ctx, *S, S->table)) return rc ? rc : rc2; }
    return rc;
}
