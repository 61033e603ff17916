// wm_seq_bias.hip — sequence bias on the plain decode path (include/wm.h wm_set_sequence_bias / wm_seq_bias_rows): what HF's
// SequenceBiasLogitsProcessor (and NoBadWordsLogitsProcessor, its -inf case) does to a row — scores + bias, the bias vector built in fp32 from the
// entries whose leading ids end the row's prefix — as an in-place edit of the fp32 logits row before any select kernel reads it.
//   k_seq_bias: grid (ceil(groups / 256), rows) x 256.  The block stages the last min(len, WM_SEQ_BIAS_MAX_LEN - 1) ids of its row's prefix in LDS;
//               one thread owns one GROUP (the entries that end in one target token: the one-token entry first, then the caller's order), walks
//               its entries in that order against LDS and does the single read-modify-write of x[target].  No atomics, no vocabulary sweep.
#include <cmath>
#include <cstring>
#include <map>
#include "wm_internal.h"

__global__ void __launch_bounds__(256)
k_seq_bias(float* __restrict__ logits, int Vpad, const int* __restrict__ ids, int ids_stride, const int* __restrict__ lens, int len_cap, SeqBiasDev sb)
{
    __shared__ int tail[WM_SEQ_BIAS_MAX_LEN];
    const int row = blockIdx.y, tid = threadIdx.x;
    const int len = min(max(lens[row], 0), len_cap);
    const int nt = min(len, WM_SEQ_BIAS_MAX_LEN - 1);         // the ids an entry's m - 1 <= 15 leading ids can be compared with
    if (tid < nt) tail[tid] = ids[(size_t)row * ids_stride + (len - nt) + tid];
    __syncthreads();
    const int g = blockIdx.x * 256 + tid;
    if (g >= sb.ngroups) return;
    float s = 0.0f;
    const int e1 = sb.gstart[g + 1];
    for (int e = sb.gstart[g]; e < e1; ++e) {
        const int m = sb.elen[e];
        const float b = sb.ebias[e];
        if (m == 1) { s = s + b; continue; }                  // (first of its group: 0 + b, HF's `bias += length_1_bias`)
        if (m > len) continue;                                // HF: an entry longer than the context is skipped (m - 1 <= len - 1 <= nt below)
        const int* et = sb.etok + (size_t)e * WM_SEQ_BIAS_MAX_LEN;
        bool match = true;
        for (int j = 0; j < m - 1; ++j) match = match && tail[nt - (m - 1) + j] == et[j];
        s = s + (match ? b : 0.0f);                           // HF: bias[:, last] += where(matching_rows, b, 0.0)
    }
    float* x = logits + (size_t)row * Vpad + sb.gtok[g];
    *x = *x + s;
}

// the grouped form of a table (host) and its device copy.  The device buffers are allocated once, at the maximum size
struct SeqBiasTable {
    std::vector<int> gtok, gstart, elen, etok;       // etok: [entries][WM_SEQ_BIAS_MAX_LEN]
    std::vector<float> ebias;
    int ngroups() const { return (int)gtok.size(); }
};
struct wm_seq_bias_state {
    DevBuf<int> gtok, gstart, elen, etok;
    DevBuf<float> ebias;
    bool set = false;
    SeqBiasTable table;                              // what wm_set_sequence_bias was given (set == true)
};

// checks of wm_set_sequence_bias, then the groups: one per target token in the order of their first appearance, the one-token entry first, then
// the caller's order
static int seq_bias_lower(wm_ctx* ctx, const char* who, const wm_seq_bias_params* sb, SeqBiasTable* out)
{
    const std::string w = std::string(who) + ": ";
    if (!sb->tokens || !sb->lens || !sb->bias) { ctx->err = w + "null tokens / lens / bias"; return WM_ERR_ARG; }
    if (sb->n < 1 || sb->n > WM_SEQ_BIAS_MAX) { ctx->err = w + "n must be in [1, " + std::to_string(WM_SEQ_BIAS_MAX) + "] entries"; return WM_ERR_ARG; }
    std::map<std::vector<int>, int> seen;
    std::map<int, int> group_of;                     // target token -> group
    std::vector<std::vector<int>> members;           // group -> entry indices (caller order)
    std::vector<int> first(sb->n);
    size_t off = 0;
    for (int i = 0; i < sb->n; ++i) {
        const int m = sb->lens[i];
        if (m < 1 || m > WM_SEQ_BIAS_MAX_LEN) {
            ctx->err = w + "entry " + std::to_string(i) + ": length must be in [1, " + std::to_string(WM_SEQ_BIAS_MAX_LEN) + "] tokens"; return WM_ERR_ARG; }
        first[i] = (int)off;
        std::vector<int> seq(sb->tokens + off, sb->tokens + off + m);
        off += m;
        for (int t : seq)
            if (t < 0 || t >= ctx->V) { ctx->err = w + "entry " + std::to_string(i) + ": token id " + std::to_string(t) + " outside the vocabulary"; return WM_ERR_ARG; }
        const float b = sb->bias[i];
        if (std::isnan(b) || (std::isinf(b) && b > 0.f)) { ctx->err = w + "entry " + std::to_string(i) + ": bias must be finite or -inf (NaN / +inf given)"; return WM_ERR_ARG; }
        if (!seen.emplace(seq, i).second) { ctx->err = w + "entries " + std::to_string(seen[seq]) + " and " + std::to_string(i) + " are identical (duplicate entry)"; return WM_ERR_ARG; }
        auto it = group_of.find(seq.back());
        if (it == group_of.end()) { it = group_of.emplace(seq.back(), (int)members.size()).first; members.emplace_back(); }
        std::vector<int>& mem = members[it->second];
        if (m == 1) mem.insert(mem.begin(), i); else mem.push_back(i);
    }
    SeqBiasTable t;
    t.gstart.push_back(0);
    for (const auto& mem : members) {
        for (int i : mem) {
            const int m = sb->lens[i];
            t.elen.push_back(m); t.ebias.push_back(sb->bias[i]);
            const size_t at = t.etok.size();
            t.etok.resize(at + WM_SEQ_BIAS_MAX_LEN, 0);
            std::memcpy(t.etok.data() + at, sb->tokens + first[i], (size_t)(m - 1) * sizeof(int));
        }
        t.gtok.push_back(sb->tokens[first[mem.back()] + sb->lens[mem.back()] - 1]);
        t.gstart.push_back((int)t.elen.size());
    }
    *out = std::move(t);
    return WM_OK;
}

static int seq_bias_state(wm_ctx* ctx, wm_seq_bias_state** out)
{
    if (!ctx->seq_bias_state) ctx->seq_bias_state = new wm_seq_bias_state();
    wm_seq_bias_state& S = *ctx->seq_bias_state;
    const size_t N = WM_SEQ_BIAS_MAX;
    WM_HIP(S.gtok.reserve(N)); WM_HIP(S.gstart.reserve(N + 1)); WM_HIP(S.elen.reserve(N)); WM_HIP(S.ebias.reserve(N));
    WM_HIP(S.etok.reserve(N * WM_SEQ_BIAS_MAX_LEN));
    *out = &S;
    return WM_OK;
}

// a table into the device buffers; returns with the stream idle (nothing in flight reads the buffers while they change, the host vectors may go)
static int seq_bias_upload(wm_ctx* ctx, wm_seq_bias_state& S, const SeqBiasTable& t)
{
    hipStream_t st = ctx->stream;
    WM_HIP(hipStreamSynchronize(st));
    WM_HIP(hipMemcpyAsync(S.gtok, t.gtok.data(), t.gtok.size() * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.gstart, t.gstart.data(), t.gstart.size() * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.elen, t.elen.data(), t.elen.size() * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.ebias, t.ebias.data(), t.ebias.size() * sizeof(float), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.etok, t.etok.data(), t.etok.size() * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipStreamSynchronize(st));
    return WM_OK;
}

static SeqBiasDev seq_bias_dev(const wm_seq_bias_state& S, int ngroups)
{
    SeqBiasDev d{};
    d.on = 1; d.ngroups = ngroups; d.gtok = S.gtok; d.gstart = S.gstart; d.elen = S.elen; d.ebias = S.ebias; d.etok = S.etok;
    return d;
}

void wm_seq_bias_free(wm_ctx* ctx) { delete ctx->seq_bias_state; ctx->seq_bias_state = nullptr; }

int wm_seq_bias_launch(wm_ctx* ctx, const SeqBiasDev& sb, const int* ids, int ids_stride, const int* lens, int len_cap, int nrows)
{
    if (!sb.on || sb.ngroups < 1 || nrows < 1) return WM_OK;
    k_seq_bias<<<dim3((sb.ngroups + 255) / 256, nrows), dim3(256), 0, ctx->stream>>>(ctx->logits, ctx->Vpad, ids, ids_stride, lens, len_cap, sb);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_seq_bias_begin(wm_ctx* ctx, const char* who, const wm_gen_params* gp, SeqBiasDev* out)
{
    SeqBiasDev d{};
    *out = d;
    if (!ctx->seq_bias_state || !ctx->seq_bias_state->set) return WM_OK;
    const std::string w = std::string(who) + ": ";
    if (!gp->vanilla) { ctx->err = w + "the sequence bias runs on the plain decode path only (wm_gen_params.vanilla = 1)"; return WM_ERR_ARG; }
    if (ctx->tn) { ctx->err = w + "the sequence bias is not supported with a candidate tree (medusa_choices with top-k > 1)"; return WM_ERR_ARG; }
    const wm_seq_bias_state& S = *ctx->seq_bias_state;
    const SeqBiasTable& t = S.table;
    for (int g = 0; g < t.ngroups(); ++g) {
        if (t.gtok[g] != gp->eos_token_id) continue;
        for (int e = t.gstart[g]; e < t.gstart[g + 1]; ++e)
            if (std::isinf(t.ebias[e]) && (t.elen[e] > 1 || gp->exp_decay_start >= 0)) {
                ctx->err = w + "a -inf sequence bias entry " + (t.elen[e] > 1 ? "of more than one token " : "") + "ends in eos" +
                           (t.elen[e] > 1 ? "" : " while the exponential decay is on") + ": the decay's x + |x| p would give NaN";
                return WM_ERR_ARG;
            }
    }
    *out = seq_bias_dev(S, t.ngroups());
    return WM_OK;
}

// HF generate(sequence_bias=..., bad_words_ids=...): kept on the context, read by wm_decode_begin*
extern "C" int wm_set_sequence_bias(wm_ctx* ctx, const wm_seq_bias_params* sb)
{
    if (!ctx) return WM_ERR_ARG;
    if (!sb) { if (ctx->seq_bias_state) ctx->seq_bias_state->set = false; return WM_OK; }
    SeqBiasTable t;
    if (int rc = seq_bias_lower(ctx, "wm_set_sequence_bias", sb, &t)) return rc;
    WM_HIP(hipSetDevice(ctx->device));
    wm_seq_bias_state* S = nullptr;
    if (int rc = seq_bias_state(ctx, &S)) return rc;
    if (int rc = seq_bias_upload(ctx, *S, t)) return rc;
    S->table = std::move(t); S->set = true;
    return WM_OK;
}

// Sequence-bias parity tap: caller-given rows through k_seq_bias alone (include/wm.h)
extern "C" int wm_seq_bias_rows(wm_ctx* ctx, const wm_seq_bias_params* sb, int R, const float* logits, const int32_t* prefixes, int Tmax,
                                const int32_t* lens, float* out)
{
    if (!ctx) return WM_ERR_ARG;
    if (!sb || R < 1 || !logits || !prefixes || Tmax < 1 || !lens || !out) { ctx->err = "wm_seq_bias_rows: bad arguments"; return WM_ERR_ARG; }
    if (int rc = wm_tap_check_lens(ctx, "wm_seq_bias_rows", lens, R, Tmax, false)) return rc;
    SeqBiasTable t;
    if (int rc = seq_bias_lower(ctx, "wm_seq_bias_rows", sb, &t)) return rc;
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    wm_seq_bias_state* S = nullptr;
    if (int rc = seq_bias_state(ctx, &S)) return rc;
    wm_decode_invalidate(ctx);
    wm_tap_stage s{ctx, "wm_seq_bias_rows", Tmax, WM_TAP_ROWS};
    if (int rc = s.reserve()) return rc;
    if (int rc = seq_bias_upload(ctx, *S, t)) return rc;
    const SeqBiasDev d = seq_bias_dev(*S, t.ngroups());
    const int rc = wm_tap_groups(s, R, logits, prefixes, lens, [&](int r0, int n) {
        if (int rc = wm_seq_bias_launch(ctx, d, s.pre, Tmax, s.len, Tmax, n)) return rc;
        WM_TAP_HIP(s, hipMemcpy2DAsync(out + (size_t)r0 * ctx->V, (size_t)ctx->V * sizeof(float), ctx->logits, (size_t)ctx->Vpad * sizeof(float),
                                       (size_t)ctx->V * sizeof(float), n, hipMemcpyDeviceToHost, st));
        return WM_OK;
    });
    // quirk, kept: the tap borrowed the device tables, so the context's own sticky table goes back in place — on the error path too
    if (S->set) { if (int rc2 = seq_bias_upload(ctx, *S, S->table)) return rc ? rc : rc2; }
    return rc;
}
