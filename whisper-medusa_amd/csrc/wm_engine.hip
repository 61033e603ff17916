// wm_engine.hip — C-ABI entry points of libwm.so (include/wm.h): context, parameter table,
// HBM allocation, decode-loop driver with hipGraph replay, parity taps.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "wm_select.h"

static thread_local std::string g_create_err;

static inline int rup(int x, int m) { return (x + m - 1) / m * m; }

template <class T>
static hipError_t dev_alloc(T** p, size_t n, hipStream_t st)
{
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    return hipMemsetAsync(*p, 0, std::max<size_t>(n, 1) * sizeof(T), st);
}

extern "C" int wm_abi_version(void) { return WM_ABI_VERSION; }
extern "C" int wm_build_act_fp16(void) { return WM_ACT_PLANES == 1 ? 1 : 0; }

extern "C" const char* wm_last_error(const wm_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

extern "C" void wm_destroy(wm_ctx* ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    ctx->graphs_plain.drop(); ctx->graphs_beam.drop();       // (before the buffers they name are freed)
    if (ctx->hostflags) hipHostFree(ctx->hostflags);
    void* bufs[] = {ctx->feats_own, ctx->clipmax, ctx->A1, ctx->a1, ctx->A2, ctx->eh, ctx->exn, ctx->eq, ctx->ek, ctx->evt, ctx->eff,
                    ctx->enc_out, ctx->kx, ctx->vx, ctx->kc, ctx->vc, ctx->h, ctx->hblk, ctx->hf, ctx->qbuf, ctx->xbuf, ctx->fbuf,
                    ctx->ybuf, ctx->cml, ctx->co, ctx->ticket, ctx->logits, ctx->amax, ctx->pc, ctx->part1, ctx->part2, ctx->ids, ctx->L, ctx->kvlen,
                    ctx->finished, ctx->cand, ctx->niter, ctx->hist, ctx->supmask, ctx->exppen, ctx->tap_tok, ctx->done,
                    ctx->hf_keep, ctx->hb_keep, ctx->carry, ctx->rowinfo, ctx->sinfo, ctx->steprows, ctx->rs_table, ctx->tree, ctx->sibtree, ctx->sibpart, ctx->sel_src, ctx->sel_n, ctx->sel_base, ctx->exn8, ctx->exs,
                    ctx->xn, ctx->lnstats, ctx->foldv, ctx->kx8, ctx->vx8, ctx->kxs, ctx->vxs,
                    ctx->ts.st, ctx->ts.ver, ctx->ts.part1t, ctx->ts.forced, ctx->samp.part, ctx->samp.val, ctx->samp_keys, ctx->samp.fv, ctx->samp.thr, ctx->samp.kept, ctx->lang_ids, ctx->lang_out};
    for (void* b : bufs) if (b) hipFree(b);
    wm_align_free(ctx);
    wm_score_free(ctx);
    wm_beam_free(ctx);
    wm_seq_bias_free(ctx);
    wm_constraint_free(ctx);
    wm_merge_free(ctx);
    wm_words_free(ctx);
    wm_vad_free(ctx);
    wm_stream_free(ctx);
    if (ctx->ev0) hipEventDestroy(ctx->ev0);
    if (ctx->ev1) hipEventDestroy(ctx->ev1);
    if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int wm_create(const wm_config* cfg, const wm_weights* w, int device, void* hip_stream, wm_ctx** out)
{
    g_create_err.clear();
    if (!cfg || !w || !out) { g_create_err = "wm_create: null argument"; return WM_ERR_ARG; }
    if (cfg->abi_version != WM_ABI_VERSION) { g_create_err = "wm_create: ABI version mismatch"; return WM_ERR_ARG; }
    if ((cfg->act_fp16 != 0) != (WM_ACT_PLANES == 1)) {
        g_create_err = std::string("wm_create: this library is built for the ") + (WM_ACT_PLANES == 1 ? "fp16 single-plane" : "bf16 hi / lo") +
                       " decode contract (wm_build_act_fp16), wm_config.act_fp16 asks for the other"; return WM_ERR_ARG; }
    if (cfg->d_model <= 0 || cfg->d_model % 128 || cfg->n_heads * WM_HEAD_DIM != cfg->d_model || cfg->d_model > 2048) {
        g_create_err = "wm_create: d_model must be a multiple of 128 (<= 2048) with 64-wide heads"; return WM_ERR_ARG; }
    if (cfg->ffn_dim % 128 || cfg->medusa_heads < 1 || cfg->medusa_heads > 15 || cfg->max_batch < 1 || cfg->n_mels * 3 > 256 ||
        (cfg->heads_type != WM_HEADS_LINEAR && cfg->heads_type != WM_HEADS_BLOCK) || cfg->n_tgt < 8 || cfg->n_ctx < 8) {
        g_create_err = "wm_create: unsupported configuration"; return WM_ERR_ARG; }
    // candidate tree (medusa_choices): zero / all-one entries = the chain
    TreeDev tree{};
    int tn = 0, tp = 0;
    {
        const int K = cfg->medusa_heads;
        bool chain = true, zero = true;
        for (int i = 0; i < 16; ++i) { zero = zero && cfg->medusa_choices[i] == 0; }
        for (int i = 0; i <= K; ++i) chain = chain && cfg->medusa_choices[i] == 1;
        if (!zero && !chain) {
            const int32_t* c = cfg->medusa_choices;
            bool ok = c[0] == 1;
            for (int i = 0; i <= K; ++i) ok = ok && c[i] >= 1 && c[i] <= 4;
            for (int i = K + 1; i < 16; ++i) ok = ok && c[i] == 0;
            long nodes = 0, prod = 1;
            for (int i = 0; ok && i <= K; ++i) { prod *= c[i]; nodes += prod; if (prod > WM_TREE_MAX_PATHS || nodes > WM_TREE_MAX_NODES) ok = false; }
            if (!ok) { g_create_err = "wm_create: medusa_choices must be [1, c_1..c_K] with c_k in 1..4, <= 64 tree nodes and <= 32 paths"; return WM_ERR_ARG; }
            // generate_medusa_buffers (medusa_utils.py:305-421): node (depth i, index j) has parent (i-1, j / c_i) and takes
            // the (j % c_i)-th of head i's top-c_i tokens; path p visits node (i, p / (n_paths / cumprod_i)) at depth i
            tree.K = K; tree.n_paths = (int)prod; tree.n_nodes = (int)nodes;
            int cp = 1;
            tree.start[0] = 0;
            for (int i = 0; i <= K; ++i) { cp *= c[i]; tree.cumprod[i] = cp; tree.topk[i] = c[i]; tree.start[i + 1] = tree.start[i] + cp; }
            for (int n = 0; n < WM_TREE_MAX_NODES; ++n) { tree.parent[n] = -1; for (int j = 0; j < 4; ++j) tree.children[n][j] = -1; }
            for (int i = 0; i <= K; ++i)
                for (int j = 0; j < tree.cumprod[i]; ++j) {
                    const int n = tree.start[i] + j;
                    tree.depth[n] = i;
                    if (i > 0) {
                        const int par = tree.start[i - 1] + j / c[i];
                        tree.parent[n] = par;
                        tree.children[par][j % c[i]] = n;
                    }
                    tree.anc[n] = (1ull << n) | (i > 0 ? tree.anc[tree.parent[n]] : 0ull);
                }
            for (int p = 0; p < tree.n_paths; ++p)
                for (int i = 0; i <= K; ++i) tree.retrieve[p][i] = tree.start[i] + p / (tree.n_paths / tree.cumprod[i]);
            tn = tree.n_nodes; tp = tree.n_paths;
        }
    }
    wm_ctx* ctx = new wm_ctx();
    ctx->cfg = *cfg; ctx->device = device;
    ctx->tn = tn; ctx->tp = tp; ctx->tree_host = tree;
#define CREATE_HIP(expr)                                                                       \
    do { hipError_t _e = (expr); if (_e != hipSuccess) {                                       \
        g_create_err = std::string(#expr) + ": " + hipGetErrorString(_e); wm_destroy(ctx); return WM_ERR_HIP; } } while (0)
    CREATE_HIP(hipSetDevice(device));
    if (hip_stream) ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    else { CREATE_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)); ctx->own_stream = true; }
    ctx->lp.st = ctx->stream;
    CREATE_HIP(hipEventCreate(&ctx->ev0));
    CREATE_HIP(hipEventCreate(&ctx->ev1));
    { const char* v = std::getenv("WM_PREFETCH"); ctx->prefetch = !(v && std::atoi(v) == 0); }

    const int d = ctx->d = cfg->d_model;
    ctx->H = cfg->n_heads; ctx->ffn = cfg->ffn_dim; ctx->V = cfg->vocab; ctx->Vpad = rup(cfg->vocab, 128);
    ctx->S = cfg->n_ctx; ctx->Spad = rup(cfg->n_ctx, 128); ctx->Tm = 2 * cfg->n_ctx; ctx->Tmpad = rup(ctx->Tm, 128);
    ctx->Mmax = std::max(16, rup(tn, 16));      // rows per stream of a pass: the chain's K + 1 <= 16, or the tree's nodes in 16-row query tiles
    ctx->Tmax = cfg->n_tgt; ctx->Tal = rup(cfg->n_tgt + ctx->Mmax, 32); ctx->K = cfg->medusa_heads;
    ctx->block = cfg->heads_type == WM_HEADS_BLOCK;
    ctx->nkv = cfg->dec_layers + (ctx->block ? 1 : 0);
    ctx->nres = ctx->K + (ctx->block ? 0 : 1);
    ctx->maxB = cfg->max_batch;
    ctx->K1pad = rup(3 * cfg->n_mels, 128);
    ctx->NS = (ctx->Spad + 255) / 256;
    if (ctx->NS > 8 || ctx->H > 32) { g_create_err = "wm_create: n_ctx > 2048 or more than 32 heads unsupported"; wm_destroy(ctx); return WM_ERR_ARG; }

    // ---- parameter table ----
    const bool w8 = cfg->dec_weight_fp8 != 0;
    const bool e8 = cfg->enc_fp8 != 0;
    ctx->enc_f8 = e8;
    if (e8 && (cfg->d_model % 64 || cfg->ffn_dim % 128)) { g_create_err = "wm_create: enc_fp8 needs d_model % 64 == 0 and ffn_dim % 128 == 0"; wm_destroy(ctx); return WM_ERR_ARG; }
    const int n_expected = 19 + 12 * cfg->enc_layers + 18 * ctx->nkv + (w8 ? 6 * ctx->nkv : 0) + (e8 ? 4 * cfg->enc_layers + 2 : 0);
    if (w->n_offsets != n_expected || !w->blob || !w->offsets) {
        g_create_err = "wm_create: weight table has " + std::to_string(w->n_offsets) + " entries, expected " + std::to_string(n_expected);
        wm_destroy(ctx); return WM_ERR_ARG;
    }
    const char* base = reinterpret_cast<const char*>(w->blob);
    for (int i = 0; i < w->n_offsets; ++i)
        if (w->offsets[i] >= w->blob_bytes || (w->offsets[i] & 15)) { g_create_err = "wm_create: bad weight offset"; wm_destroy(ctx); return WM_ERR_ARG; }
    int t = 0;
    auto F = [&]() { return reinterpret_cast<const float*>(base + w->offsets[t++]); };
    auto Hh = [&]() { return reinterpret_cast<const bf16_t*>(base + w->offsets[t++]); };
    ctx->win = F(); ctx->twiddle = F(); ctx->melfb = F();
    ctx->conv1_w = Hh(); ctx->conv1_b = F(); ctx->conv2_w = Hh(); ctx->conv2_b = F();
    ctx->enc_pos = F(); ctx->enc_lnf_w = F(); ctx->enc_lnf_b = F();
    ctx->tok_emb = Hh(); ctx->vocab_w = Hh(); ctx->dec_pos = F(); ctx->dec_lnf_w = F(); ctx->dec_lnf_b = F();
    ctx->heads_w = Hh(); ctx->heads_b = F(); ctx->ckv_w = Hh(); ctx->ckv_b = F();
    ctx->enc.resize(cfg->enc_layers);
    for (auto& e : ctx->enc) {
        e.ln1_w = F(); e.ln1_b = F(); e.qkv_w = Hh(); e.qkv_b = F(); e.out_w = Hh(); e.out_b = F();
        e.ln2_w = F(); e.ln2_b = F(); e.fc1_w = Hh(); e.fc1_b = F(); e.fc2_w = Hh(); e.fc2_b = F();
    }
    ctx->dec.resize(ctx->nkv);
    for (auto& e : ctx->dec) {
        e.ln1_w = F(); e.ln1_b = F(); e.qkv_w = Hh(); e.qkv_b = F(); e.out_w = Hh(); e.out_b = F();
        e.ln2_w = F(); e.ln2_b = F(); e.cq_w = Hh(); e.cq_b = F(); e.cout_w = Hh(); e.cout_b = F();
        e.ln3_w = F(); e.ln3_b = F(); e.fc1_w = Hh(); e.fc1_b = F(); e.fc2_w = Hh(); e.fc2_b = F();
    }
    if (w8)                                    // fp8 e4m3 decoder-layer matrices: one fp32 scale per output row, appended to the table
        for (auto& e : ctx->dec) { e.qkv_s = F(); e.out_s = F(); e.cq_s = F(); e.cout_s = F(); e.fc1_s = F(); e.fc2_s = F(); }
    if (e8) {                                  // fp8 MFMA encoder: e4m3 matrices (128-k unit layout, K zero-padded to 128) + per-row scales, appended last
        auto U8 = [&]() { return reinterpret_cast<const unsigned char*>(base + w->offsets[t++]); };
        for (auto& e : ctx->enc) { e.qkv_w8 = U8(); e.qkv_ws = F(); e.fc1_w8 = U8(); e.fc1_ws = F(); }
        ctx->ckv_w8 = U8(); ctx->ckv_ws = F();
    }

    // ---- HBM allocation ----
    hipStream_t st = ctx->stream;
    const size_t B = ctx->maxB, Spad = ctx->Spad, H = ctx->H, Tal = ctx->Tal;
    const size_t Menc = B * Spad;
    CREATE_HIP(dev_alloc(&ctx->feats_own, B * cfg->n_mels * ctx->Tm, st));
    CREATE_HIP(dev_alloc(&ctx->clipmax, B, st));
    CREATE_HIP(dev_alloc(&ctx->A1, B * ctx->Tmpad * ctx->K1pad, st));
    CREATE_HIP(dev_alloc(&ctx->a1, B * ctx->Tm * d, st));
    CREATE_HIP(dev_alloc(&ctx->A2, Menc * 3 * d, st));
    CREATE_HIP(dev_alloc(&ctx->eh, Menc * d, st));
    CREATE_HIP(dev_alloc(&ctx->exn, Menc * d, st));
    if (e8) { CREATE_HIP(dev_alloc(&ctx->exn8, Menc * (size_t)((d + 127) / 128 * 128), st)); CREATE_HIP(dev_alloc(&ctx->exs, Menc, st)); }
    CREATE_HIP(dev_alloc(&ctx->eq, Menc * d, st));
    CREATE_HIP(dev_alloc(&ctx->ek, Menc * d, st));
    CREATE_HIP(dev_alloc(&ctx->evt, Menc * d, st));
    CREATE_HIP(dev_alloc(&ctx->eff, Menc * ctx->ffn, st));
    CREATE_HIP(dev_alloc(&ctx->enc_out, Menc * d, st));
    CREATE_HIP(dev_alloc(&ctx->kx, (size_t)ctx->nkv * Menc * d, st));
    CREATE_HIP(dev_alloc(&ctx->vx, (size_t)ctx->nkv * Menc * d, st));
    ctx->xkv8 = cfg->cross_kv_fp8 != 0;
    if (ctx->xkv8) {
        CREATE_HIP(dev_alloc(&ctx->kx8, (size_t)ctx->nkv * Menc * d, st));
        CREATE_HIP(dev_alloc(&ctx->vx8, (size_t)ctx->nkv * Menc * d, st));
        CREATE_HIP(dev_alloc(&ctx->kxs, (size_t)ctx->nkv * B * H, st));
        CREATE_HIP(dev_alloc(&ctx->vxs, (size_t)ctx->nkv * B * H, st));
    }
    CREATE_HIP(dev_alloc(&ctx->kc, (size_t)ctx->nkv * B * H * Tal * 64, st));
    CREATE_HIP(dev_alloc(&ctx->vc, (size_t)ctx->nkv * B * H * Tal * 64, st));
    ctx->Rcap = ctx->Mmax * ctx->maxB;
    const size_t RW = ctx->Rcap;
    CREATE_HIP(dev_alloc(&ctx->h, RW * d, st));
    CREATE_HIP(dev_alloc(&ctx->hblk, RW * d, st));
    CREATE_HIP(dev_alloc(&ctx->hf, RW * d, st));
    CREATE_HIP(dev_alloc(&ctx->hf_keep, B * d, st));
    CREATE_HIP(dev_alloc(&ctx->hb_keep, B * d, st));
    CREATE_HIP(dev_alloc(&ctx->carry, B, st));
    CREATE_HIP(dev_alloc(&ctx->rowinfo, (size_t)ctx->Mmax * B, st)); CREATE_HIP(dev_alloc(&ctx->sinfo, B, st)); CREATE_HIP(dev_alloc(&ctx->steprows, 4, st));
    CREATE_HIP(dev_alloc(&ctx->sel_src, B * 16, st));
    CREATE_HIP(dev_alloc(&ctx->sel_n, B, st));
    CREATE_HIP(dev_alloc(&ctx->sel_base, B, st));
    if (ctx->tn) {
        CREATE_HIP(dev_alloc(&ctx->tree, 1, st));
        CREATE_HIP(hipMemcpyAsync(ctx->tree, &ctx->tree_host, sizeof(TreeDev), hipMemcpyHostToDevice, st));
    }
    // sibling rows (wm_config.sibling_rows): the chain's K + 1 nodes, then S leaves under the root — node K + 1 + j sits at depth 1 and sees the
    // history, the root and itself.  Only the depth / ancestor tables are used (k_embed, k_attn_mfma); candidates and acceptance stay the chain's.
    ctx->sib_cfg = 0;
    if (ctx->tn == 0 && cfg->sibling_rows > 0) {
        const int K = cfg->medusa_heads, S = std::min({(int)cfg->sibling_rows, 15 - K, 5});
        if (S > 0) {
            TreeDev sib{};               // (host staging: the copy below is awaited before the block ends)
            sib.K = K; sib.n_nodes = K + 1 + S; sib.n_paths = 1;
            for (int n = 0; n <= K; ++n) { sib.depth[n] = n; sib.parent[n] = n - 1; sib.anc[n] = (2ull << n) - 1ull; }
            for (int j = 0; j < S; ++j) { const int n = K + 1 + j; sib.depth[n] = 1; sib.parent[n] = 0; sib.anc[n] = 1ull | (1ull << n); }
            CREATE_HIP(dev_alloc(&ctx->sibtree, 1, st));
            CREATE_HIP(dev_alloc(&ctx->sibpart, (size_t)cfg->max_batch * SEL_SP * 6, st));
            CREATE_HIP(hipMemcpyAsync(ctx->sibtree, &sib, sizeof(TreeDev), hipMemcpyHostToDevice, st));
            CREATE_HIP(hipStreamSynchronize(st));
            ctx->sib_cfg = S;
        }
    }
    CREATE_HIP(dev_alloc(&ctx->qbuf, RW * d, st));
    CREATE_HIP(dev_alloc(&ctx->xbuf, 2 * RW * d, st));          // hi + lo planes
    { const char* v = std::getenv("WM_LN_FOLD"); ctx->ln_fold = !(v && std::atoi(v) == 0); }
    if (ctx->ln_fold) {
        CREATE_HIP(dev_alloc(&ctx->xn, 2 * RW * d, st));
        CREATE_HIP(dev_alloc(&ctx->lnstats, RW * (d / 16), st));
        CREATE_HIP(dev_alloc(&ctx->foldv, (size_t)ctx->nkv * (2 * (4 * d + ctx->ffn) + 3 * d), st));      // c, b' of three GEMMs + three scaled gains per layer
    }
    CREATE_HIP(dev_alloc(&ctx->fbuf, 2 * RW * ctx->ffn, st));
    CREATE_HIP(dev_alloc(&ctx->ybuf, 2 * RW * d, st));
    CREATE_HIP(dev_alloc(&ctx->cml, RW * H * ctx->NS * 2, st));
    CREATE_HIP(dev_alloc(&ctx->co, RW * H * ctx->NS * 64, st));
    CREATE_HIP(dev_alloc(&ctx->ticket, B * 32 * (WM_TREE_MAX_NODES / 16), st));
    CREATE_HIP(dev_alloc(&ctx->logits, RW * ctx->Vpad, st));
    CREATE_HIP(dev_alloc(&ctx->amax, B * WM_TREE_MAX_NODES, st));
    CREATE_HIP(dev_alloc(&ctx->pc, B * WM_TREE_MAX_NODES, st));
    CREATE_HIP(dev_alloc(&ctx->part1, RW * 16 * 4, st));
    CREATE_HIP(dev_alloc(&ctx->part2, B * WM_TREE_MAX_NODES * 16, st));
    // timestamp rules (wm_decode_begin_ts): committed state per stream, verify-row records, timestamp-region partials, decisions
    CREATE_HIP(dev_alloc(&ctx->ts.st, B, st));
    CREATE_HIP(dev_alloc(&ctx->ts.ver, std::max<size_t>(B, RW) * WM_CAND_STRIDE, st));
    CREATE_HIP(dev_alloc(&ctx->ts.part1t, RW * 16 * 4, st));
    CREATE_HIP(dev_alloc(&ctx->ts.forced, RW + B, st));
    // seeded sampling (wm_set_sampling): slice partials, the winners' perturbed values, the rows' stream keys
    CREATE_HIP(dev_alloc(&ctx->samp.part, RW * 16 * 8, st));
    CREATE_HIP(dev_alloc(&ctx->samp.val, RW + B, st));
    CREATE_HIP(dev_alloc(&ctx->samp_keys, std::max<size_t>(B, 16), st));
    // its filters (wm_set_sampling_filter): the processed rows after the decision, thresholds, kept counts; filter off until a request says otherwise
    CREATE_HIP(dev_alloc(&ctx->samp.fv, std::max<size_t>(B, 16) * ctx->Vpad, st));
    CREATE_HIP(dev_alloc(&ctx->samp.thr, RW + B, st));
    CREATE_HIP(dev_alloc(&ctx->samp.kept, RW + B, st));
    ctx->samp.top_k = 0; ctx->samp.top_p = 1.0f; ctx->samp.min_p = 0.0f;
    // language detection (wm_detect_language): the candidates and the picks of k_lang_pick
    CREATE_HIP(dev_alloc(&ctx->lang_ids, WM_LANG_MAX, st));
    CREATE_HIP(dev_alloc(&ctx->lang_out, std::max<size_t>(B, 16), st));
    const size_t Tids = ctx->Tal;
    CREATE_HIP(dev_alloc(&ctx->ids, B * Tids, st));
    CREATE_HIP(dev_alloc(&ctx->L, B, st));
    CREATE_HIP(dev_alloc(&ctx->kvlen, B, st));
    CREATE_HIP(dev_alloc(&ctx->finished, B, st));
    CREATE_HIP(dev_alloc(&ctx->cand, B * WM_CAND_STRIDE, st));
    CREATE_HIP(dev_alloc(&ctx->niter, B, st));
    CREATE_HIP(dev_alloc(&ctx->hist, 32, st));
    CREATE_HIP(dev_alloc(&ctx->supmask, (size_t)ctx->Vpad, st));
    CREATE_HIP(dev_alloc(&ctx->exppen, Tids + 1, st));
    CREATE_HIP(dev_alloc(&ctx->tap_tok, 16, st));
    CREATE_HIP(dev_alloc(&ctx->done, 4, st));
    CREATE_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->hostflags), 64, hipHostMallocMapped));
    CREATE_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->hostflags_dev), ctx->hostflags, 0));
    ctx->hostflags[0] = ctx->hostflags[1] = 0;
    if (ctx->ln_fold && wm_dec_fold_init(ctx) != WM_OK) { g_create_err = "wm_create: " + ctx->err; wm_destroy(ctx); return WM_ERR_HIP; }
    CREATE_HIP(hipStreamSynchronize(st));
#undef CREATE_HIP
    *out = ctx;
    return WM_OK;
}

extern "C" int wm_sync(wm_ctx* ctx) { WM_HIP(hipSetDevice(ctx->device)); WM_HIP(hipStreamSynchronize(ctx->stream)); return WM_OK; }

extern "C" int64_t wm_resample_len(int64_t n_in, int sr_in, int sr_out) { return wm_enc_resample_len((long)n_in, sr_in, sr_out); }

extern "C" int wm_resample(wm_ctx* ctx, const float* in, int B, int channels, int n_in, int sr_in, int sr_out, float* out)
{
    if (!ctx || !in || !out) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    return wm_enc_resample(ctx, in, B, channels, n_in, sr_in, sr_out, out);
}

extern "C" int wm_logmel(wm_ctx* ctx, const float* wav, int B, int n_samples, float* feats)
{
    if (!ctx || !wav || !feats) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    return wm_enc_logmel(ctx, wav, B, n_samples, feats);
}

extern "C" int wm_encode(wm_ctx* ctx, const float* feats, int B)
{
    if (!ctx || !feats) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    ctx->began = false;
    ctx->beam_expanded = false;         // (the encoder pass rewrites the cross K/V slots)
    return wm_enc_encode(ctx, feats, B);
}

extern "C" int wm_set_encoder_output(wm_ctx* ctx, const float* hidden, int B)
{
    if (!ctx || !hidden) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    ctx->began = false;
    ctx->beam_expanded = false;
    return wm_enc_set_output(ctx, hidden, B);
}

// the timestamp scalars of a decode / tap: ts == NULL -> off.  Validation errors go to ctx->err.
static int wm_ts_setup(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* ts, TsDev* out)
{
    TsDev t = ctx->ts;
    t.on = 0; t.tb = ctx->V; t.nots = -1; t.mit = -1; t.L = ctx->L;      // (off: the whole vocabulary is the text region)
    // repetition rules (wm_set_repeat_rules): the decode's prefixes are the committed ids and the candidates; taps / scoring point elsewhere
    const bool pen = ctx->rep.repetition_penalty != 1.0f, ngram = ctx->rep.no_repeat_ngram_size > 0;
    t.rp = (pen ? 1 : 0) | (ngram ? 2 : 0); t.rp_pen = ctx->rep.repetition_penalty; t.rp_g = ctx->rep.no_repeat_ngram_size;
    t.rp_ids = ctx->ids; t.rp_stride = ctx->Tal; t.rp_len = nullptr; t.rp_cand = ctx->cand; t.rp_flags = nullptr;
    if (t.rp && ctx->tn) { ctx->err = "repetition rules: not supported with a candidate tree (medusa_choices with top-k > 1)"; return WM_ERR_ARG; }
    if (ts) {
        if (ctx->tn) { ctx->err = "timestamps: not supported with a candidate tree (medusa_choices with top-k > 1)"; return WM_ERR_ARG; }
        const int tb = ts->timestamp_begin;
        if (tb != ts->no_timestamps_token_id + 1 || tb < 1 || ctx->V - tb < 2) {
            ctx->err = "timestamps: timestamp_begin must be no_timestamps_token_id + 1 with at least 2 timestamp tokens in the vocabulary";
            return WM_ERR_ARG;
        }
        if (gp->eos_token_id >= tb || (gp->prompt_len > 0 && gp->prompt[0] >= tb)) {
            ctx->err = "timestamps: eos and the start token must lie below timestamp_begin"; return WM_ERR_ARG; }
        t.on = 1; t.tb = tb; t.nots = ts->no_timestamps_token_id; t.mit = ts->max_initial_timestamp_index < 0 ? -1 : ts->max_initial_timestamp_index;
    }
    *out = t;
    return WM_OK;
}

int wm_proc_setup(wm_ctx* ctx, const char* who, const wm_gen_params* gp, const wm_timestamp_params* tsp, GenDev* g_out, TsDev* ts_out)
{
    if (gp->eos_token_id < 0 || gp->eos_token_id >= ctx->V) { ctx->err = std::string(who) + ": eos out of range"; return WM_ERR_ARG; }
    if (gp->prompt_len < 0 || (gp->prompt_len > 0 && !gp->prompt)) { ctx->err = std::string(who) + ": bad prompt"; return WM_ERR_ARG; }
    TsDev ts{};
    if (int rc = wm_ts_setup(ctx, gp, tsp, &ts)) return rc;
    const int P = gp->prompt_len, Tids = ctx->Tal;
    GenDev g{};
    g.P = P; g.eos = gp->eos_token_id; g.pad = gp->pad_token_id;
    g.exp_start = gp->exp_decay_start >= 0 ? gp->exp_decay_start + P : -1;
    g.thr = gp->posterior_threshold; g.alpha = gp->posterior_alpha;
    // the begin-suppress list applies at: the timestamp rules' begin_index, else the generation parameters', else the prompt length
    g.begin = (tsp && tsp->begin_index >= 0) ? tsp->begin_index : (gp->begin_index >= 0 ? gp->begin_index : P);
    g.K = ctx->K; g.V = ctx->V; g.Vpad = ctx->Vpad; g.Tids = Tids;
    std::vector<unsigned char> mask(ctx->Vpad, 0);
    for (int i = 0; i < gp->n_suppress; ++i) if (gp->suppress[i] >= 0 && gp->suppress[i] < ctx->V) mask[gp->suppress[i]] |= 1;
    for (int i = 0; i < gp->n_begin_suppress; ++i)
        if (gp->begin_suppress[i] >= 0 && gp->begin_suppress[i] < ctx->V) mask[gp->begin_suppress[i]] |= 2;
    std::vector<float> pen(Tids + 1, 0.f);
    if (g.exp_start >= 0)
        for (int t = 0; t <= Tids; ++t)     // (factor^(cur_len - start) - 1) evaluated in double like the Python scalar
            pen[t] = t > g.exp_start ? (float)(std::pow((double)gp->exp_decay_factor, (double)(t - g.exp_start)) - 1.0) : 0.f;
    WM_HIP(hipMemcpyAsync(ctx->supmask, mask.data(), mask.size(), hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipMemcpyAsync(ctx->exppen, pen.data(), pen.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));      // host vectors go out of scope
    *g_out = g; *ts_out = ts;
    return WM_OK;
}

void wm_decode_invalidate(wm_ctx* ctx, bool drop_graphs)
{
    ctx->began = false; ctx->use_done = false; ctx->host_carry = false; ctx->dev_carry = false; ctx->step_flow = false;
    if (ctx->beam_expanded) (void)wm_beam_compact(ctx);         // a beam decode that was left unfinished: the cross K/V goes back to its clips' slots
    if (drop_graphs) { ctx->graphs_plain.drop(); ctx->graphs_beam.drop(); }
}

// HF RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor inside the select and scoring kernels (include/wm.h)
extern "C" int wm_set_repeat_rules(wm_ctx* ctx, const wm_repeat_params* rp)
{
    if (!ctx) return WM_ERR_ARG;
    if (!rp) { ctx->rep = wm_repeat_params{1.0f, 0}; return WM_OK; }
    if (!(rp->repetition_penalty > 0.f) || !std::isfinite(rp->repetition_penalty)) {
        ctx->err = "wm_set_repeat_rules: repetition_penalty must be a finite number > 0"; return WM_ERR_ARG; }
    if (rp->no_repeat_ngram_size < 0 || rp->no_repeat_ngram_size > ctx->Tmax) {
        ctx->err = "wm_set_repeat_rules: no_repeat_ngram_size must be in [0, n_tgt]"; return WM_ERR_ARG; }
    ctx->rep = *rp;
    return WM_OK;
}

// Seeded sampling on the plain decode path (include/wm.h): kept on the context, read by wm_decode_begin / wm_decode_begin_ts
static int wm_sampling_check(wm_ctx* ctx, const char* who, const wm_sample_params* sp)
{
    if (!(sp->temperature > 0.f) || !std::isfinite(sp->temperature)) {
        ctx->err = std::string(who) + ": the sampling temperature must be a finite number > 0"; return WM_ERR_ARG; }
    if (sp->n_keys < 0) { ctx->err = std::string(who) + ": n_keys must not be negative"; return WM_ERR_ARG; }
    return WM_OK;
}
extern "C" int wm_set_sampling(wm_ctx* ctx, const wm_sample_params* sp)
{
    if (!ctx) return WM_ERR_ARG;
    if (!sp) { ctx->samp_set_on = false; ctx->samp_set_keys.clear(); return WM_OK; }
    if (int rc = wm_sampling_check(ctx, "wm_set_sampling", sp)) return rc;
    ctx->samp_set_on = true; ctx->samp_set_temp = sp->temperature; ctx->samp_set_seed = sp->seed;
    ctx->samp_set_keys.clear();
    if (sp->stream_keys) ctx->samp_set_keys.assign(sp->stream_keys, sp->stream_keys + sp->n_keys);
    else for (int i = 0; i < sp->n_keys; ++i) ctx->samp_set_keys.push_back((uint64_t)i);       // NULL: 0 .. n_keys - 1 (n_keys is still checked against B)
    return WM_OK;
}
static int wm_filter_check(wm_ctx* ctx, const char* who, const wm_sample_filter* f)
{
    if (f->top_k < 0) { ctx->err = std::string(who) + ": top_k must be >= 0 (0 = off)"; return WM_ERR_ARG; }
    if (!(f->top_p > 0.f && f->top_p <= 1.f)) { ctx->err = std::string(who) + ": top_p must be in (0, 1] (1 = off)"; return WM_ERR_ARG; }
    if (!(f->min_p >= 0.f && f->min_p <= 1.f)) { ctx->err = std::string(who) + ": min_p must be in [0, 1] (0 = off)"; return WM_ERR_ARG; }
    return WM_OK;
}
extern "C" int wm_set_sampling_filter(wm_ctx* ctx, const wm_sample_filter* f)
{
    if (!ctx) return WM_ERR_ARG;
    if (!f) { ctx->samp_filter_on = false; ctx->samp_filter = wm_sample_filter{0, 1.0f, 0.0f}; return WM_OK; }
    if (int rc = wm_filter_check(ctx, "wm_set_sampling_filter", f)) return rc;
    ctx->samp_filter_on = true; ctx->samp_filter = *f;
    return WM_OK;
}
// the device form of a sampling request: fl(1 / T), the seed's two words, the filter (NULL: off), the context's buffers
static SampDev wm_sampling_dev(wm_ctx* ctx, float temperature, uint64_t seed, const wm_sample_filter* f)
{
    SampDev d = ctx->samp;
    d.on = 1; d.inv_t = 1.0f / temperature; d.seed_lo = (unsigned)seed; d.seed_hi = (unsigned)(seed >> 32); d.keys = ctx->samp_keys;
    d.top_k = f ? f->top_k : 0; d.top_p = f ? f->top_p : 1.0f; d.min_p = f ? f->min_p : 0.0f;
    return d;
}

// Per-stream prompts of one length (include/wm.h): kept on the context, read by wm_decode_begin / wm_decode_begin_ts
extern "C" int wm_set_stream_prompts(wm_ctx* ctx, const int32_t* prompts, int B, int P)
{
    if (!ctx) return WM_ERR_ARG;
    if (!prompts) { ctx->sp_rows.clear(); ctx->sp_B = ctx->sp_P = 0; return WM_OK; }
    if (B < 1 || P < 1) { ctx->err = "wm_set_stream_prompts: B and P must be >= 1"; return WM_ERR_ARG; }
    ctx->sp_rows.assign(prompts, prompts + (size_t)B * P); ctx->sp_B = B; ctx->sp_P = P;
    return WM_OK;
}
// what only a decode can check of the sticky table: its shape against the decode's clips and prompt length, the ids, the timestamp rules' start token
static int wm_stream_prompts_check(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, int G)
{
    const std::string w = "wm_decode_begin: stream prompts (wm_set_stream_prompts): ";
    if (ctx->sp_P != gp->prompt_len) {
        ctx->err = w + "rows of " + std::to_string(ctx->sp_P) + " ids, wm_gen_params.prompt_len is " + std::to_string(gp->prompt_len) + " (one common length)"; return WM_ERR_ARG; }
    if (ctx->sp_B != G) { ctx->err = w + std::to_string(ctx->sp_B) + " rows for a decode of " + std::to_string(G) + " clips"; return WM_ERR_ARG; }
    for (int b = 0; b < G; ++b) {
        const int32_t* row = ctx->sp_rows.data() + (size_t)b * ctx->sp_P;
        for (int i = 0; i < ctx->sp_P; ++i)
            if (row[i] < 0 || row[i] >= ctx->V) {
                ctx->err = w + "row " + std::to_string(b) + ": token id " + std::to_string(row[i]) + " outside the vocabulary"; return WM_ERR_ARG; }
        if (tsp && row[0] >= tsp->timestamp_begin) {
            ctx->err = w + "row " + std::to_string(b) + ": timestamps: the start token must lie below timestamp_begin"; return WM_ERR_ARG; }
    }
    return WM_OK;
}

extern "C" int wm_decode_begin(wm_ctx* ctx, const wm_gen_params* gp, int B) { return wm_decode_begin_ts(ctx, gp, nullptr, B); }

extern "C" int wm_decode_begin_ts(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, int B)
{
    if (!ctx || !gp) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    if (ctx->beam_expanded) { if (int rc = wm_beam_compact(ctx)) return rc; }      // (a beam decode that was never run to its end)
    if (ctx->Benc < 1 || B != ctx->Benc) { ctx->err = "wm_decode_begin: call wm_encode with the same B first"; return WM_ERR_STATE; }
    const int P = gp->prompt_len, Tids = ctx->Tal;
    // beam search (wm_set_beam; HF _beam_search): B clips become B * n streams of the plain decode
    const bool beam = ctx->beam_set_on;
    const int nbeam = beam ? ctx->beam_set.num_beams : 1, G = B;
    if (beam) {
        if (!gp->vanilla) { ctx->err = "wm_decode_begin: beam search runs on the plain decode path only (wm_gen_params.vanilla = 1)"; return WM_ERR_ARG; }
        if (ctx->tn) { ctx->err = "wm_decode_begin: beam search is not supported with a candidate tree (medusa_choices with top-k > 1)"; return WM_ERR_ARG; }
        if (ctx->samp_set_on) { ctx->err = "wm_decode_begin: beam search and sampling (wm_set_sampling) cannot be on together"; return WM_ERR_ARG; }
        if (B * nbeam > ctx->maxB) { ctx->err = "wm_decode_begin: B * num_beams exceeds max_batch"; return WM_ERR_ARG; }
        B *= nbeam;
    }
    ctx->beam_done = false;
    if (P < 1 || P >= ctx->Tmax - ctx->K - 1) {
        // same condition class as the reference's over-long prompt ValueError (model.py:1526-1529)
        ctx->err = "wm_decode_begin: prompt length must be in [1, n_tgt - K - 2]"; return WM_ERR_ARG; }
    // per-stream prompts (wm_set_stream_prompts): row g of the table is clip g's; none set: wm_gen_params.prompt for everybody
    const int32_t* sp = ctx->sp_rows.empty() ? nullptr : ctx->sp_rows.data();
    if (sp) { if (!gp->prompt) { ctx->err = "wm_decode_begin: bad prompt"; return WM_ERR_ARG; } if (int rc = wm_stream_prompts_check(ctx, gp, tsp, G)) return rc; }
    if (!gp->vanilla && gp->accept_mode == WM_ACCEPT_TYPICAL && !(gp->temperature > 0.f)) {
        ctx->err = "wm_decode_begin: typical acceptance needs temperature > 0"; return WM_ERR_ARG; }
    SampDev sd = ctx->samp; sd.on = 0;
    if (ctx->samp_set_on) {
        if (!gp->vanilla) { ctx->err = "wm_decode_begin: sampling runs on the plain decode path only (wm_gen_params.vanilla = 1)"; return WM_ERR_ARG; }
        if (ctx->tn) { ctx->err = "wm_decode_begin: sampling is not supported with a candidate tree (medusa_choices with top-k > 1)"; return WM_ERR_ARG; }
        if ((int)ctx->samp_set_keys.size() != B) { ctx->err = "wm_decode_begin: wm_sample_params.n_keys must equal B"; return WM_ERR_ARG; }
        sd = wm_sampling_dev(ctx, ctx->samp_set_temp, ctx->samp_set_seed, ctx->samp_filter_on ? &ctx->samp_filter : nullptr);
    } else if (ctx->samp_filter_on) {
        ctx->err = "wm_decode_begin: a sampling filter is set (wm_set_sampling_filter) but this decode does not sample (wm_set_sampling)"; return WM_ERR_ARG;
    }
    SeqBiasDev sbd{};                      // sequence bias (wm_set_sequence_bias): the sticky table's device form, after what only a decode can check
    if (int rc = wm_seq_bias_begin(ctx, "wm_decode_begin", gp, &sbd)) return rc;
    ConstraintDev cd{};                    // constraint (wm_set_constraint): the same for the sticky table of allowed sequences
    if (int rc = wm_constraint_begin(ctx, "wm_decode_begin", gp, tsp, &cd)) return rc;
    // the processors' tables and the scalars of this decode
    GenDev g{}; TsDev ts{};
    if (int rc = wm_proc_setup(ctx, "wm_decode_begin", gp, tsp, &g, &ts)) return rc;
    g.max_length = std::min(gp->max_length, ctx->Tmax);
    g.hard_max_length = std::min(gp->hard_max_length, ctx->Tmax);
    g.inv_temp = (gp->accept_mode == WM_ACCEPT_TYPICAL && gp->temperature > 0.f) ? 1.0f / gp->temperature : 1.0f;
    g.force_accept = gp->force_accept; g.accept_mode = gp->accept_mode; g.vanilla = gp->vanilla;
    const bool fuse = std::getenv("WM_NO_CARRY") == nullptr;
    const bool host_carry = fuse && B == 1 && !gp->vanilla, dev_carry = fuse && B > 1 && !gp->vanilla;
    // several streams with the per-stream carry, chain candidates: the merged-step schedule (a stream that needs a base pass gets its one
    // row inside the other streams' verify pass: wm_dec_step).  WM_NO_STEP=1: the lock-step iteration (base pass + verify pass for everybody).
    const bool step_flow = dev_carry && ctx->tn == 0 && std::getenv("WM_NO_STEP") == nullptr;
    g.fuse = host_carry ? 1 : (dev_carry ? (step_flow ? 3 : 2) : 0);
    g.sib = (host_carry && ctx->tn == 0 && ctx->sib_cfg > 0 && std::getenv("WM_NO_SIBLINGS") == nullptr) ? ctx->sib_cfg : 0;
    BeamDev bd{};
    if (beam) { if (int rc = wm_beam_begin(ctx, ctx->beam_set, G, g, true, nullptr, P, &bd)) return rc; }
    // the captured graphs: this decode's slot keeps its graphs when they were captured with the same key; the other slot is not touched
    const DecGraphKey key = wm_dec_graph_key(g, B, ts, sd, sbd, cd, bd);
    DecGraphSlot& slot = beam ? ctx->graphs_beam : ctx->graphs_plain;
    if (!(key == slot.key)) { slot.drop(); slot.key = key; }
    ctx->fuse = fuse; ctx->host_carry = host_carry; ctx->dev_carry = dev_carry; ctx->step_flow = step_flow;
    ctx->gp = g; ctx->Bdec = B; ctx->ts = ts; ctx->samp = sd; ctx->sbias = sbd; ctx->cons = cd; ctx->beam = bd; ctx->beam_clips = beam ? G : 0;       // (the context's scalars are this decode's from here on)
    hipStream_t st = ctx->stream;           // uploads
    if (sd.on) WM_HIP(hipMemcpyAsync(ctx->samp_keys, ctx->samp_set_keys.data(), B * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    std::vector<int> ids((size_t)B * Tids, gp->pad_token_id), L(B, P), zero(B, 0);
    for (int b = 0; b < B; ++b) {             // (beams: stream b is a beam of clip b / nbeam)
        const int32_t* row = sp ? sp + (size_t)(b / nbeam) * P : gp->prompt;
        for (int i = 0; i < P; ++i) ids[(size_t)b * Tids + i] = row[i];
    }
    WM_HIP(hipMemcpyAsync(ctx->ids, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(ctx->L, L.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(ctx->kvlen, zero.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(ctx->finished, zero.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(ctx->niter, zero.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    WM_HIP(hipMemsetAsync(ctx->hist, 0, 32 * sizeof(long long), st));
    WM_HIP(hipMemsetAsync(ctx->done, 0, 4 * sizeof(int), st));
    WM_HIP(hipMemsetAsync(ctx->carry, 0, ctx->maxB * sizeof(int), st));
    WM_HIP(hipMemsetAsync(ctx->steprows, 0, 4 * sizeof(int), st));
    ctx->use_done = true;
    std::vector<int4> tst(B, make_int4(0, 0, -1, 0));
    if (ts.on) {                           // the committed timestamp state of the prompt's sampled part, ids[begin:P] (HF slices input_ids[begin_index:])
        for (int b = 0; b < B; ++b) tst[b] = ts_fold_ids(tst[b], ids.data() + (size_t)b * Tids, g.begin, P, ts.tb);
        WM_HIP(hipMemcpyAsync(ctx->ts.st, tst.data(), B * sizeof(int4), hipMemcpyHostToDevice, st));
    }
    if (beam) {
        if (int rc = wm_beam_seed_table(ctx, bd)) return rc;
        if (int rc = wm_beam_expand(ctx, G, nbeam)) return rc;
    }
    WM_HIP(hipStreamSynchronize(st));      // host vectors go out of scope
    ctx->hostflags[0] = 0; ctx->hostflags[1] = 0;
    ctx->began = true; ctx->first_done = false; ctx->iters = 0; ctx->ms_decode = 0.f; ctx->graph_replays = 0;
    return WM_OK;
}

static int count_unfinished(wm_ctx* ctx, int* n)
{
    std::vector<int> f(ctx->Bdec);
    WM_HIP(hipMemcpyAsync(f.data(), ctx->finished, ctx->Bdec * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    int c = 0;
    for (int v : f) c += v ? 0 : 1;
    *n = c;
    return WM_OK;
}

static int capture_graph(wm_ctx* ctx, hipGraphExec_t* out, int (*body)(wm_ctx*, int))
{
    hipStream_t st = ctx->stream;
    hipGraph_t gr = nullptr;
    *out = nullptr;
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return WM_OK; }
    const int rc = body(ctx, 1);
    const hipError_t e2 = hipStreamEndCapture(st, &gr);
    if (rc == WM_OK && e2 == hipSuccess && gr) {
        hipGraphExec_t ex = nullptr;
        if (hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0) == hipSuccess) *out = ex;
    }
    if (gr) hipGraphDestroy(gr);
    (void)hipGetLastError();
    return WM_OK;
}

extern "C" int wm_decode_run(wm_ctx* ctx, int max_iters, int* n_unfinished)
{
    if (!ctx) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    if (!ctx->began) { ctx->err = "wm_decode_run: call wm_decode_begin first"; return WM_ERR_STATE; }
    hipStream_t st = ctx->stream;
    const bool use_graph = std::getenv("WM_NO_GRAPH") == nullptr;
    DecGraphSlot& gs = ctx->beam.on ? ctx->graphs_beam : ctx->graphs_plain;       // the slot wm_decode_begin_ts keyed for this decode
    int left = 0, done = 0;
    int rc = count_unfinished(ctx, &left);
    if (rc) return rc;
    WM_HIP(hipEventRecord(ctx->ev0, st));
    if (ctx->host_carry) {
        // Single stream: the host reads {carry, finished} (host-mapped, written by k_accept) after every iteration and
        // launches the base-pass graph only when the hidden state was NOT carried over from the verify pass.
        while (left > 0 && done < max_iters) {
            if (!ctx->first_done) {
                const int p_last = wm_dec_prompt_prefix(ctx, ctx->gp.P);      // long prompts: leading chunks for their K/V only
                if (p_last < 1) return WM_ERR_HIP;
                rc = wm_dec_iteration(ctx, p_last);               // iteration 1: the base pass consumes the (last <= 16) prompt tokens
                if (rc) return rc;
                ctx->first_done = true;
            } else {
                const bool need_base = ctx->hostflags[0] == 0;
                const bool warm = ctx->iters >= 2;
                if (need_base) {
                    if (use_graph && warm && !gs.base) { rc = capture_graph(ctx, &gs.base, wm_dec_iter_base); if (rc) return rc; }
                    if (use_graph && gs.base) WM_HIP(hipGraphLaunch(gs.base, st));
                    else { rc = wm_dec_iter_base(ctx, 1); if (rc) return rc; }
                }
                if (use_graph && warm && !gs.step) { rc = capture_graph(ctx, &gs.step, wm_dec_iter_rest); if (rc) return rc; }
                if (use_graph && gs.step) { WM_HIP(hipGraphLaunch(gs.step, st)); ctx->graph_replays++; }
                else { rc = wm_dec_iter_rest(ctx, 1); if (rc) return rc; }
            }
            WM_HIP(hipStreamSynchronize(st));
            ctx->iters++; done++;
            left = ctx->hostflags[1] ? 0 : 1;
        }
    } else {
        const int poll = 4;
        while (left > 0 && done < max_iters) {
            const int burst = std::min(poll, max_iters - done);
            for (int i = 0; i < burst; ++i) {
                if (!ctx->first_done) {                       // iteration 1: the base pass consumes the P prompt tokens
                    const int p_last = wm_dec_prompt_prefix(ctx, ctx->gp.P);
                    if (p_last < 1) return WM_ERR_HIP;
                    rc = wm_dec_iteration(ctx, p_last);
                    if (rc) return rc;
                    ctx->first_done = true;
                } else {
                    int (*body)(wm_ctx*, int) = ctx->step_flow ? wm_dec_step : wm_dec_iteration;
                    // shapes are warm: capture one steady-state iteration / step
                    if (use_graph && ctx->iters >= 2 && !gs.step) { rc = capture_graph(ctx, &gs.step, body); if (rc) return rc; }
                    if (use_graph && gs.step) { WM_HIP(hipGraphLaunch(gs.step, st)); ctx->graph_replays++; }
                    else { rc = body(ctx, 1); if (rc) return rc; }
                }
                ctx->iters++; done++;
            }
            rc = count_unfinished(ctx, &left);
            if (rc) return rc;
        }
    }
    WM_HIP(hipEventRecord(ctx->ev1, st));
    WM_HIP(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    WM_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->ms_decode += ms;
    if (ctx->beam.on && left == 0) {        // every clip is done: the cross K/V goes back to the clips' slots (the state wm_encode left)
        if (int rc2 = wm_beam_compact(ctx)) return rc2;
        ctx->beam_done = true;
        left = 0;
    }
    if (n_unfinished) *n_unfinished = ctx->beam.on ? (left + ctx->beam.n - 1) / ctx->beam.n : left;
    return WM_OK;
}

extern "C" int wm_get_tokens(wm_ctx* ctx, int stream, int32_t* out, int cap, int* n)
{
    if (!ctx || !out || !n || stream < 0 || stream >= ctx->Bdec) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    if (ctx->beam.on) {                     // a beam decode: the clip's finished hypothesis of rank 0
        float score = 0.f;
        if (!ctx->beam_done) { ctx->err = "wm_get_tokens: the beam decode is not finished"; return WM_ERR_STATE; }
        return wm_get_beam_result(ctx, stream, 0, out, cap, n, &score);
    }
    int L = 0;
    WM_HIP(hipMemcpyAsync(&L, ctx->L + stream, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    L = std::min(L, ctx->gp.Tids);
    std::vector<int> ids(L);
    WM_HIP(hipMemcpyAsync(ids.data(), ctx->ids + (size_t)stream * ctx->gp.Tids, L * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    bool seen = false;                       // post-EOS overwrite, model.py:798-810
    for (int i = 0; i < L; ++i) { if (seen) ids[i] = ctx->gp.eos; else if (ids[i] == ctx->gp.eos) seen = true; }
    const int m = std::min(L, cap);
    std::memcpy(out, ids.data(), m * sizeof(int));
    *n = L;
    return WM_OK;
}

extern "C" int wm_get_stats(wm_ctx* ctx, wm_stats* out)
{
    if (!ctx || !out) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    long long h[32];
    std::vector<int> ni(std::max(ctx->Bdec, 1), 0);
    WM_HIP(hipMemcpyAsync(h, ctx->hist, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->Bdec > 0) WM_HIP(hipMemcpyAsync(ni.data(), ctx->niter, ctx->Bdec * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    std::memset(out, 0, sizeof(*out));
    out->iterations = *std::max_element(ni.begin(), ni.end());
    out->iterations_launched = ctx->iters;
    for (int i = 0; i < 16; ++i) out->accept_hist[i] = h[i];
    out->tokens_emitted = h[16];
    out->ms_logmel = ctx->ms_logmel; out->ms_encode = ctx->ms_encode; out->ms_decode = ctx->ms_decode;
    out->graph_replays = ctx->graph_replays;
    out->sibling_hits = (int32_t)h[17];
    if (ctx->step_flow && ctx->steprows) {
        int sr[4] = {0, 0, 0, 0};
        WM_HIP(hipMemcpyAsync(sr, ctx->steprows, sizeof(sr), hipMemcpyDeviceToHost, ctx->stream));       // on the context's stream like every other read
        WM_HIP(hipStreamSynchronize(ctx->stream));
        out->schedule_steps = sr[2];
    }
    return WM_OK;
}

// ---- parity taps ---------------------------------------------------------------------------
static void unpack_rows(const std::vector<bf16_t>& p, int rows, int K, float* out)
{
    const int K32 = K / 32;
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < K; ++k) {
            const uint32_t u = ((uint32_t)p[packed_index(r, k, K32)]) << 16;
            float f; std::memcpy(&f, &u, 4);
            out[(size_t)r * K + k] = f;
        }
}

extern "C" int wm_get_encoder_output(wm_ctx* ctx, int B, float* out)
{
    if (!ctx || !out || B < 1 || B > ctx->Benc) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)B * ctx->Spad * ctx->d;
    std::vector<bf16_t> p(n);
    WM_HIP(hipMemcpyAsync(p.data(), ctx->enc_out, n * sizeof(bf16_t), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<float> full(n);
    unpack_rows(p, B * ctx->Spad, ctx->d, full.data());
    for (int b = 0; b < B; ++b)
        std::memcpy(out + (size_t)b * ctx->S * ctx->d, full.data() + (size_t)b * ctx->Spad * ctx->d, (size_t)ctx->S * ctx->d * sizeof(float));
    return WM_OK;
}

extern "C" int wm_get_cross_kv(wm_ctx* ctx, int kv_layer, int stream, int head, float* k_out, float* v_out)
{
    if (!ctx || kv_layer < 0 || kv_layer >= ctx->nkv || stream < 0 || stream >= ctx->Benc || head < 0 || head >= ctx->H) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    const size_t off = (((size_t)kv_layer * ctx->Benc + stream) * ctx->H + head) * ctx->Spad * 64, n = (size_t)ctx->S * 64;
    const size_t nv = (size_t)ctx->Spad * 64;
    std::vector<bf16_t> kb(n), vb(nv);
    WM_HIP(hipMemcpyAsync(kb.data(), ctx->kx + off, n * sizeof(bf16_t), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipMemcpyAsync(vb.data(), ctx->vx + off, nv * sizeof(bf16_t), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) { const uint32_t u = ((uint32_t)kb[i]) << 16; std::memcpy(k_out + i, &u, 4); }
    for (int s = 0; s < ctx->S; ++s)            // V is stored as V^T MFMA fragments
        for (int dd = 0; dd < 64; ++dd) { const uint32_t u = ((uint32_t)vb[vfrag_index(s, dd)]) << 16; std::memcpy(v_out + (size_t)s * 64 + dd, &u, 4); }
    return WM_OK;
}

// Timestamp parity tap: caller-given rows through the decode loop's timestamp state fold and select kernels (include/wm.h).
extern "C" int wm_select_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, int R, const float* logits,
                              const int32_t* prefixes, int Tmax, const int32_t* lens, const int32_t* probe_tokens, int32_t* out_argmax,
                              float* out_p_probe, float* out_entropy, int32_t* out_ts_forced)
{
    if (!ctx) return WM_ERR_ARG;
    if (!gp || (!tsp && ctx->rep.repetition_penalty == 1.0f && ctx->rep.no_repeat_ngram_size == 0) || R < 1 || !logits || !prefixes || Tmax < 1 || !lens || !probe_tokens || !out_argmax || !out_p_probe || !out_entropy ||
        !out_ts_forced) { ctx->err = "wm_select_rows: bad arguments"; return WM_ERR_ARG; }
    bool probes_ok = true;
    for (int r = 0; r < R; ++r) probes_ok = probes_ok && probe_tokens[r] >= 0 && probe_tokens[r] < ctx->V;
    if (int rc = wm_tap_check_lens(ctx, "wm_select_rows", lens, R, Tmax, false, probes_ok, " and probe tokens inside the vocabulary")) return rc;
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    GenDev g{}; TsDev ts{};
    if (int rc = wm_proc_setup(ctx, "wm_select_rows", gp, tsp, &g, &ts)) return rc;
    g.max_length = g.hard_max_length = ctx->Tmax; g.exp_start = -1;         // no length penalty
    g.inv_temp = gp->temperature > 0.f ? 1.0f / gp->temperature : 1.0f;
    g.force_accept = -1;
    g.accept_mode = WM_ACCEPT_TYPICAL; g.vanilla = 0;
    wm_decode_invalidate(ctx);
    wm_scalars_swap swap(ctx, g, ts);
    wm_tap_stage s{ctx, "wm_select_rows", Tmax, WM_TAP_ROWS};
    if (int rc = s.reserve()) return rc;
    const int L0 = lens[0];         // quirk, kept: cur_len of the one "stream" (L[0]) is row 0's length, uploaded once per call, not per group
    WM_TAP_HIP(s, hipMemcpyAsync(ctx->L, &L0, sizeof(int), hipMemcpyHostToDevice, st));
    std::vector<float> h2((size_t)R * SEL_SP);
    if (int rc = wm_tap_groups(s, R, logits, prefixes, lens, [&](int r0, int n) {
            WM_TAP_HIP(s, hipMemcpyAsync(ctx->cand + 1, probe_tokens + r0, n * sizeof(int), hipMemcpyHostToDevice, st));
            if (int rc = wm_dec_select_rows(ctx, s.pre, s.len, n, Tmax)) return rc;
            WM_TAP_HIP(s, hipMemcpyAsync(out_argmax + r0, ctx->amax, n * sizeof(int), hipMemcpyDeviceToHost, st));
            WM_TAP_HIP(s, hipMemcpyAsync(out_p_probe + r0, ctx->pc, n * sizeof(float), hipMemcpyDeviceToHost, st));
            WM_TAP_HIP(s, hipMemcpyAsync(out_ts_forced + r0, ctx->ts.forced, n * sizeof(int), hipMemcpyDeviceToHost, st));
            WM_TAP_HIP(s, hipMemcpyAsync(h2.data() + (size_t)r0 * SEL_SP, ctx->part2, (size_t)n * SEL_SP * sizeof(float), hipMemcpyDeviceToHost, st));
            return WM_OK;
        })) return rc;
    for (int r = 0; r < R; ++r) {
        float hs = 0.f;
        for (int k = 0; k < SEL_SP; ++k) hs += h2[(size_t)r * SEL_SP + k];     // (k_accept's order)
        out_entropy[r] = -hs;
    }
    return WM_OK;
}

// Sampling parity taps: caller-given rows through k_sample1 / k_sample_fin — with a filter: k_sample1 / k_filter_prep / k_filter_row — (include/wm.h),
// row r at position lens[r] under its own prefix.  wm_sample_rows: f, out_thr, out_kept NULL.
static int wm_sample_rows_impl(wm_ctx* ctx, const char* who_, const wm_gen_params* gp, const wm_timestamp_params* tsp, const wm_sample_params* sp,
                               const wm_sample_filter* f, int R, const float* logits, const int32_t* prefixes, int Tmax, const int32_t* lens,
                               const uint64_t* keys, float* out_thr, int32_t* out_kept, int32_t* out_token, float* out_value, int32_t* out_forced)
{
    const std::string who(who_);
    if (!ctx) return WM_ERR_ARG;
    if (!gp || !sp || R < 1 || !logits || !prefixes || Tmax < 1 || !lens || !keys || !out_token || !out_value || !out_forced) {
        ctx->err = who + ": bad arguments"; return WM_ERR_ARG; }
    if (int rc = wm_sampling_check(ctx, who_, sp)) return rc;
    if (f) { if (int rc = wm_filter_check(ctx, who_, f)) return rc; }
    if (int rc = wm_tap_check_lens(ctx, who_, lens, R, Tmax, true)) return rc;
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    GenDev g{}; TsDev ts{};
    if (int rc = wm_proc_setup(ctx, who_, gp, tsp, &g, &ts)) return rc;
    g.max_length = g.hard_max_length = ctx->Tmax;
    g.inv_temp = 1.0f; g.force_accept = -1;
    g.accept_mode = WM_ACCEPT_GREEDY; g.vanilla = 1;
    wm_decode_invalidate(ctx);
    wm_scalars_swap swap(ctx, g, ts);
    const SampDev sd = wm_sampling_dev(ctx, sp->temperature, sp->seed, f);
    const bool flt = wm_filter_on(sd);
    wm_tap_stage s{ctx, who_, Tmax, WM_TAP_ROWS};
    if (int rc = s.reserve()) return rc;
    ts.rp_ids = s.pre; ts.rp_stride = Tmax; ts.rp_len = s.len;       // repetition rules: the rows' own prefixes
    // outputs no kernel writes (rules off, filter off)
    if (!wm_rules_on(ts)) std::fill(out_forced, out_forced + R, 0);
    if (!flt && out_thr) std::fill(out_thr, out_thr + R, -INFINITY);
    if (!flt && out_kept) std::fill(out_kept, out_kept + R, -1);
    std::vector<int4> recs(WM_TAP_ROWS);
    return wm_tap_groups(s, R, logits, prefixes, lens, [&](int r0, int n) {
        for (int r = 0; r < n && ts.on; ++r) {          // the row's record at its prefix length, where k_cand_fin puts stream 0's verify rows
            const int len = lens[r0 + r];
            recs[r] = ts_record(ts_fold_ids(make_int4(0, 0, -1, 0), prefixes + (size_t)(r0 + r) * Tmax, g.begin, len, ts.tb), len, g.begin, ts.tb, g.V, ts.mit);
        }
        WM_TAP_HIP(s, hipMemcpyAsync(ctx->samp_keys, keys + r0, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        if (ts.on) WM_TAP_HIP(s, hipMemcpyAsync(ts.ver, recs.data(), n * sizeof(int4), hipMemcpyHostToDevice, st));
        if (int rc = wm_sample_launch(ctx, g, ts, sd, s.len, n, 0, 1)) return rc;
        WM_TAP_HIP(s, hipMemcpyAsync(out_token + r0, ctx->amax, n * sizeof(int), hipMemcpyDeviceToHost, st));
        WM_TAP_HIP(s, hipMemcpyAsync(out_value + r0, sd.val, n * sizeof(float), hipMemcpyDeviceToHost, st));
        if (wm_rules_on(ts)) WM_TAP_HIP(s, hipMemcpyAsync(out_forced + r0, ts.forced, n * sizeof(int), hipMemcpyDeviceToHost, st));
        if (flt && out_thr) WM_TAP_HIP(s, hipMemcpyAsync(out_thr + r0, sd.thr, n * sizeof(float), hipMemcpyDeviceToHost, st));
        if (flt && out_kept) WM_TAP_HIP(s, hipMemcpyAsync(out_kept + r0, sd.kept, n * sizeof(int), hipMemcpyDeviceToHost, st));
        return WM_OK;
    });
}
extern "C" int wm_sample_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, const wm_sample_params* sp, int R,
                              const float* logits, const int32_t* prefixes, int Tmax, const int32_t* lens, const uint64_t* keys,
                              int32_t* out_token, float* out_value, int32_t* out_forced)
{
    return wm_sample_rows_impl(ctx, "wm_sample_rows", gp, tsp, sp, nullptr, R, logits, prefixes, Tmax, lens, keys, nullptr, nullptr, out_token, out_value, out_forced);
}
extern "C" int wm_filter_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* tsp, const wm_sample_params* sp, const wm_sample_filter* f,
                              int R, const float* logits, const int32_t* prefixes, int Tmax, const int32_t* lens, const uint64_t* keys,
                              float* out_thr, int32_t* out_kept, int32_t* out_forced, int32_t* out_token, float* out_value)
{
    if (ctx && (!f || !out_thr || !out_kept)) { ctx->err = "wm_filter_rows: bad arguments"; return WM_ERR_ARG; }
    return wm_sample_rows_impl(ctx, "wm_filter_rows", gp, tsp, sp, f, R, logits, prefixes, Tmax, lens, keys, out_thr, out_kept, out_token, out_value, out_forced);
}

// forward(): one decoder pass over T tokens per stream at positions pos0.., K/V appended at row pos0.
// Uses (and overwrites) the decode-loop state: call it before wm_decode_begin, or begin again afterwards.
extern "C" int wm_forward_logits(wm_ctx* ctx, int B, const int32_t* tokens, int T, int pos0, int disable_medusa, float* logits_out)
{
    if (!ctx || !tokens || !logits_out || B < 1 || B > ctx->Benc || T < 1 || T > 16 || pos0 < 0 || pos0 + T > ctx->Tmax) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int Tids = ctx->Tal, K = ctx->K, V = ctx->V, nout = disable_medusa ? 1 : K + 1;
    GenDev g = ctx->gp;
    g.K = K; g.V = V; g.Vpad = ctx->Vpad; g.Tids = Tids; g.vanilla = 0;
    ctx->gp = g;
    wm_decode_invalidate(ctx, true);        // (drops both graph slots, as ever)
    std::vector<float> rowbuf((size_t)nout * ctx->Vpad);
    for (int b = 0; b < B; ++b) {
        std::vector<int> v(T);
        for (int i = 0; i < T; ++i) v[i] = tokens[(size_t)b * T + i];
        const int kv = pos0, L = pos0 + T;
        WM_HIP(hipMemcpyAsync(ctx->ids + (size_t)b * Tids + pos0, v.data(), T * sizeof(int), hipMemcpyHostToDevice, st));
        WM_HIP(hipMemcpyAsync(ctx->kvlen + b, &kv, sizeof(int), hipMemcpyHostToDevice, st));
        WM_HIP(hipMemcpyAsync(ctx->L + b, &L, sizeof(int), hipMemcpyHostToDevice, st));
        WM_HIP(hipStreamSynchronize(st));
        int rc = wm_dec_stage_layers(ctx, b, 1, T, 0);
        if (rc) return rc;
        rc = wm_dec_stage_final(ctx, b, 1, T, 0, !disable_medusa);
        if (rc) return rc;
        for (int r = 0; r < T; ++r) {
            rc = wm_dec_stage_heads(ctx, 1, 1, r, !disable_medusa);
            if (rc) return rc;
            WM_HIP(hipMemcpyAsync(rowbuf.data(), ctx->logits, rowbuf.size() * sizeof(float), hipMemcpyDeviceToHost, st));
            WM_HIP(hipStreamSynchronize(st));
            for (int k = 0; k < nout; ++k)      // out layout [n_out][B][T][V]
                std::memcpy(logits_out + (((size_t)k * B + b) * T + r) * V, rowbuf.data() + (size_t)k * ctx->Vpad, (size_t)V * sizeof(float));
        }
    }
    return WM_OK;
}

extern "C" int wm_profile_kernel(wm_ctx* ctx, int kernel, int rows, int reps, float* ms, double* bytes)
{
    if (!ctx || !ms || !bytes || reps < 1) return WM_ERR_ARG;
    WM_HIP(hipSetDevice(ctx->device));
    return wm_dec_profile(ctx, kernel, rows, reps, ms, bytes);
}
