// wm_internal.h — engine context and internal interfaces shared by the translation units of libwm.so.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/wm.h"
#include "wm_common.h"

#define WM_HIP(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            ctx->err = std::string(#expr) + ": " + hipGetErrorString(_e);                   \
            return WM_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)

struct EncLayerW {
    const float *ln1_w, *ln1_b, *qkv_b, *out_b, *ln2_w, *ln2_b, *fc1_b, *fc2_b;
    const bf16_t *qkv_w, *out_w, *fc1_w, *fc2_w;
    // fp8 MFMA encoder (wm_config.enc_fp8): e4m3 copies of the LayerNorm-fed matrices in the 64-k unit layout + per-row scales
    const unsigned char *qkv_w8 = nullptr, *fc1_w8 = nullptr;
    const float *qkv_ws = nullptr, *fc1_ws = nullptr;
};
struct DecLayerW {
    const float *ln1_w, *ln1_b, *qkv_b, *out_b, *ln2_w, *ln2_b, *cq_b, *cout_b, *ln3_w, *ln3_b, *fc1_b, *fc2_b;
    const bf16_t *qkv_w, *out_w, *cq_w, *cout_w, *fc1_w, *fc2_w;     // packed bf16 — or packed fp8 e4m3 when the scales below are set
    const float *qkv_s = nullptr, *out_s = nullptr, *cq_s = nullptr, *cout_s = nullptr, *fc1_s = nullptr, *fc2_s = nullptr;
    // LayerNorm folded into the three LayerNorm-fed GEMMs (wm_common.h; computed in wm_create by wm_dec_fold_init): c = W gamma, bf = b + W beta
    const float *qkv_c = nullptr, *qkv_bf = nullptr, *cq_c = nullptr, *cq_bf = nullptr, *fc1_c = nullptr, *fc1_bf = nullptr;
    // ... and the gains the producers of the folded operand multiply by: gamma * 2^-s with rs = 2^s applied to rstd by the consumer (wm_common.h FoldIn)
    const float *ln1_g = nullptr, *ln2_g = nullptr, *ln3_g = nullptr;
    float ln1_rs = 1.0f, ln2_rs = 1.0f, ln3_rs = 1.0f;
};

// scalars every decode kernel may need (passed by value)
struct GenDev {
    int P, eos, pad, max_length, hard_max_length, exp_start /* absolute: start + P, or -1 */;
    float thr, alpha, inv_temp;
    int accept_mode, vanilla, K, V, Vpad, Tids, fuse, force_accept;
    int begin;      // sequence length at which the begin-suppress list applies (wm_gen_params.begin_index; P when that is < 0)
    int sib;        // sibling rows of this decode's verify pass (wm_config.sibling_rows; 0 unless one stream, chain candidates, hidden-state carry)
};

// Whisper timestamp rules (wm_decode_begin_ts; HF WhisperTimeStampLogitsProcessor).  Passed by value as the trailing
// argument of the *_ts select / candidate / accept kernels (the plain kernels keep their arguments and code).
//   state  int4 per stream: {last sampled token is a timestamp, penultimate one is, last timestamp token or -1, sampled tokens} of ids[begin:L]
//   record int4 per logits row: {lo, hi, flags, 0}: timestamps outside [lo, hi] masked; flags bit 0 masks [0, eos), bit 1 masks [0, tb)
struct TsDev {
    int on, tb, nots, mit;          // timestamp_begin, <|notimestamps|>, max_initial_timestamp_index (< 0: none)
    int4* st;                       // [maxB] committed state (k_accept / k_accept_vanilla1 keep it current)
    int4* ver;                      // [max(maxB, Rcap)][WM_CAND_STRIDE] records of the verify rows (k_cand_fin folds c_0..c_i)
    float* part1t;                  // [Rcap][SEL_SP][4] timestamp-region slice partials {max, first argmax, sum exp at 1/T, sum exp at 1}
    int* forced;                    // [Rcap] the row's log-softmax decision masked all text (k_select2 / k_select_argmax)
    const int* L;                   // ctx->L (k_cand_fin: prefix length of verify row i is L + i + 1)
    // repetition rules (wm_set_repeat_rules): ride in the same kernel family (launched when on || rp).  Nothing is kept per
    // stream: every select / score block derives its slice of the two token sets from the row's prefix ids (wm_select.h rp_build)
    int rp;                         // bit 0: repetition penalty, bit 1: no-repeat n-gram
    float rp_pen; int rp_g;
    const int* rp_ids; int rp_stride;   // prefix of stream s: rp_ids + s * rp_stride, cur_len ids (decode: ctx->ids; scoring: offset in the row's record .w)
    const int* rp_len;              // tap (wm_select_rows): row i follows rp_ids + i * rp_stride, rp_len[i] ids; else NULL
    const int* rp_cand;             // verify row i of stream s also follows rp_cand[s * WM_CAND_STRIDE + 0 .. i]
    int* rp_flags;                  // scoring: [rows] the target's bits (1 penalised, 2 banned), k_score1 -> k_score2
};
// the rules kernel family (*_ts) runs when the timestamp rules or the repetition rules are on
static inline bool wm_rules_on(const TsDev& t) { return t.on || t.rp; }

// Seeded sampling on the plain decode path (wm_set_sampling).  Passed by value to k_sample1 / k_sample_fin, which stand in for
// k_select1* / k_select_argmax* in the vanilla branch of wm_dec_iteration while sampling is on; nothing else reads it (the scalars: DecGraphKey).
struct SampDev {
    int on; float inv_t;                // fl(1 / temperature): the sampling temperature (GenDev.inv_temp stays typical acceptance's)
    unsigned seed_lo, seed_hi;          // Philox key
    const unsigned long long* keys;     // DEV [rows] the 64-bit stream key of every row (counter words 2 and 3)
    float* part;                        // [Rcap][SEL_SP][8] slice partials {max text, perturbed max text, its id, max ts, sum exp ts at 1, perturbed max ts, its id, 0}
    float* val;                         // [Rcap] the winner's perturbed value (wm_sample_rows reads it)
    // top-k / top-p / min-p filters (wm_set_sampling_filter): off = 0, 1, 0.  k_filter_prep / k_filter_row read them
    int top_k; float top_p, min_p;
    float* fv;                          // [max(maxB, 16)][Vpad] the processed row after the decision
    float* thr; int* kept;              // [Rcap] the row's threshold and the number of region ids at or above it (wm_filter_rows reads them)
};
static inline bool wm_filter_on(const SampDev& sd) { return sd.top_k > 0 || sd.top_p < 1.0f || sd.min_p > 0.0f; }

// Beam search on the plain decode path (wm_set_beam; csrc/wm_beam.hip).  Passed by value to the k_beam_* kernels, which stand in for
// k_select1* / k_select_argmax* / k_accept_vanilla1* in the vanilla branch of wm_dec_iteration while beams are on; nothing else reads it.  Stream
// s = g * n + j is beam j of clip g.  The buffers belong to wm_beam_state (allocated on first use, sized for max_batch streams).
struct BeamDev {
    int on, n, G, es;               // beams per clip, clips, early_stopping (0 False, 1 True, 2 "never")
    int lp_pos;                     // length_penalty > 0 ("never": the best length is max_length - P)
    int rows_cap;                   // K/V rows per (kv layer, stream, head) of the shadow buffer (a multiple of 32)
    float* run;                     // [G * n] running scores
    float* cval; int* cbeam; int* ctok;                             // [G][2n] the step's ordered candidates
    float* fscore; int* fset; int* flen; int* fids;                 // finished table: [G][n] score, set, length; [G][n][Tids] ids
    int* heur; int* cdone;          // [G] early-stop heuristic flag (1 = improvement possible), clip done
    int* bidx; int* ntok;           // [G * n] source stream / next token of every stream (ntok < 0: the stream does not step)
    float* lse;                     // [rows][SEL_SP][2] slice partials {max, sum exp} of the raw row
    float* reg;                     // [rows][SEL_SP][4] slice partials of the processed row {max text, max timestamps, their sum exp, 0}
    float* sval; int* stok;         // [rows][SEL_SP][2 * WM_BEAM_MAX] slice candidates (accumulated value, token; token -1: none)
    const float* den;               // [Tids + 2] fl(t ** length_penalty)
    int* sh_ids; int4* sh_st;       // shadow of the ids rows [G * n][Tids] and of the committed timestamp states
    bf16_t* sh_kv;                  // shadow of the self K/V: K [nkv][G * n][H][rows_cap][64], then V the same
};

// Sequence bias on the plain decode path (wm_set_sequence_bias; csrc/wm_seq_bias.hip).  Passed by value to k_seq_bias, which edits
// the fp32 logits rows in place before k_select1* / k_sample1 / the k_beam_* select kernels read them; nothing else reads it.  The tables belong to
// wm_seq_bias_state (allocated once at their maximum size: the addresses never change); `on` and `ngroups` ride in the launch, so they are part of
// DecGraphKey (below).  Entries are stored in group order: group g = entries [gstart[g], gstart[g + 1]) that end in token gtok[g].
struct SeqBiasDev {
    int on, ngroups;
    const int* gtok;                // [ngroups] the group's target token (distinct)
    const int* gstart;              // [ngroups + 1]
    const int* elen;                // [entries] m
    const float* ebias;             // [entries]
    const int* etok;                // [entries][WM_SEQ_BIAS_MAX_LEN] the entry's first m - 1 ids
};

// Constrained decoding on the plain decode path (wm_set_constraint; csrc/wm_constraint.hip).  Passed by value to k_constraint, which
// masks the fp32 logits rows in place right behind k_seq_bias; nothing else reads it.  The two copies of the sorted table belong to
// wm_constraint_state (allocated once at their maximum size: the addresses never change); `on` and `n` ride in the launch, so they are part of
// DecGraphKey (below).
struct ConstraintDev {
    int on, n;                      // sequences
    const int* rowmaj;              // [n][WM_CONSTRAINT_MAX_LEN + 1] the sorted sequences, each closed by -2 and padded with -1
    const int* colmaj;              // [WM_CONSTRAINT_MAX_LEN + 1][n] the same, transposed
};

// What a captured decode graph was captured with: every scalar its launches carry by value.  wm_decode_begin_ts keeps the graphs of a slot (below)
// exactly when the decode's key equals the slot's.  A new scalar passed by value to a captured launch is added HERE (the struct and
// wm_dec_graph_key) and nowhere else.  Buffer pointers stay out: every buffer the launches name is allocated once per context, at its max_batch size,
// and never moves — except the beam shadow K/V, which grows with the call (wm_beam_begin).  The equality is a memcmp: no padding (asserted).
struct DecGraphKey {
    const void* sh_kv; int beam_on, n, G, es, lp_pos, rows_cap;         // BeamDev (all zero without beams)
    GenDev g; int B;                                                    // B: streams (beams: clips x beams)
    int ts_on, tb, nots, mit, rp; float rp_pen; int rp_g;               // TsDev
    int samp_on; float inv_t; unsigned seed_lo, seed_hi;                // SampDev (all zero while sampling is off)
    int top_k; float top_p, min_p;                                      // SampDev's filter (all zero while sampling is off; off: 0, 1, 0)
    int sb_on, ngroups;                                                 // SeqBiasDev
    int cons_on, cons_n;                                                // ConstraintDev (an even number of words: no tail padding)
};
static_assert(sizeof(GenDev) == 19 * 4 && sizeof(DecGraphKey) == sizeof(void*) + sizeof(GenDev) + 25 * 4, "DecGraphKey must have no padding");
static inline bool operator==(const DecGraphKey& a, const DecGraphKey& b) { return std::memcmp(&a, &b, sizeof(DecGraphKey)) == 0; }
static inline DecGraphKey wm_dec_graph_key(const GenDev& g, int B, const TsDev& ts, const SampDev& sd, const SeqBiasDev& sbd, const ConstraintDev& cd,
                                           const BeamDev& bd)
{
    DecGraphKey k{};
    k.g = g; k.B = B; k.sb_on = sbd.on; k.ngroups = sbd.ngroups; k.cons_on = cd.on; k.cons_n = cd.n;
    k.ts_on = ts.on; k.tb = ts.tb; k.nots = ts.nots; k.mit = ts.mit; k.rp = ts.rp; k.rp_pen = ts.rp_pen; k.rp_g = ts.rp_g;
    if (sd.on) { k.samp_on = sd.on; k.inv_t = sd.inv_t; k.seed_lo = sd.seed_lo; k.seed_hi = sd.seed_hi; k.top_k = sd.top_k; k.top_p = sd.top_p; k.min_p = sd.min_p; }
    if (bd.on) { k.beam_on = bd.on; k.n = bd.n; k.G = bd.G; k.es = bd.es; k.lp_pos = bd.lp_pos; k.rows_cap = bd.rows_cap; k.sh_kv = bd.sh_kv; }
    return k;
}
// The captured graphs of one kind of decode and their key.  step: one steady-state iteration / merged step / beam step (single-stream carry path:
// what follows the base pass); base: that path's base pass.  drop() is the only place a graph is destroyed (hidden: it adds no exported symbol)
struct DecGraphSlot {
    DecGraphKey key{};
    hipGraphExec_t step = nullptr, base = nullptr;
    __attribute__((visibility("hidden"))) void drop() { for (hipGraphExec_t* x : {&step, &base}) if (*x) { (void)hipGraphExecDestroy(*x); *x = nullptr; } }
};

// state after one more sampled token / the record of a row whose sampled prefix has state `st` (host: wm_decode_begin_ts, device: the select kernels)
__host__ __device__ __forceinline__ int4 ts_fold(int4 st, int tok, int tb)
{
    st.y = st.x;                                // penultimate <- last
    st.x = tok >= tb ? 1 : 0;
    if (tok >= tb) st.z = tok;
    st.w += 1;
    return st;
}
// record of a row whose sampled prefix (ids[begin:len]) has state `st`
__host__ __device__ __forceinline__ int4 ts_record(int4 st, int len, int begin, int tb, int V, int mit)
{
    const bool last = st.w >= 1 && st.x, penult = st.w < 2 || st.y;
    int lo = tb, hi = V - 1, fl = 0;
    if (last) { if (penult) lo = V; else fl |= 1; }          // pairs: after ts,ts text only; after text,ts no text below EOS
    if (st.z >= 0) lo = std::max(lo, (last && !penult) ? st.z : st.z + 1);     // never decreasing, <|0.00|> not again
    if (len == begin) { fl |= 2; if (mit >= 0) hi = std::min(hi, tb + mit); }  // first sampled token: a timestamp <= max_initial
    return make_int4(lo, hi, fl, 0);
}
// A device buffer that only grows: reserve(n) keeps the allocation while it holds n elements, else frees it and allocates anew (the contents
// are not carried over).  Converts to its pointer; freed with its owner.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    operator T*() const { return p; }
    hipError_t reserve(size_t n)
    {
        if (p && n <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
};

// Static tables of the candidate tree (device memory; medusa_utils.py:305-421).  Nodes are numbered depth by depth.
struct TreeDev {
    int n_nodes, n_paths, K, pad_;
    int topk[16];           // c_k of logits row k (row 0 = base head: 1)
    int start[17];          // first node of depth i
    int cumprod[16];        // nodes at depth i
    int depth[WM_TREE_MAX_NODES];                   // medusa_position_ids
    unsigned long long anc[WM_TREE_MAX_NODES];      // bit n of anc[m]: node n is m or one of its ancestors (rows of medusa_attn_mask)
    int parent[WM_TREE_MAX_NODES];
    int children[WM_TREE_MAX_NODES][4];             // -1 padded
    int retrieve[WM_TREE_MAX_PATHS][16];            // [path][depth] -> node (retrieve_indices)
};

// What every launch of a decode pass is given besides its own operands (wm_skinny_gemm.h launchers, wm_decoder.hip).  One per context
// (wm_ctx::lp): the entry points of wm_decoder.hip that start a pass write done / ntiles, the stage functions called after them read it.
struct DecLaunch {
    hipStream_t st = nullptr;           // the context's stream
    const int* done = nullptr;          // device flag every kernel of the pass checks on entry (all streams finished); nullptr: none
    const int* ntiles = nullptr;        // merged-step schedule: device word = 16-row token tiles that hold rows in this step; nullptr: all tiles
#ifdef WM_TIMELINE
    int tl_tag = 0;                     // timeline build: tag of the next launch (TL_SET / TL_PASS)
#endif
};

struct wm_ctx {
    wm_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DecLaunch lp;                       // launch state of the decode pass being enqueued (lp.st == stream)
    std::string err;

    // derived sizes
    int d = 0, H = 0, ffn = 0, V = 0, Vpad = 0, S = 0, Spad = 0, Tm = 0 /* mel frames 2S */, Tmpad = 0;
    int Tmax = 0 /* n_tgt */, Tal = 0 /* cache rows allocated */, K = 0, nkv = 0, nres = 0, maxB = 0;
    bool block = false;
    int NS = 1;         // cross-attention key splits (256 keys per block)
    int Rcap = 16;      // token-row capacity of the decode scratch (16 rows per stream; a candidate tree of more than 16 nodes: its node count rounded up to 16)
    int Mmax = 16;      // rows per stream a pass may carry

    // ---- parameters (pointers into the caller's blob) ----
    const float *win = nullptr, *twiddle = nullptr, *melfb = nullptr;
    const bf16_t *conv1_w = nullptr, *conv2_w = nullptr;
    const float *conv1_b = nullptr, *conv2_b = nullptr, *enc_pos = nullptr, *enc_lnf_w = nullptr, *enc_lnf_b = nullptr;
    const bf16_t *tok_emb = nullptr, *vocab_w = nullptr, *heads_w = nullptr, *ckv_w = nullptr;
    const float *dec_pos = nullptr, *dec_lnf_w = nullptr, *dec_lnf_b = nullptr, *heads_b = nullptr, *ckv_b = nullptr;
    std::vector<EncLayerW> enc;
    std::vector<DecLayerW> dec;       // nkv entries (last = medusa_block for Block)

    // ---- encoder scratch (sized for maxB clips) ----
    float* feats_own = nullptr;       // [B][n_mels][Tm]
    float* clipmax = nullptr;         // [B] ordered-int encoded
    bf16_t* A1 = nullptr;             // packed [B*Tmpad][K1pad]
    bf16_t* a1 = nullptr;             // [B][Tm][d] bf16
    bf16_t* A2 = nullptr;             // packed [B*Spad][3d]
    float* eh = nullptr;              // [B*Spad][d] fp32 residual
    bf16_t* exn = nullptr;            // packed [B*Spad][d]
    bf16_t *eq = nullptr, *ek = nullptr, *evt = nullptr;   // [B][H][Spad][64] / vt [B][H][64][Spad]
    bf16_t* eff = nullptr;            // packed [B*Spad][ffn]
    bf16_t* enc_out = nullptr;        // packed [B*Spad][d]
    int K1pad = 0;
    bool enc_f8 = false;              // fp8 MFMA encoder path
    unsigned char* exn8 = nullptr;    // packed fp8 [B*Spad][d] (LayerNorm output as e4m3)
    float* exs = nullptr;             // [B*Spad] row scales of exn8
    const unsigned char* ckv_w8 = nullptr; const float* ckv_ws = nullptr;

    // ---- caches ----
    bf16_t *kx = nullptr, *vx = nullptr;   // cross K/V [nkv][Benc][H][Spad][64]
    // wm_config.cross_kv_fp8: e4m3 copies (K row-major [Spad][64] bytes; V^T fragments with the dim-tile pairs of a lane adjacent:
    // [Spad/32][2][64 lanes][16 B]) + one fp32 scale per (kv layer, stream, head) each; written by wm_enc_quant_cross_kv
    unsigned char *kx8 = nullptr, *vx8 = nullptr; float *kxs = nullptr, *vxs = nullptr;
    bool xkv8 = false;
    bf16_t *kc = nullptr, *vc = nullptr;   // self K/V  [nkv][maxB][H][Tal][64]
    int Benc = 0;                          // batch of the last wm_encode

    // ---- decode row scratch (<= WM_MAX_ROWS_SKINNY rows per chunk) ----
    float *h = nullptr, *hblk = nullptr, *hf = nullptr, *qbuf = nullptr;    // hf: [maxB*16][d] post-final-LN rows
    float *hb_keep = nullptr;                                               // Medusa-Block: carried block-layer output row per stream
    float *hf_cur = nullptr, *hf_keep = nullptr;                            // current chunk's rows; carried row per stream
    int* carry = nullptr;                                                   // [maxB] next base pass is redundant
    // merged-step schedule (several streams, chain candidates; wm_decoder.hip wm_dec_step): per step and stream, written by k_step_begin
    int4* rowinfo = nullptr;                                                // [Mmax * maxB] dense rows of the step's pass: {stream, index inside the stream, position of its row 0, kind 0 none / 1 base / 2 verify}
    int4* sinfo = nullptr;                                                  // [maxB] {first dense row, row count, position of row 0, mode}
    int* steprows = nullptr;                                                // [4] {dense rows of the pass, their 16-row tiles, 0, 0}
    bool step_flow = false;
    // candidate tree (medusa_choices with top-k > 1); tn == 0: the chain
    int tn = 0, tp = 0;
    TreeDev tree_host{};
    TreeDev* tree = nullptr;
    TreeDev* sibtree = nullptr;     // wm_config.sibling_rows: depth / ancestor tables of the chain + S leaves under the root (nodes K+1 .. K+S)
    int sib_cfg = 0;                // S the context was created for (0: off)
    float2* sibpart = nullptr;      // [maxB][SEL_SP slices][6] (value, token): the slice winners of head 1's row (k_select1 -> k_cand_fin)
    const unsigned long long* cur_anc = nullptr;                            // ancestor masks of the pass being enqueued (verify pass of a tree)
    int *sel_src = nullptr, *sel_n = nullptr, *sel_base = nullptr;          // K/V rows of the chosen path to move: [maxB*16], [maxB], [maxB]
    bool fuse = true;
    bool host_carry = false;                                                // single-stream runs: the host skips the base pass
    float* rs_table = nullptr; int rs_og = 0, rs_nw = 0, rs_width = 0;     // cached resampling filter bank [taps][phases]
    bool dev_carry = false;                                                 // several streams: per-stream carry flags on the device
    int *hostflags = nullptr, *hostflags_dev = nullptr;                     // host-mapped {carry, finished}
    bf16_t *xbuf = nullptr, *fbuf = nullptr, *ybuf = nullptr;
    // LayerNorm fold (round 6): operand gamma o x of the next LayerNorm-fed GEMM (hi / lo planes, written by the launch that produced x), the
    // rows' statistics partials [d / 16 tiles][Rcap rows] and the fold vectors of every decoder layer; WM_LN_FOLD=0 keeps the LayerNorm launches
    bf16_t* xn = nullptr; float2* lnstats = nullptr; float* foldv = nullptr;
    bool ln_fold = false;
    float *cml = nullptr, *co = nullptr;   // cross-attention partials
    int* ticket = nullptr;                 // [16 streams][H] arrival tickets of the cross-attention key splits
    float* logits = nullptr;               // [32][Vpad]
    int* amax = nullptr; float *pc = nullptr;                   // select outputs, [maxB*16]
    float *part1 = nullptr, *part2 = nullptr;                   // select slice partials [16][SEL_SP][4] / [maxB*16][SEL_SP]

    // ---- decode state ----
    int *ids = nullptr, *L = nullptr, *kvlen = nullptr, *finished = nullptr, *cand = nullptr, *niter = nullptr;
    long long* hist = nullptr;             // [16] accept histogram + [16]=tokens emitted
    unsigned char* supmask = nullptr;      // [Vpad] bit0 suppress, bit1 begin-suppress
    float* exppen = nullptr;               // [Tids+1] (factor^(t-start) - 1) as float
    int* tap_tok = nullptr;
    int* done = nullptr;                   // [0] = all streams finished, [1] = number of finished streams
    bool use_done = false;
    // gp / ts / samp / sbias / cons / beam: the scalars of the decode or call in flight, nothing else (the graphs' keys live in the slots below)
    GenDev gp{};
    TsDev ts{};                            // timestamp rules (ts.on = 0: off); buffers allocated in wm_create
    wm_repeat_params rep{1.0f, 0};         // wm_set_repeat_rules: sticky until cleared (neutral = off)
    // wm_set_sampling: sticky until cleared.  samp_set = what the caller gave (keys copied to the host vector; empty: 0 .. B - 1), samp = the
    // current decode's (on = 0: off); its buffers (part, val, samp_keys) are allocated in wm_create
    bool samp_set_on = false; float samp_set_temp = 1.0f; uint64_t samp_set_seed = 0; std::vector<uint64_t> samp_set_keys;
    // wm_set_sampling_filter: sticky until cleared, read only while sampling is on (a decode that does not sample refuses it)
    bool samp_filter_on = false; wm_sample_filter samp_filter{0, 1.0f, 0.0f};
    SampDev samp{};
    unsigned long long* samp_keys = nullptr;    // [max(maxB, 16)]
    // wm_set_beam: sticky until cleared.  beam = the current decode's (on = 0: off); its buffers live in beam_state
    bool beam_set_on = false; wm_beam_params beam_set{};
    BeamDev beam{};
    struct wm_beam_state* beam_state = nullptr;
    int beam_clips = 0;                         // G of the current beam decode
    bool beam_expanded = false;                 // the cross K/V sits replicated (slot g * n + j); wm_decode_run / wm_decode_invalidate move it back
    bool beam_done = false;                     // the last decode was a beam decode and all its clips are done (wm_get_beam_result)
    // wm_set_sequence_bias: sticky until cleared.  seq_bias_state: the device tables and the host copy of what the caller set; sbias: this decode's
    struct wm_seq_bias_state* seq_bias_state = nullptr;
    SeqBiasDev sbias{};
    // wm_set_constraint: sticky until cleared.  cons_state: the device tables and the host copy of what the caller set; cons: this decode's
    struct wm_constraint_state* cons_state = nullptr;
    ConstraintDev cons{};
    // wm_set_stream_prompts: sticky until cleared.  The rows [sp_B][sp_P] of the clips' prompts (empty: off, every stream starts from wm_gen_params.prompt);
    // wm_decode_begin_ts checks them against its decode and seeds ctx->ids / ctx->ts.st from them.  Nothing on the device: no launch carries them
    std::vector<int32_t> sp_rows; int sp_B = 0, sp_P = 0;
    // language detection (wm_lang.hip): the candidate ids [WM_LANG_MAX] and the picks [max(maxB, 16)] of k_lang_pick, allocated in wm_create
    int *lang_ids = nullptr, *lang_out = nullptr;
    // wm_merge_windows (wm_merge.hip): its workspace and event pair, allocated on first use; nothing of the decode state
    struct wm_merge_state* merge_state = nullptr;
    // wm_set_word_table / wm_word_spans (wm_words.hip): the vocabulary's bytes, a workspace and an event pair of their own; nothing of the decode state
    struct wm_words_state* words_state = nullptr;
    // wm_vad_windows (wm_vad.hip): its workspace and event pair, allocated on first use; nothing of the decode state
    struct wm_vad_state* vad_state = nullptr;
    // wm_stream_agree (wm_stream.hip): its workspace and event pair, allocated on first use; nothing of the decode state
    struct wm_stream_state* stream_state = nullptr;
    int Bdec = 0;
    bool began = false, first_done = false;
    long long iters = 0;
    // a decode with beams works on graphs_beam, every other on graphs_plain: a key that differs drops that slot alone, each survives the other's calls
    DecGraphSlot graphs_plain, graphs_beam;
    int graph_replays = 0;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool prefetch = true;           // in-launch next-operand prefetch blocks (WM_PREFETCH=0 turns them off)
    float ms_logmel = 0.f, ms_encode = 0.f, ms_decode = 0.f;

    // ---- token timestamps (wm_align.hip): workspace of the last wm_token_timestamps call, allocated on first use ----
    struct wm_align_state* align = nullptr;
    DevBuf<int> tap_buf;            // parity taps: a row group's prefixes and lengths (wm_tap_stage below); grows on first use, freed with the context
    struct wm_score_state* score = nullptr;     // token log-probabilities (wm_score.hip): row descriptors, slice partials and outputs, allocated on first use
    bool replay = false;            // a teacher-forced replay pass is being enqueued: the cross-q launch must leave its fp32 rows in qbuf (no WM_FUSE_CQ)
};

// implemented in wm_encoder.hip
long wm_enc_resample_len(long n_in, int sr_in, int sr_out);
int wm_enc_resample(wm_ctx* ctx, const float* in, int B, int channels, int n_in, int sr_in, int sr_out, float* out);
int wm_enc_logmel(wm_ctx* ctx, const float* wav, int B, int n_samples, float* feats);
int wm_enc_encode(wm_ctx* ctx, const float* feats, int B);
int wm_enc_set_output(wm_ctx* ctx, const float* hidden, int B);
int wm_enc_quant_cross_kv(wm_ctx* ctx, int B);      // cross_kv_fp8: the e4m3 copy of the projected cross-K/V of B streams
// implemented in wm_decoder.hip
int wm_dec_stage_layers(wm_ctx* ctx, int b0, int nb, int Mper, int mode /*0 base, 1 verify*/);
int wm_dec_stage_final(wm_ctx* ctx, int b0, int nb, int Mper, int mode, int medusa);
int wm_dec_stage_heads(wm_ctx* ctx, int nsel, int sel_mul, int sel_off, int medusa);
int wm_dec_pass(wm_ctx* ctx, int b0, int nb, int Mper, int mode, int medusa, int all_rows);
int wm_dec_iteration(wm_ctx* ctx, int Mper_base);   // one full iteration over all streams
int wm_dec_prompt_prefix(wm_ctx* ctx, int P);       // K/V of a long prompt's leading chunks; returns the tokens left (<= 16), < 0 on error
int wm_dec_iter_base(wm_ctx* ctx, int Mper_base);   // base pass layers + final LN
int wm_dec_iter_rest(wm_ctx* ctx, int Mper_base);
int wm_dec_step(wm_ctx* ctx, int);   // heads, candidates, verify pass, accept
int wm_dec_profile(wm_ctx* ctx, int kernel, int rows, int reps, float* ms, double* bytes);
int wm_dec_fold_init(wm_ctx* ctx);   // c = W gamma, b' = b + W beta of every LayerNorm-fed decoder GEMM (needs ctx->foldv)
// Teacher-forced replay (token timestamps: wm_align.hip; token log-probabilities: wm_score.hip).  Input positions [0, npos) of streams
// [b0, b0 + nb) go through embed + decoder layers [0, n_layers) in 16-row tiles, exactly the launches of a base pass.  The ids (tokens HOST
// [.][Tmax], lens HOST, indexed by stream; zero past a stream's length: computed and ignored) are uploaded at the context's stride; a tile
// sets kvlen to its first position pos0 and runs Mper = min(16, npos - pos0) rows.  Hooks (may be null): layer(ctx, l, pos0, Mper, arg)
// behind layer l, while ctx->qbuf still holds its cross-attention query rows (fp32 [nb * Mper][d], scaled by 0.125); tile(ctx, pos0, Mper,
// arg) behind the tile's last layer.  The caller has called wm_decode_invalidate and holds a wm_scalars_swap (below).
struct wm_replay_hooks {
    int (*layer)(wm_ctx*, int, int, int, void*) = nullptr;
    int (*tile)(wm_ctx*, int, int, void*) = nullptr;
    void* arg = nullptr;
};
int wm_dec_replay(wm_ctx* ctx, int b0, int nb, const int32_t* tokens, int Tmax, const int32_t* lens, int npos, int n_layers, const wm_replay_hooks& hooks);
// a replay call's streams against the last encode: B <= Benc, lens in [1, min(Tmax, n_tgt)], n_prompt in [min_prompt, lens]; errors under `who`
int wm_replay_check(wm_ctx* ctx, const char* who, int B, int Tmax, const int32_t* lens, const int32_t* n_prompt, int min_prompt);
// implemented in wm_sample.hip: k_sample1 + k_sample_fin over `nrows` rows of ctx->logits, row r at position pos[r] (DEV), keys sd.keys[r]; the token goes
// to ctx->amax[out_row0 + r], the decision to ts.forced[out_row0 + r] (rules on), the winner's perturbed value to sd.val[out_row0 + r].  tap = 0: row r
// is stream r of the decode (record from ts.st[r], prefix ids of stream r); 1: a tap row (record ts.ver[r], prefix ts.rp_ids + r * ts.rp_stride)
int wm_sample_launch(wm_ctx* ctx, const GenDev& gp, const TsDev& ts, const SampDev& sd, const int* pos, int nrows, int out_row0, int tap);
// implemented in wm_beam.hip (beam search on the plain decode path; include/wm.h wm_set_beam)
int wm_beam_check(wm_ctx* ctx, const char* who, const wm_beam_params* bp);      // the parameter checks of wm_set_beam
// the device form of a beam request over G clips: allocates / grows the state (shadow K/V only with `kv`), uploads the length-penalty table and
// resets the running scores (init_scores HOST [G * n] or NULL: [0, -1e9, ..] per clip), the finished table (entries of len0 ids, not set) and the
// flags.  Ends with the stream idle.  wm_beam_seed_table: the table's ids rows start as the streams' ids rows (after the caller has uploaded ctx->ids).
int wm_beam_begin(wm_ctx* ctx, const wm_beam_params& bp, int G, const GenDev& g, bool kv, const float* init_scores, int len0, BeamDev* out);
int wm_beam_seed_table(wm_ctx* ctx, const BeamDev& bd);
// one beam step behind the base pass: select (rows = streams of ctx->logits, lengths ctx->L), bookkeeping, reorder (self K/V only with `kv`)
int wm_beam_step(wm_ctx* ctx, const GenDev& gp, const TsDev& ts, const BeamDev& bd, bool kv);
int wm_beam_expand(wm_ctx* ctx, int G, int n);      // cross K/V of clip g: slot g -> slots g * n .. g * n + n - 1; Benc becomes G * n
int wm_beam_compact(wm_ctx* ctx);                   // and back (slot g * n -> g) when it sits expanded; Benc becomes G again
void wm_beam_free(wm_ctx* ctx);
// implemented in wm_seq_bias.hip (sequence bias on the plain decode path; include/wm.h wm_set_sequence_bias)
// the device form of the context's sticky table for a decode that begins: on = 0 when none is set.  Checks what only the decode knows (the path, the
// candidate tree, eos against the -inf entries; errors under `who`).
int wm_seq_bias_begin(wm_ctx* ctx, const char* who, const wm_gen_params* gp, SeqBiasDev* out);
// k_seq_bias over `nrows` rows of ctx->logits: row r under the prefix ids + r * ids_stride of lens[r] ids (DEV; clamped to [0, len_cap])
int wm_seq_bias_launch(wm_ctx* ctx, const SeqBiasDev& sb, const int* ids, int ids_stride, const int* lens, int len_cap, int nrows);
void wm_seq_bias_free(wm_ctx* ctx);
// implemented in wm_constraint.hip (constrained decoding on the plain decode path; include/wm.h wm_set_constraint)
// the device form of the context's sticky table for a decode that begins: on = 0 when none is set.  Checks what only the decode knows (the path, the
// candidate tree, the timestamp rules, the exponential decay, eos and the suppress lists against the sequences; errors under `who`).
int wm_constraint_begin(wm_ctx* ctx, const char* who, const wm_gen_params* gp, const wm_timestamp_params* tsp, ConstraintDev* out);
// k_constraint over `nrows` rows of ctx->logits: row r under the prefix ids + r * ids_stride of lens[r] ids (DEV; clamped to [0, len_cap]), of which
// the first gp.P are the decoder prompt
int wm_constraint_launch(wm_ctx* ctx, const ConstraintDev& cd, const GenDev& gp, const int* ids, int ids_stride, const int* lens, int len_cap, int nrows);
void wm_constraint_free(wm_ctx* ctx);
// implemented in wm_merge.hip (stitching overlapping long-form windows; include/wm.h wm_merge_windows)
void wm_merge_free(wm_ctx* ctx);
// implemented in wm_words.hip (grouping token ids into words; include/wm.h wm_set_word_table / wm_word_spans)
void wm_words_free(wm_ctx* ctx);
// the device copy of the vocabulary table for the other kernels that read it (wm_stream.hip): n_tokens, 0 without a table
int wm_words_table(const wm_ctx* ctx, const unsigned char** blob, const int** offsets);
// implemented in wm_vad.hip (speech windows of long recordings; include/wm.h wm_vad_windows)
void wm_vad_free(wm_ctx* ctx);
// implemented in wm_stream.hip (the agreement step of live transcription; include/wm.h wm_stream_agree)
void wm_stream_free(wm_ctx* ctx);
// implemented in wm_align.hip
void wm_align_free(wm_ctx* ctx);
// implemented in wm_score.hip
void wm_score_free(wm_ctx* ctx);
// implemented in wm_engine.hip
// The logits processors of a decode / tap / scoring call, derived in ONE place so that scoring applies exactly what the decode applied:
// checks eos and the prompt pointer (errors under `who`), derives the timestamp scalars (tsp == NULL: off), fills the GenDev fields that depend on the parameter structs and
// the context alone (P, eos, pad, exp_start, thr, alpha, begin, K, V, Vpad, Tids; the rest zero: the caller's) and uploads the suppress /
// begin-suppress mask (ctx->supmask) and the length-penalty table (ctx->exppen).  Returns with the stream idle.
int wm_proc_setup(wm_ctx* ctx, const char* who, const wm_gen_params* gp, const wm_timestamp_params* tsp, GenDev* g, TsDev* ts);
// A call outside the decode loop (replay, parity tap, forward pass) overwrites what a decode in flight lives on (ids, L, kvlen, self K/V,
// the processors' tables).  Clears `began` (wm_decode_run refuses until the next wm_decode_begin) and the modes the launches read off the
// context: use_done (no early exit on the done flag), host_carry / dev_carry (no carried hidden rows), step_flow (no merged-step schedule;
// wm_get_stats reports no schedule_steps).  The captured graphs depend only on their DecGraphKey and on buffer addresses: both slots are kept for
// a following wm_decode_begin with the same key, unless drop_graphs (wm_forward_logits).
void wm_decode_invalidate(wm_ctx* ctx, bool drop_graphs = false);
// A call's own scalars in ctx->gp / ctx->ts for the lifetime of the object; the decode's come back on every exit path.  Not for the graphs (their
// keys live in the slots) but for the readers of a finished decode: after a replay or tap wm_get_tokens reads the decode's gp.Tids / gp.eos, and
// wm_token_timestamps / wm_forward_logits start from its ctx->gp.  (wm_get_beam_result reads ctx->beam, wm_get_stats counters: never swapped.)
struct wm_scalars_swap {
    wm_ctx* ctx; GenDev gp; TsDev ts;
    wm_scalars_swap(wm_ctx* c, const GenDev& g, const TsDev& t) : ctx(c), gp(c->gp), ts(c->ts) { c->gp = g; c->ts = t; }
    wm_scalars_swap(const wm_scalars_swap&) = delete;
    ~wm_scalars_swap() { ctx->gp = gp; ctx->ts = ts; }
};
// timestamp parity tap (wm_select_rows): R <= WM_TAP_ROWS rows already in ctx->logits, probe tokens in cand[1 .. R], cur_len in L[0];
// prefixes DEV [R][Tmax], lengths DEV [R]
int wm_dec_select_rows(wm_ctx* ctx, const int* pre_dev, const int* len_dev, int R, int Tmax);

// ---- parity taps: one row-group driver --------------------------------------------------------------------------------------
// Rows per group of a tap.  15, not 16: wm_dec_select_rows treats a group as ONE stream of R + 1 rows with the probe tokens in cand[1 .. R], and a
// stream's pass carries at most 16 rows.  (wm_score_rows / wm_topk_rows take ctx->Rcap rows per group: what the logits scratch holds.)
constexpr int WM_TAP_ROWS = 15;

// n caller-given rows [n][V] (HOST) -> rows [0, n) of ctx->logits at the Vpad stride
static inline hipError_t wm_tap_upload_logits(wm_ctx* ctx, const float* rows, int n)
{
    return hipMemcpy2DAsync(ctx->logits, (size_t)ctx->Vpad * sizeof(float), rows, (size_t)ctx->V * sizeof(float), (size_t)ctx->V * sizeof(float), n,
                            hipMemcpyHostToDevice, ctx->stream);
}
// The one range check of a tap's lens: every lens[r] in [1, Tmax], or in [1, min(Tmax, n_tgt)] with cap_n_tgt.  also_ok / also: a second condition
// of the call reported in the same sentence (wm_select_rows: its probe tokens)
static inline int wm_tap_check_lens(wm_ctx* ctx, const char* who, const int32_t* lens, int R, int Tmax, bool cap_n_tgt, bool also_ok = true, const char* also = "")
{
    const int hi = cap_n_tgt ? std::min(Tmax, ctx->Tmax) : Tmax;
    bool ok = also_ok;
    for (int r = 0; r < R; ++r) ok = ok && lens[r] >= 1 && lens[r] <= hi;
    if (ok) return WM_OK;
    ctx->err = std::string(who) + ": lens must be in [1, " + (cap_n_tgt ? "min(Tmax, n_tgt)" : "Tmax") + "]" + also;
    return WM_ERR_ARG;
}
// timestamp state of the sampled tokens ids[from:to] (from < 0: 0) on top of `st` (host: wm_decode_begin_ts and the taps)
static inline int4 ts_fold_ids(int4 st, const int32_t* ids, int from, int to, int tb)
{
    for (int t = std::max(from, 0); t < to; ++t) st = ts_fold(st, ids[t], tb);
    return st;
}

// The staging of one tap call: the call's name for its HIP errors, the group capacity, and the device copy of a group's prefixes and lengths in
// ctx->tap_buf — ONE layout: [cap][Tmax] ids, behind them [cap] lengths, behind those `extra` ints of the tap's own.
struct wm_tap_stage {
    wm_ctx* ctx; const char* who; int Tmax, cap;
    int *pre = nullptr, *len = nullptr, *extra = nullptr;
    int fail(hipError_t e) const
    {
        if (e == hipSuccess) return WM_OK;
        ctx->err = std::string(who) + ": " + hipGetErrorString(e);
        return WM_ERR_HIP;
    }
    int reserve(size_t n_extra = 0)         // (a tap without prefixes, wm_lang_pick_rows, does not call it: pre / len stay null)
    {
        if (int rc = fail(ctx->tap_buf.reserve((size_t)cap * Tmax + cap + n_extra))) return rc;
        pre = ctx->tap_buf; len = pre + (size_t)cap * Tmax; extra = len + cap;
        return WM_OK;
    }
    // rows [r0, r0 + n) of the call -> rows [0, n) of ctx->logits, pre and len (prefixes / lens NULL: none)
    hipError_t upload(int r0, int n, const float* logits, const int32_t* prefixes, const int32_t* lens) const
    {
        hipError_t e = wm_tap_upload_logits(ctx, logits + (size_t)r0 * ctx->V, n);
        if (e == hipSuccess && prefixes) e = hipMemcpyAsync(pre, prefixes + (size_t)r0 * Tmax, (size_t)n * Tmax * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && lens) e = hipMemcpyAsync(len, lens + r0, n * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
        return e;
    }
};
#define WM_TAP_HIP(stage, expr) do { if (int _rc = (stage).fail(expr)) return _rc; } while (0)
// The one loop over a tap's row groups: upload a group, body(r0, n) — the tap's own uploads, launches and downloads, enqueued; returns WM_OK or
// its error —, then the stream is awaited, because the next group reuses the staging (the device buffers and the body's host vectors).  Stops at
// the first error; returns with the stream idle.
template <class Body>
static int wm_tap_groups(const wm_tap_stage& s, int R, const float* logits, const int32_t* prefixes, const int32_t* lens, Body body)
{
    int rc = WM_OK;
    for (int r0 = 0; r0 < R && rc == WM_OK; r0 += s.cap) {
        const int n = std::min(s.cap, R - r0);
        rc = s.fail(s.upload(r0, n, logits, prefixes, lens));
        if (rc == WM_OK) rc = body(r0, n);
        if (rc == WM_OK) rc = s.fail(hipStreamSynchronize(s.ctx->stream));
    }
    if (rc) (void)hipStreamSynchronize(s.ctx->stream);
    return rc;
}
