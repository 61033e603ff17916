// wm_stream.hip — the agreement step of live transcription on the device (include/wm.h wm_stream_agree): LocalAgreement-2 (Macháček
// et al. 2023) for all sessions of a tick, on the bytes of the vocabulary (the table of wm_set_word_table), stated in csrc/wm_stream.h.
//   k_stream_agree: grid (sessions) x 256.  Step 1 (late prefix): every lane takes every 256th word of the new hypothesis, block minimum.  Step 2
//                   (overlap with the committed tail): at most 15 word compares, lane 0.  Step 3 (agreement with the previous hypothesis): every lane
//                   walks the two byte streams of every 256th word pair up to its first mismatch, block minimum.  Step 4 (sentence end): every lane
//                   looks backwards from the last agreed word, block maximum.  The steps are separated by block barriers (k0 feeds step 3, m step 4).
//                   Integers and bytes only, no atomics, plain vector stores by lane 0; two runs give the same bytes.
#include "wm_internal.h"
#include "wm_stream.h"

struct wm_stream_state {
    DevBuf<int> dev;                    // [3 x (words S+1 | tok NW+1 | ids NI) | times 2 NW_new | last_cs S || skip S | commit S | ender S]
    std::vector<int32_t> host, back;    // the upload and the download, packed in the same order
    hipEvent_t ev0 = nullptr, ev1 = nullptr;     // (its own pair: the context's may belong to a decode in progress)
    ~wm_stream_state() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); }
};

void wm_stream_free(wm_ctx* ctx) { delete ctx->stream_state; ctx->stream_state = nullptr; }

struct StreamDev {
    const int* words[3]; const int* tok[3]; const int* ids[3];        // new, prev, tail
    const int* times; const int* last_cs;
};

// all 256 threads call it; `red` holds one slot per wave
__device__ __forceinline__ int block_min(int v, int* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();                                          // the readers of the reduction before are through
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return min(min(red[0], red[1]), min(red[2], red[3]));
}

__global__ void __launch_bounds__(256)
k_stream_agree(const unsigned char* __restrict__ blob, const int* __restrict__ offsets, StreamDev d, ws_params p, int S, int* __restrict__ out)
{
    __shared__ int red[4];
    __shared__ int s_ov;
    const int s = blockIdx.x, tid = threadIdx.x;
    const ws_table tab = {blob, offsets};
    ws_session ss;
    ss.nw = {d.tok[0], d.ids[0], d.words[0][s], d.words[0][s + 1] - d.words[0][s]};
    ss.pv = {d.tok[1], d.ids[1], d.words[1][s], d.words[1][s + 1] - d.words[1][s]};
    ss.tl = {d.tok[2], d.ids[2], d.words[2][s], d.words[2][s + 1] - d.words[2][s]};
    ss.times = d.times; ss.last_cs = d.last_cs[s];
    // every value that steers a barrier is uniform over the block: all threads reach all barriers
    int k0 = block_min(ws_late(ss, p, tid, 256), red);
    if (tid == 0) s_ov = ws_overlap(tab, ss, p, k0);
    __syncthreads();
    k0 += s_ov;
    const int m = block_min(ws_mismatch(tab, ss, k0, tid, 256), red);
    const int e = -block_min(-ws_last_ender(tab, ss, k0, m, tid, 256), red);
    if (tid == 0) { out[s] = k0; out[S + s] = m; out[2 * S + s] = e; }
}

// the shape of one list: fills nw / ni (its words and ids); false with ctx->err set
static bool list_shape(wm_ctx* ctx, const char* name, const wm_stream_list* l, int S, int cap_per_session, size_t* nw, size_t* ni)
{
    const std::string who = std::string("wm_stream_agree: ") + name;
    if (!l->words || !l->tok || !l->ids) { ctx->err = who + ": null pointer (words, tok, ids)"; return false; }
    if (l->words[0] != 0) { ctx->err = who + ".words[0] must be 0"; return false; }
    for (int s = 0; s < S; ++s) {
        if (l->words[s + 1] < l->words[s]) { ctx->err = who + ".words must ascend (words[" + std::to_string(s + 1) + "] < words[" + std::to_string(s) + "])"; return false; }
        if (l->words[s + 1] > WM_STREAM_WORDS_MAX) { ctx->err = who + ": more than WM_STREAM_WORDS_MAX = " + std::to_string(WM_STREAM_WORDS_MAX) + " words in one call"; return false; }
        if (cap_per_session && l->words[s + 1] - l->words[s] > cap_per_session) {
            ctx->err = who + ": session " + std::to_string(s) + " has " + std::to_string(l->words[s + 1] - l->words[s]) + " words, more than WM_STREAM_TAIL = " + std::to_string(cap_per_session);
            return false;
        }
    }
    *nw = (size_t)l->words[S];
    if (l->tok[0] != 0) { ctx->err = who + ".tok[0] must be 0"; return false; }
    for (size_t w = 0; w < *nw; ++w) {
        if (l->tok[w + 1] <= l->tok[w]) { ctx->err = who + ": a word without ids (tok[" + std::to_string(w + 1) + "] <= tok[" + std::to_string(w) + "]): tok must ascend strictly"; return false; }
        if (l->tok[w + 1] > WM_STREAM_IDS_MAX) { ctx->err = who + ": more than WM_STREAM_IDS_MAX = " + std::to_string(WM_STREAM_IDS_MAX) + " ids in one call"; return false; }
    }
    *ni = (size_t)l->tok[*nw];
    return true;
}

extern "C" int wm_stream_agree(wm_ctx* ctx, int S, const wm_stream_list* new_list, const wm_stream_list* prev_list, const wm_stream_list* tail_list,
                               const int32_t* times, const int32_t* last_cs, const wm_stream_params* params,
                               int32_t* skip, int32_t* commit, int32_t* ender, float* ms)
{
    if (!ctx) return WM_ERR_ARG;
    if (ms) *ms = 0.f;
    if (!new_list || !prev_list || !tail_list || !times || !last_cs || !skip || !commit || !ender) {
        ctx->err = "wm_stream_agree: null pointer (new_list, prev_list, tail_list, times, last_cs, skip, commit, ender)";
        return WM_ERR_ARG;
    }
    if (S < 1 || S > WM_STREAM_SESSIONS_MAX) { ctx->err = "wm_stream_agree: S must be in [1, " + std::to_string(WM_STREAM_SESSIONS_MAX) + "] sessions"; return WM_ERR_ARG; }
    ws_params p = {WM_STREAM_LATE_CS, WM_STREAM_NEAR_CS, WM_STREAM_TAIL};
    if (params) { p.late_cs = params->late_cs; p.near_cs = params->near_cs; p.max_ngram = params->max_ngram; }
    if (p.late_cs < 0) { ctx->err = "wm_stream_agree: late_cs = " + std::to_string(p.late_cs) + " must be >= 0"; return WM_ERR_ARG; }
    if (p.near_cs < 0) { ctx->err = "wm_stream_agree: near_cs = " + std::to_string(p.near_cs) + " must be >= 0"; return WM_ERR_ARG; }
    if (p.max_ngram < 1 || p.max_ngram > WM_STREAM_TAIL) { ctx->err = "wm_stream_agree: max_ngram = " + std::to_string(p.max_ngram) + " must be in [1, " + std::to_string(WM_STREAM_TAIL) + "]"; return WM_ERR_ARG; }
    const wm_stream_list* L[3] = {new_list, prev_list, tail_list};
    const char* names[3] = {"new", "prev", "tail"};
    size_t nw[3], ni[3];
    for (int k = 0; k < 3; ++k)
        if (!list_shape(ctx, names[k], L[k], S, k == 2 ? WM_STREAM_TAIL : 0, &nw[k], &ni[k])) return WM_ERR_ARG;
    if (nw[0] + nw[1] + nw[2] > (size_t)WM_STREAM_WORDS_MAX) { ctx->err = "wm_stream_agree: the three lists hold more than WM_STREAM_WORDS_MAX = " + std::to_string(WM_STREAM_WORDS_MAX) + " words"; return WM_ERR_ARG; }
    if (ni[0] + ni[1] + ni[2] > (size_t)WM_STREAM_IDS_MAX) { ctx->err = "wm_stream_agree: the three lists hold more than WM_STREAM_IDS_MAX = " + std::to_string(WM_STREAM_IDS_MAX) + " ids"; return WM_ERR_ARG; }
    const unsigned char* blob = nullptr;
    const int* offsets = nullptr;
    const int n_tokens = wm_words_table(ctx, &blob, &offsets);
    if (n_tokens < 1) { ctx->err = "wm_stream_agree: no vocabulary table (wm_set_word_table)"; return WM_ERR_STATE; }
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < ni[k]; ++i)
            if (L[k]->ids[i] < 0 || L[k]->ids[i] >= n_tokens) {
                ctx->err = std::string("wm_stream_agree: ") + names[k] + ".ids[" + std::to_string(i) + "] = " + std::to_string(L[k]->ids[i]) + " outside the table's [0, " + std::to_string(n_tokens) + ")";
                return WM_ERR_ARG;
            }
    if (!ctx->stream_state) ctx->stream_state = new wm_stream_state();
    wm_stream_state& W = *ctx->stream_state;
    WM_HIP(hipSetDevice(ctx->device));
    if (!W.ev0) WM_HIP(hipEventCreate(&W.ev0));
    if (!W.ev1) WM_HIP(hipEventCreate(&W.ev1));
    size_t o_words[3], o_tok[3], o_ids[3], o = 0;
    for (int k = 0; k < 3; ++k) { o_words[k] = o; o += (size_t)S + 1; o_tok[k] = o; o += nw[k] + 1; o_ids[k] = o; o += ni[k]; }
    const size_t o_times = o, o_last = o_times + 2 * nw[0], n_up = o_last + S, n_all = n_up + 3 * (size_t)S;
    W.host.resize(n_up); W.back.resize(3 * (size_t)S);
    int32_t* h = W.host.data();
    for (int k = 0; k < 3; ++k) {
        std::memcpy(h + o_words[k], L[k]->words, ((size_t)S + 1) * sizeof(int32_t));
        std::memcpy(h + o_tok[k], L[k]->tok, (nw[k] + 1) * sizeof(int32_t));
        if (ni[k]) std::memcpy(h + o_ids[k], L[k]->ids, ni[k] * sizeof(int32_t));
    }
    if (nw[0]) std::memcpy(h + o_times, times, 2 * nw[0] * sizeof(int32_t));
    std::memcpy(h + o_last, last_cs, (size_t)S * sizeof(int32_t));
    hipStream_t st = ctx->stream;
    WM_HIP(hipStreamSynchronize(st));                         // (the workspace may grow: nothing of an earlier call is in flight)
    WM_HIP(W.dev.reserve(n_all));
    int* d = W.dev;
    StreamDev sd;
    for (int k = 0; k < 3; ++k) { sd.words[k] = d + o_words[k]; sd.tok[k] = d + o_tok[k]; sd.ids[k] = d + o_ids[k]; }
    sd.times = d + o_times; sd.last_cs = d + o_last;
    WM_HIP(hipEventRecord(W.ev0, st));
    WM_HIP(hipMemcpyAsync(d, h, n_up * sizeof(int32_t), hipMemcpyHostToDevice, st));
    k_stream_agree<<<dim3(S), dim3(256), 0, st>>>(blob, offsets, sd, p, S, d + n_up);
    WM_HIP(hipGetLastError());
    WM_HIP(hipMemcpyAsync(W.back.data(), d + n_up, 3 * (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    WM_HIP(hipEventRecord(W.ev1, st));
    WM_HIP(hipEventSynchronize(W.ev1));
    WM_HIP(hipStreamSynchronize(st));
    if (ms) WM_HIP(hipEventElapsedTime(ms, W.ev0, W.ev1));
    std::memcpy(skip, W.back.data(), (size_t)S * sizeof(int32_t));
    std::memcpy(commit, W.back.data() + S, (size_t)S * sizeof(int32_t));
    std::memcpy(ender, W.back.data() + 2 * (size_t)S, (size_t)S * sizeof(int32_t));
    return WM_OK;
}
