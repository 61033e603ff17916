// wm_words.hip — grouping token ids into words on the device (include/wm.h wm_set_word_table / wm_word_spans): what transformers'
// _combine_tokens_into_words (models/whisper/tokenization_whisper.py) does per row with one tokenizer.decode per token on a growing list and two
// list-rewriting punctuation passes, stated on the bytes of the vocabulary as one left-to-right walk with carried state (csrc/wm_words.h).
//   k_word_spans: grid (rows) x 256, a row in tiles of WW_TILE tokens.  Per tile every thread summarises tokens into LDS — the table gather, the
//                 token's first bytes, its map on the UTF-8 states — then thread 0 walks the tile in order: the piece cut, the word rule, the
//                 prepend run and the append rule all look backwards only (HF's right-to-left prepend pass merges a candidate into the next word
//                 that is none: a run; its emptied slots are transparent to the append pass), so a word start is final when it is written.  The
//                 byte work of the substring tests ends at the first byte that leaves the set: two bytes of an ordinary word.  Behind the walk the
//                 threads turn the word starts into times and mean log-probabilities, one word each.  No atomics, no order dependence: thread 0
//                 alone writes the starts, the barrier orders them in front of the readers.
#include "wm_internal.h"
#include "wm_words.h"

struct wm_words_state {
    DevBuf<unsigned char> blob;         // the vocabulary's bytes, back to back
    DevBuf<int> offsets;                // [n_tokens + 1]
    int n_tokens = 0;
    DevBuf<int> dev;                    // [first R+1 | modes R | ids N | times 2N | logprobs N || n_words R | word_first N+R | word_times 2N | word_logprobs N]
    std::vector<int32_t> host, back;    // the upload and the download, packed in the same order
    hipEvent_t ev0 = nullptr, ev1 = nullptr;     // (its own pair: the context's may belong to a decode in progress)
    ~wm_words_state() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); }
};

void wm_words_free(wm_ctx* ctx) { delete ctx->words_state; ctx->words_state = nullptr; }

int wm_words_table(const wm_ctx* ctx, const unsigned char** blob, const int** offsets)
{
    const wm_words_state* S = ctx->words_state;
    if (!S || S->n_tokens < 1) return 0;
    *blob = S->blob; *offsets = S->offsets;
    return S->n_tokens;
}

__global__ void __launch_bounds__(256)
k_word_spans(const unsigned char* __restrict__ blob, const int* __restrict__ offsets, const int* __restrict__ first, const int* __restrict__ modes,
             const int* __restrict__ ids, const float* __restrict__ times /* null: none */, const float* __restrict__ logprobs /* null: none */,
             int* __restrict__ n_words, int* word_first, float* __restrict__ word_times, float* __restrict__ word_logprobs)
{
    __shared__ uint64_t occ[3 * 256];
    __shared__ uint64_t t_fn[WW_TILE], t_head[WW_TILE];
    __shared__ int t_off[WW_TILE], t_len[WW_TILE];
    __shared__ int s_nw;
    const int r = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < 3 * 256; i += 256) occ[i] = ww_occ(i >> 8, i & 255);
    const int base = first[r], len = first[r + 1] - base, unicode = modes[r];
    int* wf = word_first + base + r;                          // row r owns len + 1 slots
    ww_state s;
    ww_init(s);                                               // (thread 0's copy is the one that counts)
    // len is uniform over the block: the barriers are reached by all threads or by none
    for (int t0 = 0; t0 < len; t0 += WW_TILE) {
        const int n = min(WW_TILE, len - t0);
        __syncthreads();                                      // the walk of the tile before is over (first round: occ is complete)
        for (int k = tid; k < n; k += 256) {
            const int id = ids[base + t0 + k];
            const int off = offsets[id], l = offsets[id + 1] - off;
            const unsigned char* p = blob + off;
            uint64_t head = 0;
            for (int i = 0; i < l && i < WW_HEAD; ++i) head |= (uint64_t)p[i] << (8 * i);
            t_fn[k] = ww_token_fn(p, l); t_head[k] = head; t_off[k] = off; t_len[k] = l;
        }
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < n; ++k) ww_token(s, occ, unicode, t0 + k, t_fn[k], t_head[k], t_len[k], blob + t_off[k], wf);
    }
    __syncthreads();
    if (tid == 0) { s_nw = ww_finish(s, occ, unicode, len, wf); n_words[r] = s_nw; }
    __syncthreads();                                          // thread 0's word starts are visible to the block
    const int nw = s_nw;
    if (!times && !logprobs) return;
    for (int w = tid; w < nw; w += 256) {
        const int a = wf[w], b = wf[w + 1];
        if (times) {
            word_times[2 * (size_t)(base + w)] = times[2 * (size_t)(base + a)];
            word_times[2 * (size_t)(base + w) + 1] = times[2 * (size_t)(base + b - 1) + 1];
        }
        if (logprobs) {
            float sum = 0.f;
            for (int k = a; k < b; ++k) sum += logprobs[base + k];        // ascending token order
            word_logprobs[base + w] = sum / (float)(b - a);
        }
    }
}

extern "C" int wm_set_word_table(wm_ctx* ctx, const uint8_t* bytes, const int32_t* offsets, int n_tokens)
{
    if (!ctx) return WM_ERR_ARG;
    if (!bytes || !offsets) { ctx->err = "wm_set_word_table: null pointer (bytes, offsets)"; return WM_ERR_ARG; }
    if (n_tokens < 1 || n_tokens > WM_WORDS_TOKENS_MAX) { ctx->err = "wm_set_word_table: n_tokens must be in [1, " + std::to_string(WM_WORDS_TOKENS_MAX) + "]"; return WM_ERR_ARG; }
    if (offsets[0] != 0) { ctx->err = "wm_set_word_table: offsets[0] must be 0"; return WM_ERR_ARG; }
    for (int t = 0; t < n_tokens; ++t)
        if (offsets[t + 1] <= offsets[t]) {
            ctx->err = "wm_set_word_table: offsets must ascend strictly, every token has at least one byte (offsets[" + std::to_string(t + 1) + "] <= offsets[" + std::to_string(t) + "])";
            return WM_ERR_ARG;
        }
    if (offsets[n_tokens] > WM_WORDS_BYTES_MAX) { ctx->err = "wm_set_word_table: " + std::to_string(offsets[n_tokens]) + " bytes exceed WM_WORDS_BYTES_MAX = " + std::to_string(WM_WORDS_BYTES_MAX); return WM_ERR_ARG; }
    if (!ctx->words_state) ctx->words_state = new wm_words_state();
    wm_words_state& S = *ctx->words_state;
    WM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    WM_HIP(hipStreamSynchronize(st));                         // (an earlier table may be replaced: no wm_word_spans launch is in flight)
    S.n_tokens = 0;
    WM_HIP(S.blob.reserve((size_t)offsets[n_tokens]));
    WM_HIP(S.offsets.reserve((size_t)n_tokens + 1));
    WM_HIP(hipMemcpyAsync(S.blob, bytes, (size_t)offsets[n_tokens], hipMemcpyHostToDevice, st));
    WM_HIP(hipMemcpyAsync(S.offsets, offsets, ((size_t)n_tokens + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    WM_HIP(hipStreamSynchronize(st));
    S.n_tokens = n_tokens;
    return WM_OK;
}

extern "C" int wm_word_spans(wm_ctx* ctx, int R, const int32_t* first, const int32_t* ids, const int32_t* modes, const float* times, const float* logprobs,
                             int32_t* n_words, int32_t* word_first, float* word_times, float* word_logprobs, float* ms)
{
    if (!ctx) return WM_ERR_ARG;
    if (ms) *ms = 0.f;
    if (!first || !ids || !modes || !n_words || !word_first) { ctx->err = "wm_word_spans: null pointer (first, ids, modes, n_words, word_first)"; return WM_ERR_ARG; }
    if (times && !word_times) { ctx->err = "wm_word_spans: times given without word_times"; return WM_ERR_ARG; }
    if (logprobs && !word_logprobs) { ctx->err = "wm_word_spans: logprobs given without word_logprobs"; return WM_ERR_ARG; }
    if (R < 1 || R > WM_WORDS_ROWS_MAX) { ctx->err = "wm_word_spans: R must be in [1, " + std::to_string(WM_WORDS_ROWS_MAX) + "] rows"; return WM_ERR_ARG; }
    if (first[0] != 0) { ctx->err = "wm_word_spans: first[0] must be 0"; return WM_ERR_ARG; }
    for (int r = 0; r < R; ++r) {
        if (first[r + 1] < first[r]) { ctx->err = "wm_word_spans: first must ascend (first[" + std::to_string(r + 1) + "] < first[" + std::to_string(r) + "])"; return WM_ERR_ARG; }
        if (first[r + 1] > WM_WORDS_IDS_MAX) { ctx->err = "wm_word_spans: more than WM_WORDS_IDS_MAX = " + std::to_string(WM_WORDS_IDS_MAX) + " ids in one call"; return WM_ERR_ARG; }
        if (modes[r] != WM_WORDS_SPACES && modes[r] != WM_WORDS_UNICODE) { ctx->err = "wm_word_spans: modes[" + std::to_string(r) + "] = " + std::to_string(modes[r]) + " is neither WM_WORDS_SPACES nor WM_WORDS_UNICODE"; return WM_ERR_ARG; }
    }
    if (!ctx->words_state || ctx->words_state->n_tokens < 1) { ctx->err = "wm_word_spans: no vocabulary table (wm_set_word_table)"; return WM_ERR_STATE; }
    wm_words_state& S = *ctx->words_state;
    const size_t N = (size_t)first[R];
    for (size_t k = 0; k < N; ++k)
        if (ids[k] < 0 || ids[k] >= S.n_tokens) {
            ctx->err = "wm_word_spans: ids[" + std::to_string(k) + "] = " + std::to_string(ids[k]) + " outside the table's [0, " + std::to_string(S.n_tokens) + ")";
            return WM_ERR_ARG;
        }
    WM_HIP(hipSetDevice(ctx->device));
    if (!S.ev0) WM_HIP(hipEventCreate(&S.ev0));
    if (!S.ev1) WM_HIP(hipEventCreate(&S.ev1));
    const size_t o_first = 0, o_modes = o_first + R + 1, o_ids = o_modes + R, o_time = o_ids + N, o_lp = o_time + (times ? 2 * N : 0),
                 n_up = o_lp + (logprobs ? N : 0),
                 o_nw = n_up, o_wf = o_nw + R, o_wt = o_wf + N + R, o_wl = o_wt + (times ? 2 * N : 0), n_all = o_wl + (logprobs ? N : 0);
    S.host.resize(n_up); S.back.resize(n_all - n_up);
    std::memcpy(S.host.data() + o_first, first, ((size_t)R + 1) * sizeof(int32_t));
    std::memcpy(S.host.data() + o_modes, modes, (size_t)R * sizeof(int32_t));
    if (N) std::memcpy(S.host.data() + o_ids, ids, N * sizeof(int32_t));
    if (times && N) std::memcpy(S.host.data() + o_time, times, 2 * N * sizeof(float));
    if (logprobs && N) std::memcpy(S.host.data() + o_lp, logprobs, N * sizeof(float));
    hipStream_t st = ctx->stream;
    WM_HIP(hipStreamSynchronize(st));                         // (the workspace may grow: nothing of an earlier call is in flight)
    WM_HIP(S.dev.reserve(n_all));
    int* d = S.dev;
    WM_HIP(hipEventRecord(S.ev0, st));
    WM_HIP(hipMemcpyAsync(d, S.host.data(), n_up * sizeof(int32_t), hipMemcpyHostToDevice, st));
    k_word_spans<<<dim3(R), dim3(256), 0, st>>>(S.blob, S.offsets, d + o_first, d + o_modes, d + o_ids,
                                                times ? reinterpret_cast<const float*>(d + o_time) : nullptr,
                                                logprobs ? reinterpret_cast<const float*>(d + o_lp) : nullptr,
                                                d + o_nw, d + o_wf, reinterpret_cast<float*>(d + o_wt), reinterpret_cast<float*>(d + o_wl));
    WM_HIP(hipGetLastError());
    WM_HIP(hipMemcpyAsync(S.back.data(), d + o_nw, (n_all - n_up) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    WM_HIP(hipEventRecord(S.ev1, st));
    WM_HIP(hipEventSynchronize(S.ev1));
    WM_HIP(hipStreamSynchronize(st));
    if (ms) WM_HIP(hipEventElapsedTime(ms, S.ev0, S.ev1));
    const int32_t* h = S.back.data();
    std::memcpy(n_words, h, (size_t)R * sizeof(int32_t));
    std::memcpy(word_first, h + (o_wf - n_up), (N + R) * sizeof(int32_t));
    // a row's slots behind its n_words are not the kernel's to write: what the caller reads there is zero
    for (int r = 0; r < R; ++r) {
        const size_t b = (size_t)first[r], len = (size_t)first[r + 1] - b, nw = (size_t)n_words[r];
        for (size_t w = nw + 1; w <= len; ++w) word_first[b + r + w] = 0;
        if (times) {
            std::memcpy(word_times + 2 * b, h + (o_wt - n_up) + 2 * b, 2 * nw * sizeof(float));
            std::fill(word_times + 2 * (b + nw), word_times + 2 * (b + len), 0.f);
        }
        if (logprobs) {
            std::memcpy(word_logprobs + b, h + (o_wl - n_up) + b, nw * sizeof(float));
            std::fill(word_logprobs + b + nw, word_logprobs + b + len, 0.f);
        }
    }
    return WM_OK;
}
