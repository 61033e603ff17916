/* wm.h — C-ABI of libwm.so, the MI355X (gfx950) Whisper-Medusa inference engine.
 *
 * The reference (aiola-lab/whisper-medusa) is pure Python and has no FFI; its boundary for
 * this path is the Python API `WhisperMedusaModel.from_pretrained()/generate()/forward()`
 * (whisper_medusa/models/model.py:265-291, :1419-1779, :1223-1347).  The entry points below
 * are what a native back end for that API binds; every declaration cites the reference
 * interface it replaces.  The Python drop-in (whisper-medusa_amd/whisper_medusa/api.py)
 * calls them through ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: all functions return 0 on success, <0 on error (wm_last_error(ctx) gives the
 * text; WM_ERR_* below).  Handles are opaque.  Pointers marked DEV are device (HBM)
 * pointers, HOST are host pointers.  One context = one GPU + one HIP stream; a context is
 * not thread-safe, distinct contexts are independent (and may run concurrently from different host threads).
 * Ordering: the work runs on the context's own stream; device inputs must be complete before the call (the caller
 * synchronises whatever produced them) and every entry point returns after its work has finished, so outputs can be
 * read from any stream.  Nothing here takes a torch type.
 */
#ifndef WM_H_
#define WM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WM_ABI_VERSION 9

#define WM_OK 0
#define WM_ERR_ARG (-1)      /* bad argument / unsupported configuration (reference: ValueError, model.py:225-229) */
#define WM_ERR_HIP (-2)      /* HIP runtime failure */
#define WM_ERR_STATE (-3)    /* call sequence violated (e.g. decode before encode) */
#define WM_ERR_NOMEM (-4)

#define WM_HEADS_LINEAR 0    /* medusa_heads_type="base_head"   (model.py:235-246) */
#define WM_HEADS_BLOCK 1     /* medusa_heads_type="medusa_block" (model.py:248-256) */

#define WM_ACCEPT_GREEDY 0   /* temperature==0 branch, medusa_utils.py:547-560 */
#define WM_ACCEPT_TYPICAL 1  /* temperature!=0 branch, medusa_utils.py:562-588 (what generate() runs, model.py:1877-1881) */

typedef struct wm_ctx wm_ctx;

/* Mirrors MedusaConfig + the Whisper dims it inherits (utils/config_and_args.py:17-62). */
typedef struct wm_config {
    int32_t abi_version;        /* = WM_ABI_VERSION */
    int32_t d_model;            /* multiple of 64; head_dim is 64 */
    int32_t enc_layers, dec_layers;
    int32_t n_heads;            /* d_model / 64 (encoder == decoder) */
    int32_t ffn_dim;            /* encoder_ffn_dim == decoder_ffn_dim */
    int32_t vocab;
    int32_t n_mels;             /* 80 */
    int32_t n_ctx;              /* max_source_positions (1500): encoder frames per clip */
    int32_t n_tgt;              /* max_target_positions (448) */
    int32_t medusa_heads;       /* K = medusa_num_heads, <= 15 */
    int32_t heads_type;         /* WM_HEADS_* */
    int32_t max_batch;          /* streams the context is sized for */
    int32_t dec_weight_fp8;     /* 1: the six matrices of every decoder layer are fp8 e4m3 (OCP) in the packed layout, with one fp32
                                 * scale per output row appended to the table (BASELINE.json configs[4]); 0: bf16 */
    int32_t medusa_choices[16]; /* MedusaConfig.medusa_choices = [1, c_1, .., c_K] (utils/config_and_args.py:17-62; consumed by
                                 * generate_medusa_buffers / generate_candidates, medusa_utils.py:305-458): head k contributes its
                                 * top-c_k tokens, the candidate tree is their cartesian product.  All zero or all one = the chain
                                 * [1]*(K+1) every shipped checkpoint uses.  Limits: sum_i prod_{l<=i} c_l <= 64 nodes (the verify
                                 * pass of a stream is up to four 16-row query tiles), prod c_l <= 32 paths, c_k <= 4 — e.g. K = 10
                                 * with top-2 on the first two heads: [1,2,2,1,1,1,1,1,1,1,1] = 39 nodes.  Each node attends
                                 * to the history and to its own ancestors and sits at position L + depth — the mask / position
                                 * ids the reference builds (medusa_utils.py:343-363) and then never hands to its decoder. */
    int32_t enc_fp8;            /* 1: the encoder GEMMs fed by a LayerNorm (QKV, FC1) and the cross-K/V projection run on the CDNA4
                                 * fp8 MFMA v_mfma_f32_16x16x128_f8f6f4 (twice the bf16 MFMA rate; BASELINE.json configs[4]), operands in
                                 * the 128-k unit layout [R/16][Kp/128][2][64 lanes][16 B] (K zero-padded to Kp = 128 ceil(K / 128);
                                 * whisper_medusa/weights.py pack_matrix_fp8_k128): e4m3 weights with one fp32 scale per output row — 4 table
                                 * entries per encoder layer (qkv, qkv scales, fc1, fc1 scales) + 2 (cross-K/V) appended after the
                                 * decoder scales, the bf16 entries of those matrices may then be 16-byte placeholders — and the
                                 * LayerNorm output quantised to e4m3 with one scale per token row; 0: bf16 */
    int32_t act_fp16;           /* the decode numerics contract (ABI v8).  0: every decoder GEMM operand is a bf16 hi / lo pair
                                 * (~17 mantissa bits, two planes, two MFMAs per weight fragment), decoder matrices bf16.  1: ONE fp16 plane
                                 * (11 bits: the precision of the reference's own half-precision inference, model.py:1223-1347 under
                                 * torch.float16), one v_mfma_f32_16x16x32_f16 per weight fragment; the blob then holds the decoder-layer
                                 * matrices, the Medusa heads and the packed vocabulary projection as fp16 (exact from bf16 for |w| >= 2^-17;
                                 * whisper_medusa/weights.py build_blob(act_fp16=True)).  A library is BUILT for one contract
                                 * (wm_build_act_fp16(): libwm.so 0, libwm_f16.so 1); wm_create refuses the other. */
    int32_t cross_kv_fp8;       /* 1 (BASELINE.json configs[4]; ABI v8): the decode loop reads the encoder cross-K/V — the dominant HBM stream of a
                                 * batched step, 245.8 MB per stream and pass in bf16 — from an fp8 e4m3 copy with ONE fp32 scale per (kv layer,
                                 * stream, head) for K and one for V (scale = max|x| / 448 over the head's 1500 x 64 values), written by a
                                 * quantisation pass behind wm_encode's cross-K/V projection (HF WhisperAttention cross branch,
                                 * modeling_whisper.py:322-335); K's scale rides on the query, V's on the normalised output.  The bf16 projection
                                 * stays in HBM (wm_get_cross_kv returns it).  0: the bf16 cache. */
    int32_t sibling_rows;       /* ABI v9.  S > 0 (one stream, candidate chain): the verify pass carries, in the spare rows of its 16-row tile, head 1's
                                 * top-2 .. top-(S+1) tokens as LEAVES under the root (position L + 1, attending the history, the root and
                                 * themselves; S <= 15 - medusa_heads, <= 5).  Acceptance is evaluated on the chain exactly as without them
                                 * (medusa_utils.py:526-641: the emitted ids are the reference's); when the chain accepts nothing (a = 0) and
                                 * argmax v_0 — the next root, model.py:710-713 — is one of the siblings, that row's post-LN state IS the
                                 * state the next base pass would compute for it: its K/V rows move to position L + 1 and the base pass is
                                 * skipped (the hidden-state carry of an accept length > 0, extended to a = 0).  0: off. */
} wm_config;

/* Packed parameter blob (layout: whisper_medusa/weights.py).  The blob
 * stays owned by the caller and must outlive the context.  Replaces the state-dict load of
 * model.py:273-278. */
typedef struct wm_weights {
    const void* blob;           /* DEV */
    uint64_t blob_bytes;
    const uint64_t* offsets;    /* HOST: byte offset of every tensor, canonical order */
    int32_t n_offsets;
} wm_weights;

/* Per-call generation parameters: what generate() derives from generation_config
 * (model.py:1168-1207 processors, :1635-1639 lengths, :774-793 stop rules,
 * medusa_utils.py:14-18 posterior constants). */
typedef struct wm_gen_params {
    const int32_t* prompt;          /* HOST, decoder prompt ids (model.py:1519-1537) */
    int32_t prompt_len;             /* P = begin_index */
    int32_t eos_token_id, pad_token_id;
    const int32_t* suppress;        /* HOST, SuppressTokensLogitsProcessor list */
    int32_t n_suppress;
    const int32_t* begin_suppress;  /* HOST, SuppressTokensAtBeginLogitsProcessor list */
    int32_t n_begin_suppress;
    int32_t max_length;             /* MaxLengthCriteria: stop when L >= max_length */
    int32_t hard_max_length;        /* model.py:789-793: stop when L + K >= this */
    int32_t exp_decay_start;        /* ExponentialDecayLengthPenalty start (relative to P); <0 = off */
    float exp_decay_factor;
    float posterior_threshold, posterior_alpha;   /* 0.09 / 0.3 */
    float temperature;              /* divides verify logits in typical mode (1.0 via generate()) */
    int32_t accept_mode;            /* WM_ACCEPT_* */
    int32_t vanilla;                /* 1 = plain greedy decoding on the base head (anchor measurement) */
    int32_t begin_index;            /* sequence length at which the begin-suppress list applies (SuppressTokensAtBeginLogitsProcessor
                                     * begin_index).  < 0: prompt_len.  With `prompt_ids` the reference hands HF the number of init tokens
                                     * only (model.py:1537 `begin_index = init_tokens.shape[1]`, :1640-1644 set_begin_index), not the
                                     * length of the whole decoder prompt — the caller passes that number here */
    int32_t force_accept;           /* measurement knob (bench.py acceptance-sensitivity rows): >= 0 forces every iteration's accept
                                     * length to min(force_accept, K) whatever the posterior says — the tokens are then meaningless,
                                     * the cost of an iteration at that acceptance is not; < 0 = off (always, outside benchmarks) */
} wm_gen_params;

typedef struct wm_stats {
    int64_t iterations;             /* decode iterations the slowest stream needed since wm_decode_begin */
    int64_t iterations_launched;    /* iterations enqueued (polling granularity; extra ones are device-side no-ops) */
    int64_t tokens_emitted;         /* sum over streams of tokens appended after the prompt */
    int64_t accept_hist[16];        /* histogram of accept length a (0..K), all streams */
    float ms_logmel, ms_encode, ms_decode;   /* hipEvent-timed on the context's stream, last call of each */
    int32_t graph_replays;          /* decode iterations that ran as hipGraph replays */
    int32_t schedule_steps;         /* merged-step schedule (several streams, candidate chain): passes that carried rows since
                                     * wm_decode_begin (a stream's iteration takes one pass, two after an accept length of 0);
                                     * 0 = lock-step schedule (base pass + verify pass per iteration) */
    int32_t sibling_hits;           /* wm_config.sibling_rows: iterations with accept length 0 whose next root was a sibling row (base pass skipped) */
} wm_stats;

/* ---- lifecycle (replaces WhisperMedusaModel.from_pretrained / .to(device), model.py:265-291) ---- */
int wm_create(const wm_config* cfg, const wm_weights* w, int device, void* hip_stream /* hipStream_t or NULL */,
              wm_ctx** out);
void wm_destroy(wm_ctx* ctx);
const char* wm_last_error(const wm_ctx* ctx);     /* ctx may be NULL: last create error */
int wm_abi_version(void);
/* the decode numerics contract this library was compiled for (wm_config.act_fp16 must equal it) */
int wm_build_act_fp16(void);

/* ---- audio front door (replaces what the reference's callers do with torchaudio before the
 * feature extractor: `input_speech.mean(dim=0)` and `torchaudio.transforms.Resample(sr, 16000)`, README.md:120-125,
 * eval_whisper_medusa.py:41-45).  Channel-mean downmix + windowed-sinc polyphase resampling with torchaudio 2.2.2's
 * default filter (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).
 * in: DEV float32 [B][channels][n_in]; out: DEV float32 [B][wm_resample_len(n_in, sr_in, sr_out)].
 * sr_in == sr_out: downmix only. */
int64_t wm_resample_len(int64_t n_in, int sr_in, int sr_out);    /* ceil(n_in * sr_out / sr_in) */
int wm_resample(wm_ctx* ctx, const float* in, int B, int channels, int n_in, int sr_in, int sr_out, float* out);

/* ---- F0 log-mel (replaces WhisperProcessor.__call__, eval_whisper_medusa.py:46-50) ----
 * wav: DEV float32 [B][n_samples] already padded/trimmed to n_samples = 320*n_ctx (480000).
 * feats: DEV float32 [B][n_mels][2*n_ctx]. */
int wm_logmel(wm_ctx* ctx, const float* wav, int B, int n_samples, float* feats);
/* Log-mel of whole recordings (WhisperFeatureExtractor(truncation=False)): the same arithmetic over n_samples / 160 frames, the clamp at
 * the maximum of the whole recording.  wav: DEV float32 [B][n_samples], n_samples any positive multiple of 160 (clips of one call are
 * zero-padded as audio to the longest: HF padding="longest"); feats: DEV float32 [B][n_mels][n_samples/160].  B <= max_batch. */
int wm_logmel_long(wm_ctx* ctx, const float* wav, int B, int n_samples, float* feats);
/* The windows of one round of sequential long-form decoding, one launch (HF _get_input_segment: slice at the stream's seek, zero pad):
 *   out[w][m][f] = f < n_valid[w] ? feats[clip[w]][m][seek[w] + f] : 0.0f
 * feats: DEV float32 [n_clips][n_mels][frames]; clip, seek, n_valid: HOST int32 [Bw]; out: DEV float32 [Bw][n_mels][2*n_ctx].
 * WM_ERR_ARG, with out untouched: clip[w] outside [0, n_clips), seek[w] < 0, n_valid[w] outside [0, 2*n_ctx], seek[w] + n_valid[w] > frames. */
int wm_gather_windows(wm_ctx* ctx, const float* feats, int n_clips, int frames, const int32_t* clip, const int32_t* seek,
                      const int32_t* n_valid, int Bw, float* out);

/* ---- F1+F2 encoder and cross-KV projection (replaces the encoder call of
 * _prepare_encoder_decoder_kwargs_for_generation, model.py:1005-1011, and the cross K/V
 * projection hidden in the first decoder pass).  feats: DEV float32 [B][n_mels][2*n_ctx]. */
int wm_encode(wm_ctx* ctx, const float* feats, int B);
/* forward(encoder_outputs=...) (model.py:1223-1243, :1232: a caller-supplied `encoder_outputs[0]` replaces the encoder pass, HF
 * WhisperModel.forward): hidden = DEV float32 [B][n_ctx][d_model] last hidden state (after the encoder's final LayerNorm).  It is
 * stored bf16 like wm_encode's own output and the cross K/V of every decoder layer are projected from it; afterwards the context
 * is in the state wm_encode leaves.  Not available on an enc_fp8 context (WM_ERR_ARG). */
int wm_set_encoder_output(wm_ctx* ctx, const float* hidden, int B);

/* Whisper timestamp rules for one decode (additive to ABI v9).  Stands in for the `return_timestamps=True` branch the reference leaves
 * as a TODO (model.py:1171-1175): HF WhisperGenerationMixin.generate builds a WhisperTimeStampLogitsProcessor(generation_config,
 * begin_index) (transformers generation/logits_process.py) and runs it after the other processors on every step.  The engine applies
 * it inside its select kernels to every logits row with that row's OWN prefix: base / head rows the committed ids[:L], verify row i
 * ids[:L] + c_0 .. c_i.  Timestamp token t means (t - timestamp_begin) * time_precision seconds. */
typedef struct wm_timestamp_params {
    int32_t timestamp_begin;             /* first timestamp token = no_timestamps_token_id + 1; the timestamps are [timestamp_begin, vocab) */
    int32_t no_timestamps_token_id;      /* always masked */
    int32_t max_initial_timestamp_index; /* generation_config.max_initial_timestamp_index; < 0 = none */
    int32_t begin_index;                 /* the processor's begin_index (ids[begin_index:] are the sampled tokens); < 0: the wm_gen_params one */
} wm_timestamp_params;

/* Repetition rules (additive to ABI v9).  Stand in for HF RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor
 * (transformers generation/logits_process.py), which GenerationMixin._get_logits_processor puts FIRST in the chain for
 * generation_config.repetition_penalty / no_repeat_ngram_size; the reference ignores both fields (its generate() never builds them,
 * model.py:1168-1207).  For a logits row with prefix `pre` (all ids the row follows, decoder prompt included):
 *   1. penalty p: every token n of set(pre): x[n] = x[n] < 0 ? x[n] * p : x[n] / p  (on the raw fp32 logit, a true division);
 *   2. n-gram size g, len(pre) >= g: every token that followed an earlier occurrence of pre[len-g+1:] inside pre becomes -inf
 *      (g == 1: every token of pre);
 *   then the processors of wm_gen_params, then the timestamp rules.  A banned token is -inf whatever follows (HF: a banned EOS under
 *   the exponential decay is -inf + inf * k = NaN; the engine keeps -inf — the one deviation).
 * Prefixes are each row's OWN (the convention of the timestamp rules): base / Medusa-head rows of a stream the committed ids[:L], verify
 * row i ids[:L] + c_0 .. c_i, a scored position t ids[:t], a tap row its given prefix.  The select kernels derive both sets from the ids
 * on the device (no per-stream state): sibling rows (wm_config.sibling_rows) stay on and the hidden-state carry needs nothing new — a
 * carried row is selected in the next iteration, under the ids committed by then.
 * Sticky on the context until cleared (NULL, or p == 1 and g == 0); read by wm_decode_begin, wm_decode_begin_ts, wm_score_tokens,
 * wm_select_rows (whose timestamp argument may then be NULL) and wm_score_rows.  WM_ERR_ARG (wm_last_error says why): p <= 0 or not finite,
 * g < 0 or g > n_tgt; and from the calls that read them: a candidate tree (medusa_choices with top-k > 1) while rules are on. */
typedef struct wm_repeat_params { float repetition_penalty; int32_t no_repeat_ngram_size; } wm_repeat_params;
int wm_set_repeat_rules(wm_ctx* ctx, const wm_repeat_params* rp /* NULL = off */);

/* Seeded sampling on the plain decode path (additive to ABI v9; csrc/wm_sample.hip).  Stands in for HF generate(do_sample=True,
 * temperature=T) as WhisperGenerationMixin.generate_with_fallback uses it for its retries (the reference copies that loop, model.py:1842-2013, and
 * has no Medusa-with-sampling branch either): the processors run, then the temperature warper, then a draw from the softmax.  The engine draws by
 * Gumbel-max over counter-based noise.  A token at sequence position t (the index it takes in ids; t = L[s] when it is chosen):
 *   1. the processed row v: the repetition rules, then the processors of wm_gen_params, then the timestamp masks, each under the row's own prefix;
 *   2. timestamp rules on: the log-softmax decision on v at temperature 1, BEFORE the temperature (HF: processors, then warpers): text is masked
 *      when logsumexp(v[tb:]) > max(v[:tb]);
 *   3. token = argmax_n (v_n * (1/T) + g_n) over what step 2 leaves (one fp32 fused multiply-add per token, 1/T rounded to fp32); ties: the lower id;
 *   4. g_n = -logf(-logf(u_n)), u_n = (2 * (x_n >> 9) + 1) * 2^-24: every u is exact in fp32 and lies in [2^-24, 1 - 2^-24], so g is finite
 *      (-2.81 .. 16.64); logf is the correctly-specified library function, not the fast intrinsic.
 * x_n = word (n & 3) of Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) with key (seed_lo, seed_hi)
 * and counter (n >> 2, t, key_lo, key_hi), `key` the 64-bit stream key the caller gives each stream.  A token's noise therefore depends on
 * (seed, stream key, position, token id) alone: not on the batch slot, the batch size, the slicing of the vocabulary or graph replay.
 * Without a filter this samples softmax(v / T) over the WHOLE distribution — openai-whisper's Categorical(logits / T); HF's default top_k = 50
 * warper is not applied by default (the deviation): wm_set_sampling_filter below adds top_k / top_p / min_p as one value threshold per row.  HF's
 * own top_k= / top_p= keywords stay refused by the Python layer, which has sampling_top_k= / sampling_top_p= / sampling_min_p= for the engine's.
 * Sticky on the context until cleared (NULL); read by wm_decode_begin / wm_decode_begin_ts, which then return WM_ERR_ARG (wm_last_error says why)
 * when n_keys != B, when wm_gen_params.vanilla == 0 (sampling runs on the plain decode path only) or on a candidate-tree context.  wm_set_sampling
 * itself: WM_ERR_ARG for a temperature that is not finite or <= 0, n_keys < 0.  wm_gen_params.temperature keeps its meaning (typical acceptance). */
typedef struct wm_sample_params { float temperature; uint64_t seed; const uint64_t* stream_keys /* HOST [n_keys]; NULL: 0..B-1 */; int32_t n_keys; } wm_sample_params;
int wm_set_sampling(wm_ctx* ctx, const wm_sample_params* sp /* NULL = off */);

/* Top-k, top-p and min-p filters of the seeded draw (additive to ABI v9; csrc/wm_sample.hip k_filter_prep / k_filter_row): HF's
 * TopKLogitsWarper, TopPLogitsWarper and MinPLogitsWarper, min_tokens_to_keep = 1, as ONE fp32 value threshold tau per row, applied between steps
 * 2 and 3 above.  R = the ids step 2 leaves with v_n > -inf, m = max_R v, a_n = fl(fl(v_n - m) * fl(1/T)) (1/T > 0 keeps the order, so the whole
 * filter is defined on v):
 *   top_k >= 1 (0 = off): tau_k = the k-th largest value of {v_n : n in R}, counted with multiplicity; -inf when |R| <= k.  Keep v_n >= tau_k: ties
 *      at the k-th place are all kept, as `scores < topk(scores, k)[0][..., -1]` keeps them.  Pure ordering: exact on every row.
 *   0 < top_p < 1 (1 = off): on the set K1 top-k leaves, q_n = exp(a_n) / sum_K1 exp(a_j); a value x is kept iff the values strictly greater
 *      than x hold less than top_p of the mass (TopPLogitsWarper removes the ascending prefix whose cumulative mass is <= 1 - top_p), so the
 *      maximum always stays.  Equal values share one fate; HF's sort may split a tie at the boundary (the one deviation: a superset of HF's set).
 *      The engine adds the masses as integers: round(expf(a_n) * 2^40) in 64 bits, so that the sum does not depend on its order (error of the
 *      quantisation <= V * 2^-41 of the largest mass); tau_p = the value at which the sum, from the largest value down, first reaches
 *      ceil(top_p * total), the product taken in fp64: a total above 2^53 units (up to V * 2^40, about 2^56) rounds by up to 4 units on its way
 *      to fp64 and the product by as much again — deterministic (a function of the integer total alone) and at most 2^-36 of the largest mass.
 *   0 < min_p <= 1 (0 = off): keep n iff expf(a_n) >= min_p (MinPLogitsWarper: the ratio to the maximum survives HF's renormalisation); tau_m =
 *      the smallest value of R that passes.
 *   tau = max(tau_k, tau_p, tau_m); step 3 becomes the arg-max over {n in R : v_n >= tau} of the same fused multiply-add with the same noise.  The
 *      comparison is a float comparison (-0.0 == +0.0).  A filter that keeps everything gives today's token and perturbed value bit for bit.
 * The filtered draw depends on (seed, stream key, position, the row's values) alone: no float is added in an order that the batch slot, the batch
 * size, the grid or graph replay could change.  Sticky like wm_set_sampling and read only while sampling is on: wm_decode_begin* returns WM_ERR_ARG
 * when a filter is set and the decode does not sample.  The setter: WM_ERR_ARG for top_k < 0, top_p outside (0, 1], min_p outside [0, 1]. */
typedef struct wm_sample_filter { int32_t top_k; float top_p; float min_p; } wm_sample_filter;
int wm_set_sampling_filter(wm_ctx* ctx, const wm_sample_filter* f /* NULL = off */);

/* Beam search on the plain decode path (additive to ABI v9; csrc/wm_beam.hip).  Stands in for HF generate(num_beams=n) with
 * do_sample off — GenerationMixin._beam_search (transformers generation/utils.py) and its helpers _get_top_k_continuations,
 * _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic, _beam_search_has_unfinished_sequences — which the
 * reference refuses (model.py:1153-1156).  Beam j of clip b is stream b * n + j of a plain decode of B * n streams, all at one length L; the model
 * runs as the ordinary base pass.  One step, everything on the device (P = the whole decoder prompt length, V = vocab):
 *   1. The row of stream s is w = log_softmax(raw logits) FIRST (fp32: x - (m + logf(sum exp(x - m))), the sum in 16 slice partials); the
 *      processors then run ON THE LOG-PROBABILITIES with no renormalisation afterwards (HF: `log_probs = logits_processor(ids, log_probs)`): the
 *      repetition rules, then the processors of wm_gen_params — the exponential decay reads abs(w[eos]) —, then the timestamp rules (their own
 *      decision compares logsumexp(w[tb:]) with max(w[:tb]) of the processed row) — each row under its OWN beam's prefix, at the common length L.
 *   2. Each clip keeps the best 2n of the n * V accumulated values a = running_score[j] + w[j][token] (one fp32 add).  A candidate HITS when its
 *      token is EOS or L + 1 >= max_length.  The next running beams are the best n of a + (hit ? -1e9f : 0) (HF's fp32 -1e9 arithmetic, the
 *      running score keeps that sum).  Only hits among the first n ranks can enter the finished table (n entries, initially -1e9 / not set), scored
 *      a / fl((L + 1 - P) ** length_penalty) (the power in double, rounded to fp32, a true fp32 division), then + -1e9f when early_stopping is
 *      True and the table is full, + -1e9f when the heuristic flag is off, + -1e9f for every candidate that may not enter, in that order.
 *      The initial running scores are [0, -1e9, ...].
 *   3. torch.topk leaves ties open; the engine orders by value descending, then by (beam, token) ascending, and in the finished-table merge an
 *      older entry comes before a new one (old entries by their table index).
 *   4. After L += 1 the heuristic flag is and-ed with any_j(running_score[0] / fl(len ** length_penalty) > (set[j] ? min(finished scores) : -1e9)),
 *      len = max_length - P for early_stopping "never" with length_penalty > 0, else L - P.  A clip is done when the flag is off, or
 *      early_stopping is True and every table entry is set, or all 2n candidates hit (HF's three-way condition, taken per clip: a clip's result does
 *      not depend on its batch).  A done clip's streams keep stepping as no-ops.  The output is the finished table, never the running beams.
 * Then stream s takes over the self K/V rows [0, L), the ids row and the committed timestamp state of stream beam_idx[s] (through a shadow buffer:
 * gather, then write back) and appends its token.  The encoder ran once per clip: wm_decode_begin replicates the cross K/V of clip b (slot b) to
 * slots b * n .. b * n + n - 1 (the fp8 copy and its scales included) and wm_decode_run moves it back (slot b * n -> b) when the last clip is
 * done, so that the context is in the state wm_encode left and the replay entry points (wm_score_tokens, wm_token_timestamps) work unchanged.
 * length_penalty is read as fp32.  Sticky on the context until cleared (NULL), like wm_set_sampling; read by wm_decode_begin / wm_decode_begin_ts,
 * whose B is then the number of CLIPS.  WM_ERR_ARG (wm_last_error says why) from wm_set_beam: num_beams outside [2, WM_BEAM_MAX], a penalty that
 * is not finite, early_stopping outside 0..2; from wm_decode_begin*: wm_gen_params.vanilla == 0, a candidate-tree context, sampling set at the same
 * time, B * num_beams > max_batch. */
#define WM_BEAM_MAX 8
typedef struct wm_beam_params { int32_t num_beams; float length_penalty; int32_t early_stopping /* 0 False, 1 True, 2 "never" */; } wm_beam_params;
int wm_set_beam(wm_ctx* ctx, const wm_beam_params* bp /* NULL = off */);
/* The finished hypothesis `rank` (0 = best) of clip `clip` of the last beam decode (HF: `sequences` / `sequences_scores` of _beam_search, row
 * clip * num_return_sequences + rank): ids (prompt + generated, EOS included) to out_ids (HOST, cap entries of room), their number to *n, the
 * length-penalised score to *score.  An entry that was never set has the prompt alone and the score -1e9.  WM_ERR_STATE when the last decode was
 * no beam decode or is not finished. */
int wm_get_beam_result(wm_ctx* ctx, int clip, int rank, int32_t* out_ids /* HOST */, int cap, int* n, float* score);

/* Sequence bias on the plain decode path (additive to ABI v9; csrc/wm_seq_bias.hip).  Stands in for HF generate(sequence_bias=...) and
 * generate(bad_words_ids=...) — SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor (transformers generation/logits_process.py; the second is the
 * first with every bias -inf), which GenerationMixin._get_logits_processor puts BEFORE every other processor this engine implements; the reference
 * builds neither (model.py:1168-1207).  An entry is a token sequence of length m (1..WM_SEQ_BIAS_MAX_LEN) with a bias b.  A row with prefix ids[:len]
 * (decoder prompt included: HF's input_ids) is edited IN PLACE before anything else reads it.  For every token n that is the last id of an entry:
 *   1. s = +0.0f; a one-token entry (n,) sets s to its bias;
 *   2. every longer entry ending in n, in the CALLER'S order: when m <= len and ids[len - m + 1 .. len - 1] equals its first m - 1 ids, s = s + b
 *      (one fp32 add; an entry longer than the context is ignored, so an entry whose m - 1 leading ids would be the whole context — m = len + 1 —
 *      is ignored too);
 *   3. x[n] = x[n] + s (one fp32 add).
 * This is the arithmetic of SequenceBiasLogitsProcessor.__call__ (the bias vector is built in fp32, then scores + bias): the row equals HF's as fp32
 * values, -inf included.  No atomics touch the row and the order of the sums is fixed: a token's value does not depend on the batch slot, the batch
 * size or graph replay.  One thread owns one target token (its entries form a GROUP: the one-token entry first, then caller order); a row costs
 * `groups` read-modify-writes, never a sweep of the vocabulary.
 * Greedy and sampled plain decodes edit the raw logits row behind the base pass, before the repetition rules, the processors of wm_gen_params and the
 * timestamp rules (HF's order).  A beam decode (wm_set_beam) edits it AFTER the log-softmax normaliser of the raw row is taken (HF: processors run on
 * log_softmax(raw)): the engine computes (x + s) - lse where HF computes (x - lse) + s — equal up to one fp32 rounding.
 * Sticky on the context until cleared (NULL), like wm_set_repeat_rules; read by wm_decode_begin / wm_decode_begin_ts only (the scoring and alignment
 * replays do not know the bias).  The tables live in device memory allocated once at their maximum size: a captured graph stays valid across tables
 * with the same number of groups.  WM_ERR_ARG (wm_last_error names the cause) from wm_set_sequence_bias: n outside [1, WM_SEQ_BIAS_MAX], a length
 * outside [1, WM_SEQ_BIAS_MAX_LEN], an id outside [0, vocab), a bias that is NaN or +inf, two identical entries; from wm_decode_begin*, which know eos
 * and the path: wm_gen_params.vanilla == 0, a candidate-tree context, a -inf entry of more than one token whose last id is eos — or a one-token one
 * while the exponential decay is on — (the decay's x + |x| p would turn it into NaN). */
#define WM_SEQ_BIAS_MAX 1024       /* entries */
#define WM_SEQ_BIAS_MAX_LEN 16     /* tokens per entry */
typedef struct wm_seq_bias_params {
    const int32_t* tokens;   /* HOST, the entries' ids back to back */
    const int32_t* lens;     /* HOST [n], 1..WM_SEQ_BIAS_MAX_LEN */
    const float*   bias;     /* HOST [n], finite or -inf */
    int32_t n;
} wm_seq_bias_params;
int wm_set_sequence_bias(wm_ctx* ctx, const wm_seq_bias_params* sb /* NULL = off */);

/* Constrained decoding on the plain decode path (additive to ABI v9; csrc/wm_constraint.hip).  Stands in for HF
 * generate(prefix_allowed_tokens_fn=...) — PrefixConstrainedLogitsProcessor (transformers generation/logits_process.py), the interface this replaces —
 * in the one form a decode loop whose logits never leave the device can run: the callback that walks a FIXED LIST of token sequences (a trie).  The
 * reference builds no such processor (model.py:1168-1207).  A table is a non-empty set S of distinct sequences of 1..WM_CONSTRAINT_MAX_LEN ids in
 * [0, vocab); eos stands inside none of them and closes every one implicitly.  For a row with prefix ids[:len], P = wm_gen_params.prompt_len (one for
 * all streams, also under wm_set_stream_prompts), g = ids[P:len], t = len - P, the allowed set A(g) is
 *   every s[t] of the s in S with len(s) > t and s[:t] == g; plus eos when some s == g (a sequence that is a prefix of another gives both); eos alone
 *   when no s starts with g (the function is total: HF's processor raises on an empty list instead),
 * and the row is edited IN PLACE: x[v] stays for v in A(g), every other element becomes -inf.  Allowed elements are not rewritten, so the row equals
 * HF's scores + mask as fp32 values on rows without +inf / NaN.  Nothing is kept per stream: the set is derived from the row's own ids on every step
 * (two binary searches over the sorted table, ceil(log2(n + 1)) dependent loads whatever t is), so beam reorders, finished streams and the tap need
 * nothing.  HF's order puts the processor behind sequence bias, repetition penalty, no-repeat n-grams and bad words and before the suppress lists; a
 * -inf mask commutes with all of them, so the engine applies it to the raw row right behind the sequence bias — under beams behind the log-softmax
 * normaliser, where the bias goes.  It does not commute with the exponential decay on eos (-inf + inf p is NaN in HF too): refused.
 * Sticky on the context until cleared (NULL), like wm_set_sequence_bias; read by wm_decode_begin / wm_decode_begin_ts only (the scoring and alignment
 * replays do not know the mask).  The tables live in device memory allocated once at their maximum size: a captured graph stays valid across tables
 * with the same number of sequences.  WM_ERR_ARG (wm_last_error names the cause) from wm_set_constraint: n outside [1, WM_CONSTRAINT_MAX], a length
 * outside [1, WM_CONSTRAINT_MAX_LEN], an id outside [0, vocab), two identical sequences; from wm_decode_begin*, which know eos, the path and the lists:
 * wm_gen_params.vanilla == 0, a candidate-tree context, timestamp rules on (a timestamp is never in the set: the rules would force a row of -inf),
 * the exponential decay on, eos inside a sequence, an id of a sequence in the suppress list, a first id in the begin-suppress list. */
#define WM_CONSTRAINT_MAX 16384    /* sequences */
#define WM_CONSTRAINT_MAX_LEN 32   /* ids per sequence, the closing eos not counted */
typedef struct wm_constraint_params {
    const int32_t* tokens;   /* HOST, the sequences' ids back to back */
    const int32_t* lens;     /* HOST [n], 1..WM_CONSTRAINT_MAX_LEN */
    int32_t n;
} wm_constraint_params;
int wm_set_constraint(wm_ctx* ctx, const wm_constraint_params* c /* NULL = off */);

/* Per-stream decoder prompts of ONE common length (additive to ABI v9).  Stands in for the rows HF's
 * WhisperGenerationMixin._retrieve_init_tokens builds for generate(language=[...]) — one row of init tokens per clip, which differ in the language
 * token alone — and which the reference never builds (model.py:1519-1537 takes one language).  prompts: HOST int32 [B][P], copied; clip b of the next
 * decodes starts from row b.  wm_gen_params.prompt stays what it is — the caller passes a representative row (stream 0's) — and keeps every scalar it
 * defines: P, begin_index, the start of the exponential decay, max_length.  The rows differ in ids only, and the ids of a decode are per-stream state
 * already (ids, L, kvlen, the committed timestamp state): the prompt pass reads each stream's own row, no select kernel changes and the keys of the
 * captured graphs do not see the table — two tables reuse one graph.  With timestamp rules the committed state of ids[begin_index:P] is folded per
 * stream.  With beams (wm_set_beam) B is the number of CLIPS: every beam of clip g starts from row g and the "never set" entry of its finished table
 * (wm_get_beam_result) is row g.  The replays (wm_score_tokens, wm_token_timestamps) take full id rows and need nothing.
 * Sticky on the context until cleared (NULL), like wm_set_repeat_rules / wm_set_sequence_bias; read by wm_decode_begin / wm_decode_begin_ts only.
 * WM_ERR_ARG from wm_set_stream_prompts: B < 1, P < 1 with prompts given; from wm_decode_begin* (wm_last_error names the cause): P !=
 * wm_gen_params.prompt_len, B != the decode's number of clips, an id outside [0, vocab), timestamp rules on and a row whose first id is not below
 * timestamp_begin.  Prompts of different lengths (ragged rows) do not exist. */
int wm_set_stream_prompts(wm_ctx* ctx, const int32_t* prompts /* HOST [B][P], NULL = off */, int B, int P);

/* ---- F3..F14 the Medusa decode loop (replaces _medusa_greedy_search, model.py:404-835) ---- */
int wm_decode_begin(wm_ctx* ctx, const wm_gen_params* gp, int B);
/* wm_decode_begin with the timestamp rules on (ts != NULL; NULL = wm_decode_begin).  WM_ERR_ARG (wm_last_error says why): a candidate tree
 * (medusa_choices with top-k > 1), timestamp_begin != no_timestamps_token_id + 1, eos / the first prompt token not below timestamp_begin,
 * or fewer than 2 timestamp tokens in the vocabulary.  Replaces generate(return_timestamps=True) of the reference / HF. */
int wm_decode_begin_ts(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* ts, int B);
/* Runs up to max_iters iterations (each = base pass + verify pass + accept), replayed from a
 * hipGraph after the first; returns the number of unfinished streams in *n_unfinished.
 * Several streams with candidate chains run the merged-step schedule: max_iters then counts STEPS (one pass each:
 * a stream whose last accept length was 0 spends one step on its base row and verifies in the next; the emitted
 * tokens, accept histogram and per-stream iteration counts are those of the lock-step schedule).
 * Environment: WM_NO_STEP=1 lock-step schedule, WM_NO_CARRY=1 no hidden-state carry, WM_NO_GRAPH=1 eager launches. */
int wm_decode_run(wm_ctx* ctx, int max_iters, int* n_unfinished);
/* ids (prompt + generated, post-EOS overwrite of model.py:798-810 applied) of one stream.  After a beam decode (wm_set_beam): `stream` is the
 * clip and the ids are its finished hypothesis of rank 0 (wm_get_beam_result). */
int wm_get_tokens(wm_ctx* ctx, int stream, int32_t* out /* HOST */, int cap, int* n);
int wm_get_stats(wm_ctx* ctx, wm_stats* out /* HOST */);
int wm_sync(wm_ctx* ctx);

/* ---- token-level timestamps (additive to ABI v9; csrc/wm_align.hip) ----
 * Stands in for HF WhisperGenerationMixin._extract_token_timestamps (transformers generation_whisper.py; `return_token_timestamps=True`,
 * which the reference refuses): HF reads the cross-attentions its autoregressive decode collected; a Medusa loop has none, so the engine
 * replays the FINAL ids teacher-forced (a causal decoder gives every position the same query either way) and taps the alignment heads. */
typedef struct wm_align_params {
    const int32_t* heads;        /* HOST [n_heads][2] = (decoder layer, head): generation_config.alignment_heads.  Layers index Whisper's
                                  * decoder layers (the Medusa-Block extra layer is never one) */
    int32_t n_heads;             /* 1 .. 64 */
    int32_t median_filter_width; /* odd, 1 .. 15; config.median_filter_width (7): HF _median_filter */
    float time_precision;        /* 0.02; read as the decimal it was written from, so that frame * time_precision is HF's double product */
} wm_align_params;
/* Per stream b: ids tokens[b][0 .. lens[b]) (the stream's own end: EOS included, padding excluded), the first n_prompt[b] of them decoder
 * input.  The N = lens - n_prompt - 1 rows of input positions n_prompt .. lens - 2 are aligned to F = n_ctx frames (num_frames[b] / 2 when
 * given): softmax over all n_ctx frames, crop, z-score over the rows, median filter, mean over the heads, DTW (HF _dynamic_time_warping);
 * out[b][t] = 0 for t < n_prompt, the time of the first frame of row t - n_prompt after it, the last value again for the last token and
 * for t >= lens[b].  N <= 1: zeros (nothing is launched for that stream).  Needs wm_encode (else WM_ERR_STATE); WM_ERR_ARG for a layer /
 * head out of range, an even width, lens[b] > n_tgt, n_prompt[b] > lens[b].  The scores read the bf16 cross-K, also on a cross_kv_fp8
 * context (whose bf16 projection stays resident).  Overwrites the decode state like wm_forward_logits (begin again afterwards).  The
 * probabilities live in a workspace allocated on first use and capped (512 MB; WM_ALIGN_WS_MB): the streams are worked in groups that fit. */
int wm_token_timestamps(wm_ctx* ctx, const wm_align_params* ap, int B, const int32_t* tokens /* HOST [B][Tmax] */, int Tmax,
                        const int32_t* lens /* HOST [B] */, const int32_t* n_prompt /* HOST [B] */, const int32_t* num_frames /* HOST [B] or NULL */,
                        float* out /* HOST [B][Tmax] seconds */, float* ms /* hipEvent time of replay + alignment, may be NULL */);

/* ---- token log-probabilities and the no-speech probability (additive to ABI v9; csrc/wm_score.hip) ----
 * Stands in for what HF's greedy decode returns with output_scores (GenerationMixin: `scores[i]`, the processed logits of step i) as consumed by
 * WhisperGenerationMixin._retrieve_avg_logprobs (log_softmax at temperature 1, gathered at the emitted ids), and for WhisperNoSpeechDetection
 * (transformers generation/logits_process.py: softmax of the UNPROCESSED logits of the <|startoftranscript|> row at no_speech_token_id).  The
 * reference refuses no_speech_threshold (model.py:1201-1205) and ignores logprob_threshold.  A Medusa loop processes the rows of an iteration
 * under one shared length (model.py:689-694), so "the scores of step i" do not exist inside it: the engine replays the FINAL ids teacher-forced
 * through all decoder layers in 16-row tiles (the context's own decode contract) and scores every row under its OWN length. */
typedef struct wm_score_params {
    int32_t no_speech_token_id;  /* < 0: no_speech_prob is not computed.  HF: generation_config.no_speech_token_id, default no_timestamps_token_id - 1 */
    int32_t sot_index;           /* index of <|startoftranscript|> in the prompt; < 0: 0.  With prompt_ids it is len(prompt_ids) (HF reads index 0 there) */
} wm_score_params;
/* Per stream b: ids tokens[b][0 .. lens[b]) (the stream's own end: EOS included, padding excluded), scored from position n_prompt[b] on.  For
 * n_prompt <= t < lens: z = base-head logits of input position t - 1; the processors of gp with cur_len = t (exponential decay, begin-suppress at
 * t == begin_index, suppress list; prompt_len / begin_index as wm_decode_begin_ts reads them), then — ts != NULL — HF
 * WhisperTimeStampLogitsProcessor with prefix tokens[b][0 .. t); logprobs[b][t] = log_softmax(processed row)[tokens[b][t]] in fp32, -inf where that
 * id is masked; 0 for t < n_prompt and t >= lens.  no_speech_prob[b] (may be NULL) = softmax(raw row of input position sot_index)[no_speech_token_id].
 * Needs wm_encode (else WM_ERR_STATE); WM_ERR_ARG (wm_last_error says which) for lens[b] > n_tgt, n_prompt[b] > lens[b] or < 1, an id outside the
 * vocabulary, sot_index outside the prompt.  Overwrites the decode state like wm_forward_logits (begin again afterwards).  *ms: hipEvent time of
 * replay + vocabulary projection + scoring. */
int wm_score_tokens(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* ts /* NULL: rules off */, const wm_score_params* sp /* may be NULL */,
                    int B, const int32_t* tokens /* HOST [B][Tmax] */, int Tmax, const int32_t* lens /* HOST [B] */, const int32_t* n_prompt /* HOST [B] */,
                    float* logprobs /* HOST [B][Tmax] */, float* no_speech_prob /* HOST [B] or NULL */, float* ms /* may be NULL */);

/* ---- token alternatives: the best ids of every scored row and the rank of the emitted one (additive to ABI v9; csrc/wm_score.hip) ----
 * Stands in for what a caller of HF's output_scores does with `scores[i]` (torch.topk of its log_softmax) and for the `top_logprobs` of the
 * OpenAI-style APIs, without the rows leaving the device: two kernels behind the scoring kernels of wm_score_tokens, on the same processed rows
 * AFTER the timestamp rules' log-softmax decision (a row the decision forces to a timestamp keeps no text). */
#define WM_TOPK_MAX 8
/* wm_score_tokens plus, for every scored position n_prompt <= t < lens: top_ids[b][t][0 .. topk) / top_logprobs[b][t][0 .. topk) = the topk best
 * tokens of the processed row and their log_softmax values, ordered by value descending, then id ascending; a row that keeps fewer than topk finite
 * entries ends in (-1, -inf).  An id's entry is bit-equal to logprobs[b][t] where it is the emitted id.  ranks[b][t] = 1 + the number of tokens ahead
 * of tokens[b][t] in that order, 0 where it is masked.  Unscored positions: -1, -inf, 0.  logprobs / no_speech_prob / *ms and every error as
 * wm_score_tokens, from the same launches; WM_ERR_ARG (wm_last_error names it) for topk outside [1, WM_TOPK_MAX]. */
int wm_score_tokens_topk(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* ts /* NULL: rules off */, const wm_score_params* sp /* may be NULL */,
                         int B, const int32_t* tokens /* HOST [B][Tmax] */, int Tmax, const int32_t* lens /* HOST [B] */, const int32_t* n_prompt /* HOST [B] */,
                         int topk, float* logprobs /* HOST [B][Tmax] */, float* no_speech_prob /* HOST [B] or NULL */,
                         int32_t* top_ids /* HOST [B][Tmax][topk] */, float* top_logprobs /* HOST [B][Tmax][topk] */, int32_t* ranks /* HOST [B][Tmax] */,
                         float* ms /* may be NULL */);

/* ---- language detection on the device (additive to ABI v9; csrc/wm_lang.hip) ----
 * Stands in for HF WhisperGenerationMixin.detect_language (transformers generation_whisper.py), which the reference reaches through
 * _retrieve_init_tokens when `language` is None (model.py:1519-1537): one decoder pass over <|startoftranscript|>, every id that is no language token
 * masked to -inf, arg-max.  Needs wm_encode with the same B (else WM_ERR_STATE).  One base pass over start_token at position 0 for all B streams —
 * the launches of wm_forward_logits(.., T = 1, pos0 = 0, disable_medusa = 1), one batch instead of stream by stream — then k_lang_pick: one block
 * per row gathers the n candidates lang_ids (HOST int32 [n]) from the row and reduces them (wave64 shuffles, one LDS round across the waves; no
 * atomics, no sweep of the vocabulary).  out[b] (HOST int32 [B]) = the candidate with the largest value, among equal values the SMALLEST TOKEN ID —
 * what HF's mask + argmax and torch.argmax on the CPU return; the answer does not depend on the order of lang_ids, the row's slot or B.  B ints come
 * back, never a logits row.  A NaN candidate counts as -inf; when every candidate is -inf the smallest id wins.  *ms (may be NULL): hipEvent time of
 * pass + pick.  Overwrites the decode state like wm_forward_logits (begin again afterwards); the captured graphs are kept.
 * WM_ERR_ARG (wm_last_error names the cause): n outside [1, WM_LANG_MAX], an id outside [0, vocab), two equal ids, start_token outside the
 * vocabulary, a null pointer. */
#define WM_LANG_MAX 256
int wm_detect_language(wm_ctx* ctx, int B, const int32_t* lang_ids /* HOST [n] */, int n, int32_t start_token, int32_t* out /* HOST [B] */,
                       float* ms /* may be NULL */);

/* ---- stitching overlapping long-form windows (additive to ABI v9; csrc/wm_merge.hip) ----
 * Stands in for the merge of the Hugging Face ASR pipeline over strided chunks (pipelines/automatic_speech_recognition.py chunk_iter cuts them):
 * transformers' _find_longest_common_sequence (models/whisper/tokenization_whisper.py), a Python loop over up to len(left) + len(right) shifts per
 * boundary — one numpy compare per shift, a Python generator per shift with token timestamps.  Here: one kernel, one launch for all boundaries of
 * all recordings of a call.
 * Clip c owns the windows first[c] .. first[c + 1], in time order; W = first[C].  Window w holds the TEXT ids tokens[w][0 .. lens[w]) (prompt, EOS
 * and padding already removed) and contributes tokens[w][keep[w][0] .. keep[w][1]) to its clip: the clip's text is those slices in order.
 * Per clip, over its non-empty windows (lens[w] == 0: keep = (0, 0), and the window is no link of the chain — the left sequence carries over, as
 * the pipeline's `if current_tokens:` has it): a = 0 for the first; left = that window from a on, L ids, right = the next window, R ids.  For
 * every shift i in 1 .. L + R - 1: left_start = max(0, L - i), left_stop = min(L, L + R - i), right_start = max(0, i - L), right_stop = min(R, i);
 * matches = the positions with equal ids — with times != NULL also time_left <= time_right, compared as the float32 values given —; score = the
 * double (double)matches / i + (double)i / 10000.0 (two IEEE divisions, one addition: HF's Python floats).  A shift counts with matches > 1; the
 * best score wins, among equal scores the smallest i; none counting: (L, L, 0, 0), a plain concatenation.  left_mid = (left_start + left_stop) / 2,
 * right_mid = (right_start + right_stop) / 2: keep[w] = (a, a + left_mid), the next window starts at a = right_mid; the last non-empty window keeps
 * (a, lens[w]).  A clip of one window keeps all of it; a clip may own no window.
 * k_merge_windows: one block of 256 threads per clip walks the clip's chain with both sequences in LDS; the shifts of a boundary are spread over
 * the threads, the best (score, i) is reduced by wave64 shuffles and one LDS round (no atomics; integer counts, so no order dependence).
 * One upload, one launch, one download of 2 W ints on the context's stream, in a workspace of its own (allocated on first use, freed by
 * wm_destroy).  Reads and writes nothing of the decode state: no wm_encode needed, the captured graphs and a decode in progress are untouched.
 * *ms (may be NULL): hipEvent time of upload + kernel + download.
 * WM_ERR_ARG (wm_last_error names the cause): a null pointer, C < 1, first not ascending from 0, W > WM_MERGE_WINDOWS_MAX, lens[w] outside
 * [0, min(Tmax, WM_MERGE_LEN_MAX)]. */
#define WM_MERGE_LEN_MAX      512     /* tokens per window */
#define WM_MERGE_WINDOWS_MAX 4096     /* windows per call, all clips together */
int wm_merge_windows(wm_ctx* ctx, int C, const int32_t* first /* HOST [C+1] */,
                     const int32_t* tokens /* HOST [W][Tmax] */, int Tmax, const int32_t* lens /* HOST [W] */,
                     const float* times /* HOST [W][Tmax] or NULL */,
                     int32_t* keep /* HOST [W][2] */, float* ms /* may be NULL */);

/* ---- grouping token ids into words (additive to ABI v9; csrc/wm_words.hip, csrc/wm_words.h) ----
 * Stands in for transformers' _combine_tokens_into_words (models/whisper/tokenization_whisper.py: _split_tokens_on_unicode, _split_tokens_on_spaces,
 * _merge_punctuations), the grouping behind the ASR pipeline's return_timestamps="word": there one tokenizer.decode per token on a growing list and
 * two list-rewriting passes, here one kernel launch for all rows of a call, on the bytes of the vocabulary.
 * wm_set_word_table: the bytes of token t are bytes[offsets[t] .. offsets[t + 1]), t < n_tokens (= eos_token_id: text ids only).  Uploaded once; the
 * context owns its device copy, a later call replaces it, wm_destroy frees it.  WM_ERR_ARG (wm_last_error names the cause): a null pointer, n_tokens
 * outside [1, WM_WORDS_TOKENS_MAX], offsets not strictly ascending from 0 (every token has at least one byte), more than WM_WORDS_BYTES_MAX bytes.
 * wm_word_spans: row r is the ids[first[r] .. first[r + 1]) (text ids, every one below the table's n_tokens; a row may be empty and has no cap on
 * its length), under modes[r].  The words of a row are contiguous runs that partition it in order: n_words[r] and the ascending start indices
 * word_first[first[r] + r + (0 .. n_words[r])], the last of them the row's length (row r owns len + 1 slots; those behind are zero).
 *   Pieces: append the bytes of each token in turn; a piece closes behind token t when the bytes gathered since the last close are strict UTF-8
 *   (what bytes.decode("utf-8") accepts).  Tokens left over at the end of the row are a last piece of their own.
 *   Words, WM_WORDS_SPACES: a piece opens a new word if its first byte is 0x20, or strip(piece) is a substring of !"#$%&'()*+,-./:;<=>?@[\]^_`{|}~
 *   (the empty string is one: a whitespace-only piece counts as punctuation), or there is no word yet; else it is appended to the last word.
 *   strip is Python's: the code points with str.isspace() — U+0009-000D, 001C-0020, 0085, 00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F, 3000 —
 *   leave at both ends; on bytes, their UTF-8 encodings.  WM_WORDS_UNICODE (HF: chinese, japanese, thai, lao, myanmar, cantonese): every piece is
 *   a word.
 *   Prepend pass (HF: right to left, i = n - 2, j = n - 1): word i merges into word j when it starts with 0x20 and strip(word i) is a substring
 *   of "'“¡¿([{- ; else j = i.  The last word is never tested.  Stated forwards: a maximal run of such words joins the word behind it.
 *   Append pass (left to right, i = 0, j = 1): word j merges into word i when word i does not end in 0x20 and word j, unstripped, is a substring of
 *   "'.。,，!！?？:：”)]}、 ; else i = j.  A slot the first pass emptied is the empty string and passes the test, as in HF; it changes no cut.
 *   Substring tests are on UTF-8 bytes (equal to tests on code points for valid text).
 * Equal to transformers for rows whose concatenated bytes are valid UTF-8 without U+FFFD; outside (a truncated character at the end of a row, a
 * stray continuation byte: HF's replacement-character bookkeeping cuts elsewhere) the rules above are the contract.
 * times (may be NULL): float32 (start, end) per id; word_times[first[r] + w] = (start of the word's first token, end of its last).  logprobs (may be
 * NULL): float32 per id; word_logprobs[first[r] + w] = the float32 sum in ascending token order divided by the count in float32.  Entries behind a
 * row's n_words are zero.
 * k_word_spans: one block of 256 threads per row, the row in tiles of 1024 tokens: the threads gather every token's bytes from the table and
 * summarise them into LDS (first bytes, the token as a map on the nine states of strict UTF-8), thread 0 walks the tile under carried state (the
 * UTF-8 state, the open piece, word and prepend run with their streamed substring tests), then the threads fill times and log-probabilities, a word
 * each.  No atomics, plain vector stores, nothing depends on an order of execution.
 * One upload, one launch, one download on the context's stream, in a workspace and with an event pair of its own (allocated on first use, freed
 * by wm_destroy).  Reads and writes nothing of the decode state: no wm_encode needed, no wm_decode_invalidate, the captured graphs and a decode in
 * progress (between wm_decode_begin and wm_decode_run) are untouched.  *ms (may be NULL): hipEvent time of upload + kernel + download.
 * WM_ERR_ARG (wm_last_error names the cause): a null pointer (times without word_times, logprobs without word_logprobs), R outside
 * [1, WM_WORDS_ROWS_MAX], first not ascending from 0, first[R] > WM_WORDS_IDS_MAX, a mode that is neither constant, an id outside the table.
 * WM_ERR_STATE: no table set. */
#define WM_WORDS_SPACES  0
#define WM_WORDS_UNICODE 1
#define WM_WORDS_ROWS_MAX    65536          /* rows per call */
#define WM_WORDS_IDS_MAX     (4 << 20)      /* ids per call, all rows together */
#define WM_WORDS_TOKENS_MAX  (1 << 20)      /* vocabulary entries */
#define WM_WORDS_BYTES_MAX   (64 << 20)     /* bytes of the vocabulary */
int wm_set_word_table(wm_ctx* ctx, const uint8_t* bytes /* HOST [offsets[n_tokens]] */, const int32_t* offsets /* HOST [n_tokens+1] */, int n_tokens);
int wm_word_spans(wm_ctx* ctx, int R, const int32_t* first /* HOST [R+1] */, const int32_t* ids /* HOST [first[R]] */,
                  const int32_t* modes /* HOST [R] */, const float* times /* HOST [first[R]][2] or NULL */,
                  const float* logprobs /* HOST [first[R]] or NULL */,
                  int32_t* n_words /* HOST [R] */, int32_t* word_first /* HOST [first[R] + R] */,
                  float* word_times /* HOST [first[R]][2]; may be NULL without times */,
                  float* word_logprobs /* HOST [first[R]]; may be NULL without logprobs */, float* ms /* may be NULL */);

/* ---- speech windows of long recordings (additive to ABI v9; csrc/wm_vad.hip, csrc/wm_vad.h) ----
 * The recipe WhisperX and faster-whisper (vad_filter=True) made standard — find the speech, cut only at pauses, pack the speech into windows of at
 * most one model window — with an energy detector in the place of a trained VAD model: the contract below is the engine's own, as sampling_top_k's
 * and allowed_sequences' are.
 * Inputs: C recordings of 16 kHz mono float32 on the DEVICE, samples[c * n_max + i]; n_samples[c] (HOST, in [1, n_max]): samples behind it count as
 * 0 and are not read.  T_c = ceil(n_samples[c] / 160) frames of 10 ms: the log-mel's hop, a frame index is a mel frame index.
 * Parameters (wm_vad_params; WM_ERR_ARG names the cause): 0 < k_off <= k_on; 0 <= abs_off <= abs_on, finite; q_permille in [0, 1000];
 * min_silence >= 1, min_speech >= 1, pad >= 0, F >= 2 (the longest window), all in frames and at most WM_VAD_FRAMES_MAX.
 * Per recording:
 *   1. Energy: E[t] = sum over k < 160 of x[160 t + k]^2 in float32, in this order: sixteen partial sums p_j = sum over i = 0..9 of
 *      x[160 t + 16 i + j]^2, i ascending, every term a rounded multiply followed by a rounded add (no fused multiply-add); then p_j += p_{j+8},
 *      p_j += p_{j+4}, p_j += p_{j+2}, p_0 += p_1.  A float32 numpy loop gives the same bits.
 *   2. Loud level: R = the order statistic of rank (q_permille * (T - 1)) / 1000 (64-bit integer division) among E[0 .. T), values ordered by
 *      their float32 bit patterns as unsigned integers (E >= +0: the numeric order); no interpolation.
 *   3. Thresholds: thr_on = fmaxf(R * k_on, abs_on), thr_off = fmaxf(R * k_off, abs_off), one float32 multiply each.  The detector is relative to
 *      the recording's loud level, not to a noise floor: a recording without pauses degrades to "all speech" (cut at its quietest frames by
 *      step 6), never to "no speech"; digital silence (R = 0) falls under abs_on.
 *   4. Hysteresis: s[-1] = 0; s[t] = 1 if E[t] >= thr_on, 0 if E[t] < thr_off, else s[t-1].
 *   5. Regions: the maximal runs [a, b) of s = 1; neighbours whose gap a' - b < min_silence merge; merged regions with b - a < min_speech are
 *      dropped; then padding: neighbours with gap g both move by pad if g >= 2 * pad, else both meet at b + g / 2 (integer division); the first
 *      start is max(0, a - pad), the last stop min(T, b + pad).
 *   6. Split: a region with b - a > F is cut at c, the frame of smallest E (bit-pattern order, the smallest t among equals) in
 *      [a + F/2, a + F], ends inclusive: emit [a, c), a = c, repeat.
 *   7. Pack, greedy over the pieces in order: a window opens at a piece's start u and absorbs following pieces while stop - u <= F; the window
 *      is (u, last stop).  Every window is at most F frames, starts and ends inside a region, and every region frame lies in exactly one window.
 * Outputs (HOST): n_regions[c] and n_windows[c]; the (start, stop) frame pairs back to back in the order of the recordings — the padded regions of
 * step 5 (before splitting) in regions, the windows of step 7 in windows.  cap_regions / cap_windows: the pairs the caller's buffers hold; a result
 * that does not fit is WM_ERR_ARG, the message names the needed counts, and no output is written.  Bounds a caller can size by: a recording has at
 * most (T + min_silence) / (min_speech + min_silence) + 1 regions and at most that plus T / (F / 2) windows.
 * Parity taps, each may be NULL: E [sum of T_c] back to back, R / thr_on / thr_off [C].
 * Limits: WM_VAD_CLIPS_MAX recordings, WM_VAD_FRAMES_MAX frames per recording (46 h), WM_VAD_TOTAL_FRAMES_MAX frames per call,
 * WM_VAD_WINDOWS_MAX windows per call (more: WM_ERR_ARG, "split the call").
 * Kernels: all per-frame work is parallel over frames — the energy with 16 lanes per frame, R by a radix select over the bit patterns (LDS
 * histograms merged with integer vector atomics), the hysteresis as a running maximum over "2 t + on if decisive, else -1", the run boundaries
 * compacted by a prefix sum; scan state crosses blocks by chained launches (tile summaries, a scan of the summaries, apply), never by blocks
 * waiting on each other.  The per-region stage walks on one lane per recording, the search of step 6 is a block-wide reduction.  Ten launches
 * per call whatever C; integers and bit patterns only: two runs give the same bytes.
 * On the context's stream, in a workspace and with an event pair of its own (allocated on first use, freed by wm_destroy).  Reads and writes
 * nothing of the decode state: no wm_encode needed, no wm_decode_invalidate, the captured graphs and a decode in progress (between wm_decode_begin
 * and wm_decode_run) are untouched.  *ms (may be NULL): hipEvent time of upload + kernels + download. */
#define WM_VAD_CLIPS_MAX         4096
#define WM_VAD_FRAMES_MAX        (1 << 24)      /* frames per recording */
#define WM_VAD_TOTAL_FRAMES_MAX  (1 << 25)      /* frames per call, all recordings together */
#define WM_VAD_WINDOWS_MAX       65536          /* windows per call */
typedef struct wm_vad_params {
    float k_on, k_off;                  /* thresholds relative to the loud level R */
    float abs_on, abs_off;              /* absolute floors of the thresholds (frame energies) */
    int32_t q_permille;                 /* the rank of R */
    int32_t min_silence, min_speech;    /* frames */
    int32_t pad;                        /* frames */
    int32_t F;                          /* frames: the longest window */
} wm_vad_params;
int wm_vad_windows(wm_ctx* ctx, int C, const float* samples /* DEVICE [C][n_max] */, int64_t n_max, const int64_t* n_samples /* HOST [C] */,
                   const wm_vad_params* params,
                   int32_t* n_regions /* HOST [C] */, int32_t* regions /* HOST [cap_regions][2] */, int cap_regions,
                   int32_t* n_windows /* HOST [C] */, int32_t* windows /* HOST [cap_windows][2] */, int cap_windows,
                   float* E /* HOST [sum T_c] or NULL */, float* R /* HOST [C] or NULL */, float* thr_on /* HOST [C] or NULL */,
                   float* thr_off /* HOST [C] or NULL */, float* ms /* may be NULL */);

/* ---- live transcription: the agreement step of streaming sessions (additive to ABI v9; csrc/wm_stream.hip, csrc/wm_stream.h) ----
 * The LocalAgreement-2 policy of Macháček et al., "Turning Whisper into Real-Time Transcription System" (2023), known from the whisper_streaming
 * tool: a recording grows chunk by chunk, its rolling buffer is transcribed again on every tick, and a word is committed once two consecutive
 * hypotheses agree on it.  One call decides that for the S sessions of a tick; the contract below is the engine's own, as wm_vad_windows' is.
 * Word lists.  Each session has three lists of words, all given as token ids: new_list (this tick's hypothesis), prev_list (the uncommitted rest
 * of the last tick's hypothesis) and tail_list (at most WM_STREAM_TAIL committed words, in order, newest last).  A list is three HOST arrays
 * (wm_stream_list): words[S + 1], ascending from 0 — session s owns the words words[s] .. words[s + 1]); tok[words[S] + 1], ascending strictly
 * from 0 — word w is the ids[tok[w] .. tok[w + 1]), at least one id per word; ids[tok[words[S]]], text ids below the n_tokens of wm_set_word_table.
 * times: int32 (start, end) per word of new_list, in CENTISECONDS on the recording's clock.  last_cs[s]: the end of the session's last committed
 * word, 0 before the first commit.  params (NULL: the defaults): late_cs >= 0 (WM_STREAM_LATE_CS), near_cs >= 0 (WM_STREAM_NEAR_CS), max_ngram in
 * [1, WM_STREAM_TAIL] (default WM_STREAM_TAIL).
 * Key of a word: the bytes of its tokens, concatenated in order, with every leading and every trailing byte 0x20 removed — no other whitespace,
 * inner bytes are kept, an all-space word has the empty key.  Two words are equal iff their keys are byte-equal: case and punctuation count,
 * tokenisation does not (" hel" + "lo" = " hello" = "hello").
 * Per session, with n / P / C the words of new / prev / tail:
 *   1. Late words: k0 = the smallest w with start[w] > last_cs - late_cs, or n if there is none (a prefix, not a filter).
 *   2. Overlap with what is committed, only if k0 < n, C > 0 and |start[k0] - last_cs| < near_cs: for i = 1 .. min(C, n - k0, max_ngram), ascending,
 *      test whether the last i words of tail equal new[k0 .. k0 + i) word for word; at the first i that matches, k0 += i and the loop stops.
 *   3. Agreement: m = the largest m <= min(n - k0, P) with new[k0 + j] == prev[j] for all j < m.
 *   4. Sentence end: ender = the largest w in [k0, k0 + m) whose key ends in one of . ? ! 。 (E3 80 82) ？ (EF BC 9F) ！ (EF BC 81), or -1.
 * Outputs (HOST int32 [S] each): skip = k0, commit = m, ender.  The caller commits new[k0 .. k0 + m) and keeps new[k0 + m ..) as the next prev.
 * k_stream_agree: one block of 256 threads per session, one launch.  Step 1 is a block minimum over the words, step 2 at most 15 word compares on
 * one lane, step 3 a block minimum over the first mismatch — every lane walks the two byte streams of every 256th word pair through the table, a
 * counter of pending spaces drops the trailing ones without look-ahead —, step 4 a block maximum; block barriers between the steps.  Integers
 * and bytes only, no atomics, plain vector stores: two runs give the same bytes.
 * One upload, one launch, one download on the context's stream, in a workspace and with an event pair of its own (allocated on first use, freed
 * by wm_destroy).  Reads and writes nothing of the decode state: no wm_encode needed, no wm_decode_invalidate, the captured graphs and a decode in
 * progress (between wm_decode_begin and wm_decode_run) are untouched.  *ms (may be NULL): hipEvent time of upload + kernel + download.
 * WM_ERR_ARG (wm_last_error names the cause): a null pointer, S outside [1, WM_STREAM_SESSIONS_MAX], words or tok not ascending from 0, a word
 * without ids, more than WM_STREAM_TAIL tail words for a session, an id outside the table, more than WM_STREAM_WORDS_MAX words or
 * WM_STREAM_IDS_MAX ids in the three lists together, a parameter out of range.  WM_ERR_STATE: no table set. */
#define WM_STREAM_TAIL          5               /* committed words per session in tail_list; the longest overlap tested */
#define WM_STREAM_SESSIONS_MAX  4096            /* sessions per call */
#define WM_STREAM_WORDS_MAX     (1 << 20)       /* words per call, the three lists together */
#define WM_STREAM_IDS_MAX       (4 << 20)       /* ids per call, the three lists together */
#define WM_STREAM_LATE_CS       10              /* default late_cs */
#define WM_STREAM_NEAR_CS       100             /* default near_cs */
typedef struct wm_stream_list {
    const int32_t* words;               /* HOST [S+1] */
    const int32_t* tok;                 /* HOST [words[S]+1] */
    const int32_t* ids;                 /* HOST [tok[words[S]]] */
} wm_stream_list;
typedef struct wm_stream_params {
    int32_t late_cs;                    /* words starting at or before last_cs - late_cs are dropped from the front */
    int32_t near_cs;                    /* the overlap test applies when the first kept word starts within near_cs of last_cs */
    int32_t max_ngram;                  /* the longest overlap tested, 1 .. WM_STREAM_TAIL */
} wm_stream_params;
int wm_stream_agree(wm_ctx* ctx, int S, const wm_stream_list* new_list, const wm_stream_list* prev_list, const wm_stream_list* tail_list,
                    const int32_t* times /* HOST [new_list->words[S]][2] */, const int32_t* last_cs /* HOST [S] */,
                    const wm_stream_params* params /* NULL: the defaults */,
                    int32_t* skip /* HOST [S] */, int32_t* commit /* HOST [S] */, int32_t* ender /* HOST [S] */, float* ms /* may be NULL */);

/* ---- parity taps (test-only views of intermediate state; no reference equivalent except
 * forward(), model.py:1223-1347) ---- */
/* encoder output [B][n_ctx][d_model] as float32 to HOST */
int wm_get_encoder_output(wm_ctx* ctx, int B, float* out /* HOST */);
/* One decoder pass for stream 0..B-1 over T (<=16) tokens each at positions pos0.., appending
 * K/V at kv row pos0; logits_out HOST float32 [n_out][B][T][vocab], n_out = 1 if disable_medusa
 * else K+1 (all T rows, as forward() returns).  Uses (and overwrites) the decode-loop state: call it
 * before wm_decode_begin, or begin again afterwards. */
int wm_forward_logits(wm_ctx* ctx, int B, const int32_t* tokens /* HOST [B][T] */, int T, int pos0,
                      int disable_medusa, float* logits_out);
/* Timestamp parity tap: R caller-given logits rows (HOST float32 [R][vocab]) through the decode loop's state fold and select kernels
 * (k_select1_ts / k_select2_ts), as verify rows whose prefixes are prefixes[r][0 .. lens[r]) (HOST int32 [R][Tmax]).  The
 * suppress and begin-suppress lists of gp apply with cur_len = lens[0] for every row (the reference's one-length convention), the
 * exponential decay does not; the sampling temperature is gp->temperature.  Outputs (HOST, [R] each): the processed arg-max, p(probe_tokens[r]) under the softmax at 1/T, the entropy
 * H = -sum p log(p + 1e-5) (medusa_utils.py:566-568), and 1 where the log-softmax decision masked all text.  What it stands in for: HF
 * WhisperTimeStampLogitsProcessor.__call__ on one row plus the typical-acceptance statistics.  Overwrites the decode state like
 * wm_forward_logits (begin again afterwards).  Any R >= 1 (worked in groups of WM_TAP_ROWS, csrc/wm_internal.h). */
int wm_select_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* ts, int R, const float* logits, const int32_t* prefixes,
                   int Tmax, const int32_t* lens, const int32_t* probe_tokens, int32_t* out_argmax, float* out_p_probe, float* out_entropy,
                   int32_t* out_ts_forced);
/* Sampling parity tap, the counterpart of wm_select_rows with the same row chunking: R caller-given logits rows (HOST float32 [R][vocab]) through
 * k_sample1 / k_sample_fin, row r under prefix prefixes[r][0 .. lens[r]) (HOST int32 [R][Tmax]) at position lens[r] — its own length for the
 * processors of gp, exponential decay included — with stream key keys[r] (HOST [R]); ts NULL: timestamp rules off (the repetition rules of the
 * context apply either way).  sp: temperature and seed (stream_keys / n_keys are not read).  Outputs (HOST, [R] each): the drawn token, the winner's
 * perturbed value v / T + g, and 1 where the log-softmax decision masked all text.  WM_ERR_ARG for lens outside [1, min(Tmax, n_tgt)] or a bad
 * temperature.  Overwrites the processors' tables and the stream keys of the decode state (begin again afterwards).  Any R >= 1. */
int wm_sample_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* ts /* may be NULL */, const wm_sample_params* sp, int R,
                   const float* logits, const int32_t* prefixes, int Tmax, const int32_t* lens, const uint64_t* keys /* HOST [R] */,
                   int32_t* out_token, float* out_value /* winner's perturbed value */, int32_t* out_forced);
/* Filter parity tap, the counterpart of wm_sample_rows with the same inputs plus the filter f (not NULL; all three off is allowed and runs
 * wm_sample_rows' kernels): the rows go through k_sample1 / k_filter_prep / k_filter_row.  Outputs (HOST, [R] each): out_thr the row's threshold tau
 * (-inf: nothing is cut), out_kept the number of ids the decision leaves with v >= tau (both only written while a filter is on: -inf and -1
 * otherwise), then wm_sample_rows' forced, token and value.  WM_ERR_ARG as wm_sample_rows, and for a filter wm_set_sampling_filter refuses. */
int wm_filter_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* ts /* may be NULL */, const wm_sample_params* sp,
                   const wm_sample_filter* f, int R, const float* logits, const int32_t* prefixes, int Tmax, const int32_t* lens,
                   const uint64_t* keys /* HOST [R] */, float* out_thr, int32_t* out_kept, int32_t* out_forced, int32_t* out_token, float* out_value);
/* Beam-search parity tap (HF GenerationMixin._beam_search steps b to g on caller-given rows): S steps of logits (HOST float32 [S][G][n][vocab],
 * n = bp->num_beams, G clips) through the select, bookkeeping and ids-reorder kernels of the beam decode — no model, no K/V.  Stream s = g * n + j
 * starts from prefixes[s][0 .. prefix_len) (HOST int32 [G * n][Tmax]; one common length, >= gp->prompt_len = P of the length penalty) with running
 * score init_scores[s] (HOST [G * n]; NULL: HF's first-step [0, -1e9, ..] per clip); ts NULL: timestamp rules off (the repetition rules of the
 * context apply either way).  A clip that is done stops changing; the steps it took go to out_steps[g] (S when it never finished).
 * Outputs (HOST): per step the ordered 2n candidates of every clip — cand_val / cand_beam / cand_tok [S][G][2n] (entries of a clip's steps past its
 * end are not defined) — and beam_idx [S][G * n] (the source stream of every stream, s itself for a clip that is done); at the end the finished
 * table — fin_ids [G][n][Tmax], fin_len / fin_score / fin_set [G][n] — and the running beams: run_ids [G * n][Tmax], run_len [G * n], run_score
 * [G * n].  WM_ERR_ARG (wm_last_error says why): G * n > max_batch, prefix_len outside [max(P, 1), Tmax], prefix_len + S > min(Tmax, n_tgt), a bad
 * bp.  Overwrites the decode state like wm_forward_logits (begin again afterwards). */
int wm_beam_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* ts /* may be NULL */, const wm_beam_params* bp, int G, int S,
                 const float* logits, const int32_t* prefixes, int Tmax, int prefix_len, const float* init_scores /* may be NULL */,
                 float* cand_val, int32_t* cand_beam, int32_t* cand_tok, int32_t* beam_idx, int32_t* out_steps,
                 int32_t* fin_ids, int32_t* fin_len, float* fin_score, int32_t* fin_set, int32_t* run_ids, int32_t* run_len, float* run_score);
/* Sequence-bias parity tap (HF SequenceBiasLogitsProcessor.__call__ on caller-given rows): the kernel alone, no model.  R rows (HOST float32
 * [R][vocab]) through k_seq_bias under the entries of sb (checked and grouped as wm_set_sequence_bias does; the context's own sticky table is
 * untouched and back in place afterwards), row r under prefix prefixes[r][0 .. lens[r]) (HOST int32 [R][Tmax]); out (HOST float32 [R][vocab]) = the
 * edited rows.  WM_ERR_ARG (wm_last_error names the cause) for a bad sb, R < 1, lens outside [1, Tmax].  Overwrites ctx->logits of the decode state
 * (begin again afterwards).  Any R >= 1 (worked in groups of WM_TAP_ROWS, csrc/wm_internal.h). */
int wm_seq_bias_rows(wm_ctx* ctx, const wm_seq_bias_params* sb, int R,
                     const float* logits /* HOST [R][vocab] */,
                     const int32_t* prefixes /* HOST [R][Tmax] */, int Tmax, const int32_t* lens /* [R] */,
                     float* out /* HOST [R][vocab] */);
/* Constraint parity tap (HF PrefixConstrainedLogitsProcessor.__call__ on caller-given rows): the kernel alone, no model.  R rows (HOST float32
 * [R][vocab]) through k_constraint under the sequences of c (checked and sorted as wm_set_constraint does; the context's own sticky table is
 * back in place afterwards), row r under prefix prefixes[r][0 .. lens[r]) (HOST int32 [R][Tmax]) whose first prompt_len ids are the decoder prompt;
 * out (HOST float32 [R][vocab]) = the masked rows, n_allowed[r] (may be NULL) = |A| of row r.  WM_ERR_ARG (wm_last_error names the cause) for a bad
 * c, eos outside the vocabulary or inside a sequence, R < 1, lens outside [1, Tmax] or below prompt_len.  Overwrites ctx->logits of the decode state
 * (begin again afterwards).  Any R >= 1 (worked in groups of WM_TAP_ROWS, csrc/wm_internal.h). */
int wm_constraint_rows(wm_ctx* ctx, const wm_constraint_params* c, int eos, int prompt_len, int R,
                       const float* logits /* HOST [R][vocab] */,
                       const int32_t* prefixes /* HOST [R][Tmax] */, int Tmax, const int32_t* lens /* [R] */,
                       float* out /* HOST [R][vocab] */, int32_t* n_allowed /* HOST [R], may be NULL */);
/* Language-pick parity tap (HF detect_language's mask + argmax on caller-given rows): k_lang_pick alone, no model.  R rows (HOST float32 [R][vocab])
 * under the candidates lang_ids (HOST int32 [n]); out (HOST int32 [R]) as wm_detect_language defines it.  WM_ERR_ARG (wm_last_error names the cause)
 * as wm_detect_language's for lang_ids / n, and for R < 1 or a null pointer.  Overwrites ctx->logits of the decode state (begin again afterwards).
 * Any R >= 1 (worked in groups of WM_TAP_ROWS, csrc/wm_internal.h). */
int wm_lang_pick_rows(wm_ctx* ctx, int R, const float* logits /* HOST [R][vocab] */, const int32_t* lang_ids /* HOST [n] */, int n,
                      int32_t* out /* HOST [R] */);
/* The K/V reorder of a beam step alone (HF: Cache.reorder_cache(beam_idx) behind _beam_search step g): stream s < B_streams takes over the self
 * K/V rows [0, len) of every kv layer from stream beam_idx[s] (HOST int32 [B_streams], each in [0, B_streams)), through the shadow buffer;
 * beam_idx[s] == s moves nothing.  WM_ERR_ARG for B_streams outside [1, max_batch], len outside [1, n_tgt], an index out of range.  Overwrites
 * kvlen of the decode state (begin again afterwards). */
int wm_beam_reorder_kv(wm_ctx* ctx, int B_streams, const int32_t* beam_idx /* HOST */, int len);
/* Scoring parity tap, the counterpart of wm_select_rows: R caller-given logits rows (HOST float32 [R][vocab]) through the scoring kernels of
 * wm_score_tokens only, row r under prefix prefixes[r][0 .. lens[r]) (HOST int32 [R][Tmax]) with cur_len = lens[r] — its own length, exponential
 * decay included — and target targets[r]; ts NULL: rules off.  out_logprob HOST [R]: what HF's log_softmax(processors(row))[target] gives, -inf for
 * a masked target.  WM_ERR_ARG for lens outside [1, min(Tmax, n_tgt)] or a target outside the vocabulary.  Overwrites the processors' tables of the
 * decode state (begin again afterwards).  Any R >= 1. */
int wm_score_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* ts, int R, const float* logits, const int32_t* prefixes,
                  int Tmax, const int32_t* lens, const int32_t* targets, float* out_logprob);
/* Alternatives parity tap, the counterpart of wm_score_rows with the same rows, prefixes, lengths, targets, checks and error codes: row r through the
 * scoring kernels and the two top-k kernels.  Outputs (HOST): top_ids / top_logprobs [R][topk] and ranks [R] as wm_score_tokens_topk defines them.
 * WM_ERR_ARG (wm_last_error names it) for topk outside [1, WM_TOPK_MAX].  Overwrites the processors' tables of the decode state.  Any R >= 1. */
int wm_topk_rows(wm_ctx* ctx, const wm_gen_params* gp, const wm_timestamp_params* ts, int R, const float* logits, const int32_t* prefixes,
                 int Tmax, const int32_t* lens, const int32_t* targets, int topk, int32_t* top_ids, float* top_logprobs, int32_t* ranks);
/* Alignment parity taps: views of the last wm_token_timestamps call.  WM_ERR_STATE for a stream whose workspace group is no longer
 * resident (only the last group is) or that had fewer than 2 rows.  Probabilities of alignment head a (the softmax of HF WhisperAttention's
 * cross branch, modeling_whisper.py, before any crop): HOST float32 [N][n_ctx]. */
int wm_get_align_probs(wm_ctx* ctx, int stream, int a, float* out);
/* The matrix handed to the DTW (HF _extract_token_timestamps: normalised, median-filtered, averaged over the heads): HOST float32 [N][F]. */
int wm_get_align_matrix(wm_ctx* ctx, int stream, float* out);
/* HF _dynamic_time_warping on the NEGATION of `matrix` (HOST float32 [N][F]) by the engine's kernel: first_frame HOST [N] (time index of the
 * first path element of every text row), the path in forward order (text_indices, time_indices; HOST, N + F entries of room) and its length. */
int wm_dtw(wm_ctx* ctx, const float* matrix, int N, int F, int32_t* first_frame, int32_t* path_text, int32_t* path_time, int* path_len);
/* cross K/V of one kv-layer/stream/head: HOST float32 [n_ctx][64] each */
int wm_get_cross_kv(wm_ctx* ctx, int kv_layer, int stream, int head, float* k_out, float* v_out);
/* Times `reps` launches of one decode-path kernel class in its current shape with hipEvents on
 * the context stream (bench.py roofline leg).  kernel: 0 = the weight-streaming GEMMs of one decoder
 * layer pass (all 6), 1..6 = one of them (LN1+QKV, out-proj, LN2+cross-q, cross-out, LN3+FC1+GELU, FC2),
 * 7 = the shared vocabulary projection; rows = token rows (<= 16 x max_batch).  Returns avg ms per rep
 * in *ms and the weight bytes those launches stream in *bytes.  No reference counterpart (measurement). */
int wm_profile_kernel(wm_ctx* ctx, int kernel, int rows, int reps, float* ms, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* WM_H_ */
