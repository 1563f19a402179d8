/*
 * tgx.h — the drop-in boundary of the MI355X decode path (C ABI, no C++/torch types).
 *
 * TinyGPT has no FFI of its own: the device is a tinytorch::Device value threaded through
 * GPTConfig -> ModelLoader::load -> every nn::Module (reference: src/engine/GPTEngine.h:25-32,
 * src/huggingface/ModelLoader.cpp:25-89) and CPU-vs-CUDA dispatch happens inside TinyTorch.
 * This header defines the boundary at the seams the reference does expose — the virtual
 * GPTModel interface (src/model/GPTModel.h:80-106), KVCacheManager (src/engine/CacheManager.h:18-55),
 * Sampler::sample (src/engine/Sampler.h:30, Sampler.cpp:23-79) and the AsyncTokenPipeline hook
 * (src/engine/GPTEngine.cpp:17-35).  Each entry point names the reference interface it replaces.
 *
 * Conventions (mirroring the reference's: bool returns + LOGE, exceptions disabled,
 * src/CMakeLists.txt:63-67; single engine thread, server/HttpServer.cpp:118-163):
 *   - every function returns a tgx_status (0 = ok) and never throws across the ABI;
 *   - one opaque context per GPU; all calls on a context come from one host thread;
 *   - the caller owns host buffers; the library owns device memory and one HIP stream;
 *   - host buffers may be pageable; ids are int64 like the reference's token tensors.
 */
#ifndef TGX_H
#define TGX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 5): per-row sequence lifecycle (tgx_reset_row / tgx_forward_row / tgx_sample_row / tgx_past_length_row); tgx_get_option added and
 * tgx_engine_read_stats + the options engine.*, pf.*, attn.fold_*, lmhead.fuse_finalize removed since 2. */
/* (round 7, still 3: additive) per-row sampler settings and device-side stop — tgx_set_row_sampler / tgx_set_row_stop / tgx_decode_rows. */
/* (still 3: additive) tgx_forward_rows; tgx_fork_row — a live row copied into other rows, its full paged KV blocks shared by reference. */
/* (still 3: additive) tgx_extend_row / tgx_truncate_row — a live row grows by several positions in one pass, or is rolled back: prefix reuse without a second prefill. */
/* (still 3: additive) tgx_splice_row — ranges cut out of the middle of a live row's cache, the keys behind them re-rotated: context shift without a second prefill. */
/* (still 3: additive) tgx_verify_row — greedy speculative decoding: a row's draft tokens verified in ONE pass, the row left as after the accepted decode steps. */
/* (still 3: additive) tgx_verify_row_sampled — the same under the row's own sampler: exact by the draw identity; tgx_read_pass_logits — the pass's logits (diagnostic). */
/* (still 3: additive) tgx_verify_tree — a token TREE of guesses verified in one pass: each position attends its own branch, the accepted branch is compacted in place. */
/* (still 3: additive) tgx_verify_rows — the drafts of several rows verified in ONE joint pass and ONE accept launch; n_draft 0 rows step along. */
/* (still 3: additive) tgx_set_row_logprobs / tgx_read_row_logprobs — per-token log-probabilities (chosen token and top-N) recorded on the device into a per-row ring. */
/* (still 3: additive) tgx_score_row — a prompt pass that also returns the log-probability of every token the caller SUPPLIED (echo, perplexity, ranking). */
/* (still 3: additive) tgx_row_snapshot_bytes / tgx_save_row / tgx_restore_row — a live row saved to host memory and restored into any row of any context of the same geometry. */
/* (still 3: additive) tgx_embed_rows — the pooled final hidden state (last / mean / first) of several texts in one ragged pass, without lm_head. */
/* (still 3: additive) tgx_beam_select / tgx_beam_advance — beam search: the joint ranking of several rows' distributions on the device, a group of rows re-seated in place. */
#define TGX_ABI_VERSION 3

#if defined(__GNUC__)
#define TGX_API __attribute__((visibility("default")))
#else
#define TGX_API
#endif

typedef struct tgx_ctx tgx_ctx;

typedef enum tgx_status {
  TGX_OK = 0,
  TGX_ERR_INVALID = 1,     /* bad argument (null pointer, batch/seq out of range, ...)        */
  TGX_ERR_UNSUPPORTED = 2, /* family / dtype / head_dim this backend does not implement       */
  TGX_ERR_DEVICE = 3,      /* a HIP call failed; tgx_last_error() has the HIP error string     */
  TGX_ERR_STATE = 4,       /* call order violated (forward before finalize, missing tensors)  */
  TGX_ERR_NOMEM = 5,       /* host or device allocation failed                                */
  TGX_ERR_NAME = 6,        /* tensor name not part of this model ("Unexpected key")           */
  TGX_ERR_SHAPE = 7,       /* "shape not equal for tensor" (SafeTensors.cpp:187-193)          */
  TGX_ERR_CONTEXT = 8      /* pastLength + seq would exceed contextSize()                     */
} tgx_status;

/* GPTModelType (src/model/GPTModel.h:71-78) */
typedef enum tgx_family {
  TGX_FAMILY_GPT2 = 1,
  TGX_FAMILY_LLAMA = 2,
  TGX_FAMILY_QWEN2 = 3,
  TGX_FAMILY_QWEN3 = 4,
  TGX_FAMILY_MISTRAL = 5
} tgx_family;

/* tinytorch::DType values the CLI accepts (examples/inference/main.cpp:82-88) */
typedef enum tgx_dtype { TGX_F32 = 0, TGX_BF16 = 1, TGX_F16 = 2 } tgx_dtype;

/*
 * What the family factories derive from config.json (src/huggingface/ModelConfig.cpp:63-122,
 * src/model/ModelLlama.h:21-53, ModelQwen2.h:23-45, ModelMistral.h:23-40, ModelGPT2.h:226-230).
 */
typedef struct tgx_model_desc {
  int32_t family;         /* tgx_family                                                          */
  int32_t hidden;         /* hidden_size / n_embd                                                */
  int32_t layers;         /* num_hidden_layers / n_layer                                         */
  int32_t heads;          /* num_attention_heads / n_head                                        */
  int32_t kv_heads;       /* num_key_value_heads (must divide heads, Attention.h:38)             */
  int32_t head_dim;       /* hidden/heads for llama/qwen2/mistral (ModelLlama.h:37)              */
  int32_t inter;          /* intermediate_size (4*n_embd for GPT-2, ModelGPT2.h:96)              */
  int32_t vocab;          /* vocab_size                                                          */
  int32_t max_ctx;        /* GPTModel::contextSize(): KV capacity and RoPE table length          */
  int32_t qkv_bias;       /* 1 for Qwen2 (ModelQwen2.h:26-31) and GPT-2                          */
  int32_t tied;           /* tie_word_embeddings: lm_head aliases embed_tokens (GPTModel.h:39-41)*/
  int32_t compute_dtype;  /* tgx_dtype the model is cast to after load (ModelLoader.cpp:84)      */
  float norm_eps;         /* rms_norm_eps / layer_norm_epsilon                                   */
  float rope_theta;       /* rope_theta                                                          */
  float rope_factor;      /* llama3 RopeScalingConfig.factor; 0 = std::nullopt (no scaling)      */
  float rope_low_freq;    /* .lowFreqFactor                                                      */
  float rope_high_freq;   /* .highFreqFactor                                                     */
  int32_t rope_orig_ctx;  /* .originalMaxPositionEmbeddings                                      */
  int32_t n_positions;    /* GPT-2 wpe rows; 0 otherwise                                         */
  int32_t max_batch;      /* rows of independent KV state to allocate (>= 1)                     */
  int32_t qk_norm;        /* 1: per-head RMSNorm on q and k before RoPE (AttentionWithQKNorm,    */
                          /*    src/layer/Attention.h:128-167; Qwen3, ModelQwen3.h:23-40)        */
} tgx_model_desc;

/* SamplerConfig (src/engine/Sampler.h:13-22).  Greedy iff temperature<=0 && top_k<=0 &&
 * top_p>=1 && min_p<=0 (Sampler.cpp:15-21). */
typedef struct tgx_sampler_cfg {
  float temperature;
  int64_t top_k;
  float top_p;
  float min_p;
} tgx_sampler_cfg;

/* ---- lifetime ---------------------------------------------------------------------------- */

/* Number of visible MI355X devices (the `--device mi355x` probe; reference branch:
 * examples/inference/main.cpp:76-80). */
TGX_API int tgx_device_count(int* out_count);

/* == Model{Llama,Qwen2,Mistral}::Model*(config, device) (e.g. src/model/ModelLlama.h:57-65):
 * validates the description, binds the GPU, allocates parameter storage in compute_dtype. */
TGX_API int tgx_create(const tgx_model_desc* desc, int device_ordinal, tgx_ctx** out_ctx);

/* == SafeTensors::loadInternal -> Storage::copyOnDevice for ONE named tensor
 * (src/util/SafeTensors.cpp:157-215).  `hf_name` is the checkpoint key; q/k/v and gate/up land in
 * the row slices of the merged weights exactly like MergedLinear's LinearRef views
 * (src/layer/Linear.h:64-79).  Shape must match (TGX_ERR_SHAPE); an unknown key is TGX_ERR_NAME
 * (the reference warns "Unexpected key" and continues — callers may ignore that status).
 * ndim < 0 is a name probe: nothing is copied; TGX_ERR_NAME = unknown key, TGX_OK = a key this path knows and
 * ignores, TGX_ERR_SHAPE = a parameter the model needs (the loader uses it for tensors whose file dtype it cannot convert).
 * `src_dtype` is the dtype of `host`; conversion to compute_dtype happens on upload
 * (bf16->fp32 exact, fp32->bf16 round-to-nearest-even), == model().to(dtype), ModelLoader.cpp:84. */
TGX_API int tgx_upload(tgx_ctx* ctx, const char* hf_name, const void* host, const int64_t* shape, int ndim,
               int src_dtype);

/* == model().eval() + GPTModel::init(): checks every tensor arrived (TGX_ERR_STATE names the
 * first missing key in tgx_last_error), builds the RoPE tables (nn::RoPE ctor, ModelLlama.h:41-42),
 * allocates the KV cache for max_batch x max_ctx tokens and instantiates the decode graph. */
TGX_API int tgx_finalize(tgx_ctx* ctx);

TGX_API void tgx_destroy(tgx_ctx* ctx);

/* ---- the hot path ------------------------------------------------------------------------ */

/* == GPTModel::forward(inputIds[B,S]) + narrow-to-last-position (src/model/GPTModel.h:86,
 * src/engine/GPTEngine.cpp:96-97).  `ids` is a row-major host array [batch][seq] (left-padded by
 * the caller, no mask — GPTEngine.cpp:95).  Appends seq positions to every row's KV cache
 * (KVCacheManager::append, CacheManager.h:24-42) and leaves the last-position logits [batch][vocab]
 * on the device for tgx_sample / tgx_read_logits.  seq>1 with pastLength>0 is rejected with
 * TGX_ERR_INVALID (the reference would run it non-causally, Attention.h:108; its engine never does). */
TGX_API int tgx_forward(tgx_ctx* ctx, const int64_t* ids, int batch, int seq);

/* Copies the logits of the last tgx_forward / decode step to `out` [batch*vocab] as fp32.
 * rounded=1: values as the reference's logits tensor holds them (rounded to compute_dtype);
 * rounded=0: the fp32 accumulators before that rounding (for tolerance checks). */
TGX_API int tgx_read_logits(tgx_ctx* ctx, float* out, int rounded);

/* == Sampler::sample(logits[B,V]) (src/engine/Sampler.cpp:23-79) on the current logits.
 * The sampled ids become the device-resident "next token" of every row; if out_ids != NULL they
 * are also copied to the host ([batch], int64).  `seed` drives the multinomial draw (the
 * reference's RNG stream is not reproducible; greedy ignores it). */
TGX_API int tgx_sample(tgx_ctx* ctx, const tgx_sampler_cfg* cfg, uint64_t seed, int64_t* out_ids);

/* == the decode loop body of GPTEngine::generateSync (src/engine/GPTEngine.cpp:165-168), n_steps
 * times: nextToken = sample(forward(nextToken)).  Token ids and positions stay on the GPU between
 * steps; out_ids (may be NULL) receives [n_steps][batch] int64. */
TGX_API int tgx_decode(tgx_ctx* ctx, const tgx_sampler_cfg* cfg, uint64_t seed, int n_steps, int64_t* out_ids);

/* == AsyncTokenPipeline (src/engine/GPTEngine.cpp:17-35) for generateAsync's one-step lookahead
 * (GPTEngine.cpp:196-217), batch row 0.  tgx_step_async enqueues one decode step and returns
 * immediately with a ticket; tgx_fetch_token blocks until the step with that ticket has sampled
 * and returns its id.  Ticket 0 refers to the token produced by the last tgx_sample. */
TGX_API int tgx_step_async(tgx_ctx* ctx, const tgx_sampler_cfg* cfg, uint64_t seed, int64_t* out_ticket);
TGX_API int tgx_fetch_token(tgx_ctx* ctx, int64_t ticket, int32_t* out_id);

/* == GPTModel::resetCache() (src/model/GPTModel.h:91-94): pastLength back to 0 for all rows. */
TGX_API int tgx_reset_cache(tgx_ctx* ctx);

/* == KVCacheManager::pastLength (src/engine/CacheManager.h:44-51).  With rows of different lengths (see the per-row calls below): the LONGEST
 * row of the batch — the length every capacity check uses. */
TGX_API int64_t tgx_past_length(const tgx_ctx* ctx);

/* ---- per-row sequence lifecycle (ABI 3) ---------------------------------------------------
 * The kernel-contract half of the reference's continuous-batching TODO (README.md:33-34): the reference's KVCacheManager holds ONE pastLength for
 * the whole batch (src/engine/CacheManager.h:44-51) and its engine rebuilds the batch per request (src/engine/GPTEngine.cpp:67-84,180-232), so a
 * finished sequence blocks its slot until the longest one ends.  Here every row owns its cache slab and its device-resident position, and the
 * step kernels read the position per row: a row can be retired and another prompt prefilled into it while the other rows keep their state.
 * What a row keeps is the semantics of a solo sequence (Attention.h:71-112 over its own keys [0, pastLength_row]): its logits equal those of the
 * same prompt run alone up to the summation-order differences between kernel paths (tests/test_hip_rows.py).
 *
 * tgx_reset_row      == resetCache() for ONE row: its pastLength back to 0; the other rows and the batch size are untouched.  The row is now
 *                       RETIRED: tgx_decode / tgx_step_async keep stepping the live rows without waiting for it (a finished sequence with no queued
 *                       prompt stalls nobody).  It still rides in the steps (it decodes from position 0 on its stale token; its ids and logits in
 *                       tgx_decode's output / tgx_read_logits are meaningless and harmless) and counts for neither tgx_past_length nor the context
 *                       check; tgx_past_length_row reports 0 for it.  With every row retired there is nothing to step: tgx_decode refuses.
 * tgx_forward_row    == GPTModel::forward(inputIds[1,S]) for ONE row of the live batch: a retired `row` < batch (refill) or `row` == batch (the
 *                       batch grows by one row, up to max_batch); a live row must be retired first (tgx_reset_row).  Leaves the row's last-position
 *                       logits in its slot of tgx_read_logits; the row is live again but has no current token until tgx_sample_row (or tgx_sample)
 *                       ran — tgx_decode refuses until then.
 * tgx_sample_row     == Sampler::sample on ONE row's logits; the id becomes that row's device-resident next token.
 * tgx_past_length_row   the row's own pastLength.
 * tgx_forward_rows   == n tgx_forward_row calls (in array order) in ONE prefill pass, up to summation order: prompt i (lens[i] ids, the prompts back to back in
 *                       `ids`) into row rows[i].  Each row follows tgx_forward_row's rules: a retired row < batch or a new row; the new rows of a call are exactly
 *                       batch .. batch + k - 1 in any array order (the batch grows by k, up to max_batch); rows are distinct; lens[i] in [1, max_ctx]; every id in
 *                       range; a live or finished row is TGX_ERR_STATE.  Afterwards each row holds lens[i] positions and its last-position logits / argmax in its
 *                       own slot, exactly as tgx_forward_row leaves them (tgx_read_logits, tgx_sample_row, tgx_read_probs, tgx_decode / tgx_decode_rows work
 *                       unchanged); rows not named keep their state bit for bit.  ALL OR NOTHING: a refused call changes no row, moves no KV block, leaves
 *                       kv.free_tokens as it was and does not poison the context; on a paged cache the blocks of the whole call (the target rows' own blocks
 *                       plus the free list) are counted before anything is assigned (TGX_ERR_CONTEXT), and a cache of more than 1024 blocks per row
 *                       (max_ctx > 131072) is TGX_ERR_UNSUPPORTED.  n = 0 is TGX_ERR_INVALID.
 *                       The prompts run in groups of whole prompts of at most max(8192, longest prompt) workspace rows, one matrix-core pass per group (skinny or
 *                       tiled by tgx_forward's rule on the group's rows) with ONE RoPE / cache-append launch and ONE attention launch per layer for all its
 *                       prompts, and lm_head four rows per pass over its weights.  Fall-back to tgx_forward_row's one-row passes (identical results): fp32
 *                       storage, option prefill.mfma 0, layer shapes the matrix-core GEMM tile does not cover, groups of fewer than 4 rows. */
TGX_API int tgx_reset_row(tgx_ctx* ctx, int row);
TGX_API int tgx_forward_row(tgx_ctx* ctx, int row, const int64_t* ids, int seq);
/* n prompts into n rows of the live batch in ONE prefill pass: == n tgx_forward_row calls (in array order) up to summation order. */
TGX_API int tgx_forward_rows(tgx_ctx* ctx, int n, const int32_t* rows, const int64_t* ids /* sum(lens) tokens, prompts back to back */,
                             const int32_t* lens);
TGX_API int tgx_sample_row(tgx_ctx* ctx, int row, const tgx_sampler_cfg* cfg, uint64_t seed, int64_t* out_id);
TGX_API int64_t tgx_past_length_row(const tgx_ctx* ctx, int row);

/* ---- per-row sampler settings and device-side stop (additive to ABI 3) --------------------------------------------------------------------------------
 * The request half of continuous batching: the reference's worker reconfigures its engine per request (engine_->reconfigure(samplerConfig, maxNewTokens,
 * stopIds), server/HttpServer.cpp:118-163 -> src/engine/GPTEngine.cpp:67-84) and checks EOS per token (GPTEngine.cpp:196-217).  Here every row of the batch
 * carries its own settings and stop conditions on the device, and tgx_decode_rows steps them together.
 *
 *   Draw identity     a row's ids and logits under tgx_decode_rows are bit-identical to tgx_decode with that row's cfg and seed applied to the whole batch
 *                     (the draw keeps its hash of (seed, position, row)); rows that share the call do not change each other's results.
 *   Counting          the token that finishes a row (a stop id, or the max_new-th token) is reported in out_ids and counted in out_new; for every row
 *                     tgx_past_length_row after the call == its value before + out_new[row].
 *   Finished row      keeps its length (and its cache rows [0, past), never rewritten) until tgx_reset_row.  It rides along in later steps the way a retired
 *                     row does — no advance, it counts for neither tgx_past_length nor the context check — and its out_ids are -1.  One that finished at
 *                     the context size has no row left to ride on: tgx_decode_rows returns TGX_ERR_CONTEXT until it is reset.
 *   Calls             tgx_forward_row into a finished row needs tgx_reset_row first (TGX_ERR_STATE); tgx_decode_rows with no unfinished live row returns
 *                     TGX_ERR_STATE; tgx_decode, tgx_step_async and tgx_forward return TGX_ERR_STATE while any row is finished (they would advance it).
 *   Retired rows      (tgx_reset_row) ride along as in tgx_decode; their out_ids are -1, out_new and out_finish 0.  tgx_forward_row starts the row's count afresh.
 *   Paged KV          blocks are assigned up front for past + n_steps; after the call a finished row's blocks beyond ceil(past / 128) go back to the pool.  The blocks
 *                     of ALL the unfinished live rows are counted against the free list before any is assigned (tgx_decode and tgx_step_async likewise): a call
 *                     refused for want of a block (TGX_ERR_CONTEXT) assigns none, steps no row and leaves kv.free_tokens as it was.
 *   out_finish        of a row that had finished BEFORE the call repeats its reason (1 or 2); its out_new is 0 and its out_ids are -1.
 *   tgx_read_probs    after tgx_decode_rows: each row's vector under its own cfg (greedy rows read as zeros).
 *   Existing calls    tgx_decode, tgx_sample*, tgx_step_async ignore the row settings. */
#define TGX_MAX_STOP_IDS 8
/* The sampler settings of ONE row, used by tgx_decode_rows.  Kept across calls until changed; tgx_reset_row / tgx_reset_cache restore the default (greedy,
 * seed 0, no stop conditions).  Takes effect for steps enqueued after the call, stream-ordered: no host synchronisation. */
TGX_API int tgx_set_row_sampler(tgx_ctx* ctx, int row, const tgx_sampler_cfg* cfg, uint64_t seed);
/* The stop conditions of ONE row for tgx_decode_rows: finish after max_new more produced tokens (<= 0: no limit), or as soon as the row produces one of
 * stop_ids (n_stop <= TGX_MAX_STOP_IDS; 0 = none; a stop id takes precedence when both hold).  Resets the row's produced-token count.  Stream-ordered. */
TGX_API int tgx_set_row_stop(tgx_ctx* ctx, int row, int32_t max_new, const int32_t* stop_ids, int n_stop);
/* n_steps decode steps in which every live row samples with ITS OWN settings and may finish on the device.
 * out_ids [n_steps][batch] (may be NULL): the produced ids, -1 for a row after it finished.  out_new [batch] (may be NULL): tokens produced per row in this
 * call.  out_finish [batch] (may be NULL): 0 running, 1 stopped on a stop id, 2 reached max_new (the reference's FinishReason Stop / Length). */
TGX_API int tgx_decode_rows(tgx_ctx* ctx, int n_steps, int64_t* out_ids, int32_t* out_new, int32_t* out_finish);

/* ---- forking a live row (additive to ABI 3) ------------------------------------------------------------------------------------------------------------
 * n samples of one prompt (n-best / best_of) and a beam or branch taken mid-generation need the same sequence in several rows; the reference's engine rebuilds its
 * batch per request (src/engine/GPTEngine.cpp:67-84) and would prefill the prompt once per sample.  tgx_fork_row makes dst_rows[i] (i < n) copies of the live
 * row `src`: the same pastLength, the same cache rows [0, past) bit for bit, the same last logits / argmax partials / hidden row, and src's current token if it has one.
 *
 *   Source row        a live, unfinished row < batch.  A retired or finished src (or a row of the batch that holds no sequence) is TGX_ERR_STATE; src outside
 *                     [0, max_batch) is TGX_ERR_INVALID.
 *   Destination rows  follow tgx_forward_rows' rules: each a retired row < batch or a new row; the new rows of a call are exactly batch .. batch + k - 1 in any array
 *                     order (the batch grows by k, up to max_batch); distinct and != src (a duplicate, or src itself, is TGX_ERR_INVALID); a live or finished
 *                     destination is TGX_ERR_STATE.  n < 1 is TGX_ERR_INVALID.
 *   Afterwards        a destination is in exactly the state src is in: if src has no current token (fresh from tgx_forward_row) the destination needs
 *                     tgx_sample_row too; if src has one (mid-generation) the destination carries the same token and is ready for tgx_decode / tgx_decode_rows.
 *                     Its sampler settings are untouched, its stop state and produced-token count start afresh (as for an admission), and tgx_read_probs has no
 *                     vector for it until its next sampled step.  src and every row not named keep their state bit for bit.
 *   Paged KV          the floor(past / 128) FULL blocks of src are shared by reference — a block returns to the pool when the last row that maps it lets go of
 *                     it (tgx_reset_row / tgx_reset_cache / an admission into the row) — and each destination gets one fresh block for the partial tail when
 *                     past % 128 != 0: the call needs n * (past % 128 ? 1 : 0) blocks, counted against the free list plus what the destination rows give back
 *                     before anything is assigned (TGX_ERR_CONTEXT).  The cache is append-only and a shared block is full, so no later call writes into one;
 *                     tgx_write_kv refuses a range that touches one (TGX_ERR_STATE).  Unpaged: the prefix [0, past) of every layer is copied into each
 *                     destination's slab.
 *   ALL OR NOTHING    a refused call changes no row, moves no KV block, leaves kv.free_tokens as it was and does not poison the context.
 *   Cost              one copy launch per call (per 128 destinations) for all layers, both caches, all destinations and the per-row state, stream-ordered behind
 *                     the steps already enqueued; the call returns when the copy has finished, like an admission. */
TGX_API int tgx_fork_row(tgx_ctx* ctx, int src, int n, const int32_t* dst_rows);

/* ---- beam search (additive to ABI 3) --------------------------------------------------------------------------------------------------------------------
 * K hypotheses of one prompt advance together: each step ranks every (hypothesis, next token) pair by the hypothesis' running score plus the token's log-probability
 * and keeps the best K.  Emulated with the calls above a step costs K read-backs of [vocab] logits, a ranking on the host, K tgx_fork_row into freshly retired rows and
 * K one-token tgx_extend_row passes over all the weights, in 2K rows.  The two calls below do it in K rows with one small read-back and ONE batched step:
 *   tgx_beam_select(rows, scores, k)  ->  the caller picks k candidates  ->  tgx_beam_advance(rows, parent, tokens)  ->  tgx_decode_rows(1)  ->  tgx_beam_select ...
 *
 * tgx_beam_select — the joint ranking (kernels/beam.h)
 *   Inputs            rows[0 .. n): distinct live, unfinished rows that hold logits (after tgx_forward_row / tgx_extend_row, or after a step); a current token is not
 *                     needed and not looked at.  scores[i]: the finite running score of the hypothesis in rows[i].
 *   What is ranked    v_i = the row's fp32 logits (tgx_read_logits, rounded = 0) — with a logit processor or an automaton on, the processed vector tgx_sample_row would
 *                     draw from (no counting step, no state move).  lse_i is tgx_set_row_logprobs' quantity (tile sums in double, a fixed association),
 *                     lp_i(t) = (double)v_i[t] - lse_i, key(i, t) = (double)scores[i] + lp_i(t).  The joint order: key descending, then array index i ascending,
 *                     then the rank within the row (value descending, index ascending) ascending; an entry of key -inf is no candidate.
 *   Output            the prefix of the joint order that ends at the k-th candidate whose token is none of end_ids — an end-id candidate ahead of it is a hypothesis
 *                     that ends here — cut at TGX_MAX_BEAM_CAND entries or where the candidates run out; *out_n entries, each {beam = i, token,
 *                     score = (float)key, lp = (float)lp_i(token)}.  The same call returns the same bits from run to run.
 *   Refusals          TGX_ERR_INVALID: a null pointer, n or k outside [1, TGX_MAX_BEAMS], n_end outside [0, TGX_MAX_STOP_IDS], a non-finite score, a row named
 *                     twice or out of range.  TGX_ERR_STATE: a retired, empty, finished or no-logits row, a poisoned context, a call before tgx_finalize.  A refused
 *                     call changes nothing.
 *   Cost              three small launches (a tile launch over the n rows' vocabularies, a merge per row, one ranking workgroup), one synchronisation and a
 *                     528-byte read-back; the workspace is sized by the first call (a context that never selects holds none of it).
 *
 * tgx_beam_advance — the group re-seated (csrc/beam_plan.h, kernels/beam.h)
 *   Rows              rows[0 .. n_rows) distinct, n_rows <= TGX_MAX_BEAMS, each a SOURCE (a live, unfinished row that holds logits) or a SPARE (a retired or
 *                     empty row < batch, or a new row by tgx_forward_rows' rule: the new rows that RECEIVE a hypothesis must be exactly batch .. batch + m - 1).
 *                     1 <= n_next <= n_rows; parent[j] indexes rows and names a source; tokens[j] in [0, vocab).
 *   Afterwards        new hypothesis j is the sequence of rows[parent[j]] with current token tokens[j], in out_rows[j], ready for tgx_decode_rows (or
 *                     tgx_verify_rows with n_draft 0).  On row 0 the token becomes ticket 0's token.
 *   Placement         PINNED: for each source in array order that has children, its lowest-j child stays IN PLACE (no copy, no block moves); the sources without
 *                     a child are retired first, as by tgx_reset_row; the remaining children, in ascending j, take the rows that are empty now (retired
 *                     sources and spares) in ascending array index.  A group lives in K rows, and a step copies exactly n_next - (distinct parents) rows.
 *   Copied children   tgx_fork_row's destination, word for word: the full paged blocks shared by reference, one fresh tail block when past % 128 != 0, the prefix
 *                     copied on slabs; hidden row, logits, partials, position word, history words and automaton id / state travel with the copy; settings are the
 *                     caller's (a retired source's are back at their defaults, as after tgx_reset_row).  One copy launch per parent that has a copied child, then
 *                     ONE publish launch for all placed rows: the token word and the next embedding at the row's position (GPT-2: with wpe) — the row ends as a
 *                     step that produced that token would leave it.
 *   Not done here     no log-probability record is written (the candidate carries lp).  Stop conditions are the caller's: a row that finished on the device is no
 *                     legal source (TGX_ERR_STATE), so beam rows carry no stop ids and no max_new.
 *   Paged KV          ALL OR NOTHING: the fresh tail blocks are counted against the free list plus what the childless sources give back before anything is released
 *                     or assigned (TGX_ERR_CONTEXT); one table push.  Rows not named keep their state bit for bit.
 *   Refusals          TGX_ERR_INVALID: a null pointer, n_rows outside [1, TGX_MAX_BEAMS], n_next outside [1, n_rows], a row out of range or named twice, a parent
 *                     outside [0, n_rows), a token out of range, new rows that leave a gap.  TGX_ERR_STATE: a named row that finished or holds no logits, a parent
 *                     that is a spare, a poisoned context, a call before tgx_finalize.  TGX_ERR_CONTEXT: the paged budget.  A refused call changes nothing.
 *   Equivalence       tgx_beam_advance followed by one step equals, up to the order of the fp32 sums, tgx_fork_row of each parent followed by
 *                     tgx_extend_row(row, &token, 1); cache rows [0, past) are equal bit for bit.
 *   Cost              NOT YET MEASURED on the device in this tree: tools/beam_bench.py writes profiles/beam_search.txt (the step against tgx_decode_rows alone and
 *                     against the emulation above); no figure is quoted until that file exists.  On slabs a copied child costs a copy of its whole prefix. */
#define TGX_MAX_BEAMS 8
#define TGX_MAX_BEAM_CAND 32
typedef struct tgx_beam_cand { int32_t beam; int32_t token; float score; float lp; } tgx_beam_cand;
TGX_API int tgx_beam_select(tgx_ctx* ctx, int n, const int32_t* rows, const float* scores /* [n] */, int k, const int32_t* end_ids, int n_end,
                            tgx_beam_cand* out /* [TGX_MAX_BEAM_CAND] */, int32_t* out_n);
TGX_API int tgx_beam_advance(tgx_ctx* ctx, int n_rows, const int32_t* rows, int n_next, const int32_t* parent /* [n_next], index into rows */,
                             const int32_t* tokens /* [n_next] */, int32_t* out_rows /* [n_next] */);

/* ---- extending and truncating a live row (additive to ABI 3) ------------------------------------------------------------------------------------------
 * The next turn of a conversation, a request's own text after a shared (forked) prefix, a prompt admitted in pieces: "these tokens after that cached prefix" without
 * tgx_reset_row and a second prefill of the whole sequence.  tgx_extend_row appends ids[0 .. seq) at positions past .. past + seq - 1 of `row`: the result is
 * GPTModel::forward(inputIds[1, seq]) on a cache that already holds `past` positions, run CAUSALLY — new position i attends the cache and the new positions <= i.
 * (The reference's attention would run such a call without a mask — isCausal only when qLen == kvLen, Attention.h:108 — and its engine never makes one: it resets
 * its cache per request.)  So tgx_forward_row(r, A) + tgx_extend_row(r, B) equals tgx_forward_row(r, A + B) up to the order of the fp32 sums.
 *
 *   Accepted rows     a live row < batch that holds past >= 1 positions, with or without a current token, and a row that finished in tgx_decode_rows (the row stopped
 *                     on EOS and the next turn arrives): its finished state is cleared.
 *   The current token is NOT in the cache — it is the input of the next step.  tgx_extend_row DISCARDS it; a caller who wants it in the sequence passes it as ids[0].
 *   Refused           a retired or empty row, or row >= batch: TGX_ERR_STATE (use tgx_forward_row).  row outside [0, max_batch), seq < 1, an id out of range, a null
 *                     pointer: TGX_ERR_INVALID.  past + seq > max_ctx: TGX_ERR_CONTEXT.  A poisoned context: TGX_ERR_STATE.  Paged KV: the blocks for past + seq
 *                     are counted against the free list before anything is assigned (TGX_ERR_CONTEXT); a cache of more than 1024 blocks per row is
 *                     TGX_ERR_UNSUPPORTED on the matrix-core routes, as for tgx_forward_rows.
 *   ALL OR NOTHING    a refused call changes no row, moves no KV block, leaves kv.free_tokens as it was and does not poison the context.
 *   Afterwards        exactly as tgx_forward_row leaves a row: the last position's logits and argmax partials in the row's slot; no current token until
 *                     tgx_sample_row (tgx_sample on a one-row batch) — tgx_decode* refuse until then; the sampler settings kept, the stop state and the
 *                     produced-token count afresh; no tgx_read_probs vector; tgx_past_length = the longest live row.  Rows not named keep their state bit for bit.
 *   Attention         a pass of <= 128 positions over a long context runs its attention split over the keys (option extend.attn_splits: -1 automatic from a measured
 *                     context on, 0 never, N >= 1 N splits); the partials are merged in split order, so the result is the same bits from run to run. */
TGX_API int tgx_extend_row(tgx_ctx* ctx, int row, const int64_t* ids, int seq);
/* Rolls a live or finished row back to 1 <= new_len <= past positions: an aborted generation, an edited last message, a prompt that shares only a prefix with what the
 * row holds (truncate to min(common prefix, new prompt length - 1), then tgx_extend_row the rest).  Cache rows [0, new_len) are untouched; the position word and the
 * host length move; a finished state is cleared.  The logits of position new_len - 1 no longer exist, so the row then has NO LOGITS AND NO CURRENT TOKEN:
 * tgx_sample_row on it, tgx_fork_row from it, and tgx_decode / tgx_decode_rows / tgx_step_async / tgx_sample while it is in that state return TGX_ERR_STATE until
 * tgx_extend_row has run on it (tgx_reset_row ends the state as well).  new_len == past on a row whose logits are in place is a no-op that returns TGX_OK.
 * new_len < 1 (that is tgx_reset_row) and new_len > past: TGX_ERR_INVALID.  A retired or empty row: TGX_ERR_STATE.
 * Paged KV: the blocks beyond ceil(new_len / 128) lose this row's reference.  If new_len % 128 != 0 and the block that now holds the tail is shared with forked
 * siblings, the next append would write into a shared block: the row takes one fresh block, rows [0, new_len % 128) of every layer and both caches are copied into
 * it in one launch, the table entry is swapped and the shared block loses this row's reference.  With no free block that is TGX_ERR_CONTEXT and nothing changes. */
TGX_API int tgx_truncate_row(tgx_ctx* ctx, int row, int64_t new_len);

/* ---- cutting ranges out of a live row (additive to ABI 3) ----------------------------------------------------------------------------------------------
 * Generation past the context ("context shift": keep the first positions, drop half of the rest, slide the tail down), a tool result or a retrieved document
 * dropped from the middle of a long chat, "sinks + a recent window" of a stream, blocks of a paged cache freed from a long row: positions taken out of the MIDDLE of
 * a row's cache without tgx_reset_row and a second prefill of what remains.  The row's new sequence is the concatenation of the kept ranges
 * [starts[i], starts[i] + lens[i]), i < n_keep: sorted, non-empty, inside [0, past), disjoint (they may touch).  A kept position s of range i ends at
 * d = s - delta_i, delta_i = starts[i] - sum(lens[0 .. i)); new_len = sum(lens) >= 1 is written to *out_len (may be NULL).
 *
 *   What moves        for every layer and kv head: V'[d] = V[s] bit for bit; K'[d] = K[s] bit for bit where delta == 0.  Otherwise — every key is stored post-RoPE
 *                     at the position it was appended at — the pair (K[s][p], K[s][p + hd/2]) is rotated by the angle table(d) - table(s): with
 *                     (c_o, s_o) = rope_cos / rope_sin[s][p] and (c_n, s_n) = rope_cos / rope_sin[d][p],
 *                       c = fmaf(c_n, c_o, __fmul_rn(s_n, s_o)),  s = fmaf(s_n, c_o, -__fmul_rn(c_n, s_o)),
 *                     then the rotation every append site uses (x0' = fmaf(x0, c, -__fmul_rn(x1, s)), x1' = fmaf(x1, c, __fmul_rn(x0, s))) on the stored values
 *                     converted to fp32, rounded once to the storage dtype.  Both table rows are used, not the row of delta: the tables hold
 *                     cosf(fl32(inv * pos)), whose angles are not additive at large positions.  The key is then what the append kernels would have written at d,
 *                     up to one more storage rounding.
 *   Accepted rows     tgx_truncate_row's: a live or finished row < batch that holds past >= 1 positions, in any of its three states (logits and a current token,
 *                     logits only, no logits).  A finished state is cleared.
 *   Refused           a null pointer, row outside [0, max_batch), n_keep outside [1, TGX_MAX_SPLICE_RANGES], a range that is empty, unsorted, overlapping or outside
 *                     [0, past): TGX_ERR_INVALID.  A retired or empty row, row >= batch, a poisoned context, a call before tgx_finalize: TGX_ERR_STATE.  GPT-2:
 *                     TGX_ERR_UNSUPPORTED (its positions are learned and added to the hidden state: there is nothing to re-rotate).  A cache row of head_dim *
 *                     element size bytes that is no multiple of 4 (or whose half is none): TGX_ERR_UNSUPPORTED, as for tgx_fork_row.
 *   ALL OR NOTHING    a refused call changes no row, moves no KV block, leaves kv.free_tokens as it was and does not poison the context.
 *   No-op             one range [0, past) on a row whose logits are in place returns TGX_OK and changes nothing; one range [0, L), L < past, IS
 *                     tgx_truncate_row(row, L): the same bits, the same block accounting.
 *   Afterwards        the row holds new_len positions and is in tgx_truncate_row's state "no logits, no current token": tgx_sample_row, the decode calls and
 *                     tgx_fork_row return TGX_ERR_STATE until tgx_extend_row has run on it.  The current token is NOT in the cache and is discarded, as
 *                     tgx_extend_row discards it: a caller that goes on generating passes it as ids[0] of the next tgx_extend_row (which starts the
 *                     produced-token count afresh: restate the stop with the remaining max_new).  Settings, history words, automaton id / state and the logprob
 *                     count are kept, as tgx_truncate_row keeps them.  tgx_past_length is refreshed.  Rows not named keep their state bit for bit.  The call
 *                     is stream-ordered behind the steps already enqueued and does not synchronise (a first call that allocates or grows the staging buffer
 *                     does).
 *   Sampling          a sampled row's draw key hashes the POSITION of the produced token (seed, position, row): after a splice positions repeat, so a row that
 *                     is shifted and sampled with the same seed draws position p's variate again the second time it reaches p.
 *   Paged KV          f = the first position whose content changes: the end of the leading delta == 0 range (0 without one; new_len for a truncation).  Blocks
 *                     with index < f / 128 are untouched and may stay shared with forked rows; every block from f / 128 to ceil(new_len / 128) - 1 is written.
 *                     A written block that forked siblings map as well is swapped for a fresh block before anything writes to it (copy on write); if
 *                     f % 128 != 0, rows [0, f % 128) of the first one are carried over, as tgx_truncate_row carries them.  The fresh blocks are counted against
 *                     the FREE LIST ALONE before anything is assigned — the blocks the row gives back are not counted, the sum errs towards refusing — and a
 *                     shortfall is TGX_ERR_CONTEXT.  Blocks beyond ceil(new_len / 128) lose this row's reference.  Afterwards kv.free_tokens is what a row of
 *                     new_len leaves, minus the fresh blocks taken; a shared block is still full for every row that maps it.
 *   Staging           the move overlaps itself (one position's destination is another's source), so it runs through the snapshot staging buffer (option
 *                     snapshot.stage_kib caps it; one layer is always staged) in groups of whole layers: per group one gather launch (reads through the old
 *                     block table, rotates K, copies V) and one scatter launch (writes through the new one); kernels/kv_splice.h.  The buffer is allocated by the
 *                     first call that needs it: a context that never splices allocates nothing new and runs the launches it ran before.
 *   Cost              measured (profiles/splice_row.txt, tools/admit_bench.py --splice; Llama-3.2-1B bf16, one synchronised call, median of 10): 2048 -> 4 + 1024
 *                     positions (32 MiB moved) 0.07 ms on slabs / 0.08 ms paged, 8192 -> 4 + 4096 (128 MiB) 0.17 / 0.17 ms, against 6.4 and 22.5 ms for
 *                     tgx_reset_row + tgx_forward_row of the kept tokens: about 0.01 of the re-prefill at both shapes.  With the one-token tgx_extend_row that
 *                     re-feeds the current token (0.75 - 0.77 ms, the larger part of a shift) 0.13 and 0.04 of it.  Two launches per group of layers, plus,
 *                     paged, three small table launches and the tail copy of a copy on write. */
#define TGX_MAX_SPLICE_RANGES 16
TGX_API int tgx_splice_row(tgx_ctx* ctx, int row, int n_keep, const int64_t* starts, const int64_t* lens, int64_t* out_len);

/* ---- row snapshots: a live row saved to host memory and restored anywhere (additive to ABI 3) ---------------------------------------------------------------
 * Everything above keeps a sequence in device memory from admission to retirement.  A snapshot moves one off the device and back: swap-out when a paged cache has no
 * block left (TGX_ERR_CONTEXT: save a row, tgx_reset_row it, restore it later instead of a second prefill of prompt + generated tokens), a conversation or a shared
 * system prompt kept across processes (a snapshot is plain bytes: write it to a file), a sequence moved to another context — another GPU's replica, or between a
 * paged and an unpaged context.  tgx_restore_row is a tgx_fork_row whose source lives in host memory.
 *
 *   Source of a save  a live, unfinished row < batch that holds past >= 1 positions, in any of its three states: logits and a current token (mid-generation), logits
 *                     and no token (fresh from tgx_forward_row / tgx_extend_row), no logits (after tgx_truncate_row: the "prefix only" snapshot).  A retired, empty or
 *                     finished row, row >= batch, a poisoned context, a call before tgx_finalize: TGX_ERR_STATE.  A row outside [0, max_batch), a null pointer,
 *                     cap < the snapshot's size: TGX_ERR_INVALID; nothing is written then and *out_bytes is not touched.  tgx_row_snapshot_bytes applies the same
 *                     checks and returns the size tgx_save_row would write now (it changes with every step the row takes).
 *   A save            changes nothing on the device but the library's own staging buffer: the row, kv.free_tokens and every other row stay as they were — the caller
 *                     calls tgx_reset_row itself if it wants the blocks back.  Stream-ordered behind the steps already enqueued; returns when the bytes are in buf.
 *   What it holds     what tgx_fork_row's copy launch carries: cache positions [0, past) of every layer and both caches in the storage dtype, bit for bit; the
 *                     position word and the token word; iff the row holds logits, its fp32 hidden row [hidden] and its fp32 logits [vocab].  NOT held: the argmax
 *                     partials (restore recomputes them from the logits), the row's sampler / stop / logprobs / processor settings, its processor history words,
 *                     its logprob records.  Settings are the caller's, as for tgx_fork_row and tgx_forward_row; a history is restated with tgx_set_row_history.
 *                     Whether the weights behind the snapshot are the weights of the context that restores it is the caller's business, and so is the integrity
 *                     of the bytes in transit: there is no checksum.
 *   Format            version TGX_SNAPSHOT_VERSION, little-endian, independent of whether the cache it came from is paged:
 *                       [0, 128) header   0 magic "TGXSNAP\0" (8 bytes) | 8 u32 version | 12 u32 header bytes = 128 | 16 u64 total bytes |
 *                                         24 nine i32 that must match the restoring context: family, hidden, layers, heads, kv_heads, head_dim, vocab, compute_dtype,
 *                                         qk_norm | 60 u32 flags: bit 0 "holds logits", bit 1 "has a current token" (only with bit 0) | 64 i64 past |
 *                                         72 u64 state offset | 80 u64 state bytes | 88 u64 KV offset | 96 u64 KV bytes | 104 .. 127 zeros
 *                       state section     at 128: u32 position word (== past) | u32 token word (0 without bit 1) | iff bit 0: f32 hidden [hidden] | f32 logits [vocab]
 *                       KV section        at the next multiple of 16 (zeros between): [layer][K, then V][kv_head][past][head_dim] in the storage dtype; a layer's
 *                                         bytes are contiguous
 *   Restore target    tgx_forward_row's rule: a retired or empty row < batch, or row == batch (the batch grows by one, up to max_batch).  A live or finished target is
 *                     TGX_ERR_STATE; a new row other than batch, or a row outside [0, max_batch), TGX_ERR_INVALID.
 *   Restore checks    the blob is validated on the host before anything changes.  TGX_ERR_INVALID: bytes smaller than the header or not the header's total; a wrong
 *                     magic or version; section offsets or sizes that do not follow from the geometry and past; a geometry word that differs from the context's; a
 *                     position word != past; a token word outside [0, vocab) with bit 1 set; bit 1 without bit 0.  past > max_ctx: TGX_ERR_CONTEXT.  A head_dim *
 *                     element size that is no multiple of 4: TGX_ERR_UNSUPPORTED, as for tgx_fork_row.
 *   Paged KV          ceil(past / 128) fresh blocks, counted against the free list plus what the target row gives back before anything is assigned (TGX_ERR_CONTEXT);
 *                     more than 1024 blocks per row is TGX_ERR_UNSUPPORTED.  The restored row owns all its blocks: nothing is shared, no shared block is written.
 *   ALL OR NOTHING    a refused call changes no row, moves no KV block, leaves kv.free_tokens as it was and does not poison the context.
 *   Afterwards        the row is in exactly the state the source was in when it was saved: with a token it is ready for tgx_decode / tgx_decode_rows; with logits only
 *                     it needs tgx_sample_row; without logits tgx_sample_row, the decode calls and tgx_fork_row return TGX_ERR_STATE until tgx_extend_row has run on
 *                     it.  A restore is an admission: the row's settings are untouched, its stop state and produced-token count start afresh, its logprob record
 *                     count goes back to 0, tgx_read_probs has no vector for it.  tgx_past_length is refreshed; rows not named keep their state bit for bit; on row 0
 *                     the token becomes ticket 0's token, as after tgx_sample.  The call returns when the copy has finished.
 *   Reproducibility   a greedy continuation is the same bits in any row of any context.  A sampled draw hashes (seed, position, ROW): a sampled sequence continues
 *                     as it would have only when it is restored into the row index it was saved from, with its seed set again.
 *   Staging           the snapshot moves through one device buffer in groups of whole layers: per group one pack launch (kernels/kv_pack.h) and one copy for a save,
 *                     one copy and one unpack launch for a restore; the state section rides in the first group's launch.  Option snapshot.stage_kib (default 65536)
 *                     caps the buffer; one layer is always staged.  The buffer is allocated by the first save or restore: a context that never calls these
 *                     functions allocates nothing new and runs the launches it ran before.  buf may be pageable.
 *   Cost              measured (profiles/row_snapshot.txt; Llama-3.2-1B bf16, 32 KiB of cache per token, pageable host buffer, wall time of the call): save / reset +
 *                     restore 0.19 / 0.21 ms at 256 tokens (8.5 MiB), 1.28 / 1.28 ms at 2048 (64.5 MiB), 5.07 / 4.97 ms at 8192 (256.5 MiB) — 52 - 54 GB/s from 2048
 *                     tokens on, paged and unpaged alike — against 2.43 / 9.09 / 44.9 ms for tgx_reset_row + tgx_forward_row of the same length: restore wins at
 *                     every length measured (0.09 - 0.14 of the prefill). */
#define TGX_SNAPSHOT_VERSION 1
TGX_API int tgx_row_snapshot_bytes(const tgx_ctx* ctx, int row, int64_t* out_bytes);
TGX_API int tgx_save_row(tgx_ctx* ctx, int row, void* buf, int64_t cap, int64_t* out_bytes);
TGX_API int tgx_restore_row(tgx_ctx* ctx, int row, const void* buf, int64_t bytes);

/* ---- greedy speculative decoding: verifying a row's draft in one pass (additive to ABI 3) ---------------------------------------------------------------
 * A decode step streams the weights once for one position; a pass over a few positions of ONE sequence streams them once as well (tgx_extend_row).  A caller that
 * can guess the next tokens (a draft: prompt lookup, a small model) has the model check the guess in one pass.  `row` is a live, unfinished row that has a current
 * token t0 (device resident; the host need not know it) and `past` positions in its cache.  The call runs ONE causal pass — tgx_extend_row's, with its routes and
 * attention forms — over the inputs [t0, draft[0], .., draft[n_draft - 1]] at positions past .. past + n_draft, computes the logits of EVERY one of these
 * n_draft + 1 positions and each position's greedy token g[i] (highest value, lowest index on a tie).  a = the number of leading i with g[i] == draft[i]; the
 * row produces a + 1 tokens: draft[0 .. a - 1] followed by g[a].
 *
 *   Afterwards        the row stands exactly as after a + 1 greedy steps of tgx_decode_rows: length past + a + 1, current token g[a], the logits slot and argmax
 *                     partials those of the position that produced g[a], the next embedding gathered (GPT-2: with wpe at the advanced position).  The result
 *                     equals those steps up to the order of the fp32 sums — the contract between kernel paths.  Cache rows beyond the new length were written by
 *                     the pass and are DEAD: nothing reads them, and the cache stays append-only from the new length.
 *   Stop conditions   the row's own (tgx_set_row_stop): the produced tokens are counted against max_new and the stop set one by one, in order, on the device, and
 *                     acceptance ends at the token that finishes the row.  out_finish is 0 / 1 / 2 as in tgx_decode_rows; out_n <= a + 1 tokens are returned in
 *                     out_ids (the call's own read-back: the call returns when the pass has finished, like an admission); tgx_past_length_row grows by exactly
 *                     out_n.  A finished row then behaves as after tgx_decode_rows.
 *   Sampler           greedy only: a row whose settings (tgx_set_row_sampler) are not greedy is TGX_ERR_UNSUPPORTED.
 *   Refused           null pointers, row outside [0, max_batch), n_draft outside [1, TGX_MAX_DRAFT], a draft id out of range: TGX_ERR_INVALID.  A retired, empty
 *                     or finished row, a row without a current token (fresh from tgx_forward_row / tgx_extend_row), a truncated row that holds no logits, a
 *                     poisoned context: TGX_ERR_STATE.  past + n_draft + 1 > max_ctx: TGX_ERR_CONTEXT.  Paged KV: the blocks for past + n_draft + 1 are counted
 *                     against the free list before anything is assigned (TGX_ERR_CONTEXT); more than 1024 blocks per row: TGX_ERR_UNSUPPORTED as for tgx_extend_row.
 *   ALL OR NOTHING    a refused call changes no row, moves no KV block, leaves kv.free_tokens as it was and does not poison the context.
 *   Paged KV          blocks are assigned for the whole pass up front; afterwards the row's blocks beyond ceil(new length / 128) go back to the pool, so
 *                     kv.free_tokens is what a row of the new length leaves.  The first new position falls into a block the row owns; shared (forked) blocks are
 *                     never written.
 *   Other rows        keep their state bit for bit and do not step.
 *   Steps and tickets the call is no decode step: it is stream-ordered behind the steps already enqueued, writes neither the token log nor the host ring and moves
 *                     no ticket, so tgx_step_async / tgx_fetch_token tickets and tgx_decode's ids stay exact; the produced ids come back in out_ids only.  On row 0
 *                     the last produced token becomes ticket 0's token (as after tgx_sample).
 *   tgx_read_probs    as after a greedy step: the row reads as zeros (and with no sampled row in the batch the call is TGX_ERR_STATE, as it always is).
 *   Cost              one weight pass for the layers, and for lm_head one pass on the matrix-core route of 5-16 positions, ceil((n_draft + 1) / 4) otherwise. */
#define TGX_MAX_DRAFT 15
TGX_API int tgx_verify_row(tgx_ctx* ctx, int row, const int64_t* draft, int n_draft, int64_t* out_ids /* [n_draft + 1] */, int32_t* out_n, int32_t* out_finish);

/* ---- speculative decoding under sampling: verifying a draft with the row's own sampler (additive to ABI 3) ----------------------------------------------
 * tgx_verify_row for a row that SAMPLES.  A sampled token here is a pure function of its position's fp32 logits, the row's sampler settings and the draw key
 * (row seed, index of the produced token, row) — tgx_decode_rows draws with nothing else.  The token s[i] the row would draw at position i of the pass is
 * therefore known from that position's logits alone, and "accept while the draft equals the draw" produces precisely the ids tgx_decode_rows would have
 * produced: the output distribution is untouched by construction, with no rejection-sampling arithmetic.  For a point-mass draft (prompt lookup) a draft token
 * is accepted with its probability under the filtered distribution, as in textbook speculative sampling.
 *
 *   The pass          tgx_verify_row's: the inputs [t0, draft[0], .., draft[n_draft - 1]] at positions past .. past + n_draft, the logits v_i of every position.
 *                     s[i] = the token the row's OWN settings (tgx_set_row_sampler: cfg and seed) draw from v_i with the key (row seed, past + i + 1, row), the
 *                     key tgx_decode_rows would use for the token at that index.  a = the number of leading i with s[i] == draft[i]; the row produces a + 1
 *                     tokens: draft[0 .. a - 1] followed by s[a].
 *   Greedy row        the call IS tgx_verify_row: the same launches, the same bits.
 *   Afterwards        the row stands as after out_n steps of tgx_decode_rows, up to the order of the fp32 sums: length past + out_n, current token the last
 *                     produced id, the logits slot and argmax partials those of the position that produced it, the next embedding gathered (GPT-2: with wpe).
 *                     tgx_sample_row with the row's cfg and seed right after the call returns the last produced id again (same logits, same key).
 *   Everything else   the refusals and their order, ALL OR NOTHING, the stop-condition walk (on the device, token by token), the paged-KV block accounting, "other
 *                     rows keep their state bit for bit", steps and tickets: as for tgx_verify_row, word for word.  A logit processor on: TGX_ERR_UNSUPPORTED
 *                     unless option verify.processors is 1 (below).  tgx_verify_row itself still refuses a sampled row.
 *   Log-probabilities recorded as by tgx_verify_row, one record per produced token: the MODEL's distribution, which the sampler does not touch.
 *   tgx_read_probs    the row has no vector until its next sampled step (the rule of tgx_fork_row): the pass's scratch is not the row's.
 *   Memory            the first call on a sampled row allocates the positions' sampler workspace: 16 x vocab x 12 bytes of compacted lists and 16 scratch
 *                     records.  A context that never makes such a call allocates nothing new and runs exactly the launches it ran before; greedy calls
 *                     through this entry allocate only what tgx_verify_row allocates.
 *   Cost              tgx_verify_row's, plus ONE sampler chain of the row's cfg whose launches carry the n_draft + 1 positions on blockIdx.y (3 launches for
 *                     T / top-p, the CLI default).  Measured (profiles/verify_sampled.txt; Llama-3.2-1B bf16, context 2048, T 0.8 / top-p 0.9, ms per call):
 *                     1.313 / 1.250 / 1.312 at 4 / 8 / 16 positions against 1.297 / 1.239 / 1.303 for the greedy verify of the same build: +0.010 .. +0.016,
 *                     less than the +0.037 one row's chain adds to a decode step (0.788 against 0.750). */
TGX_API int tgx_verify_row_sampled(tgx_ctx* ctx, int row, const int64_t* draft, int n_draft, int64_t* out_ids /* [n_draft + 1] */, int32_t* out_n, int32_t* out_finish);

/* ---- verifying processed rows: speculative decoding for rows with penalties, a logit bias or an automaton (additive to ABI 3) ------------------------------
 * tgx_set_option(ctx, "verify.processors", 1) — default 0, read back by tgx_get_option, set any time after tgx_finalize, read at each call.  At 0 every call
 * returns, launches and allocates what it did before the option existed.  At 1 the CHAIN calls — tgx_verify_row, tgx_verify_row_sampled, tgx_verify_rows, a
 * TGX_ADV_STEP row of tgx_advance_rows, a chain-shaped tgx_verify_tree — accept a row with a logit processor on (penalties, bias list, automaton; below), and a
 * call on rows with no processor on still runs exactly the launches and bits of option 0.  Nothing in the processors needs one launch per token:
 *
 *   Positions         the pass's inputs are in[0] = t0 (the row's current token), in[1 ..] = the draft.  Position i of the row's M positions sees
 *                       history  w_i[e] = the row's word for e with its count raised by #{ j <= i : in[j] == e } (saturating, the prompt bit kept): what i + 1
 *                                counting steps would have left;
 *                       state    s_i = the row's state word moved by in[0 .. i] under the step's rule (an entry that is NONE leaves the state where it is);
 *                       vector   the four-stage formula below on the pass's raw logits v_i with w_i, the row's bias list and s_i — the same code and roundings
 *                                as a step's processor launch.
 *   Choice            g[i] = the lowest-index argmax of position i's processed vector (a greedy row), or the draw of the row's chain over it with the key
 *                     (seed, past + i + 1, row) — a pure function of the processed fp32 vector, the settings and the key, as in tgx_decode_rows.  The accept
 *                     walk, the stop-set / max_new counting, out_ids / out_n / out_finish and the paged-block trim are unchanged.
 *   Afterwards        with n = out_n: the row's history words are raised by in[0 .. n - 1] and by nothing else (the tokens the n equivalent steps consume; the
 *                     rejected tail and the last produced token are not counted); its state word is s_{n-1}.  Both are committed on the device behind the walk.
 *                     The logits slot and argmax partials are the RAW ones of the producing position: tgx_read_logits and the logprobs ring stay the model's.
 *                     tgx_sample_row with the row's settings right after the call returns the last produced id again (the history and state as they stand are
 *                     what position n - 1 was processed with).  No tgx_read_probs vector until the row's next sampled step.  A refused call changes neither
 *                     the history nor the state.
 *   Still refused     a processed row on a tree that is no chain (tgx_verify_tree "Not built"); every other refusal, in the same order.
 *   Memory            the first one-row call on a processed row allocates a processed slab of 16 x vocab floats with its per-tile partials and 16 state
 *                     words; the first joint call with a processed row the same for 64 positions.  A context that never makes such a call holds none of it.
 *   Cost              per call with a processed row: one one-workgroup launch that walks the automaton states (only with an automaton on) and one launch of
 *                     ceil(vocab / 1024) x positions workgroups that reads the positions' raw logits and the row's words and writes the slab; the commit
 *                     rides in the accept launch.  Positions of unprocessed rows get no workgroup.  Measured (profiles/verify_processed.txt, tools/spec_bench.py
 *                     --processors; Llama-3.2-1B bf16, context 2048, a bias list, penalties and an automaton on the row, ms per tgx_verify_row, median of 3
 *                     rounds x 9 calls): 1.290 / 1.223 / 1.279 at 4 / 8 / 16 positions against 1.289 / 1.233 / 1.303 for the same build's call with no
 *                     processor on: +0.000 / -0.011 / -0.024, at or inside the spread of the rounds' medians (0.001 .. 0.026) — the two launches do not show
 *                     in the call (the accept launch merges 126 per-tile partials per position instead of the lm_head's); 1.66 .. 1.75 times one
 *                     tgx_decode_rows step of the processed row on the parent commit's library (0.739).  On a text a regular expression forces (tgx_cli,
 *                     GPT-2 geometry, greedy): 5.58 tokens per verify pass and 5310 decode-only tokens/s against 3556 for the regex alone on the parent. */

/* ---- tree speculative decoding: verifying a token TREE in one pass (additive to ABI 3) -------------------------------------------------------------------
 * A chain of guesses stops paying at its first wrong token.  A token tree spends the same <= 16 positions of one pass on alternatives: several candidates for the
 * next token, each with its own continuation.  The draw identity of tgx_verify_row_sampled makes it exact for free: the row's draw at a given depth is ONE token,
 * so at most one child of a node matches it, and the walk follows that child.
 *
 *   The tree          tokens[i] / parent[i], i < n_nodes, in topological order: parent[i] = -1 (a child of the row's current token t0) or an index < i.  Two
 *                     children of one parent never carry the same token.
 *   The pass          t0 is pass position 0 at depth 0; node i is pass position i + 1 at depth depth(parent) + 1.  ONE pass runs all M = n_nodes + 1 positions:
 *                     position p is written to cache slot past + p, rotated (RoPE) for sequence position past + depth(p), and attends to the history [0, past)
 *                     and to exactly its ancestors and itself among the new slots.
 *   The walk          on the device, from cur = position 0: the row's settings choose g from cur's logits — greedy: highest value, lowest index on a tie;
 *                     sampled: the draw with the key (row seed, past + depth(cur) + 1, row), the key tgx_decode_rows would use for that token.  g is produced
 *                     and counted against the row's stop set / max_new.  If the row has not finished and a child of cur carries g, cur becomes that child;
 *                     otherwise the walk ends.  out_n <= max depth + 1.
 *   Afterwards        the row stands as after out_n steps of tgx_decode_rows, up to the order of the fp32 sums: length past + out_n, the current token, the
 *                     logits slot and argmax partials, the next embedding, the cache rows [0, past + out_n).  The accepted inputs' K / V rows are moved from
 *                     slot past + path[j] to slot past + j bit for bit (K was rotated for its depth, which is j: no second rotation).  Rows beyond are DEAD.
 *   A chain           parent[i] == i - 1 for every i: the call IS tgx_verify_row_sampled — the same launches, the same bits, on every route, with everything
 *                     that call supports (log-probability records included).
 *   Everything else   as for tgx_verify_row_sampled, word for word: ALL OR NOTHING, the paged-KV block accounting for past + M up front and the trim afterwards,
 *                     shared blocks never written, other rows bit for bit, steps and tickets, tgx_read_probs.  tgx_read_pass_logits returns the M positions'
 *                     logits in pass order.
 *   Refused           in this order.  Null pointers, row outside [0, max_batch), n_nodes outside [1, TGX_MAX_TREE_NODES], a token id out of range:
 *                     TGX_ERR_INVALID.  Then the row's state, as tgx_verify_row_sampled checks it and in its order: a retired, empty or finished row, no
 *                     logits, no current token: TGX_ERR_STATE; a logit processor or an automaton on: TGX_ERR_UNSUPPORTED; past + n_nodes + 1 > max_ctx:
 *                     TGX_ERR_CONTEXT.  Then the tree's shape: parent[i] outside [-1, i), two children of one parent with the same token: TGX_ERR_INVALID.
 *                     Then, for a tree that is NO chain, TGX_ERR_UNSUPPORTED when the row records log-probabilities, when the pass cannot take the skinny
 *                     matrix-core route (fp32 storage, GPT-2, option prefill.mfma or prefill.skinny at 0, shapes the skinny kernels do not cover, a head_dim
 *                     other than 64 / 128) or when a paged cache has more than 1024 blocks per row.  Last the paged cache's room: TGX_ERR_CONTEXT.
 *                     Option prefill.min_rows is a speed threshold for chains and does not bind a tree: every M in [3, 16] runs the skinny route.
 *   Not built         trees in tgx_verify_rows / tgx_advance_rows; log-probability records on a tree that is no chain; a row with a logit processor or an
 *                     automaton on a tree that is no chain, whatever option verify.processors says (a position's history and state would depend on its
 *                     branch): TGX_ERR_UNSUPPORTED.
 *   Cost              tgx_verify_row_sampled's for the same number of positions, plus ONE compaction launch of layers x kv_heads x 2 workgroups
 *                     (profiles/verify_tree.txt; Llama-3.2-1B bf16, context 2048, greedy, ms per call: 1.263 / 1.281 / 1.354 at 4 / 8 / 16 positions against
 *                     1.296 / 1.231 / 1.309 for the parent build's chain pass, whose repeated medians spread by 0.011). */
#define TGX_MAX_TREE_NODES 15   /* = TGX_MAX_DRAFT: root + nodes <= 16 positions of one pass */
TGX_API int tgx_verify_tree(tgx_ctx* ctx, int row, const int64_t* tokens /* [n_nodes] */,
                            const int32_t* parent /* [n_nodes]: -1 = child of the row's current token, else an index < i */, int n_nodes,
                            int64_t* out_ids /* [n_nodes + 1] */, int32_t* out_n, int32_t* out_finish);

/* Test / diagnostic use, like tgx_read_kv: the fp32 logits [M][vocab] of the M = n_draft + 1 positions of the last tgx_verify_row / tgx_verify_row_sampled pass,
 * or of the M = n_nodes + 1 positions of the last tgx_verify_tree pass in pass order (the row's current token, then the nodes by index); *out_rows = M.  TGX_ERR_STATE when the workspace holds no such pass: no call yet, tgx_score_row's group form or another verify call that failed has used it
 * since, or after tgx_reset_cache.  cap_rows < M: TGX_ERR_INVALID, nothing is written.  Synchronises the stream. */
TGX_API int tgx_read_pass_logits(tgx_ctx* ctx, float* out /* [cap_rows][vocab] */, int cap_rows, int32_t* out_rows);

/* ---- batched speculative decoding: the drafts of several rows verified in one pass (additive to ABI 3) --------------------------------------------------
 * tgx_verify_row_sampled for n rows at once.  A scheduler that holds a draft for some rows of its batch otherwise pays one pass over all the weights and one
 * read-back PER ROW; here the current tokens and drafts of all named rows go through ONE causal pass (the ragged pass of tgx_forward_rows, each sequence from its
 * own length), ONE lm_head over all positions and ONE accept launch, and the host reads n records back once.
 *
 *   Equivalence       the call equals n calls tgx_verify_row_sampled(rows[i], draft_i, n_draft[i], ..) in array order, up to the order of the fp32 sums (the
 *                     contract between kernel paths).  Rows are independent, so the order is immaterial.  draft_i = the n_draft[i] ids behind those of the rows
 *                     before it in `drafts`; row i's results are out_ids[i * (TGX_MAX_DRAFT + 1) ..], out_n[i], out_finish[i].
 *   Settings, keys    every row uses its OWN settings: a greedy row applies tgx_verify_row's rule, a sampled row draws position j with the key (row seed,
 *                     past_i + j + 1, row) — nothing another row does enters it.
 *   n_draft[i] == 0   legal here (unlike the one-row calls): the row takes part with its current token alone and produces exactly one token, as one
 *                     tgx_decode_rows step would.  A scheduler can advance every unfinished live row in one call, with or without a draft.
 *   Limits            M = sum(n_draft[i] + 1) <= TGX_MAX_VERIFY_POSITIONS; n in [1, max_batch]; rows distinct.
 *   Refused           per row in array order, each row's checks in tgx_verify_row_sampled's order with its codes: null pointers, a row out of range, n_draft
 *                     outside [0, TGX_MAX_DRAFT], a draft id out of range, a row named twice, n < 1, M too large: TGX_ERR_INVALID.  A retired, empty or finished
 *                     row, a row with no current token or no logits, a poisoned context: TGX_ERR_STATE.  A logit processor on any named row: TGX_ERR_UNSUPPORTED.
 *                     past_i + n_draft[i] + 1 > max_ctx for any row: TGX_ERR_CONTEXT.  More than 1024 blocks per row on a matrix-core route: TGX_ERR_UNSUPPORTED.
 *   Paged KV          the blocks of ALL named rows are counted together against the free list before any is assigned; if they do not all fit: TGX_ERR_CONTEXT.
 *   ALL OR NOTHING    a refused call changes no row, moves no block, leaves kv.free_tokens as it was and does not poison the context.
 *   Afterwards        per row, tgx_verify_row_sampled's statement word for word: length past_i + out_n[i] and the current token; the logits slot and argmax
 *                     partials of the producing position; the next embedding gathered (GPT-2: with wpe at the advanced position); the stop-condition walk on the
 *                     device, token by token; one log-probability record per produced token; no tgx_read_probs vector for a sampled row; paged blocks beyond
 *                     ceil(new length / 128) back in the pool; on row 0 the last produced id becomes ticket 0's token.  Rows not named keep their state bit for
 *                     bit and do not step; no ticket, token log or host ring moves.
 *   tgx_read_pass_logits   after this call: all M positions in call order, *out_rows = M (cap_rows up to TGX_MAX_VERIFY_POSITIONS); otherwise unchanged.
 *   Forms             read-only option `verify.last_form`: 0 no call yet, 1 the joint pass, 2 row by row.  Row by row — fp32 storage, `prefill.mfma` 0, layer
 *                     shapes the matrix-core tile does not cover, M below the matrix-core routes' minimum — runs each row's own pass, draws and accept launch
 *                     behind the joint checks and block count: the results are those of the one-row calls bit for bit.
 *   Attention         option `extend.attn_splits` as for tgx_extend_row: 0 the per-sequence prompt attention from each past_i; N >= 1 the ragged key-split form
 *                     (grid heads x N x rows; a row uses min(N, its key tiles) splits, merged in split order: the same bits from run to run); -1 splits when
 *                     the longest past_i + n_draft[i] + 1 exceeds tgx_extend_row's threshold, with min(32, 2 * CUs / (n * heads)) splits (two workgroups per
 *                     CU: measured, profiles/verify_rows.txt), unsplit below 2.  The threshold itself is the one measured for ONE row.  Read-only option
 *                     `verify.last_splits`: the splits of the last joint pass (0: unsplit).
 *   Memory            the first call sizes the joint workspace: 64 hidden rows, logits [64][vocab], argmax partials, n records, 64 draws.  A context that never
 *                     makes the call allocates nothing new and runs exactly the launches it ran before.
 *   Cost              measured (tools/spec_bench.py --rows, profiles/verify_rows.txt; Llama-3.2-1B bf16, context 2048, synchronised ms per call; baselines
 *                     from the parent commit's library).  4 positions per row, 2 / 4 / 8 rows: the joint call takes 1.29 / 1.44 / 1.92 with greedy rows and
 *                     1.35 / 1.60 / 2.14 with rows at T 0.8 / top-p 0.9, against 2.5 / 5.1 / 10.0 for as many one-row calls and 0.97 / 1.05 / 1.09 for one
 *                     plain step of those rows.  8 positions per row: 1.35 / 1.63 / 2.12 and 1.42 / 1.80 / 2.40, against 2.4 / 4.8 / 9.4.  The joint pass
 *                     beats plain stepping from a mean of 0.34 (2 rows, 4 positions, greedy) to 1.17 (8 rows, 8 positions, sampled) accepted draft tokens
 *                     per row on.  Every sampled row adds its own sampler chain, about 0.03 ms per row. */
#define TGX_MAX_VERIFY_POSITIONS 64
TGX_API int tgx_verify_rows(tgx_ctx* ctx, int n, const int32_t* rows, const int64_t* drafts /* sum(n_draft) ids, back to back */,
                            const int32_t* n_draft /* [n], each in [0, TGX_MAX_DRAFT] */, int64_t* out_ids /* [n][TGX_MAX_DRAFT + 1] */, int32_t* out_n /* [n] */,
                            int32_t* out_finish /* [n] */);

/* ---- chunked prefill: prompt chunks and live rows' steps in one ragged pass (additive to ABI 3) -----------------------------------------------------------
 * While a prompt is prefilled every live row stands still, and the weights are streamed again for the live rows' next step.  tgx_advance_rows puts both into
 * ONE causal pass over the weights: each named row either STEPs (tgx_verify_rows' "current token + draft", 0 drafts = one plain step) or is FED the next piece
 * of its prompt.  A scheduler that admits a waiting request in pieces of <= N tokens, one piece per call, bounds the stall of its live rows by one such call.
 *
 *   Kinds             kinds[i] = TGX_ADV_STEP: a live row with a current token; lens[i] in [0, TGX_MAX_DRAFT] draft ids.  TGX_ADV_FEED: lens[i] >= 1 supplied ids;
 *                     the last position's logits land in the row's slot.  TGX_ADV_FEED_MORE: lens[i] >= 1 supplied ids, more of the prompt follows: no lm_head
 *                     for this row.  `ids` holds sum(lens) ids back to back in array order (it may be NULL when that sum is 0).
 *   Equivalence       the call equals, up to the order of the fp32 sums (the contract between kernel paths): tgx_verify_rows over the STEP rows in array order;
 *                     for each FEED / FEED_MORE row on a retired or empty row < batch or a new row, tgx_forward_row(row, its ids, lens[i]); for each FEED /
 *                     FEED_MORE row on a live or finished row that holds >= 1 positions — a row in the no-logits state included — tgx_extend_row(row, its ids,
 *                     lens[i]): the current token is discarded and a finished state is cleared.  The new rows of a call are exactly batch .. batch + k - 1, as
 *                     for tgx_forward_rows.  A prompt fed in pieces leaves the row as tgx_forward_row of the whole prompt does, up to the order of the sums.
 *   FEED_MORE         afterwards the row holds past + lens[i] positions and is in tgx_truncate_row's state "no logits and no current token": tgx_sample_row,
 *                     the decode calls, tgx_fork_row and a STEP on it are TGX_ERR_STATE until a FEED, tgx_extend_row or tgx_score_row has run on it;
 *                     tgx_save_row works (the prefix-only snapshot).  An admission by FEED_MORE counts as an admission: stop state and token count afresh,
 *                     log-probability record count 0, settings kept.
 *   Outputs           STEP rows: out_ids[i * (TGX_MAX_DRAFT + 1) ..], out_n[i], out_finish[i] as tgx_verify_rows.  FEED and FEED_MORE rows: out_n[i] = 0,
 *                     out_finish[i] = 0.  Named rows otherwise end as the equivalent calls leave them; rows not named keep their state bit for bit and do not
 *                     step.  No ticket, token log or host ring moves.  tgx_read_pass_logits returns the STEP positions in call order (TGX_ERR_STATE after a call
 *                     without a STEP row).
 *   Limits            the STEP positions together (sum of lens[i] + 1) <= TGX_MAX_VERIFY_POSITIONS; all positions together <= TGX_MAX_ADVANCE_POSITIONS; n in
 *                     [1, max_batch]; rows distinct.  A call with no STEP row, or with no FEED row, is legal.
 *   Refused           first the call's own: null pointers, n out of range, a kinds[i] outside 0 .. 2, a lens[i] < 0, either position limit: TGX_ERR_INVALID.  Then
 *                     per row in array order, each row's checks in the order and with the codes of its equivalent call (tgx_verify_rows' per-row checks, a
 *                     logit processor on a STEP row -> TGX_ERR_UNSUPPORTED included; tgx_extend_row's; tgx_forward_row's), a row named twice TGX_ERR_INVALID;
 *                     then "the new rows are batch .. batch + k - 1" (TGX_ERR_INVALID) and, on a paged cache, more than 1024 blocks per row on a matrix-core
 *                     route (TGX_ERR_UNSUPPORTED).
 *   Paged KV          the blocks of ALL named rows are counted together against the free list plus what the target rows of admissions give back, before any
 *                     is assigned; if they do not all fit: TGX_ERR_CONTEXT.  STEP rows give the blocks of their rejected tail back, as after tgx_verify_rows.
 *   ALL OR NOTHING    a refused call changes no row, moves no block, leaves kv.free_tokens as it was and does not poison the context.
 *   Forms             read-only option `advance.last_form`: 0 no call yet, 1 the joint pass, 2 piecewise.  Piecewise — fp32 storage, `prefill.mfma` 0, layer
 *                     shapes the matrix-core tile does not cover, all positions together below the matrix-core routes' minimum — runs the equivalent calls one
 *                     after another behind the joint checks and block count (tgx_verify_rows, then the continuations in array order, then the admissions in
 *                     row order): the results are those calls' results bit for bit.
 *   The joint pass    the ragged pass of tgx_forward_rows with every sequence from its own length, the STEP sequences first in the workspace: one all-position
 *                     lm_head pass and one accept launch for the STEP rows (tgx_verify_rows' own; where the STEP positions alone would not take the short-prompt
 *                     route, one pass per four positions), ceil(F / 4) lm_head passes for F FEED rows (tgx_forward_rows' own), none for FEED_MORE rows; one
 *                     upload of tables + ids, one sampler chain per sampled STEP row, one read-back.
 *   Attention         option `advance.attn_tiles` (kernels/attn_mixed.h): one work list whose items carry a key range.  0: never split — the pass's list is
 *                     exactly tgx_forward_rows' list and order, one workgroup per (sequence, query block, head) walking every 64-key tile of its causal range.
 *                     N >= 1: a query block whose range exceeds N tiles is cut at tile boundaries into ranges of <= N tiles (at most 32 ranges; N is doubled
 *                     while the partials would exceed 512 MiB), each leaving an unnormalised partial; a merge launch walks a block's partials in split
 *                     order: the same bits from run to run.  At most three launches per layer (whole blocks, ranges, merge).  -1: the largest N that gives
 *                     those launches two workgroups per CU, the rule measured for tgx_verify_rows' key-split form.  The default is 16: it won or tied the
 *                     sweep of profiles/advance_rows.txt (head_dim 64, contexts up to 2048; head_dim 128 unmeasured), where -1 did not.  Read-only option
 *                     `advance.last_tiles`: the N of the last joint pass.
 *   Memory            a context that never makes the call allocates nothing new and runs exactly the launches it ran before.  The first call with a STEP row
 *                     sizes tgx_verify_rows' workspace, the first joint pass that splits a block the partials' (grown on demand).
 *   Cost              measured (tools/admit_bench.py --mixed, profiles/advance_rows.txt; Llama-3.2-1B bf16, ms per call, the baseline tgx_decode_rows(1) +
 *                     tgx_extend_row(chunk) on the parent commit's library, spread of a figure ~0.05): 8 step rows at context ~300 plus a chunk of 128 / 256 /
 *                     512 at past 256: 2.77 / 3.50 / 4.52 against 2.93 / 3.54 / 4.46 — below the two calls by more than the spread at 128, inside it at 256 and
 *                     512.  32 step rows: 3.56 / 4.14 / 5.19 against 3.32 / 3.91 / 4.83 — ABOVE the two calls, and at context 2048 6.10 against 4.20: a STEP
 *                     row's one query rides a 128-query block of the prompt attention (one of four waves works), which the batched step's own attention
 *                     kernel does not pay.  What the call buys at those shapes is the bound on the stall (one call per tick, no live row waits for a whole
 *                     prompt), not time. */
#define TGX_ADV_STEP      0
#define TGX_ADV_FEED      1
#define TGX_ADV_FEED_MORE 2
#define TGX_MAX_ADVANCE_POSITIONS 8192
TGX_API int tgx_advance_rows(tgx_ctx* ctx, int n, const int32_t* rows, const int32_t* kinds, const int64_t* ids /* sum(lens) ids back to back, in array order */,
                             const int32_t* lens /* [n] */, int64_t* out_ids /* [n][TGX_MAX_DRAFT + 1] */, int32_t* out_n /* [n] */, int32_t* out_finish /* [n] */);

/* ---- per-token log-probabilities on the device (additive to ABI 3) --------------------------------------------------------------------------------------
 * n-best ranking, beams and the completions protocol's `logprobs` / `top_logprobs` (the reference's server speaks it) need the model's opinion of the tokens it
 * produces.  For a row that produced token t from the fp32 logits v[0 .. V) — what the argmax and the sampler look at, tgx_read_logits(rounded = 0) —
 * lp(t) = v[t] - lse(v), lse(v) = max + log sum exp(v - max) with the sum taken in double in a fixed association and rounded once.  The distribution is the
 * MODEL's: temperature 1, before top-k / top-p / min-p — the same for a greedy and a sampled row.  The top-N alternatives are the first N entries of v in the order
 * (value descending, index ascending), as (id, lp) pairs in that order; the produced token need not be among them.  -inf logits rank last and have lp -inf.
 *
 *   Setting           per row: top_n = -1 off (the default), 0 the produced token's log-probability only, 1 .. TGX_MAX_LOGPROBS that many alternatives as well.
 *                     Stream-ordered and kept across calls; tgx_reset_row / tgx_reset_cache restore "off", like tgx_set_row_sampler.  The first call that switches
 *                     a row on allocates the rings (TGX_LOGPROB_RING records per row); a context that never asks allocates nothing and runs exactly the launches
 *                     it ran before.  Out-of-range row or top_n: TGX_ERR_INVALID.
 *   What records      every token a row PRODUCES while its setting is >= 0 appends one record to its ring: tgx_sample_row (the first token after an admission,
 *                     tgx_extend_row or tgx_fork_row), tgx_decode_rows (one per step of an unfinished live row, the token that finishes it included),
 *                     tgx_verify_row (out_n of them, each from the logits of the position that produced it).  A finished or retired row that rides along
 *                     records nothing.  tgx_decode, tgx_sample and tgx_step_async ignore the setting, as they ignore the other row settings.
 *   Record count      back to 0 on tgx_reset_row, tgx_reset_cache and an admission or fork INTO the row; tgx_extend_row and tgx_truncate_row keep it (truncation
 *                     does not un-record).  A fork does not copy the source's records; the destination's setting is untouched.
 *   Reading           tgx_read_row_logprobs returns the row's last n records, oldest first; 1 <= n <= min(records since the count was reset, TGX_LOGPROB_RING),
 *                     otherwise TGX_ERR_INVALID and nothing is written (the caller knows the count from out_new / out_n and its own calls).  A row that has
 *                     recorded nothing is TGX_ERR_STATE.  The call synchronises the stream, like the other readers.  out_top_* may be NULL; entries beyond a
 *                     record's own top_n are id -1 / -INFINITY.
 *   Cost              two launches behind a step's publish while some row of the batch records (one more bit of the union that keys the per-row step graphs);
 *                     switching a row between top_n 0 .. TGX_MAX_LOGPROBS is read on the device and recaptures nothing.  Records are the same bits from run to run. */
#define TGX_MAX_LOGPROBS 20
#define TGX_LOGPROB_RING 256
TGX_API int tgx_set_row_logprobs(tgx_ctx* ctx, int row, int top_n);
TGX_API int tgx_read_row_logprobs(tgx_ctx* ctx, int row, int n, float* out_lp /* [n] */, int32_t* out_top_ids /* [n][TGX_MAX_LOGPROBS] */,
                                  float* out_top_lp /* [n][TGX_MAX_LOGPROBS] */, int32_t* out_top_n /* [n] */);

/* ---- scoring a sequence: every supplied token's log-probability in one prefill pass (additive to ABI 3) ------------------------------------------------
 * The logprobs ring above holds the model's opinion of the tokens a row PRODUCES; the completions protocol's `echo` + `logprobs`, the perplexity of a checkpoint on
 * a text and the ranking of candidate continuations behind a shared prefix (tgx_fork_row) need it for the tokens the caller SUPPLIES.  tgx_score_row is a prompt
 * pass that also returns them, at the cost of one all-position lm_head instead of one pass per prefix.
 *
 *   The pass          on a retired row, an empty one or row == batch the call IS tgx_forward_row(row, ids, seq); on a live or finished row that holds >= 1
 *                     positions it IS tgx_extend_row(row, ids, seq): the same route, the same refusals in the same order with the same status codes, all or
 *                     nothing, the same block accounting on a paged cache, and the same row afterwards — the last position's logits in the row's slot, no current
 *                     token, a fresh stop state, the sampler settings kept.  The logits slot, the KV rows and every id sampled afterwards are the plain call's bits.
 *   Outputs           for i in [0, seq - 1): out_lp[i] = v_i[ids[i + 1]] - lse(v_i), v_i the fp32 logits of the pass's position i and lp as defined above
 *                     (temperature 1, the model's distribution, whatever the row's sampler).  With top_n >= 1 also the first top_n entries of v_i in the order
 *                     (value descending, index ascending) as (id, lp) pairs; entries beyond top_n are id -1 / -INFINITY.  out_top_* may be NULL.  The LAST position
 *                     scores nothing: its logits are in the row's slot (tgx_sample_row, tgx_read_logits).  ids[0]'s own score is not produced either — on the
 *                     extend form, to score the first new token as well, tgx_truncate_row(row, past - 1) and pass the dropped token as ids[0].
 *                     seq == 1 is legal and writes nothing.
 *   Refusals          top_n outside [0, TGX_MAX_LOGPROBS] and a null out_lp with seq > 1 are TGX_ERR_INVALID, checked ahead of the pass's own; nothing changes.
 *   Side effects      nothing is recorded in the row's logprobs ring and its count does not move.  The call synchronises like an admission; the scores come back
 *                     in one read-back.  A context that never calls it allocates nothing new and runs exactly the launches it ran before.
 *   How               no [seq][V] buffer exists (2048 x 128256 fp32 would be 1 GiB).  16-bit storage on the matrix-core route: groups of at most `score.rows`
 *                     positions (option; a multiple of 64, default 2048); per group the final norm, then per `score.vocab_chunk` columns (a multiple of 1024,
 *                     default 16384) one product against that slice of the lm_head rows and one tile launch that keeps, per position and 1024-entry tile of V,
 *                     (max, sum of exp, first top_n keys, the target's value); one record launch per group merges the tiles in a fixed association.  Each logit
 *                     is one K-ordered sum on one pinned kernel form and the tile partition of V is global, so the scores are the same bits for every legal
 *                     option value and from run to run.  The weights stream once per group.  Every other route (short prompts, fp32 storage, prefill by steps)
 *                     scores in groups of TGX_MAX_DRAFT + 1 positions through tgx_verify_row's all-position lm_head.  Read-only option `score.last_form`, the form of the
 *                     last call that scored a position: 0 none yet, 1 matrix cores, 2 by groups. */
TGX_API int tgx_score_row(tgx_ctx* ctx, int row, const int64_t* ids, int seq, int top_n, float* out_lp /* [seq - 1] */,
                          int32_t* out_top_ids /* [seq - 1][TGX_MAX_LOGPROBS] */, float* out_top_lp /* [seq - 1][TGX_MAX_LOGPROBS] */);

/* ---- embeddings: the pooled final hidden state of several texts in one ragged pass (additive to ABI 3) --------------------------------------------------------
 * Retrieval, reranking and classification read the model's final hidden state, not its logits (Qwen3-Embedding is a plain Qwen3 checkpoint pooled at the last
 * token).  tgx_embed_rows is tgx_forward_rows without lm_head plus one pooling pass: no [V][H] head is streamed and no logits exist afterwards.
 *
 *   Admission         exactly tgx_forward_rows' rules, checks, status codes and order: each row a retired row < batch or one of the next new rows, rows distinct, every
 *                     length in [1, max_ctx], every id in range, the 1024-block limit of a paged cache; ALL OR NOTHING — the blocks of the whole call are counted
 *                     before any is assigned; a refused call changes no row, moves no block and does not poison the context.  The call's own checks come first:
 *                     a null pointer, a pool that is none of the three, dims outside [0, hidden] are TGX_ERR_INVALID.
 *   The pass          the groups, routes and launches of tgx_forward_rows (one-row passes where no ragged route applies: fp32 storage, prefill.mfma 0, unsupported
 *                     shapes, short groups) with NO lm_head launch and no lm_head staging.
 *   The vector        per pooled position the model's final norm (model.norm; GPT-2: ln_f with bias) of the fp32 final residual — the row lm_head would be
 *                     multiplied with, rounded to the storage dtype under act.round16 as that input is.  Pooled in fp32: TGX_POOL_LAST / TGX_POOL_FIRST take one
 *                     position, TGX_POOL_MEAN is sum / len.  dims: 0 = hidden, else the first dims components are kept (Matryoshka truncation) BEFORE
 *                     normalisation; normalize != 0 divides by the L2 norm (a zero vector stays zero).  out[i] is text i's vector, [n][dims ? dims : hidden].
 *   Reproducibility   the MEAN sum is taken in an order that depends on the text's length alone: slices of 32 consecutive positions summed in position order, the
 *                     slices merged in slice order; no atomics.  The same call returns the same bits from run to run.
 *   Afterwards        release == 0: row i holds its lens[i] positions in tgx_truncate_row's no-logits state (as TGX_ADV_FEED_MORE leaves a row): tgx_extend_row,
 *                     tgx_truncate_row, tgx_reset_row and tgx_save_row work on it; the decode and sample calls are TGX_ERR_STATE until it has logits.  Its per-row
 *                     settings start afresh as for an admission.  release != 0: every named row is retired as by tgx_reset_row before the call returns and its
 *                     blocks are back in the pool (the batch size may still have grown to cover new rows).  The call synchronises: out is valid on return.  Rows
 *                     not named keep their state bit for bit.
 *   Memory            a context that never calls it allocates nothing new.  The partial sums are one hidden row per 32 pooled positions, never [M][hidden].
 *                     Read-only option `embed.last_pool_launches`: pooling launches (partials + finish) of the last call. */
#define TGX_POOL_LAST  0   /* the last position (Qwen3-Embedding, causal LMs) */
#define TGX_POOL_MEAN  1   /* the mean over all positions of the text */
#define TGX_POOL_FIRST 2   /* the first position */
typedef struct { int32_t pool; int32_t normalize; int32_t dims; int32_t release; } tgx_embed_cfg;
TGX_API int tgx_embed_rows(tgx_ctx* ctx, int n, const int32_t* rows, const int64_t* ids /* sum(lens), back to back */,
                           const int32_t* lens, const tgx_embed_cfg* cfg, float* out /* [n][dims ? dims : hidden] */);

/* ---- per-row logit processors on the device: penalties and logit bias (additive to ABI 3) -------------------------------------------------------------------
 * The completions protocol's `presence_penalty`, `frequency_penalty` and `logit_bias`, `repetition_penalty` of a checkpoint's generation_config.json, and "never
 * emit this id" (a bias of -INFINITY: EOS suppressed for a minimum length, bad-word ids) — per row, read on the device, stepped in the same graphs as the sampler
 * settings.  The raw logits are never modified: tgx_read_logits and the logprobs ring keep reading the MODEL's; tgx_read_probs returns the vector the draw used.
 *
 *   History           one 32-bit word per (row, token id): bit 31 "occurs in the prompt", bits 0 .. 30 n = the number of times the row produced the id (saturating).
 *                     tgx_set_row_history REPLACES the row's words: clear, then set from the two lists (either may be empty with a null pointer).  The library never
 *                     looks at prompt ids by itself.
 *   Counting          in a tgx_decode_rows step an unfinished live row whose processors are on (any non-neutral penalty, or a non-empty bias list) first counts its
 *                     current token — the one the step consumes.  Finished and retired rows neither count nor process (settings and a history stated for a retired
 *                     row are kept and take effect with its admission, like the log-probability setting); tokens produced while a row's processors were
 *                     off are not counted (a caller who switches penalties on mid-generation supplies the history).  tgx_extend_row and tgx_truncate_row keep the
 *                     words; tgx_fork_row copies the source's words into each destination (its settings are untouched, like its sampler settings).
 *   Formula           every operation rounded once to fp32, no fused multiply-add.  Per entry i with raw fp32 logit v:
 *                       1. if prompt-bit or n > 0:  v = v > 0 ? v / repetition : v * repetition
 *                       2. v = v - frequency * (float)n;  v = v - (n > 0 ? presence : 0)
 *                       3. if i is in the row's bias list:  v = v + bias
 *                     Temperature and the filters follow unchanged.
 *   Where             tgx_decode_rows; tgx_sample_row (the row's settings, no counting step: the row has no current token then).  tgx_decode, tgx_sample and
 *                     tgx_step_async ignore the processors, as they ignore every row setting.  tgx_verify_row on a row with a processor on is TGX_ERR_UNSUPPORTED
 *                     unless option verify.processors is 1 (the verify calls then process every position of the pass: "verifying processed rows" above).
 *   Settings          per row, kept across calls until changed, stream-ordered; the caller's arrays may be freed on return.  tgx_reset_row / tgx_reset_cache restore
 *                     the neutral settings (repetition 1, presence 0, frequency 0), empty the bias list and clear the row's history.
 *   Refusals          TGX_ERR_INVALID, nothing changes: a null cfg, a row outside [0, max_batch), repetition <= 0 or non-finite, a non-finite presence or frequency,
 *                     n outside [0, TGX_MAX_LOGIT_BIAS], a bias id out of range or named twice, a bias that is NaN or +INFINITY (-INFINITY is legal, on fewer than
 *                     vocab entries), a history id out of range.  Before tgx_finalize: TGX_ERR_STATE.
 *   Cost              the first non-neutral setting or non-empty history of a context allocates the buffers (the words, a processed-logits slab [max_batch][vocab]);
 *                     a context that never asks allocates nothing and runs exactly the launches it ran before, and neutral values on such a context are a no-op.
 *                     One launch ahead of a step's publish while some row of the batch has a processor on (one more bit of the union that keys the per-row step
 *                     graphs); the values are read on the device and changing them recaptures nothing. */
#define TGX_MAX_LOGIT_BIAS 320
typedef struct tgx_penalty_cfg { float repetition, presence, frequency; } tgx_penalty_cfg;  /* neutral: 1, 0, 0 */
TGX_API int tgx_set_row_penalties(tgx_ctx* ctx, int row, const tgx_penalty_cfg* cfg);
TGX_API int tgx_set_row_logit_bias(tgx_ctx* ctx, int row, int n, const int32_t* ids, const float* bias);  /* n = 0 clears */
TGX_API int tgx_set_row_history(tgx_ctx* ctx, int row, const int64_t* prompt_ids, int n_prompt, const int64_t* produced_ids, int n_produced);

/* ---- constrained decoding: per-row token automata stepped on the device (additive to ABI 3) ------------------------------------------------------------------
 * "Answer yes / no / maybe", "a date", "this JSON template": an allowed set that covers the whole vocabulary and changes with every token, which a bias list
 * cannot state.  The constraint is a token-level automaton resident on the device: a row carries an automaton id and a state word, the logit-processor launch
 * masks the row's logits with the allowed set of its state, and the state moves on the device as the row consumes tokens — no host round trip per token, in
 * the same multi-step graphs as every other row setting.  The host compiles a pattern into a table once per request (host/constraint.h).
 *
 *   Table             next[n_states][vocab], 16-bit words: next[s][t] = the state after token t in state s, or TGX_AUTOMATON_NONE (t is not allowed in s).  The
 *                     library knows nothing about EOS: a caller that wants a row to be able to end in state s gives its stop ids a valid target there.  Stored on
 *                     the device as it is, n_states * vocab * 2 bytes, by the one owner of device memory ("mem.live_allocs" / "mem.live_kib" count it);
 *                     tgx_automaton_destroy frees it.  The caller's array is the caller's again on return.  At most TGX_MAX_AUTOMATA live tables per context.
 *   Validation        on the host (csrc/automaton.h), before anything is allocated or copied.  TGX_ERR_INVALID: n_states outside [1, TGX_MAX_AUTOMATON_STATES],
 *                     start outside [0, n_states), an entry that is neither a state of the table nor NONE, a state with no allowed token (a dead end is the
 *                     compiler's bug, not the kernel's problem), a null pointer, a 17th live table.  Before tgx_finalize: TGX_ERR_STATE.
 *   State word        follows the history words' convention: the state after every token the row has CONSUMED while the automaton was on.  A tgx_decode_rows
 *                     step of an unfinished live row first advances the state by the row's current token (state = next[state][token]) and then masks with the
 *                     new state's allowed set.  tgx_sample_row masks with the state as it stands and advances nothing: the row has no current token then.  A
 *                     consumed token that the state does not allow leaves the state where it is — only a caller that switched the automaton on mid-stream, or
 *                     set a state that does not belong to the row's text, can feed one.  Finished and retired rows neither advance nor mask.
 *                     tgx_read_row_automaton returns the word as it stands (id -1 and state -1 for a row without one); a caller that wants the state including
 *                     the current token looks up its own table.
 *   Formula           step 4 of the processors' formula above, after the bias: an entry i with next[state][i] == NONE becomes -INFINITY.  Penalties and bias
 *                     compose with it unchanged.  The raw logits, tgx_read_logits and the logprobs ring stay the model's; tgx_read_probs returns the vector the
 *                     draw used (a disallowed id has probability exactly 0).
 *   Lifecycle         settings are stream-ordered and kept across calls.  tgx_set_row_automaton(row, id, state): id -1 switches the row off, state -1 is the table's
 *                     start.  tgx_reset_row / tgx_reset_cache switch the row off; the table lives on.  A setting made on a retired row takes effect with its
 *                     admission, like the other processors.  tgx_extend_row and tgx_truncate_row keep id and state.  tgx_fork_row copies the source's id and
 *                     state into each destination, as it copies the history words.  Snapshots do not hold the setting: settings are the caller's, and
 *                     tgx_read_row_automaton lets the caller keep it.  tgx_automaton_destroy of a table that any row, live or retired, still names is
 *                     TGX_ERR_STATE (it waits for the stream before it frees).
 *   Refusals          tgx_set_row_automaton, TGX_ERR_INVALID and nothing changes: a row outside [0, max_batch), an unknown id, a state outside [-1, n_states).
 *                     Before tgx_finalize: TGX_ERR_STATE.
 *   A processor       the automaton is a logit processor: every rule about "a processor on" applies unchanged.  tgx_verify_row, tgx_verify_row_sampled,
 *                     tgx_verify_rows and a STEP row of tgx_advance_rows refuse such a row with TGX_ERR_UNSUPPORTED unless option verify.processors is 1;
 *                     tgx_decode, tgx_sample and tgx_step_async ignore it, as they ignore every row setting.
 *   Cost              a context that never creates an automaton allocates nothing new and runs exactly the launches it ran before; so does a context that has
 *                     tables but no row using one.  The first row that names one allocates the processors' buffers (above).  While some row of the batch has one
 *                     on: the processor launch (2 * vocab more bytes read per constrained row) and, ahead of it, one one-workgroup launch that moves the state
 *                     words (one more bit of the union that keys the per-row step graphs).  Id and state are read on the device: changing them recaptures
 *                     nothing.  Measured (profiles/automaton.txt; Llama-3.2-1B bf16, ms per tgx_decode_rows step, no processor / a bias list on every row / an
 *                     automaton on every row): 1 row 0.6032 / 0.6086 / 0.6101, 8 rows 0.8082 / 0.8131 / 0.8149, 32 rows 1.1157 / 1.1358 / 1.1399 (spread of a
 *                     figure 0.5 us); the unconstrained step issues the parent build's launches, kernel for kernel.  tgx_automaton_create of a 64-state table at
 *                     V = 128256 (15.7 MiB): 25.5 ms.  Pattern compile time over a 128k vocabulary: unmeasured (no such tokenizer at hand). */
#define TGX_AUTOMATON_NONE 0xFFFFu        /* next[s][t]: token t is not allowed in state s */
#define TGX_MAX_AUTOMATON_STATES 65535    /* state ids 0 .. 65534 */
#define TGX_MAX_AUTOMATA 16               /* live tables per context */
TGX_API int tgx_automaton_create(tgx_ctx* ctx, int32_t n_states, int32_t start, const uint16_t* next /* [n_states][vocab] */, int32_t* out_id);
TGX_API int tgx_automaton_destroy(tgx_ctx* ctx, int32_t id);
TGX_API int tgx_set_row_automaton(tgx_ctx* ctx, int row, int32_t id /* -1: off */, int32_t state /* -1: the table's start */);
TGX_API int tgx_read_row_automaton(tgx_ctx* ctx, int row, int32_t* out_id, int32_t* out_state);   /* synchronises, like the other readers */

/* == GPTModel::contextSize() / numLayers() (src/model/GPTModel.h:97-98). */
TGX_API int64_t tgx_context_size(const tgx_ctx* ctx);
TGX_API int32_t tgx_num_layers(const tgx_ctx* ctx);

/* ---- diagnostics ------------------------------------------------------------------------- */

/* Last error text for this context (or for tgx_create when ctx == NULL). */
TGX_API const char* tgx_last_error(const tgx_ctx* ctx);

/* Blocks until all work enqueued on the context's stream has finished. */
TGX_API int tgx_synchronize(tgx_ctx* ctx);

/* Reads back the KV cache of (row, layer) as fp32 into k_out/v_out, each [pastLength of that row][kv_heads][head_dim]
 * (the BSHD view KVCacheManager::append returns, Attention.h:106).  Test/diagnostic use. */
TGX_API int tgx_read_kv(tgx_ctx* ctx, int row, int layer, float* k_out, float* v_out);

/* The inverse of tgx_read_kv: overwrites cache rows [0, n_rows) of (row, layer), n_rows <= pastLength, from fp32 k_in / v_in
 * [n_rows][kv_heads][head_dim] (either may be NULL), rounded once to the cache's storage dtype.  Test/diagnostic use: with the CPU path's
 * cache rows injected, a decode step is compared free of the bf16 KV-rounding floor (the reference's KVCacheManager holds the tensors
 * it was given, CacheManager.h:24-51 — there is nothing to overwrite there).  Paged KV: a range that touches a block shared with forked rows (tgx_fork_row)
 * is TGX_ERR_STATE — writing through would change the siblings. */
TGX_API int tgx_write_kv(tgx_ctx* ctx, int row, int layer, const float* k_in, const float* v_in, int64_t n_rows);

/* Per-kernel-class timing with HIP events on the context's stream (bench.py's roofline leg).  For each
 * class (TGX_KERNEL_*) the kernels of ALL layers are launched back-to-back between two events, n_reps times,
 * at the current context length; returns launch counts and summed milliseconds.  Every launch streams a
 * different layer's weights (nothing repeats out of the Infinity Cache); residual outputs go to a scratch
 * vector so pastLength, the KV cache and the current token are unchanged (the logits buffer is consumed). */
#define TGX_KERNEL_QKV 0
#define TGX_KERNEL_ATTN 1
#define TGX_KERNEL_OPROJ 2
#define TGX_KERNEL_GATEUP 3
#define TGX_KERNEL_DOWN 4
#define TGX_KERNEL_LMHEAD 5
#define TGX_KERNEL_COUNT 6
TGX_API int tgx_profile_decode(tgx_ctx* ctx, int n_reps, int64_t* launches /*[TGX_KERNEL_COUNT]*/,
                       double* total_ms /*[TGX_KERNEL_COUNT]*/);

/* Final probability vector(s) [batch*vocab] of the last non-greedy tgx_sample / decode step: what the
 * reference passes to multinomial (Sampler.cpp:77) — zero where top-k/top-p/min-p removed a token.  A step
 * does not materialise the vector (the draw needs per-tile sums only): this call evaluates it from what the
 * step left on the device — valid until the next tgx_forward / tgx_forward_row / tgx_set_logits replaces the
 * logits (TGX_ERR_STATE then); rows whose last step was greedy read as zeros. */
TGX_API int tgx_read_probs(tgx_ctx* ctx, float* out);

/* Injects logits [batch][vocab] as if a forward had produced them, so that Sampler::sample can be
 * exercised on its own (the reference's Sampler takes any [B,V] tensor, Sampler.h:30). */
TGX_API int tgx_set_logits(tgx_ctx* ctx, const float* logits, int batch);

/* Launch-geometry knobs for tuning sweeps (results stay within the parity tolerances; summation order may change):
 *   "<class>.ks"   waves sharing a row pair's K range (1/2/4), class in {qkv,oproj,gateup,down,lmhead}
 *   "<class>.bpc"  grid cap in workgroups per CU ("lmhead.bpc" only before tgx_finalize)
 *   "<class>.packed_bpc"  the same for the class's exponent-packed batch-1 launch, class in {gateup,down,lmhead} (default 3 / 4 / 4; "lmhead.packed_bpc" only before tgx_finalize)
 *   "attn.nsplit"  KV splits per kv head (<= 32, before tgx_finalize); "attn.gmax" query heads per attention workgroup
 *   "attn.direct_max"  contexts up to this many keys run attention as one workgroup per head group, without the combine launch (default 768 at head_dim 64, 384 at 128; 0 = never)
 *   "graph" 0/1    hipGraph replay vs eager launches; "graph.steps" decode steps per graph for long tgx_decode calls
 *   "prefill.min_rows"  prompts shorter than this take passes through the decode kernels instead of the batched prefill (default 7)
 *   "prefill.splitk" 0/1  split K over workgroups when a prompt gives the GEMMs few row tiles (default 1)
 *   "prefill.mfma" 0/1  batched matrix-core prefill vs passes through the decode kernels; "prefill.gemm_tm" 64/128 row tile
 *   "act.round16" 0/1  (default 0) numerics contract: 1 = the input of every Linear is rounded to the storage dtype (round-to-nearest-even) before the
 *                  product — what a module constructed in config.torch_dtype sees (ModelLlama.h:62) — instead of entering in fp32.  The matrix-core
 *                  products of the prefill and of batched steps then take one 16-bit term per activation instead of two or three;
 *                  fp32 storage: no effect.  Set it before the first tgx_forward of a sequence: the cache of a sequence must be filled under one contract
 *   "kv.budget_tokens"  (default 0; set BEFORE tgx_finalize, which sizes the caches; 16-bit storage dtypes) PAGED KV — the kernel contract of the reference's
 *                  "Paged Attention" TODO (README.md:32-34).  0: every row owns a max_ctx slab ([layer][kv_head][max_ctx][hd], max_batch x max_ctx tokens of
 *                  cache whatever the rows hold).  N > 0: the caches are pools of 128-token blocks worth N tokens in all, shared by the rows; a row's blocks are
 *                  assigned as its sequence grows (a device-resident block table per row, read by the attention and cache-append kernels) and returned by
 *                  tgx_reset_row / tgx_reset_cache; max_ctx stays the per-row limit.  A call that would need a block when none is free returns TGX_ERR_CONTEXT and
 *                  changes nothing (retire a row, retry).  Results are those of the unpaged cache, bit for bit on the same kernels (tests/test_hip_paged.py);
 *                  tgx_get_option "kv.free_tokens" = the unassigned blocks' worth of tokens (-1 when unpaged)
 *   "extend.attn_splits"  (default -1) the attention of a tgx_extend_row pass of <= 128 positions (16-bit storage): -1 = split over the keys (kernels/attn_extend.h) from
 *                  the measured context on, min(32, CUs / heads) splits; 0 = never (the per-row prompt attention, which also serves longer passes, fp32 storage and
 *                  passes by steps); N >= 1 = N splits (at most one per 64-key tile) wherever the split form applies.  tgx_get_option reads it back
 *   "advance.attn_tiles"  (default 16) the attention of a tgx_advance_rows joint pass: a query block whose causal key range exceeds this many 64-key tiles is cut into
 *                  ranges of at most that many (kernels/attn_mixed.h); 0 = never split, -1 = the largest target that gives the launches two workgroups per CU.
 *                  tgx_get_option reads it back, and the read-only "advance.last_form" / "advance.last_tiles" (tgx_advance_rows above)
 *   "weights.fp8" 0/1  (default 0; set BEFORE tgx_finalize, TGX_ERR_STATE afterwards; bf16 storage, not GPT-2 — anything else makes tgx_finalize return
 *                  TGX_ERR_UNSUPPORTED) FP8 WEIGHTS, opt-in and LOSSY: tgx_finalize quantizes every matrix of the classes in "weights.fp8_classes" — gate_up
 *                  (the merged gate | up matrix), down, and lm_head (embed_tokens when tied) — to OCP E4M3 codes with one power-of-two scale per output row and
 *                  OVERWRITES the bf16 master in place with the dequantized values, so prefill, batched steps, verify / advance passes, score, embed and beam
 *                  select all compute the same model as the batch-1 step, which streams the codes (kernels/gemv_fp8.h: half the bytes of these matrices per
 *                  token).  Rule per output row r (the gate and up rows are rows of the merged matrix):
 *                    1. amax is the largest |w| of the row.  Write amax = m * 2^x with m in [0.5, 1) (frexp).
 *                    2. e_r = x - 9 if m <= 0.875, else x - 8.  This is the smallest e with amax <= 448 * 2^e.
 *                    3. Clamp e_r to >= -117, so the smallest non-zero dequantized value stays a normal bf16.
 *                    4. An all-zero row takes e_r = 0.
 *                    5. code = round-to-nearest, ties-to-even, of the exact quotient w / 2^e_r onto the OCP e4m3fn grid.  Subnormals of step 2^-9 are
 *                       included and the sign is kept, so -0 stays -0.  The codes 0x7f and 0xff (NaN) are never produced.
 *                    6. dq = code * 2^e_r.  It is always exactly representable in bf16.
 *                    7. A selected matrix that holds a non-finite weight or a |w| >= 2^100 makes tgx_finalize return TGX_ERR_UNSUPPORTED and name the tensor.
 *                  A context with the option on therefore equals, bit for bit, an ordinary context that was uploaded dq (tests/fp8_ref.py is the rule in numpy).
 *                  A matrix whose shape the 8-bit stream does not cover (more than 8 chunks of 8 weights per lane: K > 16384) is quantized all the same and
 *                  served by the plain kernel on the dequantized master.  A class quantized this way gets no exponent-packed copy ("weights.packed").
 *                  MEMORY: the bf16 masters stay (every multi-row path reads them), so the option COSTS one byte per weight of the selected classes, about
 *                  1.07 GB on Llama-3.2-1B.  Out of scope: qkv / o_proj, multi-row steps and prefill reading the codes, dropping the masters, pre-quantized
 *                  checkpoints with other scales, per-group scales, an FP8 KV cache
 *   "weights.fp8_classes"  (default 7; before tgx_finalize) which classes "weights.fp8" quantizes: bit 0 gate_up, bit 1 down, bit 2 lm_head
 *   "debug.*"      experiment switches (tools/gemv_dissect.py, tools/attn_dissect.py; live only in a -DTGX_DISSECT=1 build) */
TGX_API int tgx_set_option(tgx_ctx* ctx, const char* key, int value);

/* Reads back what the library would do for the CURRENT batch size (no reference counterpart; callers that time a decode region use it to keep the
 * region on one attention form instead of mirroring the defaults):
 *   "attn.direct_limit"  decode steps at contexts up to this many keys run the direct attention form (batch-1 steps at head_dim 64: with the
 *                        o_proj product in the same launch), beyond it the split form
 *   "attn.nw4_limit"     ... and up to this many keys its four-wave variant (0 = never)
 *   "graph.steps"        decode steps per captured multi-step graph
 * Read-only figures: "weights.packed_matrices" / "weights.packed_fallbacks" / "weights.packed_max_row_esc" (after tgx_finalize), "kv.free_tokens" (above),
 *   "weights.fp8_matrices"   matrices that "weights.fp8" gave an 8-bit stream (after tgx_finalize) ...
 *   "weights.fp8_fallbacks"  ... and matrices it quantized that the plain kernel serves on the dequantized master, and
 *   "mem.live_allocs"    device buffers the context holds now: weights, caches, and the workspaces that were sized at first use or grown since ...
 *   "mem.live_kib"       ... and their bytes, rounded up to KiB.  A workspace that grows replaces its buffer: a context's figures depend on the largest shapes it has
 *                        served (and on "act.round16" at the last growth), not on the way there — what a test can hold memory to on a device that others use */
TGX_API int tgx_get_option(const tgx_ctx* ctx, const char* key, int* out_value);

/* Algorithmic HBM bytes one decoded token streams at context length T (SURVEY.md §8d formula).  Matrices stored exponent-packed (option "weights.packed",
 * bf16 storage) count with the bytes the batch-1 step really streams: their packed planes and escape records instead of 2 bytes per weight; matrices with an
 * 8-bit stream (option "weights.fp8") likewise: their code planes as laid out plus one 4-byte scale per row. */
TGX_API int64_t tgx_bytes_per_token(const tgx_ctx* ctx, int64_t T);

TGX_API int tgx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TGX_H */
