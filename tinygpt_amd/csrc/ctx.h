// ctx.h — the context of the MI355X shim (include/tgx.h) and the host-side launch interface shared by its translation units:
//   abi.hip          C ABI entry points, weight upload, step graphs, decode loop, prompt admission (route, pass issuer, tgx_forward_row / tgx_forward_rows),
//                    the device side of paged-KV block assignment (table pushes) and tgx_fork_row with its copy launch (kernels/kv_fork.h)
//   kv_pool.h        KvPool: the paged cache's block bookkeeping (free list, per-block row counts, the table's host mirror) — host-only, checked on a CPU
//   row_snapshot.h   the byte format of a row snapshot (tgx_save_row / tgx_restore_row): header, size formula, validation — host-only, checked on a CPU
//   dev_mem.h        DevMem: the owner of every device allocation of the context (dev_alloc / dev_free / dev_grow below) — host-only, checked on a CPU
//   decode.hip       batch-1..4 decode step: GEMV launches (kernels/gemv.h, oproj_sliced.h), lm_head, greedy finalize
//   attn.hip         decode attention launches (kernels/attn_decode.h, attn_decode_mfma.h)
//   sampler.hip      Sampler::sample (kernels/sampler.h)
//   prefill.hip      batched MFMA prefill, 16-bit storage (kernels/prefill.h, gemm_dma.h); the device tables of a ragged pass; the launches of tgx_score_row (kernels/score.h)
//                    and tgx_embed_rows (kernels/embed_pool.h) behind a pass
//   prefill_f32.hip  batched prefill, fp32 storage (kernels/gemm_f32.h)
//   skinny.hip       batched decode step / short prompts on the skinny MFMA GEMMs (kernels/skinny*.h)
// One context = one GPU = one HIP stream; every call comes from one host thread.  There is NO CPU path in this library.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tgx.h"
#include "kernels/common.h"
#include "kv_pool.h"
#include "dev_mem.h"

using tgx::bf16_t;
typedef unsigned char ebyte;   // parameter / KV-cache storage in the compute dtype: offsets are elements * ctx.esz

namespace tgx { struct SampScratch; struct LpRecord; struct LpRow; }

constexpr int MAX_TICKET_EVENTS = 64;
constexpr int HOST_RING = 256;

// a bf16 matrix in the lossless 12-bit exponent-packed form (kernels/gemv_packed.h; option weights.packed): made once in tgx_finalize beside the bf16 original,
// read by the batch-1 decode launches of its class.  P == nullptr: not packed (option off, class not adopted, other dtype / shape, or a row's escapes overflowed)
struct PackedMat {
  unsigned char* P = nullptr;     // planes, N * row_bytes
  tgx::u32x4* rec = nullptr;      // [N][ks] escape records, one per (row, K-part)
  long long row_bytes = 0;
  unsigned int e0h4 = 0;          // E0h * 0x01010101: the window's base in every byte
  int ks = 0;                     // the K split the planes are laid out for: a launch with another split takes the plain kernel
  int max_row_esc = 0;            // most escapes in one row
  long long n_esc = 0;            // escapes of the matrix
};

// the 8-bit stream of a matrix quantized by option weights.fp8 (kernels/gemv_fp8.h): E4M3 codes in the batch-1 launch's layout and one power-of-two scale per
// row, made in tgx_finalize; the bf16 master beside it holds the dequantized values.  Q == nullptr: no stream (option off, class not selected, or a shape the
// layout does not cover — the plain kernel then reads the dequantized master)
struct Fp8Mat {
  unsigned char* Q = nullptr;     // code planes, N * row_bytes
  float* scale = nullptr;         // [N] 2^e_r
  long long row_bytes = 0;
  int ks = 0;                     // the K split the planes are laid out for: a launch with another split takes the plain kernel
};

struct LayerW {
  ebyte *in_norm = nullptr, *post_norm = nullptr;
  ebyte *wqkv = nullptr, *bqkv = nullptr, *wo = nullptr, *wgu = nullptr, *wdown = nullptr;
  PackedMat pgu, pdown;         // wgu / wdown exponent-packed
  Fp8Mat qgu, qdown;            // wgu / wdown as 8-bit streams (option weights.fp8)
  ebyte *q_norm = nullptr, *k_norm = nullptr;   // Qwen3 [head_dim]
  bool q_norm_ok = false, k_norm_ok = false;
  // one bit per checkpoint tensor that lands in a merged weight: q, k, v, gate, up (bits 0-4) and the q/k/v biases (bits 5-7) — a tensor
  // uploaded twice must not stand in for a missing one of the same size
  int merged_filled = 0;
  bool in_norm_ok = false, post_norm_ok = false, wo_ok = false, wdown_ok = false;
  // GPT-2 (ModelGPT2.h:23-135): LayerNorm biases and a bias on every Conv1D; wgu holds c_fc [inter][hidden]
  ebyte *in_norm_b = nullptr, *post_norm_b = nullptr, *bo = nullptr, *bfc = nullptr, *bdown = nullptr;
  int gpt2_filled = 0;      // bit per GPT-2 tensor of the layer (12 of them)
};

struct RowState {       // independent KV/sequence state of one batch row
  float *x = nullptr, *q = nullptr, *attn = nullptr, *h = nullptr;   // fp32 activations
  float* k_raw = nullptr;   // Qwen3: un-normalised k of the current position
  float* logits = nullptr;
  float* probs = nullptr;   // final probabilities of the last sampled step [V]
  float* part_val = nullptr;
  int* part_idx = nullptr;
  float* attn_part = nullptr;
  int *tok = nullptr, *pos = nullptr;
  long long* prompt = nullptr;
  ebyte *kcache = nullptr, *vcache = nullptr;   // [layers][kv_heads][max_ctx][hd] in the compute dtype; paged KV: the pools [layers][blocks][kv_heads][KV_BLOCK][hd], shared by the rows
  const int* tbl = nullptr;                     // paged KV: this row's block table on the device
};

struct RowHost {        // host state of one batch row
  int64_t past = 0;     // mirror of the row's own device pos (tgx_reset_row / tgx_forward_row, include/tgx.h)
  bool tok = false;     // the row has a current token (sampled after its last forward)
  bool idle = false;    // the row was retired (tgx_reset_row) and not refilled: it rides in the steps, nothing waits for it, its output means nothing
  bool nologits = false;   // the row was truncated (tgx_truncate_row) and not extended since: its slot's logits belong to a position it no longer holds, so nothing may sample, step or fork from it
  char fin = 0;         // the finish reason of the last tgx_decode_rows readback (0 running, 1 stop id, 2 max_new) — a finished row keeps its length, rides along without advancing and counts for neither `past` nor the context check
  int64_t lp_count = 0; // mirror of the row's device-side record counter (tgx_read_row_logprobs): records appended since the count was reset
  bool probs_ok = false; tgx_sampler_cfg probs_cfg{};   // the row's last sampled step was a non-greedy one, and its sampler configuration (tgx_read_probs evaluates the vector on demand)
  bool probs_proc = false;   // ... and it drew from the processed logits (kernels/logit_proc.h): tgx_read_probs evaluates the vector from that slab
  int auto_id = -1;          // the automaton the row names (tgx_set_row_automaton; -1: none) — a setting: restart() keeps it, tgx_reset_row / tgx_reset_cache clear it
  // the slot starts over at `len` positions: no current token, its logits its own; what its last sampled step left (probs_ok, probs_cfg) stays
  void restart(int64_t len, bool idle_, char fin_) { past = len; tok = nologits = false; idle = idle_; fin = fin_; }
};

struct Tune {
  int ks = 1;    // waves sharing one unit's K range (1, 2, 4)
  int bpc = 4;   // grid cap in workgroups per CU
  // the same for the class's exponent-packed batch-1 launch (gate_up, down, lm_head; option <class>.packed_bpc) — the plain kernel of the class (fallen-back
  // matrices, other dtypes, batched steps) keeps bpc.  gate_up: 3 (tgx_create; -13 us per token on Llama-3.2-1B, also ahead on the 3B and Qwen2.5-0.5B shapes);
  // down and lm_head measured best at 4.  The lm_head's value is read at tgx_finalize, where lm_grid is fixed (profiles/packed_kpart_geometry.txt).
  int packed_bpc = 4;
};

struct Profiler {
  bool on = false;
  hipEvent_t ev[2 * 8] = {};
  int64_t launches[TGX_KERNEL_COUNT] = {};
  double ms[TGX_KERNEL_COUNT] = {};
};

// where the QKV product of a one-sequence prefill may finish its rows (prefill.hip launch_prefill -> launch_gemm)
struct QkvEpi { bf16_t *q_hi = nullptr, *q_lo = nullptr, *k = nullptr, *v = nullptr; int past = 0; const int* tbl = nullptr; };     // past: the position of the pass's first row (RoPE, cache append)

// a scoring pass (tgx_score_row): positions [0, n_score) of the pass each score the id at the next position
struct ScoreCall {
  int top_n = 0, n_score = 0;
  const long long* ids = nullptr;                     // the pass's ids on the device (the row's prompt buffer)
  void* host = nullptr; size_t host_bytes = 0;        // where the call's read-back lands: lp [n] (| top ids | top lps)
};

// an embedding pass (tgx_embed_rows): the pass issues no lm_head; behind it the pooled final-norm hidden state of every text (kernels/embed_pool.h)
struct EmbedCall {
  static constexpr int SLICE = 32;                    // == tgx::EMB_SLICE: pooled positions per row of the partials
  int pool = 0, normalize = 0, dims = 0;              // dims: resolved (hidden when the caller passed 0)
  int n = 0;                                          // texts of the call
  int cur = 0;                                        // the text a one-row pass carries (issue_pass)
  std::vector<int> tab;                               // host image of the device table, [n] x tgx::EmbedText {row0, np, slice0, pad}: ONE upload ahead of the passes
  int slices = 0;                                     // rows of the partials of the whole call
  float* host_out = nullptr;                          // where the read-back lands: [n][dims]
  int np(int t) const { return tab[(size_t)t * 4 + 1]; }
};

namespace tgx { struct RgSeq; struct RgItem; struct MixItem; }
// one ragged prefill pass of tgx_forward_rows: prompt i at workspace rows [first[i], first[i] + lens[i]) into batch row rows[i], positions 0 .. lens[i] - 1.
// abi.hip groups the prompts (the host fields, M, longest) and uploads the call's buffer; ragged_tables (prefill.hip) lays out and fills the device tables
struct RaggedPass {
  int n = 0, M = 0, longest = 0;
  const int *rows = nullptr, *lens = nullptr, *first = nullptr;   // host [n]
  const long long* ids = nullptr;            // device [M]: the pass's ids, prompts back to back
  const tgx::RgSeq* seq = nullptr;           // device [n] (kernels/prefill.h)
  const int* tok_seq = nullptr;              // device [M]: the prompt of each workspace row
  const tgx::RgItem* items = nullptr;        // device: the prompt-attention work list, heaviest first
  int n_items = 0;
  // tgx_verify_rows: sequence i continues its row from position past[i] (host [n]; nullptr: an admission, every one from 0).  ext_ns > 0: the attention is the ragged
  // key-split form (kernels/attn_extend.h attn_extend_rg_kernel) with that many splits, its partials sized by ensure_extend_rg_ws; 0: the work-list form
  const int* past = nullptr;
  int ext_ns = 0;
  // tgx_advance_rows (advance_tables): `items` holds the whole query blocks only; the blocks cut into key ranges are the two lists of the mixed attention
  // (kernels/attn_mixed.h), their partials mix_slots records of ctx.mix_part.  n_mix_split == 0: the work-list form alone
  const tgx::MixItem *mix_split = nullptr, *mix_merge = nullptr;
  int n_mix_split = 0, n_mix_merge = 0, mix_slots = 0;
};

inline void* hip_dev_alloc(size_t bytes) { void* p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }      // the library's two uses of the
inline void hip_dev_free(void* p) { (void)hipFree(p); }                                                                         // device allocator: tgx_ctx::mem
struct tgx_ctx {
  tgx_model_desc d{};
  DevMem mem{hip_dev_alloc, hip_dev_free};      // owns every device buffer below: tgx_destroy frees by its record, not by a list of names
  int device = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;
  std::string err;
  bool finalized = false;

  int dt = tgx::DT_BF16;   // storage dtype of parameters and KV cache (kernel template argument)
  size_t esz = 2;          // bytes per stored element
  ebyte *embed = nullptr, *lm_head = nullptr, *final_norm = nullptr;
  ebyte *wpe = nullptr, *final_norm_b = nullptr;      // GPT-2: learned positions [n_positions][H], ln_f.bias
  bool embed_ok = false, lm_head_ok = false, final_norm_ok = false, wpe_ok = false, final_norm_b_ok = false;
  bool gpt2 = false;
  std::vector<LayerW> L;
  // option weights.packed (read at tgx_finalize; default 1): bf16 gate_up / down / lm_head weights also stored exponent-packed for the batch-1 decode stream.
  // weights.packed_classes: which classes (bit 0 gate_up, 1 down, 2 lm_head).  Default: gate_up and lm_head — on Llama-3.2-1B the packed lm_head launch is
  // 14 us shorter and the packed gate_up launch 0.6 us per layer (1.5 us at its own 3 workgroups per CU, Tune::packed_bpc).  The packed down launch stays off:
  // with the escape records kept per (row, K-part) — 15 of its 16 matrices packed, a tenth of its waves with a record instead of a third — the step with it
  // measures the same as without it (0.6286 against 0.6288 ms, inside the run-to-run spread; profiles/packed_kpart_geometry.txt, profiles/packed_weights_hl.txt).
  // packed_matrices / packed_fallbacks: matrices packed / fallen back to plain
  int weights_packed = 1, packed_classes = 5, packed_matrices = 0, packed_fallbacks = 0, packed_max_row_esc = 0;
  PackedMat plm;                // the lm_head matrix (embed when tied) exponent-packed
  // option weights.fp8 (read at tgx_finalize; default 0, lossy): the matrices of the classes in weights.fp8_classes (bit 0 gate_up, 1 down, 2 lm_head) are
  // quantized to E4M3 codes with a power-of-two scale per row (the rule: include/tgx.h); the bf16 masters are overwritten with the dequantized values, so every
  // path computes the same model, and the batch-1 launches read the 8-bit streams.  A class quantized this way gets no exponent-packed copy.
  // fp8_matrices / fp8_fallbacks: matrices with a stream / quantized but served by the plain kernel
  int weights_fp8 = 0, fp8_classes = 7, fp8_matrices = 0, fp8_fallbacks = 0;
  Fp8Mat qlm;                   // the lm_head matrix (embed when tied) as an 8-bit stream
  float *rope_cos = nullptr, *rope_sin = nullptr;
  std::vector<RowState> rows;   // views into the per-row slabs below (constant row stride: batched GEMV walks them)
  float *slab_x = nullptr, *slab_q = nullptr, *slab_kraw = nullptr, *slab_attn = nullptr, *slab_h = nullptr, *slab_logits = nullptr;
  float *slab_probs = nullptr, *slab_part_val = nullptr, *slab_attn_part = nullptr;
  int *slab_part_idx = nullptr, *slab_tok = nullptr, *slab_pos = nullptr;
  long long* slab_prompt = nullptr;
  ebyte *slab_k = nullptr, *slab_v = nullptr;
  size_t kv_row_elems = 0, attn_part_row = 0;
  // prefill-by-steps processes up to 4 consecutive POSITIONS of one sequence per pass (rows of the batched kernels that share one
  // KV cache: kv_stride 0, pos[r] = past + r): fp32 storage, prompts shorter than 4 tokens, shapes the GEMM tile does not cover
  RowState chunk[4];
  float *ch_x = nullptr, *ch_q = nullptr, *ch_kraw = nullptr, *ch_attn = nullptr, *ch_h = nullptr, *ch_part = nullptr;
  int* ch_pos = nullptr;

  int64_t past = 0;       // host mirror of the device-resident pos: the LONGEST row of the batch (all rows, unless the per-row calls made them differ)
  std::vector<RowHost> row_host;   // [max_batch]
  // tgx_decode_rows (include/tgx.h): per-row sampler settings and stop conditions.  row_req [max_batch] on the device (kernels/common.h RowReq), pushed by value
  // in stream order; row_req_host mirrors the pushed fields
  tgx::RowReq* row_req = nullptr;
  std::vector<tgx::RowReq> row_req_host;
  int row_union = -1;     // steps being issued / captured: -1 = the launch-wide cfg (tgx_decode), else the ROWU_* union of the rows' chains (tgx_decode_rows)
  int batch = 0;          // rows used by the last forward
  bool have_logits = false, have_token = false;

  int* step = nullptr;    // device: number of decode steps finalized (monotonic)
  int* step_done = nullptr;   // device: rows of the current step that have read `step` (batches; 0 between steps)
  int* tok_log = nullptr; // device ring [log_cap][rows]
  int log_cap = 0;
  int* host_ring = nullptr;  // pinned host ring [HOST_RING][rows]
  int* host_ring_dev = nullptr;
  int64_t steps_issued = 0;
  hipEvent_t ticket_ev[MAX_TICKET_EVENTS] = {};
  int32_t last_sampled0 = -1;

  hipGraphExec_t step_graph = nullptr;      // the current entry of the cache below
  hipGraphExec_t multi_graph = nullptr;   // graph_steps consecutive decode steps (tgx_decode with many steps)
  // captured step graphs by (batch, sampler config, attention form): a generation that crosses an attention-form limit, or an engine that alternates between
  // sampler configurations / batch sizes, re-uses what it captured before instead of re-capturing (round 3; round 2 dropped the graphs at every change)
  // (per-row steps are keyed on the union of the rows' chains, not on cfg values: the kernels read every row's settings from row_req)
  struct GraphSet { hipGraphExec_t step = nullptr, multi = nullptr; int batch = 0; tgx_sampler_cfg cfg{}; int rows = -1; bool direct = false, mfma = false, nw4 = false; unsigned long long used = 0; };
  GraphSet graph_cache[6];
  unsigned long long graph_clock = 0;
  int graph_cur = -1;
  bool mirror_to_host = true;             // finalize / pick kernels also store the token into the pinned host ring (tgx_fetch_token)
  int graph_steps = 16;                   // measured: 1 -> 1389 tok/s, 8 -> 1396, 16 -> 1399 (the gap between two graph launches is ~4 us)
  unsigned long long* seed_dev = nullptr;
  unsigned long long seed_on_dev = 0;         // value last copied to seed_dev: an unchanged seed costs no copy and no stream sync
  bool seed_valid = false;
  tgx::SampScratch* samp_scratch = nullptr;   // [max_batch] histograms / thresholds / partial sums of the staged sampler
  unsigned long long* samp_list_comp = nullptr;   // [max_batch][vocab] compacted threshold-bin entries of a filter (kernels/sampler.h): composite keys ...
  float* samp_list_v = nullptr;                   // ... and logit / T
  bool have_probs = false;
  bool use_graph = true;

  Tune tune[TGX_KERNEL_COUNT];   // per kernel class: K-split and workgroups per CU
  int lm_grid = 0, attn_nsplit = 1, attn_nsplit_opt = 0;
  // batched-prefill workspace (grown on demand to the longest prompt seen)
  int ws_rows = 0;
  float *ws_x = nullptr, *ws_out = nullptr;           // [S][H] residual stream, [S][max(q+2kv, 2I)] GEMM output
  bf16_t *ws_ah = nullptr, *ws_al = nullptr;          // [S][max(H, qd, I)] GEMM A operand (hi, lo)
  bf16_t* ws_al2 = nullptr;                           // [S][H] third term for the QKV projection
  bf16_t *ws_qh = nullptr, *ws_ql = nullptr;          // [S][qd] rotated queries (hi, lo)
  bf16_t *ws_hh = nullptr, *ws_hl = nullptr;          // [S][I] siluMul output (hi, lo): the down product's A operand
  float* ws_part = nullptr; size_t ws_part_bytes = 0;   // split-K slabs of the short-prompt GEMMs
  bool poisoned = false;                                // a pass failed after some of its kernels were issued (device-side position / cache / counters may have moved): every entry point refuses until tgx_reset_cache
  const char* launch_fault = nullptr;                   // a launcher could not issue a kernel (a combination that is not instantiated): the issuing entry point fails with it
  int* ws_pos = nullptr;                                // fp32 prefill: [rows] positions of the prompt rows
  float* ws_ssq = nullptr;                              // [32][SK_NCB] partial sums of squares of the batched step's rows
  int gemm_splitk = 1;       // experiment: 0 disables split-K
  int wide_n_min = 2;        // ... from this many chips' worth of its workgroups (option prefill.wide_n_min)
  QkvEpi qkv_epi;
  int attn_dma = 1;          // option prefill.attn_dma: head_dim 64 prompts of three or more workgroups per CU take kernels/attn_prefill_dma.h (0 never, 2 always)
  int attn_ksplit = 1;       // option prefill.attn_ksplit: key split inside the prefill attention workgroup (0 never, 1 auto: head_dim 128, and head_dim 64 below three workgroups per CU, 2 always)
  int qk_fuse = 1;           // experiment: 0 keeps Qwen3's separate q/k norm launch
  // option prefill.skinny_rows: prompts of up to this many workspace rows take the skinny GEMMs (32: round 2; 33-64: four activation blocks, round 3).
  // Measured ms per prompt, four-block skinny / tiled split-K: Llama-3.2-1B S = 33 1.48 / 1.51, 48 1.51 / 1.58, 64 1.57 / 1.70; Qwen2.5-0.5B S = 48 1.46 / 1.81;
  // Llama-3.2-3B S = 48 3.54 / 3.33, Mistral-7B 6.76 / 5.52 — four blocks put 8 MFMAs + 9 LDS fragment reads behind every 32 k of a weight row: at
  // hidden > 2048 the tiled path's weight stream is faster (option prefill.skinny_hidden_max)
  // 65-128 rows: hidden <= 2048 only (abi.hip SKINNY_HIDDEN_MAX_WIDE)
  int prefill_skinny_rows = 128;
  int prefill_skinny_hidden_max = 8192;   // (the 2048 limit of the panel-kernel form is gone with the LDS-DMA ring kernel: Llama-3.2-3B S = 48 3.12 -> 2.98 ms, Mistral-7B 5.36 / 5.38)
  int skinny_dma = 1;          // option skinny.dma: products on stored 16-bit terms (two terms) run on the LDS-DMA ring kernel (kernels/skinny_dma.h)
  int skinny_dma_oproj = 2;    // option skinny.dma_oproj: the matrix-core attention of a batched step writes 16-bit terms, the o_proj product takes that kernel
  int decode_step_rows = 128;   // option decode.step_rows: rows of a batch that share one pass over the weights in the matrix-core step (32: round 2; 128: eight blocks on the LDS-DMA ring kernel — Llama-3.2-1B B = 128 2.99 -> 2.32 ms/step, Mistral-7B 13.25 -> 10.47)
  int prefill_skinny = 1;    // option prefill.skinny: 0 sends prompts of <= 32 rows through the tiled GEMMs as well
  // decode batches of at least this many rows run their Linears as skinny MFMA GEMMs (option decode.mfma_min_batch).  Measured ms/step,
  // GEMV row groups vs matrix cores: Llama-3.2-1B B = 2 0.794 / 0.991, B = 3 ~1.45 / 1.003, B = 4 1.042 / 1.007; Mistral-7B B = 4 5.04 / 4.01
  int decode_mfma_min = 3;
  bool prefill_mfma = true;
  int prefill_min_rows = 4;  // prompts shorter than this go through the decode kernels, 4 positions per pass (set in tgx_create)
  int prefill_f32_min_rows = 16;   // fp32 storage: prompts from this length on take the f32-input MFMA GEMMs (64-row tiles; option prefill.f32_min_rows)
  int gemm_tm = 0;           // experiment: force the GEMM row tile (64 / 128); 0 = by the number of tiles
  int debug_attn = 0;        // experiment: AttnArgs.dbg
  int attn_gmax = 0;         // experiment: query heads per attention workgroup (default 2)
  int attn_direct_nw4 = 0;   // option attn.direct_nw4: contexts up to this many keys run the direct attention form with four waves per head (set in tgx_create)
  bool attn_nw4 = false;     // mode of the launches being issued / captured
  int attn_raw_fuse = 2;     // option attn.raw_fuse: that form also finishes the QKV product (slab sums, bias, q / k norm, RoPE, cache append) in its prologue
  int attn_batch_mfma = 17;  // option attn.batch_mfma: batches of this many rows and more run their direct-form attention on the matrix cores (0 = never)
  int attn_direct_max = 384; // contexts up to this many keys take the one-workgroup-per-head attention (no split, no combine launch); set in tgx_create
  bool attn_direct = false;  // mode of the launches being issued / captured
  // contexts from attn_mfma_min keys on take the MFMA decode attention (kernels/attn_decode_mfma.h); like the direct form it is a mode of the
  // captured step: the graphs are re-captured when a decode call crosses the limit.  Not for Qwen3's fused q/k norm, not for fp32 storage.
  int skinny_terms = 1;            // option skinny.terms: batches of 17-32 rows take gate_up's activations as terms prepared once per layer (round 3)
  int skinny_ksplit = 1;           // wide products (gate_up, lm_head) of the batched step on the barrier-free K-split kernel (option skinny.ksplit)
  int defer_reduce = 1;            // split-K slabs of the prefill's N = hidden / QKV products are summed by the next row-wise kernel (option prefill.defer_reduce)
  int attn_mfma_min = -1;          // -1: the measured crossover of the geometry (attn_mfma_threshold); option attn.mfma_min overrides
  bool attn_mfma = false;
  int debug_gemv = 0;        // experiment: GemvArgs.dbg = value & 15 for the kernel classes selected by bits 8.. (1 << (8 + class))
  int debug_skip = 0;        // experiment: bit0 skip attn decode kernel, bit1 skip combine (results invalid)
  int prof_same_layer = 0;   // experiment: tgx_profile_decode replays ONE layer's weights (Infinity-Cache resident)
  // option oproj.sliced (default 1): batch-1 decode steps on the split attention form run o_proj K-sliced with the merge of the attention splits in its
  // prologue (kernels/oproj_sliced.h): no attn_combine launch; the residual stream between o_proj and down lives in fixed-point accumulators
  int oproj_sliced = 1;
  // option act.round16 (default 0): the input of every Linear is rounded to the storage dtype — the part of the reference's 16-bit-module contract
  // (ModelLlama.h:62) that has a price: the matrix-core products then take ONE 16-bit term per activation.  ws_zero: the "lo term"
  // every stored-term product reads in this mode
  int act16 = 0, act16_kernels = 1;
  int wide_8k_eff = 76;      // (Llama-3.2-1B S = 1152 7.28 -> 6.78 ms, 1280 7.52 -> 6.95, 1400 8.45 -> 8.14; at 87 % fill the 256 x 256 tiles win again) option prefill.wide_8k_eff (per cent): gate_up on 128 x 128 tiles when the 256 x 256 tiling's rounds are filled less than this
  int qkv_nosplit = 1;       // option prefill.qkv_nosplit: the balanced QKV launch instead of K slabs when it alone covers 3/4 of the chip
  int splitk_8k = 1;         // option prefill.splitk_8k: N = hidden products of 129-1500-row prompts as 2-4 K slabs on the eight-wave LDS-DMA kernel
  bf16_t* ws_zero = nullptr;
  // batch-1 steps on the direct attention form (short contexts, head_dim 64): the o_proj product runs in the attention launch's epilogue (attn_decode_kernel
  // template OPJ) — 4 launches per layer; the direct form then serves contexts up to attn_fused_max keys, with four wave-loads per softmax block up to attn_fused_nw4 keys and eight beyond (four waves per head either way); was: four / eight waves up to attn_fused_nw4
  int oproj_fused = 1, attn_fused_max = 640, attn_fused_nw4 = 384;
  // ---- paged KV (round 6; option kv.budget_tokens before tgx_finalize; include/tgx.h).  The caches become pools of KV_BLOCK-token blocks shared by the rows; a row's
  // blocks are assigned on the host as its sequence grows (before the launch that writes them) and returned by tgx_reset_row / tgx_reset_cache: `kv` (kv_pool.h)
  int kv_budget_tokens = 0;        // > 0: paged
  bool kv_paged = false;
  KvPool kv;                       // set up in tgx_finalize when paged: blocks, free list, the table's host mirror; kv.n_blocks() / kv.tbl_stride() size the pools and the table
  int* kv_tbl = nullptr;           // device [max_batch][kv.tbl_stride()]
  long long* slab_acc = nullptr;   // [max_batch][hidden], resting at zero between layers
  // tgx_forward_rows: the call's buffer (the RaggedPass device tables, then the ids; one upload per call) and four staging rows for the lm_head of scattered target rows
  unsigned char* rg_buf = nullptr; size_t rg_bytes = 0;
  float *rg_x = nullptr, *rg_logits = nullptr, *rg_part_val = nullptr; int* rg_part_idx = nullptr;
  // ---- tgx_extend_row / tgx_truncate_row (include/tgx.h)
  // option extend.attn_splits: the key-split attention of a continuation pass of <= 128 positions (kernels/attn_extend.h): -1 automatic, 0 never (the per-row prompt
  // attention with `past`), N >= 1 N splits (clamped to the key tiles).  Automatic: min(32, CUs / heads) splits once past + S exceeds extend_attn_min{64,128} (head_dim)
  // — the smallest measured context at which the split form wins by more than the spread of the measurement at every extension length (tools/admit_bench.py --extend,
  // profiles/extend_row.txt; ms per tgx_extend_row, per-row kernel / 8 splits, S = 16 / 64 / 128 new tokens):
  //   Llama-3.2-1B (head_dim 64, 16 layers)   past 256: 1.066 / 1.009, 1.345 / 1.332, 1.812 / 1.793 (the last two inside the spread)   past 512: 1.189 / 1.061, 1.441 / 1.369, 1.916 / 1.836
  //                                           past 2048: 1.884 / 1.165, 1.939 / 1.433, 2.398 / 1.897     past 8192: 4.625 / 1.492, 3.968 / 1.713, 4.463 / 2.169
  //   Mistral-7B shapes (head_dim 128, 2 layers)  past 512: 0.360 / 0.344, 0.482 / 0.475, 0.646 / 0.634 (about one spread: the same kernel read 0.360 and 0.374 in that run)
  //                                           past 1024: 0.401 / 0.348, 0.510 / 0.476, 0.673 / 0.635     past 8192: 0.933 / 0.418, 0.945 / 0.541, 1.108 / 0.698
  int extend_attn_splits = -1;
  int extend_attn_min64 = 512, extend_attn_min128 = 1024;
  float* ext_part = nullptr; size_t ext_part_bytes = 0;      // the splits' partials [ns][heads][attn_extend_part_vals][256] (kernels/attn_extend.h)
  // ---- tgx_verify_row (include/tgx.h; kernels/verify.h): the M <= VERIFY_ROWS positions of a verify pass — their hidden rows (the routes without a one-pass
  // lm_head stage them here, four to a pass over the weights), logits and argmax partials, and the record the accept launch leaves for the host.  Sized at first use
  enum { VERIFY_ROWS = TGX_MAX_DRAFT + 1 };
  float *vf_x = nullptr, *vf_logits = nullptr, *vf_part_val = nullptr; int *vf_part_idx = nullptr, *vf_rec = nullptr;
  // tgx_verify_tree: the device tables of the pass's token tree, VT_* ints each slot of 16 (depth, parent position, the accepted path; the ancestor masks as 16-bit
  // words in the fourth).  Allocated by the first non-chain tree call
  enum { VT_DEPTH = 0, VT_PAR = 16, VT_PATH = 32, VT_ANC = 48, VT_INTS = 64 };
  int* vt_tab = nullptr;
  int vf_pass_rows = 0;      // the positions of the verify pass whose logits vf_logits holds (tgx_read_pass_logits); 0: none, or another call has used the workspace since
  // ... and tgx_verify_row_sampled on a sampled row: the staged sampler's scratch and compacted lists for the VERIFY_ROWS positions (the pass's, not the row's) and
  // their draws.  Allocated by the first such call (vs_alloc): a context that never makes one holds none of it
  tgx::SampScratch* vs_scratch = nullptr;
  unsigned long long* vs_list_comp = nullptr;    // [VERIFY_ROWS][vocab]
  float* vs_list_v = nullptr;
  int* vs_draws = nullptr;                       // [VERIFY_ROWS]
  // ---- tgx_verify_rows (include/tgx.h): the joint pass over M <= VERIFY_POSITIONS positions of several rows — the hidden rows, logits and argmax partials of every
  // position, one record per named row, the sampled rows' draws, and the accept launch's per-row argument table.  Sized by the first call (ensure_verify_rows_ws):
  // a context that never makes it holds none of it.  Option verify.last_form (read-only): 0 no call yet, 1 the joint pass, 2 row by row
  enum { VERIFY_POSITIONS = TGX_MAX_VERIFY_POSITIONS };
  float *vj_x = nullptr, *vj_logits = nullptr, *vj_part_val = nullptr; int *vj_part_idx = nullptr, *vj_rec = nullptr, *vj_draws = nullptr;
  unsigned char* vj_args = nullptr;              // [max_batch] tgx::VerifyArgs
  std::vector<unsigned char> vj_args_host;       // ... and the host copy the upload reads
  bool vf_pass_joint = false;                    // vf_pass_rows counts positions of vj_logits (a tgx_verify_rows joint pass), not of vf_logits
  // ---- option verify.processors (include/tgx.h; kernels/logit_proc.h logit_proc_pos_kernel): 1 lets the chain verify calls take rows with a logit processor on.
  // The processed slab of the pass's positions with its per-tile partials and the positions' automaton states — VERIFY_ROWS slots for the one-row calls (vp_*),
  // VERIFY_POSITIONS for the joint ones (vpj_*) — each allocated by the first call that verifies a processed row (ensure_verify_proc_ws)
  int verify_processors = 0;
  float *vp_logits = nullptr, *vp_part_val = nullptr; int *vp_part_idx = nullptr, *vp_states = nullptr;
  float *vpj_logits = nullptr, *vpj_part_val = nullptr; int *vpj_part_idx = nullptr, *vpj_states = nullptr;
  int verify_last_form = 0, verify_last_splits = 0;      // ... and `verify.last_splits` (read-only): the key splits of the last joint pass's attention (0: unsplit)
  // ---- tgx_advance_rows (include/tgx.h): prompt chunks and live rows' steps in one ragged pass.  Option advance.attn_tiles: the tile target of the mixed attention
  // (kernels/attn_mixed.h; csrc/attn_worklist.h): 0 never split (the work-list form alone), N >= 1 query blocks of more than N key tiles are cut into ranges of <= N
  // tiles (<= 32 ranges), -1 automatic: the largest target that gives the attention's launches two workgroups per CU (attn_worklist.h auto_target) — the rule
  // profiles/verify_rows.txt measured for attn_extend_rg_kernel.  Default 16, by the sweep of profiles/advance_rows.txt (tools/admit_bench.py --mixed; Llama-3.2-1B
  // bf16, head_dim 64, ms per call, 0 / 4 / 8 / 16 / -1; spread of a figure ~0.1): 32 step rows at context 2048 + a chunk of 256: 6.49 / 6.43 / 6.26 / 6.10 / 6.47
  // (-1 chose 0: the whole blocks alone are four workgroups per CU); 8 step rows at 300 + a chunk of 512 at past 512: 4.48 / 4.58 / 4.66 / 4.48 / 4.66 (-1 chose 9).
  // 16 wins or ties at both; the two-per-CU rule does not carry over to this kernel.  UNMEASURED: head_dim 128, contexts beyond 2048, targets above 16.
  // Read-only: advance.last_form (0 no call yet, 1 the joint pass, 2 piecewise), advance.last_tiles (the target the last joint pass ran with).
  // mix_part: the ranges' partials, grown by the first joint pass that splits
  int advance_attn_tiles = 16, advance_last_form = 0, advance_last_tiles = 0;
  float* mix_part = nullptr; size_t mix_part_bytes = 0;
  // ---- per-token log-probabilities (include/tgx.h tgx_set_row_logprobs; kernels/logprobs.h).  Allocated by the first call that switches a row on: the rows' record
  // rings and counters, and the tile launch's partials for max(max_batch, VERIFY_ROWS) rows (a verify pass puts its positions where a step puts its rows)
  tgx::LpRecord* lp_ring = nullptr;          // [max_batch][TGX_LOGPROB_RING]
  tgx::LpRow* lp_rows = nullptr;             // [max_batch]
  float* lp_tile_max = nullptr;              // [rows][tiles]
  double* lp_tile_sum = nullptr;             // [rows][tiles]
  unsigned long long* lp_tile_keys = nullptr;   // [rows][tiles][TGX_MAX_LOGPROBS]
  // ---- tgx_score_row (include/tgx.h; kernels/score.h).  Allocated by the first call that scores (a context that never does holds none of it).
  // Options score.rows / score.vocab_chunk: the positions per group and the vocabulary columns per product of the matrix-core form (multiples of 64 / of the
  // 1024-entry tile).  Measured (profiles/score_row.txt, Llama-3.2-1B seq 2048 top_n 20, ms per call, rows x chunk): 512 x 16384 17.05, 1024 x 8192 16.83,
  // 1024 x 16384 16.68, 1024 x 32768 16.33, 2048 x 8192 16.47, 2048 x 16384 16.21, 2048 x 32768 16.25 (spread of a figure ~0.3) -> 2048 x 16384: a 128 MiB product
  // beside a 64 MiB weight slice at hidden 2048 (whether the tile launch then reads the product from the Infinity Cache was not measured: no counter run).
  // score.last_form (read-only): the last call that scored a position: 0 none yet, 1 matrix cores, 2 by groups of VERIFY_ROWS
  int score_rows = 2048, score_vocab_chunk = 16384, score_last_form = 0;
  float* sc_logits = nullptr; size_t sc_logits_bytes = 0;            // [group rows][chunk] the product of one vocabulary chunk
  unsigned char* sc_part = nullptr; size_t sc_part_bytes = 0;        // one group's tile sums | keys | maxima | target values, laid out for sc_part_rows rows
  int sc_part_rows = 0;
  unsigned char* sc_out = nullptr; size_t sc_out_bytes = 0;          // the call's lp [n] | top ids [n][TGX_MAX_LOGPROBS] | top lps: one read-back
  // ---- tgx_embed_rows (include/tgx.h; kernels/embed_pool.h).  Allocated by the first call (a context that never embeds holds none of it), grown to the largest call:
  // em_buf = the call's text table | out [n][dims] | partials [slices][H] (one row per EMB_SLICE pooled positions: never [M][H]); em_stage = the [EMB_SLICE][H] staging
  // slice of prefill by steps.  embed.last_pool_launches (read-only option): pooling launches of the last call (partials + finish)
  unsigned char* em_buf = nullptr; size_t em_bytes = 0;
  float* em_stage = nullptr; size_t em_stage_bytes = 0;
  size_t em_off_out = 0, em_off_part = 0;             // byte offsets of the last call's sections in em_buf
  int embed_last_launches = 0;
  // ---- per-row logit processors (include/tgx.h tgx_set_row_penalties / tgx_set_row_logit_bias / tgx_set_row_history; kernels/logit_proc.h).  Allocated by the first
  // non-neutral setting or non-empty history (proc_alloc): a context that never asks holds none of it and runs the launches it ran before
  unsigned int* proc_hist = nullptr;         // [max_batch][vocab] history words: bit 31 "in the prompt", bits 0 .. 30 times produced
  int* proc_bias_ids = nullptr;              // [max_batch][TGX_MAX_LOGIT_BIAS]
  float* proc_bias_val = nullptr;
  float* proc_logits = nullptr;              // [max_batch][vocab] the processed logits of the rows' last processed step
  float* proc_part_val = nullptr;            // [max_batch][ceil(vocab / 1024)] their per-tile (max, lowest index)
  int* proc_part_idx = nullptr;
  // ---- token automata (include/tgx.h tgx_automaton_create; automaton.h holds the checks): the live tables, each [n_states][vocab] 16-bit words from c->mem.  A row
  // names one by RowHost::auto_id; its table pointer and state word live in its RowReq.  A context that never creates one holds none of it
  struct AutoTable { unsigned short* next = nullptr; int n_states = 0, start = 0; };
  AutoTable automata[TGX_MAX_AUTOMATA];
  // ---- row snapshots (include/tgx.h tgx_save_row / tgx_restore_row; row_snapshot.h, kernels/kv_pack.h): the staging buffer a snapshot moves through in groups of
  // whole layers (the state section in front of the first group's).  Allocated by the first save or restore, grown to the largest group seen; option
  // snapshot.stage_kib caps it (one layer is always staged).  tgx_splice_row (kernels/kv_splice.h) moves its groups of layers through the same buffer, the row's
  // new block table in front of them
  unsigned char* snap_stage = nullptr; size_t snap_stage_bytes = 0;
  int snapshot_stage_kib = 65536;
  // ---- beam search (include/tgx.h tgx_beam_select; kernels/beam.h): the tile maxima, sums and keys of TGX_MAX_BEAMS rows, the rows' lse and first keys, and the
  // call's record, in ONE buffer sized by the first tgx_beam_select: a context that never selects holds none of it (tgx_beam_advance needs no workspace)
  unsigned char* beam_ws = nullptr;
  float* scratch_x = nullptr;   // [hidden] residual sink for tgx_profile_decode
  Profiler prof;
};

// ---- errors: every launcher returns void / a count; a kernel it could not issue is recorded in launch_fault and turned into a status by the entry point
int set_err(tgx_ctx* c, int code, const char* fmt, ...);

#define HIP_OK(c, call)                                                                          \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      return set_err((c), TGX_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

#define LAUNCH_OK(c)                                                                             \
  do {                                                                                           \
    if ((c)->launch_fault) { const char* f_ = (c)->launch_fault; (c)->launch_fault = nullptr; return set_err((c), TGX_ERR_UNSUPPORTED, "%s", f_); } \
  } while (0)

// Runs `body` with DT bound to the context's storage dtype as a compile-time constant (kernel template argument).
#define TGX_DT_SWITCH(dt_, ...)                                                          \
  switch (dt_) {                                                                         \
    case tgx::DT_BF16: { constexpr int DT = tgx::DT_BF16; __VA_ARGS__; } break;          \
    case tgx::DT_F16: { constexpr int DT = tgx::DT_F16; __VA_ARGS__; } break;            \
    default: { constexpr int DT = tgx::DT_F32; __VA_ARGS__; } break;                     \
  }

// The MFMA prefill kernels exist for the two 16-bit storage dtypes.
#define TGX_DT16_SWITCH(dt_, ...)                                                        \
  if ((dt_) == tgx::DT_F16) { constexpr int DT = tgx::DT_F16; __VA_ARGS__; }             \
  else { constexpr int DT = tgx::DT_BF16; __VA_ARGS__; }

// ---- device memory: every buffer of the context comes from c->mem (dev_mem.h) and is freed by tgx_destroy at the latest.  dev_grow: *p, of *bytes bytes, holds `need`
// bytes after it — a growth loses the contents and first waits for the stream (launches in flight may read the old buffer; dropping captured graphs that point
// into it is the caller's business); on failure *p == nullptr and *bytes == 0
template <typename T>
int dev_alloc(tgx_ctx* c, T** p, size_t n) {
  *p = static_cast<T*>(c->mem.alloc(n * sizeof(T)));
  return *p ? TGX_OK : set_err(c, TGX_ERR_DEVICE, "dev_alloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(hipPeekAtLastError()));
}
template <typename T> void dev_free(tgx_ctx* c, T** p) { c->mem.release(*p); *p = nullptr; }
template <typename T>
int dev_grow(tgx_ctx* c, T** p, size_t* bytes, size_t need) {
  if (need <= *bytes) return TGX_OK;
  HIP_OK(c, hipStreamSynchronize(c->stream));
  void* q = *p; const bool ok = c->mem.grow(&q, bytes, need); *p = static_cast<T*>(q);
  return ok ? TGX_OK : set_err(c, TGX_ERR_DEVICE, "dev_grow to %zu bytes failed: %s", need, hipGetErrorString(hipPeekAtLastError()));
}

namespace tgx { struct AttnArgs; struct FinalizeArgs; struct AttnPrefillArgs; struct RopeKvArgs; }
// the device tables of a token tree's pass (tgx_verify_tree; csrc/verify_tree_plan.h): per pass position its depth and its ancestor-or-self mask
struct TreePass { const int* depth; const unsigned short* anc; };

// ---- abi.hip
void drop_step_graphs(tgx_ctx* c);
int kv_ensure_blocks(tgx_ctx* c, int row, long long tokens);       // paged KV: row `row` may hold `tokens` tokens after this (assigns blocks, updates the device table, stream-ordered)
bool is_greedy(const tgx_sampler_cfg* s);   // Sampler.cpp:15-21
bool row_records(const tgx_ctx* c, int row);   // the row records log-probabilities in the steps (tgx_set_row_logprobs; not while it is retired)
// ---- decode.hip (kernels/gemv.h, kernels/oproj_sliced.h)
int gemv_grid(const tgx_ctx* c, int units, int ks, int bpc);
int quantize_weights(tgx_ctx* c); // tgx_finalize, ahead of pack_weights: option weights.fp8 (dequantized masters in place, the 8-bit streams and row scales)
int pack_weights(tgx_ctx* c);     // tgx_finalize: the exponent-packed copies of the bf16 gate_up / down / lm_head matrices (option weights.packed)
bool oproj_sliced_ok(const tgx_ctx* c, int R, long long kv_stride);
bool oproj_fused_capable(const tgx_ctx* c);                               // static conditions (geometry, dtype, option)
bool oproj_fused_ok(const tgx_ctx* c, int R, long long kv_stride);       // ... and this launch is a batch-1 step on the direct form
int launch_layer_kernel(tgx_ctx* c, RowState* rv, int R, int l, int cls, float* resid, long long kv_stride);   // returns the number of launches issued
void launch_layers(tgx_ctx* c, RowState* rv, int R, long long kv_stride);
void launch_layers(tgx_ctx* c, int row0, int R);
void launch_lm_head(tgx_ctx* c, int row0, int R);
void launch_lm_head_at(tgx_ctx* c, const float* x, float* logits, float* part_val, int* part_idx, int R);   // R rows at row strides from these pointers
tgx::FinalizeArgs make_finalize_args(tgx_ctx* c, int row, bool advance_pos, bool log_step);
void launch_finalize_greedy(tgx_ctx* c, int row0, int R, bool advance_pos, bool log_step);   // one finalize_greedy launch per row
void launch_finalize_rows(tgx_ctx* c, int row0, int M);                                     // the batched step's greedy finalize (+ step counter)
void launch_embed_chunk(tgx_ctx* c, const long long* ids, int R, int pos0);
void launch_add_pos(tgx_ctx* c, int* pos, int n);
void launch_argmax_partials(tgx_ctx* c, const float* logits, int V, float* part_val, int* part_idx);
void launch_verify_first_id(tgx_ctx* c, int row);         // tgx_verify_row: prompt[0] of the row <- its current token
void launch_verify_accept(tgx_ctx* c, int row, int M, const int* draws = nullptr, bool processed = false);    // (processed: g[i] from the vp_* partials, the history and state committed) ... and the accept launch over the M positions in the vf_* workspace (kernels/verify.h); draws: the positions' sampled ids
// tgx_verify_rows, the joint pass: sequence i = row rows[i], M_i = n_draft[i] + 1 positions at slice first[i] of the vj_* workspace and of the pass's ids
void launch_verify_first_ids(tgx_ctx* c, long long* ids, int n, const int* rows, const int* first);          // ids[first[i]] <- row rows[i]'s current token, one launch
void launch_verify_accept_rows(tgx_ctx* c, const long long* ids, int n, const int* rows, const int* first, const int* n_draft, const char* sampled, const char* processed = nullptr);   // one workgroup per row -> vj_rec[i]; processed[i]: row i chooses from the vpj_* slab and commits its history and state
// tgx_verify_tree: the walk over a token tree (draws as above; vt_tab holds the tree's tables) -> vf_rec and the accepted path; then the accepted branch's K / V rows
// of every layer from slot past + path[j] to slot past + j (kernels/kv_tree.h), stream-ordered behind the walk: path and count are read on the device
void launch_verify_accept_tree(tgx_ctx* c, int row, int M, const int* draws);
void launch_kv_tree_compact(tgx_ctx* c, int row, int M, int past);
size_t verify_args_bytes();                                // one entry of the accept launch's table (vj_args)
// ---- attn.hip (kernels/attn_decode.h, attn_decode_mfma.h)
bool attn_batch_on_mfma(const tgx_ctx* c, int R);
void launch_attn(tgx_ctx* c, const tgx::AttnArgs& a, int R, bool combine = true);   // combine = false: the caller's o_proj merges the split records
int attn_set_attrs(tgx_ctx* c);
// ---- sampler.hip (kernels/sampler.h)
void launch_sample(tgx_ctx* c, int row0, int R, const tgx_sampler_cfg& cfg, bool advance_pos, bool log_step, bool processed = false);   // processed: from the processed logits (launch_logit_proc ran for these rows)
enum { ROWU_GREEDY = 1, ROWU_K = 2, ROWU_P = 4, ROWU_M = 8, ROWU_SUM = 16, ROWU_LP = 32, ROWU_PROC = 64, ROWU_AUTO = 128 };   // stages of a per-row step: greedy finalize, top-k, top-p, min-p, partial sums + pick; some row records log-probabilities; some row has a logit processor on; ... an automaton among them (its state advances ahead of the processor launch)
void launch_sample_rows(tgx_ctx* c, int row0, int R, int un);              // tgx_decode_rows: every row with its own settings (a decode step's sampler)
int row_union_of(const tgx_ctx* c);
void launch_probs(tgx_ctx* c, int row, const tgx_sampler_cfg& cfg, bool processed = false);
int vs_alloc(tgx_ctx* c);                                                    // tgx_verify_row_sampled: the positions' sampler workspace, at first use
int vs_rezero(tgx_ctx* c);                                                   // ... its scratch back to the zero state the chain expects (tgx_reset_cache; stream-ordered; a no-op without the workspace)
void launch_sample_positions(tgx_ctx* c, int row, int M, const tgx_sampler_cfg& cfg, int joint_first = -1, const int* depth = nullptr, bool processed = false);   // the uniform chain of the row's cfg over the M positions in the vf_* workspace -> vs_draws (nothing of the row changes); joint_first >= 0: over the row's slice of the vj_* workspace -> its slice of vj_draws
int proc_alloc(tgx_ctx* c);                                                  // the logit processors' buffers, at first use
bool row_processed(const tgx_ctx* c, int row);                               // the row has a logit processor on (not while it is retired)
int ensure_verify_proc_ws(tgx_ctx* c, bool joint);                          // the vp_* (one-row calls) or vpj_* (joint calls) workspace, at first use
// the processors over a verify pass's positions (option verify.processors): the automaton walk, then the positions launch, for the n STEP rows with processed[j]
// set — row rows[j]'s lens[j] positions from workspace row first[j], its inputs at ids[j] on the device; joint: the vj_* / vpj_* workspace, else vf_* / vp_*
void launch_logit_proc_positions(tgx_ctx* c, int n, const int* rows, const int* first, const int* lens, const long long* const* ids, const char* processed, bool joint);
void launch_logit_proc(tgx_ctx* c, int row0, int R, bool step);            // raw logits of rows [row0, row0 + R) -> the processed slab and partials (step: count the current tokens)
// beam search (kernels/beam.h): the three launches of tgx_beam_select over rows[0 .. n) and the read-back of its record (the caller checked every argument); the
// publish launch of tgx_beam_advance: row rows[j] takes tokens[j] as its current token and the next embedding at its position
int beam_select_run(tgx_ctx* c, int n, const int32_t* rows, const float* scores, int k, const int32_t* end_ids, int n_end, tgx_beam_cand* out, int32_t* out_n);
void launch_beam_publish(tgx_ctx* c, int n, const int* rows, const int32_t* tokens);
int sampler_alloc(tgx_ctx* c);
int logprobs_alloc(tgx_ctx* c);                                              // the rings, counters and tile partials, at first use
void launch_logprobs(tgx_ctx* c, int row0, int R, bool force);             // behind a step's publish: the rows that record and produced a token (force: tgx_sample_row)
void launch_logprobs_verify(tgx_ctx* c, int row, int M, int joint_first = -1, int joint_i = 0);   // behind tgx_verify_row's accept launch: one record per produced token (joint_first >= 0: the row's slice of the vj_* workspace, its record vj_rec[joint_i])
// ---- prefill.hip (kernels/prefill.h, gemm_dma.h)
bool prefill_shapes_ok(const tgx_model_desc& d);
int ensure_prefill_ws(tgx_ctx* c, int S);
int ensure_ws_part(tgx_ctx* c, size_t need);      // ws_part holds `need` bytes after this (a growth drops the step graphs: a captured batched step points into the old slabs)
void launch_prefill(tgx_ctx* c, int row0, int NB, int S, int past);      // past: the rows' common pastLength (their positions are past .. past + S - 1) — explicit, not read from the context
void launch_prefill_ragged(tgx_ctx* c, const RaggedPass& rg);           // the same pass over the sequences of rg (each from its rg.past, default 0)
// the device tables of p (RgSeq [n], token -> prompt map [M], attention work list [n_items]; each 16-byte aligned) as one block: sets p.n_items and returns the block's
// size; with `host` (16-byte aligned) it also fills the block there and points p.seq / tok_seq / items into its copy at `dev`
size_t ragged_tables(const tgx_ctx* c, RaggedPass& p, unsigned char* host, const unsigned char* dev);
// tgx_advance_rows: the same block with the attention lists of csrc/attn_worklist.h at tile target `target` (>= 0) behind it — the whole blocks as p.items, the
// ranges and merge items as p.mix_split / p.mix_merge (at target 0 exactly ragged_tables' block); advance_attn_target: option advance.attn_tiles resolved for p
// (raised while the partials would exceed 512 MiB); ensure_mix_ws: the partials' workspace for p.mix_slots records, before the pass is issued
size_t advance_tables(const tgx_ctx* c, RaggedPass& p, unsigned char* host, const unsigned char* dev, int target);
int advance_attn_target(const tgx_ctx* c, const RaggedPass& p);
int ensure_mix_ws(tgx_ctx* c, const RaggedPass& p);
void launch_embed_ragged(tgx_ctx* c, const RaggedPass& rg);
void launch_rope_kv_split_ragged(tgx_ctx* c, const tgx::RopeKvArgs& a, const RaggedPass& rg, long long layer_off);
void launch_attn_prefill_ragged(tgx_ctx* c, const tgx::AttnPrefillArgs& a, const RaggedPass& rg, long long layer_off, bool allow_lean);
int prefill_set_attrs(tgx_ctx* c);
int ensure_score_ws(tgx_ctx* c, int seq, bool tiled);          // tgx_score_row: the workspace of a pass of seq positions (tiled: the matrix-core form's product buffer as well)
void launch_score_tiles(tgx_ctx* c, const ScoreCall& sc, const float* logits, long long stride, int col0, int width, int R, int pos0);   // the tile launch over [R][width] logits = entries [col0, col0 + width) of positions pos0 ..
void launch_score_record(tgx_ctx* c, const ScoreCall& sc, int R, int pos0);                                                           // ... the group's records, behind the tile launches of the whole vocabulary
void launch_score_tiled(tgx_ctx* c, const ScoreCall& sc);      // the matrix-core form over ws_x behind launch_prefill
// tgx_embed_rows (kernels/embed_pool.h): the call's workspace before anything changes; the table upload ahead of the passes; the partials of texts [t0, t0 + nt) of
// a pass over ws_x (ONE launch); one slice of text t from the staging slice (prefill by steps); the finish launch over all texts and the read-back, behind the passes
int ensure_embed_ws(tgx_ctx* c, EmbedCall& em);
int embed_upload_table(tgx_ctx* c, const EmbedCall& em);
void launch_embed_pool(tgx_ctx* c, const EmbedCall& em, int t0, int nt);
void launch_embed_pool_stage(tgx_ctx* c, const EmbedCall& em, int t, int slice, int cnt);
int launch_embed_finish(tgx_ctx* c, const EmbedCall& em);
int extend_attn_splits(const tgx_ctx* c, int S, int past);   // key splits of a continuation pass's attention (0: the per-row prompt attention)
int ensure_extend_ws(tgx_ctx* c, int S, int past);           // ... and their partials' workspace, before the pass is issued
// tgx_verify_rows: the key splits of a ragged continuation pass (p.n sequences, p.past set) by option extend.attn_splits -> p.ext_ns, and the partials' workspace
int ensure_extend_rg_ws(tgx_ctx* c, RaggedPass& p);
void launch_attn_prefill(tgx_ctx* c, const tgx::AttnPrefillArgs& a, bool allow_lean, const unsigned short* anc = nullptr);   // anc: a token tree's device masks (TreePass)
void launch_rope_kv_split(tgx_ctx* c, const tgx::RopeKvArgs& a, int S, const int* depth = nullptr);                           // depth: a token tree's device depths (TreePass)
void launch_norm_terms(tgx_ctx* c, float* x, const ebyte* norm_w, int M, int H, int nsplit, bool third = false);
void launch_embed_rows(tgx_ctx* c, const long long* ids, float* X, int M, int S);
// ---- prefill_f32.hip (kernels/gemm_f32.h)
int ensure_f32_part(tgx_ctx* c, int rows);
void launch_prefill_f32(tgx_ctx* c, int row0, int NB, int S, int past);   // past: as launch_prefill
// ---- skinny.hip (kernels/skinny.h, skinny_ksplit.h, skinny_dma.h)
bool decode_mfma_ok(const tgx_ctx* c);
int ensure_skinny_ws(tgx_ctx* c, int rows);
void launch_decode_step_mfma(tgx_ctx* c, int row0, int M, const tgx_sampler_cfg& cfg);
void launch_prefill_skinny(tgx_ctx* c, int row0, int NB, int S, int past, const RaggedPass* rg = nullptr, const TreePass* tree = nullptr);   // past: as launch_prefill; rg: a ragged pass of rg->M rows (from position 0) instead of rows [row0, row0 + NB); tree (NB == 1, no rg): the S positions are a token tree's
void launch_lm_head_skinny(tgx_ctx* c, int M, float* logits, float* part_val, int* part_idx, float* x = nullptr);   // model.norm -> lm_head of ALL M rows of ws_x behind launch_prefill_skinny as ONE pass over the weights (the batched step's form) + their argmax partials (stride lm_grid)
int skinny_set_attrs(tgx_ctx* c);
