/*
 * tgx_oracle.c — CPU restatement of TinyGPT's decode path.  TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library;
 * the product (tinygpt_amd/) never links, imports or falls back to it.
 *
 * What it restates (structure and order of operations; reference = /root/reference):
 *   CausalLM::forward            src/model/GPTModel.h:51-58
 *   DecoderLayer::forward        src/layer/DecoderLayer.h:38-43
 *   Attention::forward           src/layer/Attention.h:71-112   (qkv -> split BSHD -> RoPE@pastLength
 *                                                               -> cache append -> attention -> o_proj)
 *   MergedLinear row order       src/layer/Linear.h:64-79       (q,k,v / gate,up)
 *   GatedMLP::forward, SiLUMul   src/layer/GatedMLP.h:37-41, src/layer/Activation.h:14-17
 *   KVCacheManager               src/engine/CacheManager.h:24-51
 *   Sampler::sample              src/engine/Sampler.cpp:15-79
 *   family flags                 src/model/ModelLlama.h:21-53, ModelQwen2.h:26-34, ModelMistral.h:25-29
 *   GPT-2 stack                  src/model/ModelGPT2.h:23-208
 *   engine loop                  src/engine/GPTEngine.cpp:94-99,154-174
 *
 * The arithmetic itself lives in the reference's un-vendored submodule keith2018/TinyTorch
 * (.gitmodules:1-3; pinned SHA unrecoverable, directory empty), so it cannot be compiled here.
 * Per-op numerics therefore follow HF `transformers` (the source of the checkpoints the reference
 * loads by name) and are PINNED by tests/golden/ — vectors generated in the build container from
 * transformers 5.15 / torch 2.10 CPU by tools/gen_fixtures.py.  The reference itself holds no test
 * for this path, so relative to TinyTorch's own kernels parity is unpinned; relative to
 * HF it is pinned.
 *
 * Numerics contract.  compute_dtype bf16 means: parameters and the KV cache are STORED in
 * bf16 (round-to-nearest-even once, at upload / at cache append); every activation between ops and all
 * arithmetic is fp32.  compute_dtype fp16 is the same with IEEE half storage; fp32 stores everything in fp32.
 *   Linear      y = sum_k x_k w_k [+ b]                 fp32 accumulate over exact bf16->fp32 weights
 *   RMSNorm     y = w * (x * (1/sqrt(mean(x^2)+eps)))   (HF LlamaRMSNorm order)
 *   RoPE        fp32 cos/sin tables; y = x*cos + rot_half(x)*sin   (HF apply_rotary_pos_emb)
 *   KV cache    K (after RoPE) and V rounded to bf16 when appended (bf16 mode)
 *   attention   fp32 scores (q.k)*hd^-1/2, fp32 softmax, fp32 P.V
 *   MLP         h = silu(g) * u;  residual x = x + y;  logits fp32
 * Why activations are not rounded to bf16 like a torch-bf16 module would: two bf16-rounding implementations
 * with different fp32 summation order agree either bit-for-bit or only to the bf16 noise floor (a 1-ulp flip
 * re-amplifies at every later rounding; measured 3-6e-3 on logits), so north_star's "1e-3 relative" is only
 * a meaningful bar for an fp32 activation path.  TGXO_TORCH_ROUNDING=1 restores per-op rounding for study.
 *
 * Test hooks beyond the ABI (oracle_ffi.ORACLE_EXTRA): set_reorder, set_act16, set_torch_rounding, set_one_row_dots, set_logits, set_next_token, and for
 * the key-range tests tgxo_write_kv (cache rows from the host, rounded once to the storage dtype), tgxo_set_past (a written cache holds n positions, no
 * prefill) and tgxo_set_ablate_key (attend() loses one key position: the yardstick of tests/test_oracle_plant.py's sensitivity sweep).
 */
#define _GNU_SOURCE
#include <math.h>
#include <omp.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define TGXO_EXPORT __attribute__((visibility("default")))

enum { F_GPT2 = 1, F_LLAMA = 2, F_QWEN2 = 3, F_QWEN3 = 4, F_MISTRAL = 5 };
enum { DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2 };

typedef struct {
  int32_t family, hidden, layers, heads, kv_heads, head_dim, inter, vocab, max_ctx, qkv_bias, tied, compute_dtype;
  float norm_eps, rope_theta, rope_factor, rope_low_freq, rope_high_freq;
  int32_t rope_orig_ctx, n_positions, max_batch, qk_norm;
} desc_t;

typedef struct { float temperature; int64_t top_k; float top_p; float min_p; } sampler_cfg_t;

/* A parameter matrix [rows][cols] held either as bf16 bits or fp32, plus an optional fp32 bias. */
typedef struct {
  int64_t rows, cols;
  uint16_t* wb;
  float* wf;
  float* bias;
  int64_t filled_rows; /* upload bookkeeping */
  int bias_filled;
  int transposed_src;  /* GPT-2 Conv1D stores [in][out]; we transpose on upload */
} mat_t;

typedef struct { float* w; float* b; int filled_w, filled_b; } vec_t;

typedef struct {
  vec_t in_norm, post_norm;      /* input_layernorm / post_attention_layernorm, or ln_1 / ln_2 (with bias) */
  vec_t q_norm, k_norm;          /* Qwen3 per-head RMSNorm weights [head_dim] (Attention.h:128-167) */
  mat_t qkv, o, gate_up, down;   /* GPT-2: c_attn, c_proj, c_fc, mlp.c_proj */
} layer_t;

typedef struct tgxo_ctx {
  desc_t d;
  int bf16;
  int f16;                       /* compute_dtype fp16: parameters and KV cache hold half-rounded values */
  int round_act;
  int act16;                     /* tgxo_set_act16: the input of every Linear is rounded to the storage dtype first (the reference's bf16 modules see bf16 tensors, ModelLlama.h:62) */
  int reorder;                   /* tgxo_set_reorder: every reduction runs in the REVERSE element order (a second, equally valid fp32 schedule) */
  int ablate_key;                /* tgxo_set_ablate_key: attend() gives this key position the score -inf (-1 = off) */
  mat_t embed, wpe, lm_head;
  vec_t final_norm;
  layer_t* L;
  float *rope_cos, *rope_sin;    /* [max_ctx][head_dim/2], already R()-rounded */
  float* kcache;                 /* [max_batch][layers][max_ctx][kv_dim] */
  float* vcache;
  int64_t past;
  int finalized;
  int last_batch;
  float* logits;                 /* [max_batch][vocab] fp32 accumulators */
  int64_t* next_tok;             /* [max_batch] */
  char err[256];
} tgxo_ctx;

static char g_err[256];

/* ---------------------------------------------------------------- rounding helpers */
static inline float bf16_to_f32(uint16_t b) {
  uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f;
}
static inline uint16_t f32_to_bf16(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float rbf(float f) { return bf16_to_f32(f32_to_bf16(f)); }
#define R(c, x) ((c)->round_act ? rbf(x) : (x))       /* activations: identity unless TGXO_TORCH_ROUNDING */
#define RKV(c, x) ((c)->bf16 ? rbf(x) : ((c)->f16 ? rhf(x) : (x)))   /* storage rounding: KV cache, norm weights, biases */

static float half_to_f32(uint16_t h) {
  uint32_t s = (h >> 15) & 1, e = (h >> 10) & 0x1f, m = h & 0x3ff, u;
  if (e == 0) {
    if (m == 0) u = s << 31;
    else { e = 127 - 15 + 1; while (!(m & 0x400)) { m <<= 1; e--; } m &= 0x3ff; u = (s << 31) | (e << 23) | (m << 13); }
  } else if (e == 31) u = (s << 31) | 0x7f800000u | (m << 13);
  else u = (s << 31) | ((e + 127 - 15) << 23) | (m << 13);
  float f; memcpy(&f, &u, 4); return f;
}

/* fp32 -> IEEE half, round-to-nearest-even, subnormals kept (== torch .to(float16), v_cvt_f16_f32) */
static uint16_t f32_to_half(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
  if (a >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);
  if (a < 0x33000000u) return (uint16_t)sign;
  const int e = (int)(a >> 23) - 127;
  const uint32_t m = (a & 0x7fffffu) | 0x800000u;
  const int shift = e >= -14 ? 13 : 13 + (-14 - e);
  uint32_t q = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
  if (rem > halfway || (rem == halfway && (q & 1u))) q++;
  uint32_t h = e >= -14 ? ((uint32_t)(e + 15) << 10) + (q - 0x400u) : q;
  if (h >= 0x7c00u) h = 0x7c00u;
  return (uint16_t)(sign | h);
}
static inline float rhf(float f) { return half_to_f32(f32_to_half(f)); }

/* ---------------------------------------------------------------- allocation */
static int mat_alloc(tgxo_ctx* c, mat_t* m, int64_t rows, int64_t cols, int bias) {
  memset(m, 0, sizeof(*m));
  m->rows = rows; m->cols = cols;
  if (c->bf16) m->wb = (uint16_t*)calloc((size_t)(rows * cols), 2);
  else m->wf = (float*)calloc((size_t)(rows * cols), 4);
  if (bias) m->bias = (float*)calloc((size_t)rows, 4);
  return (m->wb || m->wf) && (!bias || m->bias);
}
static void mat_free(mat_t* m) { free(m->wb); free(m->wf); free(m->bias); memset(m, 0, sizeof(*m)); }
static int vec_alloc(vec_t* v, int64_t n, int bias) {
  memset(v, 0, sizeof(*v));
  v->w = (float*)calloc((size_t)n, 4);
  if (bias) v->b = (float*)calloc((size_t)n, 4);
  return v->w && (!bias || v->b);
}

static inline float src_elem(const void* host, int dt, int64_t i) {
  if (dt == DT_F32) return ((const float*)host)[i];
  if (dt == DT_BF16) return bf16_to_f32(((const uint16_t*)host)[i]);
  return half_to_f32(((const uint16_t*)host)[i]);
}

/* == model().to(dtype): store in compute dtype (bf16->fp32 exact, fp32->bf16 RNE).
 * The rows are written by the thread that will read them: the loop below is linear()'s own (blocks of 8 rows of the WHOLE matrix, schedule(static), the
 * same trip count), so with a fixed team size and pinned threads (OMP_PROC_BIND) every page of a weight matrix is first touched - and therefore placed -
 * on the NUMA node of the core that streams it in every later product.  (calloc of these sizes returns untouched mmap pages.)  A serial memcpy had put
 * a whole model on the uploading thread's node: bench.py's cpu_baseline read 2.5 GB per token through one socket's quadrant. */
static void mat_store_rows(tgxo_ctx* c, mat_t* m, int64_t row0, int64_t nrows, const void* host, int dt, int src_is_in_out) {
  const int64_t N = m->rows, K = m->cols;
  const int plain = c->bf16 && dt == DT_BF16 && !src_is_in_out;   /* same storage dtype: plain copy */
#pragma omp parallel for schedule(static)
  for (int64_t nb = 0; nb < N; nb += 8) {
    int64_t lo = nb > row0 ? nb : row0, hi = (nb + 8 < N ? nb + 8 : N);
    if (hi > row0 + nrows) hi = row0 + nrows;
    for (int64_t rr = lo; rr < hi; rr++) {
      const int64_t r = rr - row0;
      if (plain) { memcpy(m->wb + rr * K, (const uint16_t*)host + r * K, (size_t)K * 2); continue; }
      for (int64_t k = 0; k < K; k++) {
        float v = src_is_in_out ? src_elem(host, dt, k * nrows + r) : src_elem(host, dt, r * K + k);
        if (c->bf16) m->wb[rr * K + k] = f32_to_bf16(v);
        else m->wf[rr * K + k] = c->f16 ? rhf(v) : v;   /* fp16 mode: fp32 container, half-rounded values */
      }
    }
  }
  m->filled_rows += nrows;
}
static void vec_store(tgxo_ctx* c, float* dst, int64_t n, const void* host, int dt) {
  for (int64_t i = 0; i < n; i++) dst[i] = RKV(c, src_elem(host, dt, i));   /* parameters are stored in compute dtype */
}

/* ---------------------------------------------------------------- API: lifetime */
TGXO_EXPORT const char* tgxo_last_error(const tgxo_ctx* c) { return c ? c->err : g_err; }

static int fail(tgxo_ctx* c, int code, const char* fmt, const char* a) {
  snprintf(c ? c->err : g_err, 256, fmt, a);
  return code;
}

TGXO_EXPORT int tgxo_create(const desc_t* d, int device_ordinal, tgxo_ctx** out) {
  (void)device_ordinal;
  if (!d || !out) return fail(NULL, 1, "%s", "null argument");
  if (d->compute_dtype != DT_F32 && d->compute_dtype != DT_BF16 && d->compute_dtype != DT_F16) return fail(NULL, 2, "%s", "unknown compute dtype");
  if (d->heads <= 0 || d->kv_heads <= 0 || d->heads % d->kv_heads) return fail(NULL, 1, "%s", "heads % kv_heads != 0");
  if (d->head_dim % 2) return fail(NULL, 1, "%s", "odd head_dim");
  tgxo_ctx* c = (tgxo_ctx*)calloc(1, sizeof(tgxo_ctx));
  if (!c) return 5;
  c->d = *d;
  if (c->d.max_batch < 1) c->d.max_batch = 1;
  c->bf16 = d->compute_dtype == DT_BF16;
  c->f16 = d->compute_dtype == DT_F16;
  c->ablate_key = -1;
  { const char* e = getenv("TGXO_TORCH_ROUNDING"); c->round_act = c->bf16 && e && e[0] == '1'; }
  int H = d->hidden, I = d->inter, V = d->vocab;
  int qd = d->heads * d->head_dim, kvd = d->kv_heads * d->head_dim;
  int gpt2 = d->family == F_GPT2;
  int ok = mat_alloc(c, &c->embed, V, H, 0);
  if (gpt2) ok &= mat_alloc(c, &c->wpe, d->n_positions, H, 0);
  if (!d->tied && !gpt2) ok &= mat_alloc(c, &c->lm_head, V, H, 0);
  ok &= vec_alloc(&c->final_norm, H, gpt2);
  c->L = (layer_t*)calloc((size_t)d->layers, sizeof(layer_t));
  for (int l = 0; l < d->layers && ok; l++) {
    layer_t* y = &c->L[l];
    ok &= vec_alloc(&y->in_norm, H, gpt2) && vec_alloc(&y->post_norm, H, gpt2);
    if (d->qk_norm) ok &= vec_alloc(&y->q_norm, d->head_dim, 0) && vec_alloc(&y->k_norm, d->head_dim, 0);
    ok &= mat_alloc(c, &y->qkv, qd + 2 * kvd, H, d->qkv_bias || gpt2);
    ok &= mat_alloc(c, &y->o, H, qd, gpt2);
    ok &= mat_alloc(c, &y->gate_up, gpt2 ? I : 2 * I, H, gpt2);
    ok &= mat_alloc(c, &y->down, H, I, gpt2);
  }
  size_t kvn = (size_t)c->d.max_batch * d->layers * d->max_ctx * kvd;
  c->kcache = (float*)calloc(kvn, 4);
  c->vcache = (float*)calloc(kvn, 4);
  c->logits = (float*)calloc((size_t)c->d.max_batch * V, 4);
  c->next_tok = (int64_t*)calloc((size_t)c->d.max_batch, 8);
  if (!ok || !c->kcache || !c->vcache || !c->logits || !c->next_tok) { *out = c; return fail(c, 5, "%s", "allocation failed"); }
  *out = c;
  return 0;
}

TGXO_EXPORT void tgxo_destroy(tgxo_ctx* c) {
  if (!c) return;
  mat_free(&c->embed); mat_free(&c->wpe); mat_free(&c->lm_head);
  free(c->final_norm.w); free(c->final_norm.b);
  if (c->L) for (int l = 0; l < c->d.layers; l++) {
    layer_t* y = &c->L[l];
    free(y->in_norm.w); free(y->in_norm.b); free(y->post_norm.w); free(y->post_norm.b); free(y->q_norm.w); free(y->k_norm.w);
    mat_free(&y->qkv); mat_free(&y->o); mat_free(&y->gate_up); mat_free(&y->down);
  }
  free(c->L); free(c->rope_cos); free(c->rope_sin); free(c->kcache); free(c->vcache); free(c->logits); free(c->next_tok);
  free(c);
}

/* ---------------------------------------------------------------- API: upload by HF name */
static int64_t numel(const int64_t* s, int nd) { int64_t n = 1; for (int i = 0; i < nd; i++) n *= s[i]; return n; }

static int shape_is(const int64_t* s, int nd, int64_t a, int64_t b) {
  if (b < 0) return nd == 1 && s[0] == a;
  return nd == 2 && s[0] == a && s[1] == b;
}

TGXO_EXPORT int tgxo_upload(tgxo_ctx* c, const char* name, const void* host, const int64_t* shape, int nd, int dt) {
  if (!c || !name || !host || !shape) return 1;
  const desc_t* d = &c->d;
  int H = d->hidden, I = d->inter, V = d->vocab, qd = d->heads * d->head_dim, kvd = d->kv_heads * d->head_dim;
  int l = -1; char rest[128] = {0};
  (void)numel;
  if (d->family == F_GPT2) {
    /* hub layout without "transformer." (ModelGPT2.h:226); accept the prefixed form too */
    if (!strncmp(name, "transformer.", 12)) name += 12;
    if (!strcmp(name, "wte.weight")) { if (!shape_is(shape, nd, V, H)) goto bad_shape; mat_store_rows(c, &c->embed, 0, V, host, dt, 0); return 0; }
    if (!strcmp(name, "wpe.weight")) { if (!shape_is(shape, nd, d->n_positions, H)) goto bad_shape; mat_store_rows(c, &c->wpe, 0, d->n_positions, host, dt, 0); return 0; }
    if (!strcmp(name, "ln_f.weight")) { if (!shape_is(shape, nd, H, -1)) goto bad_shape; vec_store(c, c->final_norm.w, H, host, dt); c->final_norm.filled_w = 1; return 0; }
    if (!strcmp(name, "ln_f.bias")) { if (!shape_is(shape, nd, H, -1)) goto bad_shape; vec_store(c, c->final_norm.b, H, host, dt); c->final_norm.filled_b = 1; return 0; }
    if (sscanf(name, "h.%d.%127s", &l, rest) == 2 && l >= 0 && l < d->layers) {
      layer_t* y = &c->L[l];
      struct { const char* n; vec_t* v; int isb; } vs[] = {
        {"ln_1.weight", &y->in_norm, 0}, {"ln_1.bias", &y->in_norm, 1}, {"ln_2.weight", &y->post_norm, 0}, {"ln_2.bias", &y->post_norm, 1}};
      for (int i = 0; i < 4; i++) if (!strcmp(rest, vs[i].n)) {
        if (!shape_is(shape, nd, H, -1)) goto bad_shape;
        vec_store(c, vs[i].isb ? vs[i].v->b : vs[i].v->w, H, host, dt);
        if (vs[i].isb) vs[i].v->filled_b = 1; else vs[i].v->filled_w = 1;
        return 0;
      }
      struct { const char* n; mat_t* m; } ms[] = {
        {"attn.c_attn", &y->qkv}, {"attn.c_proj", &y->o}, {"mlp.c_fc", &y->gate_up}, {"mlp.c_proj", &y->down}};
      for (int i = 0; i < 4; i++) {
        size_t ln = strlen(ms[i].n);
        if (!strncmp(rest, ms[i].n, ln) && rest[ln] == '.') {
          mat_t* m = ms[i].m;
          if (!strcmp(rest + ln + 1, "weight")) {   /* Conv1D weight is [in][out] (ModelGPT2.h:26) */
            if (!shape_is(shape, nd, m->cols, m->rows)) goto bad_shape;
            mat_store_rows(c, m, 0, m->rows, host, dt, 1); return 0;
          }
          if (!strcmp(rest + ln + 1, "bias")) {
            if (!shape_is(shape, nd, m->rows, -1)) goto bad_shape;
            vec_store(c, m->bias, m->rows, host, dt); m->bias_filled = 1; return 0;
          }
        }
      }
    }
    return fail(c, 6, "Unexpected key: %s", name);
  }
  if (!strcmp(name, "model.embed_tokens.weight")) { if (!shape_is(shape, nd, V, H)) goto bad_shape; mat_store_rows(c, &c->embed, 0, V, host, dt, 0); return 0; }
  if (!strcmp(name, "lm_head.weight")) {
    if (!shape_is(shape, nd, V, H)) goto bad_shape;
    if (d->tied) return 0;   /* aliased storage (GPTModel.h:39-41): the embed copy wins, like the reference's shared tensor */
    mat_store_rows(c, &c->lm_head, 0, V, host, dt, 0); return 0;
  }
  if (!strcmp(name, "model.norm.weight")) { if (!shape_is(shape, nd, H, -1)) goto bad_shape; vec_store(c, c->final_norm.w, H, host, dt); c->final_norm.filled_w = 1; return 0; }
  if (sscanf(name, "model.layers.%d.%127s", &l, rest) == 2 && l >= 0 && l < d->layers) {
    layer_t* y = &c->L[l];
    if (!strcmp(rest, "input_layernorm.weight")) { if (!shape_is(shape, nd, H, -1)) goto bad_shape; vec_store(c, y->in_norm.w, H, host, dt); y->in_norm.filled_w = 1; return 0; }
    if (d->qk_norm && !strcmp(rest, "self_attn.q_norm.weight")) { if (!shape_is(shape, nd, d->head_dim, -1)) goto bad_shape; vec_store(c, y->q_norm.w, d->head_dim, host, dt); y->q_norm.filled_w = 1; return 0; }
    if (d->qk_norm && !strcmp(rest, "self_attn.k_norm.weight")) { if (!shape_is(shape, nd, d->head_dim, -1)) goto bad_shape; vec_store(c, y->k_norm.w, d->head_dim, host, dt); y->k_norm.filled_w = 1; return 0; }
    if (!strcmp(rest, "post_attention_layernorm.weight")) { if (!shape_is(shape, nd, H, -1)) goto bad_shape; vec_store(c, y->post_norm.w, H, host, dt); y->post_norm.filled_w = 1; return 0; }
    /* MergedLinear slices (Linear.h:64-79): q rows [0,qd), k [qd,qd+kvd), v [qd+kvd, qd+2kvd) */
    struct { const char* n; mat_t* m; int64_t row0, rows, cols; } ws[] = {
      {"self_attn.q_proj", &y->qkv, 0, qd, H}, {"self_attn.k_proj", &y->qkv, qd, kvd, H}, {"self_attn.v_proj", &y->qkv, qd + kvd, kvd, H},
      {"self_attn.o_proj", &y->o, 0, H, qd}, {"mlp.gate_proj", &y->gate_up, 0, I, H}, {"mlp.up_proj", &y->gate_up, I, I, H},
      {"mlp.down_proj", &y->down, 0, H, I}};
    for (int i = 0; i < 7; i++) {
      size_t ln = strlen(ws[i].n);
      if (!strncmp(rest, ws[i].n, ln) && rest[ln] == '.') {
        if (!strcmp(rest + ln + 1, "weight")) {
          if (!shape_is(shape, nd, ws[i].rows, ws[i].cols)) goto bad_shape;
          mat_store_rows(c, ws[i].m, ws[i].row0, ws[i].rows, host, dt, 0); return 0;
        }
        if (!strcmp(rest + ln + 1, "bias") && ws[i].m->bias) {
          if (!shape_is(shape, nd, ws[i].rows, -1)) goto bad_shape;
          vec_store(c, ws[i].m->bias + ws[i].row0, ws[i].rows, host, dt); ws[i].m->bias_filled += (int)ws[i].rows; return 0;
        }
      }
    }
  }
  return fail(c, 6, "Unexpected key: %s", name);
bad_shape:
  return fail(c, 7, "shape not equal for tensor: %s", name);
}

/* ---------------------------------------------------------------- RoPE tables (HF LlamaRotaryEmbedding + llama3 scaling) */
static void build_rope(tgxo_ctx* c) {
  const desc_t* d = &c->d;
  int half = d->head_dim / 2;
  float* inv = (float*)malloc((size_t)half * 4);
  for (int i = 0; i < half; i++) {
    float e = (float)(2 * i) / (float)d->head_dim;                 /* arange(0,dim,2).float()/dim */
    float p = (float)pow((double)d->rope_theta, (double)e);        /* base ** e in fp32 */
    inv[i] = 1.0f / p;
  }
  if (d->family == F_LLAMA && d->rope_factor > 0.f) {              /* RopeScalingConfig (ModelLlama.h:21-24) */
    float factor = d->rope_factor, lo = d->rope_low_freq, hi = d->rope_high_freq, old = (float)d->rope_orig_ctx;
    float low_wl = old / lo, high_wl = old / hi;
    for (int i = 0; i < half; i++) {
      float wl = 2.0f * (float)M_PI / inv[i];
      float v = wl > low_wl ? inv[i] / factor : inv[i];
      float smooth = (old / wl - lo) / (hi - lo);
      float sm = (1.0f - smooth) * v / factor + smooth * v;
      int medium = !(wl < high_wl) && !(wl > low_wl);
      inv[i] = medium ? sm : v;
    }
  }
  c->rope_cos = (float*)malloc((size_t)d->max_ctx * half * 4);
  c->rope_sin = (float*)malloc((size_t)d->max_ctx * half * 4);
  for (int p = 0; p < d->max_ctx; p++)
    for (int i = 0; i < half; i++) {
      float a = inv[i] * (float)p;
      c->rope_cos[(size_t)p * half + i] = R(c, cosf(a));
      c->rope_sin[(size_t)p * half + i] = R(c, sinf(a));
    }
  free(inv);
}

TGXO_EXPORT int tgxo_finalize(tgxo_ctx* c) {
  if (!c) return 1;
  const desc_t* d = &c->d;
  int gpt2 = d->family == F_GPT2;
  char nm[96];
  if (c->embed.filled_rows != d->vocab) return fail(c, 4, "Missing key: %s", gpt2 ? "wte.weight" : "model.embed_tokens.weight");
  if (!gpt2 && !d->tied && c->lm_head.filled_rows != d->vocab) return fail(c, 4, "Missing key: %s", "lm_head.weight");
  if (!c->final_norm.filled_w) return fail(c, 4, "Missing key: %s", gpt2 ? "ln_f.weight" : "model.norm.weight");
  for (int l = 0; l < d->layers; l++) {
    layer_t* y = &c->L[l];
    snprintf(nm, sizeof nm, "layer %d", l);
    if (!y->in_norm.filled_w || !y->post_norm.filled_w || y->qkv.filled_rows != y->qkv.rows || y->o.filled_rows != y->o.rows ||
        y->gate_up.filled_rows != y->gate_up.rows || y->down.filled_rows != y->down.rows)
      return fail(c, 4, "Missing key in %s", nm);
    if (d->qkv_bias && !gpt2 && y->qkv.bias_filled != y->qkv.rows) return fail(c, 4, "Missing qkv bias in %s", nm);
    if (d->qk_norm && (!y->q_norm.filled_w || !y->k_norm.filled_w)) return fail(c, 4, "Missing q_norm/k_norm in %s", nm);
  }
  if (!gpt2) build_rope(c);
  c->finalized = 1;
  c->past = 0;
  return 0;
}

/* ---------------------------------------------------------------- math kernels */
static inline float dot_row(const tgxo_ctx* c, const mat_t* m, int64_t row, const float* x) {
  int64_t K = m->cols;
  float acc = 0.f;
  if (c->reorder) {               /* the same products summed from the last element to the first (tgxo_set_reorder) */
    if (c->bf16) {
      const uint16_t* w = m->wb + row * K;
#pragma omp simd reduction(+ : acc)
      for (int64_t k = K - 1; k >= 0; k--) {
        uint32_t u = (uint32_t)w[k] << 16; float f; memcpy(&f, &u, 4);
        acc += f * x[k];
      }
    } else {
      const float* w = m->wf + row * K;
#pragma omp simd reduction(+ : acc)
      for (int64_t k = K - 1; k >= 0; k--) acc += w[k] * x[k];
    }
    return acc;
  }
  if (c->bf16) {
    const uint16_t* w = m->wb + row * K;
#pragma omp simd reduction(+ : acc)
    for (int64_t k = 0; k < K; k++) {
      uint32_t u = (uint32_t)w[k] << 16; float f; memcpy(&f, &u, 4);
      acc += f * x[k];
    }
  } else {
    const float* w = m->wf + row * K;
#pragma omp simd reduction(+ : acc)
    for (int64_t k = 0; k < K; k++) acc += w[k] * x[k];
  }
  return acc;
}

/* Four weight rows against one activation row in ONE pass over k: four independent accumulators, each summing exactly the products dot_row() sums for
 * its row in exactly dot_row()'s order (the compiler vectorises every reduction of the loop the same way it vectorises the single one), so the
 * results are BIT-IDENTICAL to four dot_row() calls (tests/test_oracle_golden.py::test_four_row_pass_is_bit_identical holds it) - only the activation
 * loads are shared and four add chains overlap. */
#define DOT4_BODY(W_T, LOADW, KLOOP)                                                         \
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;                                              \
  const W_T *w0 = w, *w1 = w + K, *w2 = w + 2 * K, *w3 = w + 3 * K;                          \
  _Pragma("omp simd reduction(+ : a0, a1, a2, a3)")                                          \
  KLOOP {                                                                                    \
    const float xv = x[k];                                                                   \
    a0 += LOADW(w0[k]) * xv; a1 += LOADW(w1[k]) * xv; a2 += LOADW(w2[k]) * xv; a3 += LOADW(w3[k]) * xv; \
  }                                                                                          \
  out[0] = a0; out[1] = a1; out[2] = a2; out[3] = a3;
#define FWD_K for (int64_t k = 0; k < K; k++)
#define REV_K for (int64_t k = K - 1; k >= 0; k--)
#define LOAD_F32(v) (v)
static inline void dot4_bf16_fwd(const uint16_t* w, const float* x, int64_t K, float* out) { DOT4_BODY(uint16_t, bf16_to_f32, FWD_K) }
static inline void dot4_bf16_rev(const uint16_t* w, const float* x, int64_t K, float* out) { DOT4_BODY(uint16_t, bf16_to_f32, REV_K) }
static inline void dot4_f32_fwd(const float* w, const float* x, int64_t K, float* out) { DOT4_BODY(float, LOAD_F32, FWD_K) }
static inline void dot4_f32_rev(const float* w, const float* x, int64_t K, float* out) { DOT4_BODY(float, LOAD_F32, REV_K) }
static inline void dot_rows4(const tgxo_ctx* c, const mat_t* m, int64_t row, const float* x, float* out) {
  const int64_t K = m->cols;
  if (c->bf16) { if (c->reorder) dot4_bf16_rev(m->wb + row * K, x, K, out); else dot4_bf16_fwd(m->wb + row * K, x, K, out); }
  else { if (c->reorder) dot4_f32_rev(m->wf + row * K, x, K, out); else dot4_f32_fwd(m->wf + row * K, x, K, out); }
}

/* y[s][n] = R(x[s] . W[n] + b[n]) for S rows of x; raw != 0 keeps the fp32 accumulator.
 * Loop order only: blocks of 8 weight rows are walked over all S activation rows, so that a prompt's activations stream from the
 * cache once per 8 rows instead of once per row (a 2048-token prompt at full model size: minutes -> tens of seconds).  Every dot
 * product is the same sum in the same element order (dot_row(), or four rows of it at once: dot_rows4()), i.e. the results are
 * bit-identical to the row-by-row order. */
static int g_one_row_dots;     /* tgxo_set_one_row_dots: test hook, forces the row-by-row form */
static void linear(const tgxo_ctx* c, const mat_t* m, const float* x, int S, float* y, int raw) {
  int64_t N = m->rows, K = m->cols;
  float* xr = NULL;
  if (c->act16 && (c->bf16 || c->f16)) {      /* option act.round16 of the MI355X library: x := storage_dtype(x), RNE, once per Linear input */
    xr = (float*)malloc((size_t)S * K * sizeof(float));
    for (int64_t i = 0; i < (int64_t)S * K; i++) xr[i] = RKV(c, x[i]);
    x = xr;
  }
  const int four = !g_one_row_dots;
#pragma omp parallel for schedule(static)
  for (int64_t nb = 0; nb < N; nb += 8) {
    int64_t ne = nb + 8 < N ? nb + 8 : N;
    for (int s = 0; s < S; s++) {
      const float* xs = x + (int64_t)s * K;
      int64_t n = nb;
      for (; four && n + 4 <= ne; n += 4) {
        float a4[4];
        dot_rows4(c, m, n, xs, a4);
        for (int j = 0; j < 4; j++) {
          float a = a4[j] + (m->bias ? m->bias[n + j] : 0.f);
          y[(int64_t)s * N + n + j] = raw ? a : R(c, a);
        }
      }
      for (; n < ne; n++) {
        float a = dot_row(c, m, n, xs) + (m->bias ? m->bias[n] : 0.f);
        y[(int64_t)s * N + n] = raw ? a : R(c, a);
      }
    }
  }
  free(xr);
}

static void rmsnorm(const tgxo_ctx* c, const float* x, const float* w, int n, float* y) {
  float ss = 0.f;
  if (c->reorder) for (int i = n - 1; i >= 0; i--) ss += x[i] * x[i];
  else for (int i = 0; i < n; i++) ss += x[i] * x[i];
  float inv = 1.0f / sqrtf(ss / (float)n + c->d.norm_eps);
  for (int i = 0; i < n; i++) y[i] = R(c, w[i] * R(c, x[i] * inv));
}

static void layernorm(const tgxo_ctx* c, const float* x, const float* w, const float* b, int n, float* y) {
  float mean = 0.f;
  if (c->reorder) for (int i = n - 1; i >= 0; i--) mean += x[i];
  else for (int i = 0; i < n; i++) mean += x[i];
  mean /= (float)n;
  float var = 0.f;
  if (c->reorder) for (int i = n - 1; i >= 0; i--) { float t = x[i] - mean; var += t * t; }
  else for (int i = 0; i < n; i++) { float t = x[i] - mean; var += t * t; }
  var /= (float)n;
  float inv = 1.0f / sqrtf(var + c->d.norm_eps);
  for (int i = 0; i < n; i++) y[i] = R(c, (x[i] - mean) * inv * w[i] + b[i]);
}

static inline float silu(float x) { return x / (1.0f + expf(-x)); }
static inline float gelu_new(float x) {
  return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}

/* rotate-half RoPE on one head vector at absolute position pos (Attention.h:81-83) */
static void rope_head(const tgxo_ctx* c, float* v, int pos) {
  int hd = c->d.head_dim, half = hd / 2;
  const float* cs = c->rope_cos + (size_t)pos * half;
  const float* sn = c->rope_sin + (size_t)pos * half;
  for (int i = 0; i < half; i++) {
    float a = v[i], b = v[i + half];
    v[i] = R(c, R(c, a * cs[i]) + R(c, -b * sn[i]));
    v[i + half] = R(c, R(c, b * cs[i]) + R(c, a * sn[i]));
  }
}

/* softmax(q.K^T * scale) . V for one query head over keys [0, nkeys) */
static void attend(const tgxo_ctx* c, const float* q, const float* K, const float* V, int nkeys, int kvd, float* out, float* sc) {
  int hd = c->d.head_dim, ro = c->reorder;
  float scale = 1.0f / sqrtf((float)hd), mx = -INFINITY;
  for (int j = 0; j < nkeys; j++) {
    const float* k = K + (size_t)j * kvd;
    float a = 0.f;
    if (ro) for (int t = hd - 1; t >= 0; t--) a += q[t] * k[t];
    else for (int t = 0; t < hd; t++) a += q[t] * k[t];
    sc[j] = a * scale;
    if (j == c->ablate_key) sc[j] = -INFINITY;   /* tgxo_set_ablate_key: the key is lost (weight exactly 0); a query whose ONLY key it is yields NaN */
    if (sc[j] > mx) mx = sc[j];
  }
  float sum = 0.f;
  for (int j = 0; j < nkeys; j++) sc[j] = expf(sc[j] - mx);
  if (ro) for (int j = nkeys - 1; j >= 0; j--) sum += sc[j];
  else for (int j = 0; j < nkeys; j++) sum += sc[j];
  float inv = 1.0f / sum;
  for (int t = 0; t < hd; t++) out[t] = 0.f;
  for (int jj = 0; jj < nkeys; jj++) {
    int j = ro ? nkeys - 1 - jj : jj;
    const float* v = V + (size_t)j * kvd;
    float p = sc[j] * inv;
    for (int t = 0; t < hd; t++) out[t] += p * v[t];
  }
  for (int t = 0; t < hd; t++) out[t] = R(c, out[t]);
}

static inline float embed_elem(const tgxo_ctx* c, const mat_t* m, int64_t row, int64_t k) {
  return c->bf16 ? bf16_to_f32(m->wb[row * m->cols + k]) : m->wf[row * m->cols + k];
}

/* ---------------------------------------------------------------- forward for one batch row */
static int forward_row(tgxo_ctx* c, int b, const int64_t* ids, int S) {
  const desc_t* d = &c->d;
  int H = d->hidden, I = d->inter, V = d->vocab, hd = d->head_dim, nh = d->heads, nkv = d->kv_heads;
  int qd = nh * hd, kvd = nkv * hd, G = nh / nkv, gpt2 = d->family == F_GPT2;
  int64_t past = c->past;
  size_t SH = (size_t)S * H;
  float* x = (float*)malloc(SH * 4);
  float* xn = (float*)malloc(SH * 4);
  float* qkv = (float*)malloc((size_t)S * (qd + 2 * kvd) * 4);
  float* att = (float*)malloc((size_t)S * qd * 4);
  float* proj = (float*)malloc(SH * 4);
  float* gu = (float*)malloc((size_t)S * 2 * I * 4);
  float* hmid = (float*)malloc((size_t)S * I * 4);
  if (!x || !xn || !qkv || !att || !proj || !gu || !hmid) return 5;

  for (int s = 0; s < S; s++) {
    int64_t id = ids[s];
    if (id < 0 || id >= V) { free(x); free(xn); free(qkv); free(att); free(proj); free(gu); free(hmid); return fail(c, 1, "%s", "token id out of range"); }
    for (int k = 0; k < H; k++) {
      float e = embed_elem(c, &c->embed, id, k);
      if (gpt2) e = R(c, e + embed_elem(c, &c->wpe, past + s, k));   /* wte(ids) + wpe(arange(past,past+S)) (ModelGPT2.h:165-169) */
      x[(size_t)s * H + k] = e;
    }
  }

  for (int l = 0; l < d->layers; l++) {
    const layer_t* y = &c->L[l];
    float* Kc = c->kcache + (((size_t)b * d->layers + l) * d->max_ctx) * kvd;
    float* Vc = c->vcache + (((size_t)b * d->layers + l) * d->max_ctx) * kvd;
#pragma omp parallel for schedule(static) if (S > 8)   /* rows are independent; every per-row sum keeps its serial order */
    for (int s = 0; s < S; s++) {
      if (gpt2) layernorm(c, x + (size_t)s * H, y->in_norm.w, y->in_norm.b, H, xn + (size_t)s * H);
      else rmsnorm(c, x + (size_t)s * H, y->in_norm.w, H, xn + (size_t)s * H);
    }
    linear(c, &y->qkv, xn, S, qkv, 0);
    /* split -> heads -> RoPE(q), RoPE(k) at pastLength -> cache append (Attention.h:94-106) */
#pragma omp parallel for schedule(static) if (S > 8)   /* rows are independent; every per-row sum keeps its serial order */
    for (int s = 0; s < S; s++) {
      float* row = qkv + (size_t)s * (qd + 2 * kvd);
      if (d->qk_norm) {   /* AttentionWithQKNorm::projectQKV (Attention.h:156-163): RMSNorm over head_dim, per head, before RoPE */
        float tmp[512];
        for (int h = 0; h < nh; h++) { rmsnorm(c, row + h * hd, y->q_norm.w, hd, tmp); memcpy(row + h * hd, tmp, (size_t)hd * 4); }
        for (int h = 0; h < nkv; h++) { rmsnorm(c, row + qd + h * hd, y->k_norm.w, hd, tmp); memcpy(row + qd + h * hd, tmp, (size_t)hd * 4); }
      }
      if (!gpt2) {
        for (int h = 0; h < nh; h++) rope_head(c, row + h * hd, (int)(past + s));
        for (int h = 0; h < nkv; h++) rope_head(c, row + qd + h * hd, (int)(past + s));
      }
      for (int t = 0; t < kvd; t++) {
        Kc[(size_t)(past + s) * kvd + t] = RKV(c, row[qd + t]);
        Vc[(size_t)(past + s) * kvd + t] = RKV(c, row[qd + kvd + t]);
      }
    }
    /* isCausal = (pastLength == 0) (Attention.h:108): query s sees keys [0, past+s]; with past>0 S must be 1 */
#pragma omp parallel
    {
      float* sc = (float*)malloc((size_t)(past + S) * 4);
#pragma omp for collapse(2) schedule(static)
      for (int s = 0; s < S; s++)
        for (int h = 0; h < nh; h++) {
          int nkeys = (int)(past + s + 1);
          attend(c, qkv + (size_t)s * (qd + 2 * kvd) + h * hd, Kc + (h / G) * hd, Vc + (h / G) * hd, nkeys, kvd,
                 att + (size_t)s * qd + h * hd, sc);
        }
      free(sc);
    }
    linear(c, &y->o, att, S, proj, 0);
#pragma omp parallel for schedule(static) if (S > 8)
    for (size_t i = 0; i < SH; i++) x[i] = R(c, x[i] + proj[i]);           /* x = x + attn(norm(x)) (DecoderLayer.h:40) */
#pragma omp parallel for schedule(static) if (S > 8)   /* rows are independent; every per-row sum keeps its serial order */
    for (int s = 0; s < S; s++) {
      if (gpt2) layernorm(c, x + (size_t)s * H, y->post_norm.w, y->post_norm.b, H, xn + (size_t)s * H);
      else rmsnorm(c, x + (size_t)s * H, y->post_norm.w, H, xn + (size_t)s * H);
    }
    linear(c, &y->gate_up, xn, S, gu, 0);
    if (gpt2) {
#pragma omp parallel for schedule(static) if (S > 8)
      for (size_t i = 0; i < (size_t)S * I; i++) hmid[i] = R(c, gelu_new(gu[i]));
    } else {
      /* siluMul: silu(x[..., :I]) * x[..., I:] (Activation.h:16; gate rows first, GatedMLP.h:46-47) */
#pragma omp parallel for schedule(static) if (S > 8)   /* rows are independent; every per-row sum keeps its serial order */
      for (int s = 0; s < S; s++)
        for (int i = 0; i < I; i++) {
          float g = gu[(size_t)s * 2 * I + i], u = gu[(size_t)s * 2 * I + I + i];
          hmid[(size_t)s * I + i] = R(c, R(c, silu(g)) * u);
        }
    }
    linear(c, &y->down, hmid, S, proj, 0);
#pragma omp parallel for schedule(static) if (S > 8)
    for (size_t i = 0; i < SH; i++) x[i] = R(c, x[i] + proj[i]);           /* x = x + mlp(norm(x)) (DecoderLayer.h:41) */
  }
  /* final norm + lm_head on the last position only (== forward over all S then narrow, GPTEngine.cpp:96-97) */
  const float* xl = x + (size_t)(S - 1) * H;
  if (gpt2) layernorm(c, xl, c->final_norm.w, c->final_norm.b, H, xn);
  else rmsnorm(c, xl, c->final_norm.w, H, xn);
  const mat_t* head = (d->tied || gpt2) ? &c->embed : &c->lm_head;
  linear(c, head, xn, 1, c->logits + (size_t)b * V, 1);
  free(x); free(xn); free(qkv); free(att); free(proj); free(gu); free(hmid);
  return 0;
}

TGXO_EXPORT int tgxo_forward(tgxo_ctx* c, const int64_t* ids, int batch, int seq) {
  if (!c || !ids) return 1;
  if (!c->finalized) return fail(c, 4, "%s", "forward before finalize");
  if (batch < 1 || batch > c->d.max_batch || seq < 1) return fail(c, 1, "%s", "batch/seq out of range");
  if (seq > 1 && c->past > 0) return fail(c, 1, "%s", "seq>1 with pastLength>0");
  if (c->past + seq > c->d.max_ctx) return fail(c, 8, "%s", "context size exceeded");
  for (int b = 0; b < batch; b++) {
    int rc = forward_row(c, b, ids + (size_t)b * seq, seq);
    if (rc) return rc;
  }
  c->past += seq;
  c->last_batch = batch;
  return 0;
}

TGXO_EXPORT int tgxo_read_logits(tgxo_ctx* c, float* out, int rounded) {
  if (!c || !out || c->last_batch < 1) return 1;
  size_t n = (size_t)c->last_batch * c->d.vocab;
  for (size_t i = 0; i < n; i++) out[i] = rounded ? R(c, c->logits[i]) : c->logits[i];
  return 0;
}

/* ---------------------------------------------------------------- sampler (Sampler.cpp:23-79) */
static uint64_t splitmix(uint64_t* s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

typedef struct { float v; int32_t i; } kv_t;
static int cmp_desc(const void* a, const void* b) {   /* value descending, index ascending: stable sort order */
  const kv_t *x = (const kv_t*)a, *y = (const kv_t*)b;
  if (x->v > y->v) return -1;
  if (x->v < y->v) return 1;
  return (x->i > y->i) - (x->i < y->i);
}

static void softmax_inplace(float* p, const float* l, int V) {
  float mx = -INFINITY;
  for (int i = 0; i < V; i++) if (l[i] > mx) mx = l[i];
  double sum = 0.0;   /* the normaliser is accumulated in double and rounded once: the result does not depend on the order
                       * of summation, so a parallel implementation can reproduce it bit for bit (sampler) */
  for (int i = 0; i < V; i++) { p[i] = expf(l[i] - mx); sum += (double)p[i]; }
  float inv = 1.0f / (float)sum;
  for (int i = 0; i < V; i++) p[i] *= inv;
}

/* Applies temperature / top-k / top-p / min-p to l[V] in place (masked entries become -inf) and
 * writes the final probabilities to probs[V].  Exposed for kept-set parity tests. */
TGXO_EXPORT int tgxo_filter_logits(const sampler_cfg_t* cfg, float* l, float* probs, int V) {
  int setT = cfg->temperature > 0.f, setK = cfg->top_k > 0, setP = cfg->top_p < 1.f, setM = cfg->min_p > 0.f;
  kv_t* srt = (kv_t*)malloc((size_t)V * sizeof(kv_t));
  float* tmp = (float*)malloc((size_t)V * 4);
  if (!srt || !tmp) { free(srt); free(tmp); return 5; }
  if (setT) for (int i = 0; i < V; i++) l[i] = l[i] / cfg->temperature;
  if (setK) {
    int k = cfg->top_k < V ? (int)cfg->top_k : V;
    for (int i = 0; i < V; i++) { srt[i].v = l[i]; srt[i].i = i; }
    qsort(srt, (size_t)V, sizeof(kv_t), cmp_desc);
    for (int i = 0; i < V; i++) l[i] = -INFINITY;
    for (int i = 0; i < k; i++) l[srt[i].i] = srt[i].v;
  }
  if (setP) {
    for (int i = 0; i < V; i++) { srt[i].v = l[i]; srt[i].i = i; }
    qsort(srt, (size_t)V, sizeof(kv_t), cmp_desc);
    for (int i = 0; i < V; i++) tmp[i] = srt[i].v;
    softmax_inplace(tmp, tmp, V);
    float cum = 0.f;
    for (int i = 0; i < V; i++) {
      cum += tmp[i];
      int keep = (cum <= cfg->top_p) || i == 0;     /* cumulativeProbs <= topP, first always kept (Sampler.cpp:52-57) */
      l[srt[i].i] = keep ? srt[i].v : -INFINITY;
    }
  }
  if (setM) {
    softmax_inplace(tmp, l, V);
    float mx = 0.f;
    for (int i = 0; i < V; i++) if (tmp[i] > mx) mx = tmp[i];
    float thr = mx * cfg->min_p;
    for (int i = 0; i < V; i++) if (tmp[i] < thr) l[i] = -INFINITY;
  }
  softmax_inplace(probs, l, V);
  free(srt); free(tmp);
  return 0;
}

TGXO_EXPORT int tgxo_sample(tgxo_ctx* c, const sampler_cfg_t* cfg, uint64_t seed, int64_t* out_ids) {
  if (!c || !cfg || c->last_batch < 1) return 1;
  int V = c->d.vocab;
  int greedy = !(cfg->temperature > 0.f || cfg->top_k > 0 || cfg->top_p < 1.f || cfg->min_p > 0.f);
  float* l = (float*)malloc((size_t)V * 4);
  float* p = (float*)malloc((size_t)V * 4);
  for (int b = 0; b < c->last_batch; b++) {
    for (int i = 0; i < V; i++) l[i] = R(c, c->logits[(size_t)b * V + i]);   /* the sampler sees compute-dtype logits */
    int64_t pick = 0;
    if (greedy) {
      float mx = l[0];
      for (int i = 1; i < V; i++) if (l[i] > mx) { mx = l[i]; pick = i; }     /* first maximal index */
    } else {
      tgxo_filter_logits(cfg, l, p, V);
      uint64_t s = seed * 0x9E3779B97F4A7C15ull + (uint64_t)c->past * 0xD1342543DE82EF95ull + (uint64_t)b;
      double u = (double)(splitmix(&s) >> 11) * (1.0 / 9007199254740992.0);
      double cum = 0.0;
      pick = -1;
      for (int i = 0; i < V; i++) { if (p[i] > 0.f) { cum += p[i]; pick = i; if (u < cum) break; } }
    }
    c->next_tok[b] = pick;
    if (out_ids) out_ids[b] = pick;
  }
  free(l); free(p);
  return 0;
}

/* == decode loop of generateSync (GPTEngine.cpp:165-168) */
TGXO_EXPORT int tgxo_decode(tgxo_ctx* c, const sampler_cfg_t* cfg, uint64_t seed, int n_steps, int64_t* out_ids) {
  if (!c || !cfg || c->last_batch < 1) return 1;
  int B = c->last_batch;
  for (int i = 0; i < n_steps; i++) {
    int rc = tgxo_forward(c, c->next_tok, B, 1);
    if (rc) return rc;
    rc = tgxo_sample(c, cfg, seed, out_ids ? out_ids + (size_t)i * B : NULL);
    if (rc) return rc;
  }
  return 0;
}

TGXO_EXPORT int tgxo_set_next_token(tgxo_ctx* c, const int64_t* ids, int batch) {
  if (!c || !ids || batch < 1 || batch > c->d.max_batch) return 1;
  for (int b = 0; b < batch; b++) c->next_tok[b] = ids[b];
  c->last_batch = batch;
  return 0;
}

TGXO_EXPORT int tgxo_set_logits(tgxo_ctx* c, const float* logits, int batch) {
  if (!c || !logits || batch < 1 || batch > c->d.max_batch) return 1;
  memcpy(c->logits, logits, (size_t)batch * c->d.vocab * 4);
  c->last_batch = batch;
  return 0;
}

/* Test hook (tests/test_oracle_reorder.py): 1 = every reduction of this context (Linear dot products, RMSNorm / LayerNorm sums, q.k, softmax sum, P.V) runs from the
 * last element to the first.  Same products, another fp32 summation order: the distance between the two schedules is the floor any OTHER correct
 * implementation (the HIP kernels) can be held to. */
TGXO_EXPORT int tgxo_set_reorder(tgxo_ctx* c, int on) { if (!c) return 1; c->reorder = on != 0; return 0; }
/* 1 = per-op rounding of every activation to bf16 (what the env switch TGXO_TORCH_ROUNDING=1 selects at create): the contract of a module constructed in
 * torch_dtype bf16 (ModelLlama.h:62, ModelLoader.cpp:84), restated op by op the way torch-bf16 / HF-bf16 rounds.  Call BEFORE tgxo_finalize (the RoPE tables
 * are rounded when they are built).  bf16 storage only.  Held against HF-bf16's logits and ids in tests/test_oracle_golden.py. */
TGXO_EXPORT int tgxo_set_torch_rounding(tgxo_ctx* c, int on) {
  if (!c) return 1;
  if (c->finalized) return fail(c, 4, "%s", "set_torch_rounding after finalize");
  c->round_act = c->bf16 && on != 0;
  return 0;
}
/* 1 = the Linear-input rounding of the library's option act.round16 (see linear()) */
TGXO_EXPORT int tgxo_set_act16(tgxo_ctx* c, int on) { if (!c) return 1; c->act16 = on != 0; return 0; }

TGXO_EXPORT int tgxo_set_one_row_dots(int on) { g_one_row_dots = on != 0; return 0; }   /* test hook: linear() one row at a time (the form the four-row pass must equal bit for bit) */
TGXO_EXPORT int tgxo_set_threads(int n) { if (n > 0) omp_set_num_threads(n); return omp_get_max_threads(); }

TGXO_EXPORT int tgxo_reset_cache(tgxo_ctx* c) { if (!c) return 1; c->past = 0; return 0; }
TGXO_EXPORT int64_t tgxo_past_length(const tgxo_ctx* c) { return c ? c->past : -1; }
TGXO_EXPORT int64_t tgxo_context_size(const tgxo_ctx* c) { return c ? c->d.max_ctx : -1; }

TGXO_EXPORT int tgxo_read_kv(tgxo_ctx* c, int row, int layer, float* k_out, float* v_out) {
  if (!c || row < 0 || row >= c->d.max_batch || layer < 0 || layer >= c->d.layers) return 1;
  size_t kvd = (size_t)c->d.kv_heads * c->d.head_dim;
  size_t off = (((size_t)row * c->d.layers + layer) * c->d.max_ctx) * kvd;
  if (k_out) memcpy(k_out, c->kcache + off, (size_t)c->past * kvd * 4);
  if (v_out) memcpy(v_out, c->vcache + off, (size_t)c->past * kvd * 4);
  return 0;
}

/* Test hooks of the key-range tests (tests/kv_plant.py, tests/test_oracle_plant.py, tests/test_hip_attn_keyrange.py).
 * tgxo_write_kv: the inverse of tgxo_read_kv — cache rows [0, n_rows) of (row, layer) from fp32 [n_rows][kv_heads][head_dim], rounded ONCE to the storage
 * dtype (what the cache append does); n_rows may reach max_ctx whatever pastLength is.  tgxo_set_past: the context then holds n positions without a prefill.
 * tgxo_set_ablate_key: attend() scores key `pos` -inf for every query, head and layer whose key range holds it (pos < nkeys); -1 = off.  The distance the
 * logits move is the yardstick the planted caches are chosen by: how far the reference itself moves when exactly that key is lost. */
TGXO_EXPORT int tgxo_write_kv(tgxo_ctx* c, int row, int layer, const float* k_in, const float* v_in, int64_t n_rows) {
  if (!c || row < 0 || row >= c->d.max_batch || layer < 0 || layer >= c->d.layers || n_rows < 0 || n_rows > c->d.max_ctx) return c ? fail(c, 1, "%s", "write_kv: row / layer / n_rows out of range") : 1;
  size_t kvd = (size_t)c->d.kv_heads * c->d.head_dim;
  size_t off = (((size_t)row * c->d.layers + layer) * c->d.max_ctx) * kvd, n = (size_t)n_rows * kvd;
  if (k_in) for (size_t i = 0; i < n; i++) c->kcache[off + i] = RKV(c, k_in[i]);
  if (v_in) for (size_t i = 0; i < n; i++) c->vcache[off + i] = RKV(c, v_in[i]);
  return 0;
}
TGXO_EXPORT int tgxo_set_past(tgxo_ctx* c, int64_t n) {
  if (!c) return 1;
  if (!c->finalized) return fail(c, 4, "%s", "set_past before finalize");
  if (n < 0 || n > c->d.max_ctx) return fail(c, 1, "%s", "set_past: n out of range");
  c->past = n;
  return 0;
}
TGXO_EXPORT int tgxo_set_ablate_key(tgxo_ctx* c, int pos) { if (!c) return 1; c->ablate_key = pos < 0 ? -1 : pos; return 0; }

/* RoPE table read-back for the golden-table test: out[2][n_pos][head_dim/2] */
TGXO_EXPORT int tgxo_read_rope(tgxo_ctx* c, int n_pos, float* out) {
  if (!c || !c->rope_cos || n_pos > c->d.max_ctx) return 1;
  size_t n = (size_t)n_pos * (c->d.head_dim / 2);
  memcpy(out, c->rope_cos, n * 4);
  memcpy(out + n, c->rope_sin, n * 4);
  return 0;
}
