// abi.hip — the extern "C" shim of include/tgx.h for MI355X (gfx950): context, weight upload by HF name, KV cache, decode-step hipGraphs and the
// decode loop.  The kernels and their launch sequences live in the sibling translation units (ctx.h lists them).
//
// One context = one GPU = one HIP stream; every call comes from one host thread (the reference's engine is
// entered by one thread only: examples/inference/main.cpp, server/HttpServer.cpp:118-163).
// There is NO CPU path in this library: every entry point either runs on the GPU or returns an error.
#include <climits>
#include <functional>
#include "ctx.h"
#include "kernels/kv_fork.h"
#include "kernels/kv_pack.h"
#include "kernels/kv_splice.h"
#include "row_snapshot.h"
#include "splice_plan.h"
#include "beam_plan.h"
#include "verify_tree_plan.h"
#include "automaton.h"

static std::string g_create_err;

int set_err(tgx_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_err = buf;
  return code;
}

namespace {

inline uint16_t host_f32_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float host_bf16_to_f32(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
inline float host_half_to_f32(uint16_t h) {
  uint32_t s = (h >> 15) & 1, e = (h >> 10) & 0x1f, m = h & 0x3ff, u;
  if (e == 0) {
    if (m == 0) u = s << 31;
    else { e = 127 - 15 + 1; while (!(m & 0x400)) { m <<= 1; e--; } m &= 0x3ff; u = (s << 31) | (e << 23) | (m << 13); }
  } else if (e == 31) u = (s << 31) | 0x7f800000u | (m << 13);
  else u = (s << 31) | ((e + 127 - 15) << 23) | (m << 13);
  float f;
  memcpy(&f, &u, 4);
  return f;
}

inline uint16_t host_f32_to_half(float f) {   // round-to-nearest-even, subnormals kept (== torch .to(float16))
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u, abs = u & 0x7fffffffu;
  if (abs > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
  if (abs >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);                // >= 65536 (or inf) -> inf; 65520..65536 handled below
  if (abs < 0x33000000u) return (uint16_t)sign;                            // < 2^-25 -> 0
  int e = (int)(abs >> 23) - 127;
  uint32_t m = (abs & 0x7fffffu) | 0x800000u;                              // 24-bit significand
  int shift = e >= -14 ? 13 : 13 + (-14 - e);                              // bits dropped (subnormal: more)
  uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
  if (rem > halfway || (rem == halfway && (q & 1u))) q++;
  uint32_t h = e >= -14 ? ((uint32_t)(e + 15) << 10) + (q - 0x400u) : q;  // carries propagate into the exponent
  if (h >= 0x7c00u) h = 0x7c00u;
  return (uint16_t)(sign | h);
}

// host -> device copy with conversion to the compute dtype (== model().to(dtype), ModelLoader.cpp:84):
// widening is exact, narrowing rounds to nearest even once.
int upload_param(tgx_ctx* c, ebyte* dst, const void* host, int64_t n, int src_dtype) {
  const int want = c->d.compute_dtype;
  if (src_dtype != TGX_BF16 && src_dtype != TGX_F32 && src_dtype != TGX_F16) return set_err(c, TGX_ERR_INVALID, "unknown source dtype %d", src_dtype);
  if (src_dtype == want) {
    HIP_OK(c, hipMemcpy(dst, host, (size_t)n * c->esz, hipMemcpyHostToDevice));
    return TGX_OK;
  }
  auto src = [&](int64_t i) -> float {
    if (src_dtype == TGX_F32) return ((const float*)host)[i];
    if (src_dtype == TGX_BF16) return host_bf16_to_f32(((const uint16_t*)host)[i]);
    return host_half_to_f32(((const uint16_t*)host)[i]);
  };
  if (want == TGX_F32) {
    std::vector<float> tmp((size_t)n);
    for (int64_t i = 0; i < n; i++) tmp[(size_t)i] = src(i);
    HIP_OK(c, hipMemcpy(dst, tmp.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  } else {
    std::vector<uint16_t> tmp((size_t)n);
    if (want == TGX_BF16) for (int64_t i = 0; i < n; i++) tmp[(size_t)i] = host_f32_to_bf16(src(i));
    else for (int64_t i = 0; i < n; i++) tmp[(size_t)i] = host_f32_to_half(src(i));
    HIP_OK(c, hipMemcpy(dst, tmp.data(), (size_t)n * 2, hipMemcpyHostToDevice));
  }
  return TGX_OK;
}

bool shape_is(const int64_t* s, int nd, int64_t a, int64_t b) {
  if (b < 0) return nd == 1 && s[0] == a;
  return nd == 2 && s[0] == a && s[1] == b;
}

// GPT-2 checkpoints (hub layout without the "transformer." prefix, ModelGPT2.h:226; the prefixed form is accepted too).
// Conv1D weights are stored [in][out] (ModelGPT2.h:26): transposed on the host into the [out][in] rows the GEMV streams.
int upload_gpt2(tgx_ctx* c, const char* name, const void* host, const int64_t* shape, int nd, int src_dtype) {
  const tgx_model_desc& d = c->d;
  const int64_t H = d.hidden, I = d.inter, V = d.vocab;
  auto bad_shape = [&]() { return set_err(c, TGX_ERR_SHAPE, "shape not equal for tensor: %s", name); };
  if (!strncmp(name, "transformer.", 12)) name += 12;
  if (!strcmp(name, "wte.weight")) { if (!shape_is(shape, nd, V, H)) return bad_shape(); c->embed_ok = true; return upload_param(c, c->embed, host, V * H, src_dtype); }
  if (!strcmp(name, "wpe.weight")) { if (!shape_is(shape, nd, d.n_positions, H)) return bad_shape(); c->wpe_ok = true; return upload_param(c, c->wpe, host, (int64_t)d.n_positions * H, src_dtype); }
  if (!strcmp(name, "ln_f.weight")) { if (!shape_is(shape, nd, H, -1)) return bad_shape(); c->final_norm_ok = true; return upload_param(c, c->final_norm, host, H, src_dtype); }
  if (!strcmp(name, "ln_f.bias")) { if (!shape_is(shape, nd, H, -1)) return bad_shape(); c->final_norm_b_ok = true; return upload_param(c, c->final_norm_b, host, H, src_dtype); }
  if (!strcmp(name, "lm_head.weight")) { if (!shape_is(shape, nd, V, H)) return bad_shape(); return TGX_OK; }   // aliases wte
  int l = -1;
  char rest[128] = {0};
  if (sscanf(name, "h.%d.%127s", &l, rest) == 2 && l >= 0 && l < d.layers) {
    LayerW& w = c->L[(size_t)l];
    struct Vec { const char* n; ebyte* p; int64_t len; };
    const Vec vecs[] = {{"ln_1.weight", w.in_norm, H}, {"ln_1.bias", w.in_norm_b, H}, {"ln_2.weight", w.post_norm, H}, {"ln_2.bias", w.post_norm_b, H},
                        {"attn.c_attn.bias", w.bqkv, 3 * H}, {"attn.c_proj.bias", w.bo, H}, {"mlp.c_fc.bias", w.bfc, I}, {"mlp.c_proj.bias", w.bdown, H}};
    for (int i = 0; i < 8; i++)
      if (!strcmp(rest, vecs[i].n)) {
        if (!shape_is(shape, nd, vecs[i].len, -1)) return bad_shape();
        w.gpt2_filled |= 1 << i;
        return upload_param(c, vecs[i].p, host, vecs[i].len, src_dtype);
      }
    struct Mat { const char* n; ebyte* p; int64_t in, out; };
    const Mat mats[] = {{"attn.c_attn.weight", w.wqkv, H, 3 * H}, {"attn.c_proj.weight", w.wo, H, H}, {"mlp.c_fc.weight", w.wgu, H, I}, {"mlp.c_proj.weight", w.wdown, I, H}};
    for (int i = 0; i < 4; i++)
      if (!strcmp(rest, mats[i].n)) {
        if (!shape_is(shape, nd, mats[i].in, mats[i].out)) return bad_shape();
        if (src_dtype != TGX_BF16 && src_dtype != TGX_F32 && src_dtype != TGX_F16) return set_err(c, TGX_ERR_INVALID, "unknown source dtype %d", src_dtype);
        const size_t es = src_dtype == TGX_F32 ? 4 : 2, n_in = (size_t)mats[i].in, n_out = (size_t)mats[i].out;
        std::vector<unsigned char> t(n_in * n_out * es);
        const unsigned char* src = static_cast<const unsigned char*>(host);
        for (size_t k = 0; k < n_in; k++)
          for (size_t n = 0; n < n_out; n++) memcpy(&t[(n * n_in + k) * es], src + (k * n_out + n) * es, es);
        w.gpt2_filled |= 1 << (8 + i);
        return upload_param(c, mats[i].p, t.data(), (int64_t)(n_in * n_out), src_dtype);
      }
    if (!strcmp(rest, "attn.bias") || !strcmp(rest, "attn.masked_bias")) return TGX_OK;   // causal-mask buffers of old hub checkpoints: not parameters
  }
  return set_err(c, TGX_ERR_NAME, "Unexpected key: %s", name);
}

// nn::RoPE tables (ctor at ModelLlama.h:41-42): HF LlamaRotaryEmbedding incl. llama3 scaling, fp32.
void build_rope_host(const tgx_model_desc& d, std::vector<float>& cs, std::vector<float>& sn) {
  const int half = d.head_dim / 2;
  std::vector<float> inv((size_t)half);
  for (int i = 0; i < half; i++) {
    const float e = (float)(2 * i) / (float)d.head_dim;
    const float p = (float)std::pow((double)d.rope_theta, (double)e);
    inv[(size_t)i] = 1.0f / p;
  }
  if (d.family == TGX_FAMILY_LLAMA && d.rope_factor > 0.f) {
    const float factor = d.rope_factor, lo = d.rope_low_freq, hi = d.rope_high_freq, old = (float)d.rope_orig_ctx;
    const float low_wl = old / lo, high_wl = old / hi;
    for (int i = 0; i < half; i++) {
      const float wl = 2.0f * (float)M_PI / inv[(size_t)i];
      const float v = wl > low_wl ? inv[(size_t)i] / factor : inv[(size_t)i];
      const float smooth = (old / wl - lo) / (hi - lo);
      const float sm = (1.0f - smooth) * v / factor + smooth * v;
      const bool medium = !(wl < high_wl) && !(wl > low_wl);
      inv[(size_t)i] = medium ? sm : v;
    }
  }
  cs.resize((size_t)d.max_ctx * half);
  sn.resize((size_t)d.max_ctx * half);
  for (int p = 0; p < d.max_ctx; p++)
    for (int i = 0; i < half; i++) {
      const float a = inv[(size_t)i] * (float)p;
      cs[(size_t)p * half + i] = cosf(a);
      sn[(size_t)p * half + i] = sinf(a);
    }
}

}  // namespace

bool is_greedy(const tgx_sampler_cfg* s) {   // Sampler.cpp:15-21
  return !(s->temperature > 0.f || s->top_k > 0 || s->top_p < 1.f || s->min_p > 0.f);
}

// Context from which the MFMA decode attention (kernels/attn_decode_mfma.h) beats the VALU kernel, measured per geometry class
// (profiles/r02_attn_long.txt): head_dim 64 with 8 kv heads from ~6k keys (Llama-3.2-1B: 11.0 -> 9.9 µs per layer at 6k, 23.3 -> 18.3 at 30k);
// two kv heads (Qwen2.5-0.5B: few workgroups) and head_dim 128 (Mistral-7B, Llama-3.2-3B) from ~14k (Mistral-7B: 25.3 -> 21.4 at 16k, 39.5 -> 31.4 at 30k).
static int attn_mfma_threshold(const tgx_ctx* c) {
  if (c->attn_mfma_min >= 0) return c->attn_mfma_min;
  return (c->d.head_dim == 64 && c->d.kv_heads >= 8) ? 6000 : 14000;
}
// The attention form of the launches about to be issued / captured, from the context the call ends at: direct (one workgroup per head, no
// combine) for short contexts, the MFMA decode attention for long ones, the VALU split form in between.  One place for all callers
// (the prefill-by-steps branch used to leave attn_mfma at whatever the previous decode call had chosen).
// contexts up to which a decode call of this batch runs the direct form / its four-wave variant: batch-1 steps whose o_proj rides in the attention
// launch (decode.hip oproj_fused_capable) keep the direct form longer and on fewer waves
static long long direct_limit(const tgx_ctx* c, int rpl, bool step) {
  if (step && rpl == 1 && c->batch == 1 && oproj_fused_capable(c)) return c->attn_fused_max;
  // (2-3 rows, round 4: the direct form stays ahead to ~2x / ~3x the batch-1 limit — Llama-3.2-1B B = 3 at context 600 0.888 -> 0.820 ms per step, at 1200 0.959 -> 0.856;
  //  crossovers measured at ~2000 / ~2800 keys there, ~900 / ~1600 on Mistral-7B, ~1400 / > 1500 on Qwen2.5-0.5B)
  return (long long)c->attn_direct_max * (rpl >= 2 ? rpl : 1);
}
static long long nw4_limit(const tgx_ctx* c, int rpl, bool step) {
  if (rpl >= 4) return 0;
  if (step && rpl == 1 && c->batch == 1 && oproj_fused_capable(c)) return c->attn_fused_nw4;
  return c->attn_direct_nw4;
}
static void update_attn_modes(tgx_ctx* c, long long past, int n_positions, int rows_per_launch = -1, bool step = true) {   // past: the context the launches start at (an argument: an admission pass starts at 0 whatever the batch's longest row); rows_per_launch: batch rows that share an attention launch (-1: the batch); step: a decode step (not the chunk rows of a prefill-by-steps pass)
  // batches (round 3): the rows themselves fill the chip, so the one-workgroup-per-(kv head, row) form stays ahead of the split form far beyond the
  // batch-1 crossover — Llama-3.2-1B at context 2k: B = 8 1.250 -> 1.105 ms/step, B = 32 2.360 -> 1.680; Mistral-7B at 600: B = 32 6.91 -> 5.47
  const int rpl = rows_per_launch < 0 ? c->batch : rows_per_launch;
  const long long direct_lim = direct_limit(c, rpl, step), nw4_lim = nw4_limit(c, rpl, step);
  c->attn_direct = past + n_positions <= direct_lim;
  c->attn_nw4 = c->attn_direct && nw4_lim > 0 && past + n_positions <= nw4_lim;
  c->attn_mfma = !c->attn_direct && past >= attn_mfma_threshold(c) && c->dt != tgx::DT_F32 && !(c->d.qk_norm && c->d.head_dim == 128 && c->qk_fuse);
}

static void launch_decode_step(tgx_ctx* c, const tgx_sampler_cfg& cfg) {
  if (decode_mfma_ok(c)) {   // more than 4 rows: every Linear is one pass over its weights for up to 32 rows (kernels/skinny.h)
    // rows per weight pass (option decode.step_rows: 32 or 64): batches beyond 32 rows take four activation blocks per skinny product (one pass over
    // the weights for up to 64 rows) instead of two passes of two blocks
    // (128 rows = eight blocks exist on the LDS-DMA ring kernel only: every product must then take stored terms, i.e. the attention a direct form that writes them)
    const bool wide_ok = c->skinny_dma && c->skinny_dma_oproj >= 2 && c->attn_direct && c->dt != tgx::DT_F32;
    const int per = c->decode_step_rows > 64 && !wide_ok ? 64 : c->decode_step_rows;
    for (int row0 = 0; row0 < c->batch; row0 += per) launch_decode_step_mfma(c, row0, std::min(per, c->batch - row0), cfg);
    return;
  }
  // batch rows share each pass over the weights in groups of 4 / 2 / 1 (the batched GEMV's R template)
  for (int row0 = 0; row0 < c->batch;) {
    const int rem = c->batch - row0, R = rem >= 4 ? 4 : (rem >= 2 ? 2 : 1);
    launch_layers(c, row0, R);
    launch_lm_head(c, row0, R);
    if (c->row_union >= 0) launch_sample_rows(c, row0, R, c->row_union);      // tgx_decode_rows: every row with its own settings
    else launch_sample(c, row0, R, cfg, /*advance_pos=*/true, /*log_step=*/true);
    row0 += R;
  }
}

static bool same_cfg(const tgx_sampler_cfg& a, const tgx_sampler_cfg& b) {
  return a.temperature == b.temperature && a.top_k == b.top_k && a.top_p == b.top_p && a.min_p == b.min_p;
}

// The decode step as a hipGraph, captured once per (batch, sampler config): `steps` consecutive steps per graph — token,
// position and step counter live on the device, so a multi-step graph is the same launch sequence repeated.
static int capture_steps(tgx_ctx* c, const tgx_sampler_cfg& cfg, int steps, hipGraphExec_t* out) {
  hipGraph_t g = nullptr;
  // multi-step graphs serve tgx_decode, which reads the ids from the device log afterwards: no per-step store over PCIe
  c->mirror_to_host = steps == 1;
  HIP_OK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < steps; i++) launch_decode_step(c, cfg);
  const hipError_t cap = hipStreamEndCapture(c->stream, &g);
  c->mirror_to_host = true;
  HIP_OK(c, cap);
  if (c->launch_fault) (void)hipGraphDestroy(g);
  LAUNCH_OK(c);
  HIP_OK(c, hipGraphInstantiate(out, g, nullptr, nullptr, 0));
  (void)hipGraphDestroy(g);
  return TGX_OK;
}

void drop_step_graphs(tgx_ctx* c) {
  bool any = false;
  for (auto& g : c->graph_cache) any |= g.step != nullptr || g.multi != nullptr;
  c->step_graph = nullptr; c->multi_graph = nullptr; c->graph_cur = -1;
  if (!any) return;
  (void)hipStreamSynchronize(c->stream);
  for (auto& g : c->graph_cache) {
    if (g.step) (void)hipGraphExecDestroy(g.step);
    if (g.multi) (void)hipGraphExecDestroy(g.multi);
    g = tgx_ctx::GraphSet{};
  }
}

static int ensure_step_graph(tgx_ctx* c, const tgx_sampler_cfg& cfg, bool want_multi) {
  if (!c->use_graph) return TGX_OK;
  int hit = -1, victim = 0;
  for (int i = 0; i < 6; i++) {
    const tgx_ctx::GraphSet& g = c->graph_cache[i];
    if (g.step && g.batch == c->batch && g.rows == c->row_union && (c->row_union >= 0 || same_cfg(g.cfg, cfg)) && g.direct == c->attn_direct && g.mfma == c->attn_mfma &&
        g.nw4 == c->attn_nw4) { hit = i; break; }
    if (!g.step) victim = i;
    else if (c->graph_cache[victim].step && g.used < c->graph_cache[victim].used) victim = i;
  }
  if (hit < 0) {
    tgx_ctx::GraphSet& g = c->graph_cache[victim];
    c->step_graph = nullptr; c->multi_graph = nullptr; c->graph_cur = -1;     // never left pointing at an evicted or half-captured set
    if (g.step || g.multi) {      // evict the least recently used set (its replays may still be in flight)
      HIP_OK(c, hipStreamSynchronize(c->stream));
      if (g.step) (void)hipGraphExecDestroy(g.step);
      if (g.multi) (void)hipGraphExecDestroy(g.multi);
      g = tgx_ctx::GraphSet{};
    }
    int rc = capture_steps(c, cfg, 1, &g.step);
    if (rc) { g = tgx_ctx::GraphSet{}; return rc; }
    g.batch = c->batch; g.cfg = cfg; g.rows = c->row_union; g.direct = c->attn_direct; g.mfma = c->attn_mfma; g.nw4 = c->attn_nw4;
    g.used = ++c->graph_clock;
    hit = victim;
  }
  tgx_ctx::GraphSet& g = c->graph_cache[hit];
  if (want_multi && !g.multi && c->graph_steps > 1) { int rc = capture_steps(c, cfg, c->graph_steps, &g.multi); if (rc) { g.multi = nullptr; return rc; } }
  g.used = ++c->graph_clock;
  c->graph_cur = hit; c->step_graph = g.step; c->multi_graph = g.multi;
  return TGX_OK;
}

// ---- paged KV: block assignment (include/tgx.h "kv.budget_tokens").  Host-side free list; the device tables are updated by a small launch that carries the
// new entries BY VALUE (stream-ordered behind the launches that still read the old ones; no host buffer has to outlive the call).
struct KvTblUpdate { int n; int idx[16]; int val[16]; };
static __global__ void kv_tbl_set_kernel(int* tbl, KvTblUpdate u) { if ((int)threadIdx.x < u.n) tbl[u.idx[threadIdx.x]] = u.val[threadIdx.x]; }
// (a fork writes whole rows of table entries: more than 16 changes travel 240 at a time)
struct KvTblUpdateWide { int n; int idx[240]; int val[240]; };
static __global__ void kv_tbl_set_wide_kernel(int* tbl, KvTblUpdateWide u) { if ((int)threadIdx.x < u.n) tbl[u.idx[threadIdx.x]] = u.val[threadIdx.x]; }

template <typename U>
static void kv_tbl_push_by(tgx_ctx* c, int* tbl, int idx0, const KvPool::Changes& changes, void (*kernel)(int*, U), size_t per, int threads) {
  for (size_t i = 0; i < changes.size(); i += per) {
    U u{};
    u.n = (int)std::min(per, changes.size() - i);
    for (int k = 0; k < u.n; k++) { u.idx[k] = changes[i + (size_t)k].first - idx0; u.val[k] = changes[i + (size_t)k].second; }
    hipLaunchKernelGGL(kernel, dim3(1), dim3(threads), 0, c->stream, tbl, u);
  }
}
// the table entries a KvPool call wrote (kv_pool.h), into the device table — or into a copy of ONE row of it at `row_copy`, whose entry 0 is flat index idx0
// (tgx_splice_row: every change of the call lies in that row)
static void kv_tbl_push(tgx_ctx* c, const KvPool::Changes& changes, int* row_copy = nullptr, int idx0 = 0) {
  int* const tbl = row_copy ? row_copy : c->kv_tbl;
  if (changes.size() > 16) kv_tbl_push_by(c, tbl, idx0, changes, kv_tbl_set_wide_kernel, 240, 256);
  else kv_tbl_push_by(c, tbl, idx0, changes, kv_tbl_set_kernel, 16, 64);
}

int kv_ensure_blocks(tgx_ctx* c, int row, long long tokens) {
  if (!c->kv_paged) return TGX_OK;
  KvPool::Changes ch;
  const int more = c->kv.blocks_for(tokens) - c->kv.row_blocks(row);
  switch (c->kv.grow(row, tokens, ch)) {
    case KvPool::GROW_BEYOND_TABLE: return set_err(c, TGX_ERR_CONTEXT, "context size exceeded: row %d wants %lld tokens (contextSize %d)", row, tokens, c->d.max_ctx);
    case KvPool::GROW_EXHAUSTED:
      return set_err(c, TGX_ERR_CONTEXT, "KV budget exhausted: row %d needs %d more blocks of %d tokens, %zu free of %d (option kv.budget_tokens = %d)", row, more,
                     tgx::KV_BLOCK, c->kv.free_blocks(), c->kv.n_blocks() - 1, c->kv_budget_tokens);
    default: kv_tbl_push(c, ch); return TGX_OK;
  }
}

// paged KV: a finished row keeps the blocks its length needs; the ones assigned up front for the steps it did not take go back to the pool
static void kv_trim_row(tgx_ctx* c, int row, long long tokens) {
  if (!c->kv_paged) return;
  KvPool::Changes ch;
  c->kv.trim(row, tokens, ch);
  kv_tbl_push(c, ch);
}
static void kv_release_row(tgx_ctx* c, int row) { kv_trim_row(c, row, 0); }       // all of the row's blocks

// one kv_fork_kernel launch: the cache geometry of the context and the span length of n_tok positions filled here, the rest (ids, kv_rows, the state segments) and
// the grid by the caller's `rest`
template <typename F>
static void launch_kv_copy(tgx_ctx* c, long long n_tok, F&& rest) {
  const tgx_model_desc& d = c->d;
  const long long tok_bytes = (long long)d.head_dim * (long long)c->esz;
  const bool v16 = tok_bytes % 16 == 0;
  tgx::KvForkArgs a{};
  a.k = c->slab_k; a.v = c->slab_v; a.kv_heads = d.kv_heads; a.n_spans = d.layers * d.kv_heads;
  if (c->kv_paged) {
    a.head_stride = tgx::KV_BLOCK * tok_bytes; a.id_stride = d.kv_heads * a.head_stride; a.layer_stride = c->kv.n_blocks() * a.id_stride;
  } else {
    a.head_stride = d.max_ctx * tok_bytes; a.layer_stride = d.kv_heads * a.head_stride; a.id_stride = (long long)c->kv_row_elems * (long long)c->esz;
  }
  a.span_vecs = n_tok * tok_bytes / (v16 ? 16 : 4);
  const dim3 grid = rest(a), block(tgx::KV_FORK_THREADS);
  if (v16) hipLaunchKernelGGL(tgx::kv_fork_kernel<tgx::u32x4>, grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL(tgx::kv_fork_kernel<unsigned int>, grid, block, 0, c->stream, a);
}

// the launches of tgx_splice_row (kernels/kv_splice.h): the row's table copied into the staging buffer, and one gather or scatter of a group of layers
static __global__ void kv_tbl_copy_kernel(int* dst, const int* src, int n) {
  for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) dst[i] = src[i];
}
template <int DT, int W>
static void launch_kv_splice_dt(tgx_ctx* c, const tgx::KvSpliceArgs& a, dim3 grid, bool scatter) {
  const dim3 block(tgx::KV_SPLICE_THREADS);
  if (scatter) hipLaunchKernelGGL((tgx::kv_splice_kernel<DT, W, true>), grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL((tgx::kv_splice_kernel<DT, W, false>), grid, block, 0, c->stream, a);
}
static void launch_kv_splice(tgx_ctx* c, const tgx::KvSpliceArgs& a, bool wide, bool scatter) {
  // the grid from the bytes to move, within eight workgroups per CU as launch_kv_fork's.  x: (moved token, chunk) items; y: rows that walk the group's spans
  const long long items = (long long)a.moved * a.chunks, cap = 8ll * c->num_cus;
  const long long gx = (items + tgx::KV_SPLICE_THREADS - 1) / tgx::KV_SPLICE_THREADS;
  const long long gy = std::max<long long>(1, std::min<long long>((long long)a.n_layers * a.kv_heads, cap / gx));
  const dim3 grid((unsigned)gx, (unsigned)gy);
  TGX_DT_SWITCH(c->dt, if (wide) launch_kv_splice_dt<DT, 4>(c, a, grid, scatter); else launch_kv_splice_dt<DT, 1>(c, a, grid, scatter));
}

// ---- per-row request state (tgx_set_row_sampler / tgx_set_row_stop / tgx_decode_rows): host-side fields travel BY VALUE in a one-thread launch, stream-ordered
// behind the steps that still read the old ones (no stream drain, no host buffer that has to outlive the call).  what: ROWQ_* bits
// (ROWQ_LP: the row's log-probability setting; ROWQ_LPCOUNT: its record count back to 0.  `lp`: the rows' logprob state once it exists (kernels/logprobs.h) — its
// `seen` word follows `produced` wherever this launch moves that)
enum { ROWQ_SAMPLER = 1, ROWQ_STOP = 2, ROWQ_STATE = 4, ROWQ_LP = 8, ROWQ_LPCOUNT = 16, ROWQ_PROC = 32, ROWQ_AUTO = 64 };      // (ROWQ_PROC: the logit processors' settings; ROWQ_AUTO: the row's automaton table and state word)
struct RowReqUpdate { int row, what; tgx::RowReq v; };
static __global__ void row_req_set_kernel(tgx::RowReq* req, RowReqUpdate u, tgx::LpRow* lp) {
  if (threadIdx.x != 0) return;
  tgx::RowReq& q = req[u.row];
  if (u.what & ROWQ_SAMPLER) { q.temperature = u.v.temperature; q.top_k = u.v.top_k; q.top_p = u.v.top_p; q.min_p = u.v.min_p; q.seed = u.v.seed; }
  if (u.what & ROWQ_STOP) {
    q.max_new = u.v.max_new; q.n_stop = u.v.n_stop;
    for (int k = 0; k < tgx::ROW_MAX_STOP; k++) q.stop[k] = u.v.stop[k];
    q.produced = 0;
  }
  if (u.what & ROWQ_STATE) { q.produced = 0; q.finished = 0; }
  if (u.what & ROWQ_LP) q.lp = u.v.lp;
  if (u.what & ROWQ_PROC) { q.proc = u.v.proc; q.n_bias = u.v.n_bias; q.repetition = u.v.repetition; q.presence = u.v.presence; q.frequency = u.v.frequency; }
  if (u.what & ROWQ_AUTO) { q.auto_next = u.v.auto_next; q.auto_state = u.v.auto_state; }
  if (lp) {
    lp[u.row].seen = q.produced;
    if (u.what & ROWQ_LPCOUNT) { lp[u.row].count = 0; lp[u.row].arrive = 0; }
  }
}
static_assert(tgx::ROW_MAX_STOP == TGX_MAX_STOP_IDS, "kernels/common.h RowReq");

static tgx::RowReq row_req_default() {   // greedy, seed 0, no stop conditions
  tgx::RowReq q{};
  q.temperature = 0.f; q.top_k = 0; q.top_p = 1.f; q.min_p = 0.f; q.seed = 0; q.max_new = 0; q.n_stop = 0;
  q.proc = 0; q.n_bias = 0; q.repetition = 1.f; q.presence = 0.f; q.frequency = 0.f;      // logit processors off
  q.auto_next = nullptr; q.auto_state = 0;                                                   // ... no automaton
  return q;
}
static void row_proc_refresh(tgx::RowReq& q) {      // proc: which processors are on (0: none — the row is copied through)
  const bool pen = q.repetition != 1.f || q.presence != 0.f || q.frequency != 0.f;
  q.proc = (pen ? tgx::PROC_PENALTY : 0) | (q.n_bias > 0 ? tgx::PROC_BIAS : 0) | (q.auto_next ? tgx::PROC_AUTOMATON : 0);
}
// does the row record log-probabilities in the steps: its setting, unless it is retired (the setting is kept on the host and travels with the admission)
bool row_records(const tgx_ctx* c, int row) { return c->row_req_host[(size_t)row].lp > 0 && !c->row_host[(size_t)row].idle; }
static void row_req_push(tgx_ctx* c, int row, int what) {
  RowReqUpdate u{};
  u.row = row; u.what = what; u.v = c->row_req_host[(size_t)row];
  if (!row_records(c, row)) u.v.lp = 0;      // a retired row rides along in the steps and counts what it publishes: on the device its setting reads "off" until it is refilled
  if (!row_processed(c, row)) u.v.proc = 0;  // ... and so do its logit processors: a retired row neither counts into the history the caller stated for its next sequence nor processes
  hipLaunchKernelGGL(row_req_set_kernel, dim3(1), dim3(64), 0, c->stream, c->row_req, u, c->lp_rows);
}
static void row_req_reset(tgx_ctx* c, int row) {   // tgx_reset_row: the default settings and a fresh state
  c->row_req_host[(size_t)row] = row_req_default();
  row_req_push(c, row, ROWQ_SAMPLER | ROWQ_STOP | ROWQ_STATE | ROWQ_LP | ROWQ_LPCOUNT | ROWQ_PROC | ROWQ_AUTO);
  c->row_host[(size_t)row].lp_count = 0;
  c->row_host[(size_t)row].auto_id = -1;      // (the table lives on: tgx_automaton_destroy)
}
static tgx_sampler_cfg row_cfg(const tgx_ctx* c, int row) {
  const tgx::RowReq& q = c->row_req_host[(size_t)row];
  tgx_sampler_cfg s{};
  s.temperature = q.temperature; s.top_k = q.top_k; s.top_p = q.top_p; s.min_p = q.min_p;
  return s;
}
static int nologits_row(const tgx_ctx* c) {   // a live row of the batch that was truncated and not extended since (tgx_truncate_row), or -1
  for (int b = 0; b < c->batch; b++) if (c->row_host[(size_t)b].nologits && !c->row_host[(size_t)b].idle) return b;
  return -1;
}
#define REFUSE_NOLOGITS(c, what)                                                                                                                     \
  do {                                                                                                                                               \
    if (nologits_row(c) >= 0) return set_err((c), TGX_ERR_STATE, "%s: row %d was truncated and holds no logits: tgx_extend_row it first", what, nologits_row(c)); \
  } while (0)
static int finished_row(const tgx_ctx* c) {   // a live row of the batch that finished on the device, or -1
  for (int b = 0; b < c->batch; b++) if (c->row_host[(size_t)b].fin && !c->row_host[(size_t)b].idle) return b;
  return -1;
}

// tgx_read_probs evaluates a row's final probabilities on demand: does any row of the batch hold the vector of a sampled step? ...
static void refresh_have_probs(tgx_ctx* c) {
  c->have_probs = false;
  for (int b = 0; b < c->batch; b++) c->have_probs = c->have_probs || c->row_host[(size_t)b].probs_ok;
}
// ... and remember what a row's last sampled step was configured with
static void note_sampled(tgx_ctx* c, int row0, int R, const tgx_sampler_cfg& cfg) {
  const bool sampled = !is_greedy(&cfg);
  for (int b = row0; b < row0 + R; b++) { c->row_host[(size_t)b].probs_cfg = cfg; c->row_host[(size_t)b].probs_ok = sampled; c->row_host[(size_t)b].probs_proc = false; }
  refresh_have_probs(c);
}

// the engine passes one seed for a whole generation (the draw mixes in position and row): only a CHANGED seed is copied — and that
// copy must drain the stream, because steps already enqueued still read the old word.  With an unchanged seed tgx_step_async returns
// without waiting for the previous step (the one-step lookahead of generateAsync, GPTEngine.cpp:196-217)
static int ensure_seed(tgx_ctx* c, const tgx_sampler_cfg& cfg, uint64_t seed) {
  const unsigned long long s = seed;
  if (is_greedy(&cfg) || (c->seed_valid && c->seed_on_dev == s)) return TGX_OK;
  HIP_OK(c, hipStreamSynchronize(c->stream));
  HIP_OK(c, hipMemcpy(c->seed_dev, &s, 8, hipMemcpyHostToDevice));
  c->seed_on_dev = s; c->seed_valid = true;
  return TGX_OK;
}

// the end of a sequence of eager launches: a launcher that could not issue a kernel fails the call — the kernels issued before the fault advanced the device-side
// state (position words, caches), so nothing of the failed pass stays in flight and the context is poisoned
static int launches_ok(tgx_ctx* c) {
  HIP_OK(c, hipGetLastError());
  if (c->launch_fault) { (void)hipStreamSynchronize(c->stream); c->poisoned = true; }
  LAUNCH_OK(c);
  return TGX_OK;
}
// ... of a prompt pass: the caller's host buffers (ids, tables) may be pageable and reused once the entry point returns
static int finish_pass(tgx_ctx* c) {
  const int rc = launches_ok(c);
  if (rc) return rc;
  HIP_OK(c, hipStreamSynchronize(c->stream));
  return TGX_OK;
}

// n steps of the token-log ring [log_cap][batch] from step `start` on (the ring wraps: two pieces), stream-ordered; the caller synchronises
static int read_tok_log(tgx_ctx* c, int64_t start, int n, int* dst) {
  const size_t B = (size_t)c->batch;
  const int64_t s0 = start % c->log_cap, first = std::min<int64_t>(n, c->log_cap - s0);
  HIP_OK(c, hipMemcpyAsync(dst, c->tok_log + (size_t)s0 * B, (size_t)first * B * 4, hipMemcpyDeviceToHost, c->stream));
  if (first < n) HIP_OK(c, hipMemcpyAsync(dst + (size_t)first * B, c->tok_log, (size_t)(n - first) * B * 4, hipMemcpyDeviceToHost, c->stream));
  return TGX_OK;
}

// rows mode (c->row_union >= 0, tgx_decode_rows): every row samples with its own settings, `cfg` and `seed` are unused, finished rows take no blocks and stay
// where they are, and the caller updates the rows' `past` from the device afterwards (rows may finish on the device)
static int run_decode_steps(tgx_ctx* c, const tgx_sampler_cfg& cfg, uint64_t seed, int n) {
  const bool rows = c->row_union >= 0;
  if (c->kv_paged) {     // every live row's next n positions have a block before the steps that write them are enqueued
    // all or nothing: the blocks of ALL the rows against the free list before any is assigned — a call refused at its third row must not leave the first two
    // holding blocks for steps that never ran (kv.free_tokens would read low until those rows are reset)
    long long need = 0;
    for (int b = 0; b < c->batch; b++)
      if (!c->row_host[(size_t)b].idle && !c->row_host[(size_t)b].fin) need += std::max(0, c->kv.blocks_for(c->row_host[(size_t)b].past + n) - c->kv.row_blocks(b));
    if (need > (long long)c->kv.free_blocks())
      return set_err(c, TGX_ERR_CONTEXT, "KV budget exhausted: %d more steps need %lld more blocks of %d tokens, %zu free of %d (option kv.budget_tokens = %d)", n, need, tgx::KV_BLOCK,
                     c->kv.free_blocks(), c->kv.n_blocks() - 1, c->kv_budget_tokens);
    for (int b = 0; b < c->batch; b++)
      if (!c->row_host[(size_t)b].idle && !c->row_host[(size_t)b].fin) { int rc = kv_ensure_blocks(c, b, c->row_host[(size_t)b].past + n); if (rc) return rc; }
  }
  if (rows) {
    for (int b = 0; b < c->batch; b++) { note_sampled(c, b, 1, row_cfg(c, b)); c->row_host[(size_t)b].probs_proc = (c->row_union & ROWU_PROC) != 0; }      // (a processed step passes every row through the processed slab)
  } else if (int rc = ensure_seed(c, cfg, seed)) return rc;
  if (!rows) note_sampled(c, 0, c->batch, cfg);
  if (decode_mfma_ok(c)) {   // the batched step's workspace must exist before the step is captured
    int rc = ensure_skinny_ws(c, std::min(c->decode_step_rows, c->batch));
    if (rc) return rc;
  }
  // a retired row rides along from wherever its position word stands (RowHost::past mirrors it); the attention form and the capacity check are chosen for the
  // longest LIVE row, so an idle row that has outrun it (the longer rows were retired since) restarts from position 0
  for (int b = 0; b < c->batch; b++)
    if (c->row_host[(size_t)b].idle && c->row_host[(size_t)b].past > c->past) {
      HIP_OK(c, hipMemsetAsync(c->rows[(size_t)b].pos, 0, 4, c->stream));
      c->row_host[(size_t)b].past = 0;
    }
  // a finished row rides at its own length (it does not count for `past`): the attention form is chosen for it as well when it is the longest
  if (rows)
    for (int b = 0; b < c->batch; b++)
      if (c->row_host[(size_t)b].fin && !c->row_host[(size_t)b].idle) c->past = std::max(c->past, c->row_host[(size_t)b].past);
  // The attention form depends on the context (four-wave direct / sixteen-wave direct / split + combine / matrix cores): a call that crosses a limit is
  // issued in chunks, each on the form of its own contexts, from the cache of captured graphs
  int remaining = n;
  while (remaining > 0) {
    int m = remaining;
    const long long lims[2] = {nw4_limit(c, c->batch, true), direct_limit(c, c->batch, true)};
    for (long long lim : lims)
      if (lim > 0 && c->past + 1 <= lim && c->past + m > lim) m = (int)(lim - c->past);
    update_attn_modes(c, c->past, m);
    if (c->use_graph) {
      const int K = c->graph_steps;
      // any multi-step call captures the K-step graph as well (a short warm-up call then leaves nothing to capture inside a later, longer
      // call); one-step streaming calls never pay for it
      int rc = ensure_step_graph(c, cfg, /*want_multi=*/m >= 2);
      if (rc) return rc;
      int i = 0;
      if (c->multi_graph) for (; i + K <= m; i += K) HIP_OK(c, hipGraphLaunch(c->multi_graph, c->stream));
      for (; i < m; i++) HIP_OK(c, hipGraphLaunch(c->step_graph, c->stream));
    } else {
      for (int i = 0; i < m; i++) launch_decode_step(c, cfg);
      if (int rc = launches_ok(c)) return rc;
    }
    c->past += m;
    if (!rows) for (int b = 0; b < c->batch; b++) c->row_host[(size_t)b].past += m;
    c->steps_issued += m;
    remaining -= m;
  }
  return TGX_OK;
}

// ---- prompt passes (tgx_forward, tgx_forward_row, tgx_forward_rows) ------------------------------------------------------------------------------------------
// The route of a prefill pass.  len: the prompt length the thresholds are tested against; rows: the workspace rows of the pass (tgx_forward: len = seq for a stack of
// rows = nb * seq; a ragged pass of tgx_forward_rows: both its M).
//   STEPS   through the decode kernels, up to 4 positions per pass: prompts shorter than 4 tokens / prefill_min_rows, fp32 storage below prefill_f32_min_rows, shapes the GEMM tile does not cover
//   F32     fp32 storage through the f32-input MFMA (prefill_f32.hip)
//   SKINNY  16-bit storage, a few rows: the weight stream of a decode step (skinny.hip; limits measured in ctx.h at prefill_skinny_rows)
//   TILED   16-bit storage through the split-term GEMMs (prefill.hip; every family incl. GPT-2)
enum PrefillRoute { ROUTE_STEPS, ROUTE_F32, ROUTE_SKINNY, ROUTE_TILED };
// 65-128 rows take the skinny route (eight blocks, LDS-DMA ring kernel only) up to this hidden size.  Measured ms per prompt, skinny / tiled: Llama-3.2-1B S = 65
// 1.65 / 1.89, 96 1.71 / 1.96, 128 1.82 / 2.05; Mistral-7B S = 96 8.01 / 7.56
constexpr int SKINNY_HIDDEN_MAX_WIDE = 2048;
static PrefillRoute prefill_route(const tgx_ctx* c, int len, int rows) {
  if (!c->prefill_mfma) return ROUTE_STEPS;
  if (c->dt == tgx::DT_F32) return len >= c->prefill_f32_min_rows ? ROUTE_F32 : ROUTE_STEPS;
  if (len < std::max(4, c->prefill_min_rows) || !prefill_shapes_ok(c->d)) return ROUTE_STEPS;
  const bool skinny = !c->gpt2 && c->prefill_skinny && c->d.vocab >= 128 &&
                      (rows <= 32 ? c->prefill_skinny_rows >= rows : (rows <= c->prefill_skinny_rows && c->d.hidden <= c->prefill_skinny_hidden_max && (rows <= 64 || (c->skinny_dma && c->d.hidden <= SKINNY_HIDDEN_MAX_WIDE))));
  return skinny ? ROUTE_SKINNY : ROUTE_TILED;
}

// the workspace of a matrix-core route for M rows, then its launches: NB rows [row0, row0 + NB) of S positions from `past`, or the ragged pass rg
static int launch_route(tgx_ctx* c, PrefillRoute rt, int M, int row0, int NB, int S, int past, const RaggedPass* rg = nullptr) {
  int rc = rt == ROUTE_SKINNY ? ensure_skinny_ws(c, M) : ensure_prefill_ws(c, M);
  if (!rc && rt == ROUTE_F32) rc = ensure_f32_part(c, M);
  if (rc) return rc;
  if (rt == ROUTE_F32) launch_prefill_f32(c, row0, NB, S, past);
  else if (rt == ROUTE_SKINNY) launch_prefill_skinny(c, row0, NB, S, past, rg);
  else if (rg) launch_prefill_ragged(c, *rg);
  else launch_prefill(c, row0, NB, S, past);
  return TGX_OK;
}

// tgx_verify_row: the logits and argmax partials of ALL M positions of a one-row pass into the vf_* workspace.  The skinny route's final residual rows (ws_x) go
// through the batched step's one-pass lm_head; every other route stages its hidden rows in vf_x (the matrix-core routes' ws_x here, prefill by steps chunk by chunk)
// and runs the GEMV lm_head four rows per pass over the weights (a group of three rides as four: vf_x holds VERIFY_ROWS rows, the fourth's results are not read)
// (src: the M hidden rows of a matrix-core route, default the first M of ws_x — a scoring pass feeds it one group of positions at a time)
// (joint: tgx_verify_rows' joint pass — the M <= VERIFY_POSITIONS positions of all its rows into the vj_* workspace, the same two forms)
static void launch_lm_head_all(tgx_ctx* c, PrefillRoute rt, int M, float* src = nullptr, bool joint = false) {
  const size_t H = (size_t)c->d.hidden, V = (size_t)c->d.vocab, P = (size_t)c->lm_grid;
  float* const x = joint ? c->vj_x : c->vf_x;
  float* const logits = joint ? c->vj_logits : c->vf_logits;
  float* const part_val = joint ? c->vj_part_val : c->vf_part_val;
  int* const part_idx = joint ? c->vj_part_idx : c->vf_part_idx;
  if (rt == ROUTE_SKINNY) { launch_lm_head_skinny(c, M, logits, part_val, part_idx, src); return; }
  if (rt != ROUTE_STEPS) (void)hipMemcpyAsync(x, src ? src : c->ws_x, (size_t)M * H * 4, hipMemcpyDeviceToDevice, c->stream);
  for (int m0 = 0; m0 < M;) {
    const int rem = M - m0, R = rem >= 3 ? 4 : rem;
    launch_lm_head_at(c, x + m0 * H, logits + m0 * V, part_val + m0 * P, part_idx + m0 * P, R);
    m0 += R;
  }
}

// tgx_score_row on the routes without the matrix-core form: the R <= VERIFY_ROWS positions from g0 through the verify form's lm_head into the vf_* workspace
// (hidden: their rows of ws_x; nullptr: staged in vf_x already, prefill by steps), then the tile and record launches of kernels/score.h over it
static void launch_score_group(tgx_ctx* c, PrefillRoute rt, const ScoreCall& sc, int g0, int R, float* hidden) {
  c->vf_pass_rows = 0;                     // the workspace no longer holds a verify pass (tgx_read_pass_logits)
  launch_lm_head_all(c, rt, R, hidden);
  launch_score_tiles(c, sc, c->vf_logits, c->d.vocab, 0, c->d.vocab, R, g0);
  launch_score_record(c, sc, R, g0);
}

// One pass of nb rows [row0, row0 + nb) over positions past .. past + seq - 1 of each (their ids are in rows[].prompt, their blocks assigned); leaves every row's
// logits and advances its position word.  `past` is an argument: tgx_forward passes the batch's pastLength, an admission 0 whatever the other rows hold.
// verify (tgx_verify_row, nb == 1): the same pass, but the logits of EVERY position land in the vf_* workspace (launch_lm_head_all) and neither the row's logits
// slot nor its position word moves — the accept launch behind the pass writes both
// sc (tgx_score_row, nb == 1): the plain pass, and behind it every position's score — the matrix-core form over ws_x on ROUTE_TILED (prefill.hip
// launch_score_tiled), groups of VERIFY_ROWS positions on every other route (prefill by steps scores each group as its chunks complete)
// em (tgx_embed_rows, nb == 1, past == 0): the pass WITHOUT its lm_head — the row's logits slot is not written — and behind it the pooled partials of text em->cur
// (kernels/embed_pool.h): one launch over ws_x on the matrix-core routes; prefill by steps copies its chunks' pooled rows into the staging slice and launches
// the same kernel per completed slice, so the slices hold the sums of the same positions in the same order on every route
static int issue_pass(tgx_ctx* c, int row0, int nb, int seq, int past, bool verify = false, const ScoreCall* sc = nullptr, const EmbedCall* em = nullptr) {
  if (sc && sc->n_score < 1) sc = nullptr;      // (one position: nothing to score)
  constexpr int SG = tgx_ctx::VERIFY_ROWS;
  const PrefillRoute rt = prefill_route(c, seq, nb * seq);
  if (rt != ROUTE_STEPS) {
    // batched prefill on the matrix cores; logits for the last position only (== forward + narrow, GPTEngine.cpp:96-97)
    const int rc = launch_route(c, rt, nb * seq, row0, nb, seq, past);
    if (rc) return rc;
    if (verify) { launch_lm_head_all(c, rt, seq); return TGX_OK; }
    for (int b = row0; b < row0 + nb && !em;) {
      const int rem = row0 + nb - b, R = rem >= 4 ? 4 : (rem >= 2 ? 2 : 1);
      launch_lm_head(c, b, R);
      b += R;
    }
    for (int b = row0; b < row0 + nb; b++) launch_add_pos(c, c->rows[(size_t)b].pos, seq);
    if (em) launch_embed_pool(c, *em, em->cur, 1);
    if (sc && rt == ROUTE_TILED) launch_score_tiled(c, *sc);
    else if (sc)
      for (int g0 = 0; g0 < sc->n_score; g0 += SG) launch_score_group(c, rt, *sc, g0, std::min(SG, sc->n_score - g0), c->ws_x + (size_t)g0 * c->d.hidden);
    return TGX_OK;
  }
  for (int b = row0; b < row0 + nb; b++) {
    RowState& r = c->rows[(size_t)b];
    // prefill by steps: up to 4 consecutive positions per pass through the decode kernels — the chunk rows share this row's cache (kv_stride 0), each attends the
    // keys up to its own position, so the result equals position-by-position passes at a quarter of the weight traffic
    update_attn_modes(c, past, seq, 1, /*step=*/false);      // the chunk rows of a pass are positions of ONE sequence
    for (int s0 = 0; s0 < seq;) {
      const int rem = seq - s0, R = rem >= 4 ? 4 : (rem >= 2 ? 2 : 1);
      launch_embed_chunk(c, r.prompt + s0, R, past + s0);
      for (int k = 0; k < R; k++) { c->chunk[k].kcache = r.kcache; c->chunk[k].vcache = r.vcache; c->chunk[k].tbl = r.tbl; }
      launch_layers(c, c->chunk, R, 0);
      s0 += R;
      if (verify) {                                      // every position's hidden state feeds lm_head
        (void)hipMemcpyAsync(c->vf_x + (size_t)(s0 - R) * c->d.hidden, c->ch_x, (size_t)R * c->d.hidden * 4, hipMemcpyDeviceToDevice, c->stream);
        if (s0 == seq) launch_lm_head_all(c, rt, seq);
        continue;
      }
      if (sc) {                                          // the chunk's hidden rows into their group's slots; a complete group (chunks of four: its boundary is a chunk's) is scored at once
        const int g0 = (s0 - R) / SG * SG;
        (void)hipMemcpyAsync(c->vf_x + (size_t)(s0 - R - g0) * c->d.hidden, c->ch_x, (size_t)R * c->d.hidden * 4, hipMemcpyDeviceToDevice, c->stream);
        if ((s0 % SG == 0 || s0 == seq) && g0 < sc->n_score) launch_score_group(c, rt, *sc, g0, std::min(s0, sc->n_score) - g0, nullptr);
      }
      if (em) {                                          // the chunk's pooled positions into the staging slice; a slice that is complete, or the text's last, is summed
        const int p_first = em->pool == TGX_POOL_MEAN || em->pool == TGX_POOL_FIRST ? 0 : seq - 1, np = em->np(em->cur);
        for (int p = s0 - R; p < s0; p++) {
          const int q = p - p_first;                     // index among the pooled positions
          if (q < 0 || q >= np) continue;
          (void)hipMemcpyAsync(c->em_stage + (size_t)(q % EmbedCall::SLICE) * c->d.hidden, c->ch_x + (size_t)(p - (s0 - R)) * c->d.hidden, (size_t)c->d.hidden * 4, hipMemcpyDeviceToDevice, c->stream);
          if ((q + 1) % EmbedCall::SLICE == 0 || q == np - 1) launch_embed_pool_stage(c, *em, em->cur, q / EmbedCall::SLICE, q % EmbedCall::SLICE + 1);
        }
      }
      if (s0 == seq) {                                   // the last position's hidden state feeds lm_head; publish token and length
        (void)hipMemcpyAsync(r.x, c->chunk[R - 1].x, (size_t)c->d.hidden * 4, hipMemcpyDeviceToDevice, c->stream);
        launch_add_pos(c, r.pos, seq);
        if (!em) launch_lm_head(c, b, 1);
      }
    }
  }
  return TGX_OK;
}

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int tgx_abi_version(void) { return TGX_ABI_VERSION; }

int tgx_device_count(int* out_count) {
  if (!out_count) return TGX_ERR_INVALID;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *out_count = 0; return set_err(nullptr, TGX_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
  *out_count = n;
  return TGX_OK;
}

const char* tgx_last_error(const tgx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int tgx_create(const tgx_model_desc* desc, int device_ordinal, tgx_ctx** out_ctx) {
  if (!desc || !out_ctx) return set_err(nullptr, TGX_ERR_INVALID, "null argument");
  *out_ctx = nullptr;
  const tgx_model_desc& d = *desc;
  if (d.family != TGX_FAMILY_LLAMA && d.family != TGX_FAMILY_QWEN2 && d.family != TGX_FAMILY_MISTRAL && d.family != TGX_FAMILY_QWEN3 && d.family != TGX_FAMILY_GPT2)
    return set_err(nullptr, TGX_ERR_UNSUPPORTED, "family %d is not implemented on mi355x (gpt2/llama/qwen2/qwen3/mistral are)", d.family);
  const bool gpt2 = d.family == TGX_FAMILY_GPT2;
  if (gpt2 && (d.kv_heads != d.heads || d.heads * d.head_dim != d.hidden)) return set_err(nullptr, TGX_ERR_INVALID, "gpt2: n_head * head_dim must equal n_embd, no grouped heads");
  if (gpt2 && d.hidden > 2048) return set_err(nullptr, TGX_ERR_UNSUPPORTED, "gpt2: n_embd %d > 2048 (the LayerNorm-fused launches are built for up to 4 slices per lane)", d.hidden);
  if (gpt2 && d.n_positions < d.max_ctx) return set_err(nullptr, TGX_ERR_INVALID, "gpt2: n_positions %d < context size %d", d.n_positions, d.max_ctx);
  if (gpt2 && d.qk_norm) return set_err(nullptr, TGX_ERR_INVALID, "gpt2 has no q/k norm");
  if (d.compute_dtype != TGX_BF16 && d.compute_dtype != TGX_F16 && d.compute_dtype != TGX_F32) return set_err(nullptr, TGX_ERR_INVALID, "unknown compute dtype %d", d.compute_dtype);
  if (d.head_dim != 64 && d.head_dim != 128) return set_err(nullptr, TGX_ERR_UNSUPPORTED, "head_dim %d (64 and 128 are built)", d.head_dim);
  if (d.heads <= 0 || d.kv_heads <= 0 || d.heads % d.kv_heads) return set_err(nullptr, TGX_ERR_INVALID, "heads %% kv_heads != 0");
  if (d.heads / d.kv_heads > 16) return set_err(nullptr, TGX_ERR_UNSUPPORTED, "GQA group size %d > 16", d.heads / d.kv_heads);
  if (d.hidden % 8 || d.inter % 8 || (d.heads * d.head_dim) % 8) return set_err(nullptr, TGX_ERR_UNSUPPORTED, "hidden/intermediate sizes must be multiples of 8");
  if (d.hidden <= 0 || d.layers <= 0 || d.inter <= 0 || d.vocab <= 0 || d.max_ctx <= 0) return set_err(nullptr, TGX_ERR_INVALID, "non-positive model dimension");
  // a launch keeps its K range in registers: at most 8 slices of 8 elements per lane and 4 waves per row pair = 16384 elements
  if (d.hidden > 16384) return set_err(nullptr, TGX_ERR_UNSUPPORTED, "hidden_size %d > 16384", d.hidden);
  if (d.inter > 65536 || d.heads * d.head_dim > 16384) return set_err(nullptr, TGX_ERR_UNSUPPORTED, "projection input wider than 65536 (intermediate) / 16384 (heads * head_dim)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_err(nullptr, TGX_ERR_DEVICE, "no HIP device visible (--device mi355x needs a GPU; there is no CPU fallback)");
  if (device_ordinal < 0 || device_ordinal >= ndev) return set_err(nullptr, TGX_ERR_INVALID, "device ordinal %d out of range [0,%d)", device_ordinal, ndev);

  tgx_ctx* c = new (std::nothrow) tgx_ctx();
  if (!c) return set_err(nullptr, TGX_ERR_NOMEM, "host allocation failed");
  *out_ctx = c;
  c->d = d;
  c->gpt2 = gpt2;
  if (gpt2) { c->d.tied = 1; c->d.qkv_bias = 1; }     // the head is wte (ModelGPT2.h:170-176); every Conv1D has a bias
  if (c->d.max_batch < 1) c->d.max_batch = 1;
  c->device = device_ordinal;
  c->dt = d.compute_dtype == TGX_BF16 ? tgx::DT_BF16 : (d.compute_dtype == TGX_F16 ? tgx::DT_F16 : tgx::DT_F32);
  c->esz = d.compute_dtype == TGX_F32 ? 4 : 2;
  HIP_OK(c, hipSetDevice(device_ordinal));
  hipDeviceProp_t prop;
  HIP_OK(c, hipGetDeviceProperties(&prop, device_ordinal));
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HIP_OK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  if (const char* e = getenv("TGX_NO_GRAPH")) c->use_graph = !(e[0] == '1');
  if (const char* e = getenv("TGX_PACKED_CLASSES")) c->packed_classes = atoi(e) & 7;      // experiments (A/B per class under an unchanged bench.py): option weights.packed_classes
  // measured crossover of the direct and the split attention (tools/sweep.py --grid attn.direct_max=0,100000): context ~850-1100 at
  // head_dim 64 (Qwen2.5-0.5B, Llama-3.2-1B), ~500 at 128 (Mistral-7B: half the tokens per wave-load)
  // round 4 (the split form lost its combine launch to the K-sliced o_proj, the 16-wave direct form its per-wave merge): Llama-3.2-1B 0.652 / 0.654 ms/token
  // split / direct at context 700, 0.654 / 0.667 at 1000; Qwen2.5-0.5B (2 kv heads: few split workgroups) 0.591 / 0.586 at 700, 0.591 / 0.600 at 1000
  c->attn_direct_max = d.head_dim == 64 ? (d.kv_heads >= 8 ? 576 : 832) : 384;
  // four waves per head up to 256 keys at head_dim 64 (Qwen2.5-0.5B 16-token prompt 0.579 -> 0.565 ms/token, Llama-3.2-1B 0.648 -> 0.634; from ~256 keys and at head_dim 128 the sixteen-wave form is ahead)
  c->attn_direct_nw4 = d.head_dim == 64 ? 192 : 0;      // (round 4: equal at ~220 keys, the sixteen-wave form ahead from ~300)
  // very short prompts: ONE pass through the batched decode kernels (4 positions) still beats the skinny MFMA prefill on small models
  // (Llama-3.2-1B: S = 4 1.00 vs 1.07 ms, S = 5 1.55 vs 1.07; Mistral-7B S = 4 4.65 vs 4.09) — tools/prefill_crossover.py, profiles/r02_prefill_short.txt
  c->prefill_min_rows = d.hidden > 2048 ? 4 : 5;
  // the packed gate_up launch at 3 workgroups per CU (768 on 256 CUs: its waves take 3, 3, 2 units instead of 2 each): Llama-3.2-1B 0.6295 -> 0.6162 ms per token,
  // -13 us over 16 launches; packed down and lm_head are best at 4 (profiles/packed_kpart_geometry.txt section 4)
  c->tune[TGX_KERNEL_GATEUP].packed_bpc = 3;
  c->tune[TGX_KERNEL_DOWN].ks = d.inter >= 8192 ? 4 : 2;  // K = intermediate_size: 4 waves split each row pair (2 below 8192 columns: Qwen2.5-0.5B 0.549 -> 0.542 ms/token, tools/sweep.py round 4)
  // qkv is the most latency-bound launch (few rows): 4 waves per row pair shorten every wave's load -> reduce chain; measured
  // ks 1 -> 4: Llama-3.2-1B 1395 -> 1411 tok/s, 3B 628 -> 637, Mistral-7B 341 -> 347; hidden 896 (Qwen2.5-0.5B) loses 2 %
  c->tune[TGX_KERNEL_QKV].ks = d.hidden >= 2048 ? 4 : 1;
  // fp32 storage (round 4, tools/sweep.py --dtype fp32): a row pair is twice the bytes — two waves per pair for gate_up / c_fc and o_proj: GPT-2 124M 0.3205 -> 0.3133 ms per
  // token (with qkv as well: 0.3104), Llama-3.2-1B 1.145 -> 1.124, Qwen2.5-0.5B 0.752 -> 0.739; 16-bit storage: no gain
  if (c->dt == tgx::DT_F32) {
    c->tune[TGX_KERNEL_GATEUP].ks = 2; c->tune[TGX_KERNEL_OPROJ].ks = 2;
    if (c->gpt2) c->tune[TGX_KERNEL_QKV].ks = 2;
  }

  const int H = d.hidden, I = d.inter, V = d.vocab, qd = d.heads * d.head_dim, kvd = d.kv_heads * d.head_dim;
  int rc;
  const size_t es = c->esz;
  if ((rc = dev_alloc(c, &c->embed, (size_t)V * H * es))) return rc;
  if (!c->d.tied && (rc = dev_alloc(c, &c->lm_head, (size_t)V * H * es))) return rc;
  if ((rc = dev_alloc(c, &c->final_norm, (size_t)H * es))) return rc;
  if (gpt2 && ((rc = dev_alloc(c, &c->wpe, (size_t)d.n_positions * H * es)) || (rc = dev_alloc(c, &c->final_norm_b, (size_t)H * es)))) return rc;
  c->L.resize((size_t)d.layers);
  for (auto& w : c->L) {
    if ((rc = dev_alloc(c, &w.in_norm, (size_t)H * es))) return rc;
    if ((rc = dev_alloc(c, &w.post_norm, (size_t)H * es))) return rc;
    if ((rc = dev_alloc(c, &w.wqkv, (size_t)(qd + 2 * kvd) * H * es))) return rc;
    if (c->d.qkv_bias && (rc = dev_alloc(c, &w.bqkv, (size_t)(qd + 2 * kvd) * es))) return rc;
    if ((rc = dev_alloc(c, &w.wo, (size_t)H * qd * es))) return rc;
    if (d.qk_norm && ((rc = dev_alloc(c, &w.q_norm, (size_t)d.head_dim * es)) || (rc = dev_alloc(c, &w.k_norm, (size_t)d.head_dim * es)))) return rc;
    if ((rc = dev_alloc(c, &w.wgu, (size_t)(gpt2 ? 1 : 2) * I * H * es))) return rc;
    if ((rc = dev_alloc(c, &w.wdown, (size_t)H * I * es))) return rc;
    if (gpt2 && ((rc = dev_alloc(c, &w.in_norm_b, (size_t)H * es)) || (rc = dev_alloc(c, &w.post_norm_b, (size_t)H * es)) || (rc = dev_alloc(c, &w.bo, (size_t)H * es)) ||
                 (rc = dev_alloc(c, &w.bfc, (size_t)I * es)) || (rc = dev_alloc(c, &w.bdown, (size_t)H * es)))) return rc;
  }
  return TGX_OK;
}

int tgx_upload(tgx_ctx* c, const char* name, const void* host, const int64_t* shape, int nd, int src_dtype) {
  if (!c || !name || !host || !shape) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  HIP_OK(c, hipSetDevice(c->device));
  const tgx_model_desc& d = c->d;
  const int64_t H = d.hidden, I = d.inter, V = d.vocab, qd = (int64_t)d.heads * d.head_dim, kvd = (int64_t)d.kv_heads * d.head_dim;
  auto bad_shape = [&]() { return set_err(c, TGX_ERR_SHAPE, "shape not equal for tensor: %s", name); };
  if (c->gpt2) return upload_gpt2(c, name, host, shape, nd, src_dtype);
  if (!strcmp(name, "model.embed_tokens.weight")) {
    if (!shape_is(shape, nd, V, H)) return bad_shape();
    c->embed_ok = true;
    return upload_param(c, c->embed, host, V * H, src_dtype);
  }
  if (!strcmp(name, "lm_head.weight")) {
    if (!shape_is(shape, nd, V, H)) return bad_shape();
    if (d.tied) return TGX_OK;   // aliased to embed_tokens (GPTModel.h:39-41)
    c->lm_head_ok = true;
    return upload_param(c, c->lm_head, host, V * H, src_dtype);
  }
  if (!strcmp(name, "model.norm.weight")) {
    if (!shape_is(shape, nd, H, -1)) return bad_shape();
    c->final_norm_ok = true;
    return upload_param(c, c->final_norm, host, H, src_dtype);
  }
  int l = -1;
  char rest[128] = {0};
  if (sscanf(name, "model.layers.%d.%127s", &l, rest) == 2 && l >= 0 && l < d.layers) {
    LayerW& w = c->L[(size_t)l];
    if (!strcmp(rest, "input_layernorm.weight")) {
      if (!shape_is(shape, nd, H, -1)) return bad_shape();
      w.in_norm_ok = true;
      return upload_param(c, w.in_norm, host, H, src_dtype);
    }
    if (d.qk_norm && (!strcmp(rest, "self_attn.q_norm.weight") || !strcmp(rest, "self_attn.k_norm.weight"))) {
      if (!shape_is(shape, nd, d.head_dim, -1)) return bad_shape();
      const bool isq = rest[10] == 'q';
      (isq ? w.q_norm_ok : w.k_norm_ok) = true;
      return upload_param(c, isq ? w.q_norm : w.k_norm, host, d.head_dim, src_dtype);
    }
    if (!strcmp(rest, "post_attention_layernorm.weight")) {
      if (!shape_is(shape, nd, H, -1)) return bad_shape();
      w.post_norm_ok = true;
      return upload_param(c, w.post_norm, host, H, src_dtype);
    }
    // MergedLinear row slices (Linear.h:64-79): [q | k | v] and [gate | up]
    struct Slot { const char* n; ebyte* base; ebyte* bias; int64_t row0, rows, cols; int kind; int bit; };
    const Slot slots[] = {
        {"self_attn.q_proj", w.wqkv, w.bqkv, 0, qd, H, 0, 0},        {"self_attn.k_proj", w.wqkv, w.bqkv, qd, kvd, H, 0, 1},
        {"self_attn.v_proj", w.wqkv, w.bqkv, qd + kvd, kvd, H, 0, 2}, {"self_attn.o_proj", w.wo, nullptr, 0, H, qd, 1, -1},
        {"mlp.gate_proj", w.wgu, nullptr, 0, I, H, 2, 3},             {"mlp.up_proj", w.wgu, nullptr, I, I, H, 2, 4},
        {"mlp.down_proj", w.wdown, nullptr, 0, H, I, 3, -1}};
    for (const Slot& s : slots) {
      const size_t ln = strlen(s.n);
      if (strncmp(rest, s.n, ln) || rest[ln] != '.') continue;
      if (!strcmp(rest + ln + 1, "weight")) {
        if (!shape_is(shape, nd, s.rows, s.cols)) return bad_shape();
        int rc = upload_param(c, s.base + (size_t)(s.row0 * s.cols) * c->esz, host, s.rows * s.cols, src_dtype);
        if (rc) return rc;
        if (s.bit >= 0) w.merged_filled |= 1 << s.bit;
        else if (s.kind == 1) w.wo_ok = true;
        else w.wdown_ok = true;
        return TGX_OK;
      }
      if (!strcmp(rest + ln + 1, "bias") && s.bias) {
        if (!shape_is(shape, nd, s.rows, -1)) return bad_shape();
        w.merged_filled |= 1 << (5 + s.bit);
        return upload_param(c, s.bias + (size_t)s.row0 * c->esz, host, s.rows, src_dtype);
      }
    }
  }
  return set_err(c, TGX_ERR_NAME, "Unexpected key: %s", name);
}

int tgx_finalize(tgx_ctx* c) {
  if (!c) return TGX_ERR_INVALID;
  HIP_OK(c, hipSetDevice(c->device));
  const tgx_model_desc& d = c->d;
  const int H = d.hidden, I = d.inter, V = d.vocab, hd = d.head_dim, qd = d.heads * hd, kvd = d.kv_heads * hd;
  if (c->gpt2) {
    if (!c->embed_ok) return set_err(c, TGX_ERR_STATE, "Missing key: wte.weight");
    if (!c->wpe_ok) return set_err(c, TGX_ERR_STATE, "Missing key: wpe.weight");
    if (!c->final_norm_ok || !c->final_norm_b_ok) return set_err(c, TGX_ERR_STATE, "Missing key: ln_f.%s", c->final_norm_ok ? "bias" : "weight");
    for (int l = 0; l < d.layers; l++)
      if (c->L[(size_t)l].gpt2_filled != 0xfff) return set_err(c, TGX_ERR_STATE, "Missing key in h.%d", l);
  }
  if (!c->gpt2 && !c->embed_ok) return set_err(c, TGX_ERR_STATE, "Missing key: model.embed_tokens.weight");
  if (!d.tied && !c->lm_head_ok) return set_err(c, TGX_ERR_STATE, "Missing key: lm_head.weight");
  if (!c->gpt2 && !c->final_norm_ok) return set_err(c, TGX_ERR_STATE, "Missing key: model.norm.weight");
  for (int l = 0; l < d.layers && !c->gpt2; l++) {
    const LayerW& w = c->L[(size_t)l];
    static const char* merged_names[8] = {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight",
                                          "self_attn.q_proj.bias", "self_attn.k_proj.bias", "self_attn.v_proj.bias"};
    for (int b = 0; b < (d.qkv_bias ? 8 : 5); b++)
      if (!(w.merged_filled & (1 << b))) return set_err(c, TGX_ERR_STATE, "Missing key: model.layers.%d.%s", l, merged_names[b]);
    if (!w.in_norm_ok || !w.post_norm_ok || !w.wo_ok || !w.wdown_ok)
      return set_err(c, TGX_ERR_STATE, "Missing key: model.layers.%d.%s", l, !w.in_norm_ok ? "input_layernorm.weight" : !w.post_norm_ok ? "post_attention_layernorm.weight" : !w.wo_ok ? "self_attn.o_proj.weight" : "mlp.down_proj.weight");
    if (d.qk_norm && (!w.q_norm_ok || !w.k_norm_ok)) return set_err(c, TGX_ERR_STATE, "Missing key: model.layers.%d.self_attn.{q,k}_norm.weight", l);
  }
  if (c->finalized) return TGX_OK;
  // a lossy option that silently does nothing would mislead: the 8-bit form exists for bf16 storage and the RMSNorm families only
  if (c->weights_fp8 && (c->dt != tgx::DT_BF16 || c->gpt2))
    return set_err(c, TGX_ERR_UNSUPPORTED, "weights.fp8 needs bf16 storage and a gated-MLP family (this context: %s%s)", c->dt == tgx::DT_BF16 ? "bf16" : (c->dt == tgx::DT_F16 ? "fp16" : "fp32"), c->gpt2 ? ", GPT-2" : "");

  std::vector<float> cs, sn;
  if (c->gpt2) {      // no rotary embedding: the qkv epilogue's rotation becomes the identity
    cs.assign((size_t)d.max_ctx * (hd / 2), 1.0f);
    sn.assign((size_t)d.max_ctx * (hd / 2), 0.0f);
  } else build_rope_host(d, cs, sn);
  int rc;
  if ((rc = dev_alloc(c, &c->rope_cos, cs.size()))) return rc;
  if ((rc = dev_alloc(c, &c->rope_sin, sn.size()))) return rc;
  HIP_OK(c, hipMemcpy(c->rope_cos, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(c, hipMemcpy(c->rope_sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));

  // one grid for every lm_head launch (it sizes the argmax partials): the packed launch's workgroups per CU where the options ask for a packed lm_head
  // (pack_weights runs below; a lm_head that then falls back, and the batched steps, run their plain kernels on this grid too)
  // (an lm_head quantized by weights.fp8 starts at the same value: gemv_fp8.h's launch takes the class's packed_bpc)
  const bool lm_packed = ((c->weights_packed && (c->packed_classes & 4)) || (c->weights_fp8 && (c->fp8_classes & 4))) && c->dt == tgx::DT_BF16 && !c->gpt2;
  c->lm_grid = gemv_grid(c, (V + 1) / 2, 1, lm_packed ? c->tune[TGX_KERNEL_LMHEAD].packed_bpc : c->tune[TGX_KERNEL_LMHEAD].bpc);
  int ns = c->num_cus / d.kv_heads;
  c->attn_nsplit = ns < 1 ? 1 : (ns > 32 ? 32 : ns);
  if (c->attn_nsplit_opt > 0) c->attn_nsplit = c->attn_nsplit_opt;

  c->rows.resize((size_t)d.max_batch);
  const size_t B = (size_t)d.max_batch;
  size_t kv_elems = (size_t)d.layers * d.kv_heads * d.max_ctx * hd;
  c->kv_row_elems = kv_elems;
  size_t kv_total = B * kv_elems;                     // elements of the K cache (and of the V cache)
  if (c->kv_budget_tokens > 0) {                      // paged KV: pools of KV_BLOCK-token blocks shared by the rows (kernels/common.h)
    if (c->dt == tgx::DT_F32) return set_err(c, TGX_ERR_UNSUPPORTED, "kv.budget_tokens: paged KV serves the 16-bit storage dtypes");
    c->kv_paged = true;
    c->kv.init(d.max_batch, d.max_ctx, c->kv_budget_tokens, tgx::KV_BLOCK);
    kv_total = (size_t)d.layers * c->kv.n_blocks() * d.kv_heads * tgx::KV_BLOCK * hd;
    c->kv_row_elems = 1;                              // "the rows are separate sequences" wherever a row stride is tested against 0; never used as a stride (decode.hip kvs)
    if ((rc = dev_alloc(c, &c->kv_tbl, B * (size_t)c->kv.tbl_stride()))) return rc;
    HIP_OK(c, hipMemset(c->kv_tbl, 0, B * (size_t)c->kv.tbl_stride() * 4));
  }
  c->attn_part_row = (size_t)d.heads * c->attn_nsplit * (hd + 4);
  if ((rc = dev_alloc(c, &c->slab_x, B * H))) return rc;
  if ((rc = dev_alloc(c, &c->slab_q, B * qd))) return rc;
  if ((rc = dev_alloc(c, &c->slab_kraw, B * kvd))) return rc;
  if ((rc = dev_alloc(c, &c->slab_attn, B * qd))) return rc;
  if ((rc = dev_alloc(c, &c->slab_h, B * I))) return rc;
  if ((rc = dev_alloc(c, &c->slab_logits, B * V))) return rc;
  if ((rc = dev_alloc(c, &c->slab_probs, B * V))) return rc;
  if ((rc = dev_alloc(c, &c->slab_part_val, B * c->lm_grid))) return rc;
  if ((rc = dev_alloc(c, &c->slab_part_idx, B * c->lm_grid))) return rc;
  if ((rc = dev_alloc(c, &c->slab_attn_part, B * c->attn_part_row))) return rc;
  if ((rc = dev_alloc(c, &c->slab_tok, B))) return rc;
  if ((rc = dev_alloc(c, &c->slab_pos, B))) return rc;
  if ((rc = dev_alloc(c, &c->slab_prompt, B * d.max_ctx))) return rc;
  if ((rc = dev_alloc(c, &c->slab_k, kv_total * c->esz))) return rc;
  if ((rc = dev_alloc(c, &c->slab_v, kv_total * c->esz))) return rc;
  HIP_OK(c, hipMemset(c->slab_tok, 0, B * 4));
  HIP_OK(c, hipMemset(c->slab_pos, 0, B * 4));
  HIP_OK(c, hipMemset(c->slab_k, 0, kv_total * c->esz));
  HIP_OK(c, hipMemset(c->slab_v, 0, kv_total * c->esz));
  for (size_t b = 0; b < B; b++) {
    RowState& r = c->rows[b];
    r.x = c->slab_x + b * H; r.q = c->slab_q + b * qd; r.k_raw = c->slab_kraw + b * kvd; r.attn = c->slab_attn + b * qd;
    r.h = c->slab_h + b * I; r.logits = c->slab_logits + b * V; r.probs = c->slab_probs + b * V;
    r.part_val = c->slab_part_val + b * c->lm_grid; r.part_idx = c->slab_part_idx + b * c->lm_grid;
    r.attn_part = c->slab_attn_part + b * c->attn_part_row;
    r.tok = c->slab_tok + b; r.pos = c->slab_pos + b; r.prompt = c->slab_prompt + b * d.max_ctx;
    r.kcache = c->slab_k + b * kv_elems * c->esz; r.vcache = c->slab_v + b * kv_elems * c->esz;
    if (c->kv_paged) { r.kcache = c->slab_k; r.vcache = c->slab_v; r.tbl = c->kv_tbl + b * (size_t)c->kv.tbl_stride(); }
  }
  if ((rc = dev_alloc(c, &c->ch_x, 4 * (size_t)H))) return rc;
  if ((rc = dev_alloc(c, &c->ch_q, 4 * (size_t)qd))) return rc;
  if ((rc = dev_alloc(c, &c->ch_kraw, 4 * (size_t)kvd))) return rc;
  if ((rc = dev_alloc(c, &c->ch_attn, 4 * (size_t)qd))) return rc;
  if ((rc = dev_alloc(c, &c->ch_h, 4 * (size_t)I))) return rc;
  if ((rc = dev_alloc(c, &c->ch_part, 4 * c->attn_part_row))) return rc;
  if ((rc = dev_alloc(c, &c->ch_pos, 4))) return rc;
  for (size_t k = 0; k < 4; k++) {
    RowState& r = c->chunk[k];
    r.x = c->ch_x + k * H; r.q = c->ch_q + k * qd; r.k_raw = c->ch_kraw + k * kvd; r.attn = c->ch_attn + k * qd; r.h = c->ch_h + k * I;
    r.attn_part = c->ch_part + k * c->attn_part_row; r.pos = c->ch_pos + k;
  }
  c->log_cap = d.max_ctx > 1024 ? d.max_ctx : 1024;
  if ((rc = dev_alloc(c, &c->step, 1)) || (rc = dev_alloc(c, &c->step_done, 1))) return rc;
  if ((rc = dev_alloc(c, &c->seed_dev, 1))) return rc;
  if ((rc = sampler_alloc(c))) return rc;
  if ((rc = dev_alloc(c, &c->scratch_x, (size_t)H))) return rc;
  HIP_OK(c, hipMemset(c->scratch_x, 0, (size_t)H * 4));
  if ((rc = dev_alloc(c, &c->tok_log, (size_t)c->log_cap * d.max_batch))) return rc;
  HIP_OK(c, hipMemset(c->step, 0, 4));
  HIP_OK(c, hipMemset(c->step_done, 0, 4));
  HIP_OK(c, hipHostMalloc((void**)&c->host_ring, (size_t)HOST_RING * d.max_batch * 4, hipHostMallocMapped));
  HIP_OK(c, hipHostGetDevicePointer((void**)&c->host_ring_dev, c->host_ring, 0));
  for (int i = 0; i < MAX_TICKET_EVENTS; i++) HIP_OK(c, hipEventCreateWithFlags(&c->ticket_ev[i], hipEventDisableTiming));
  for (int i = 0; i < 2; i++) HIP_OK(c, hipEventCreate(&c->prof.ev[i]));
  if ((rc = prefill_set_attrs(c)) || (rc = skinny_set_attrs(c)) || (rc = attn_set_attrs(c))) return rc;
  // fixed-point accumulators of the K-sliced o_proj (kernels/oproj_sliced.h): zero between layers
  if ((rc = dev_alloc(c, &c->slab_acc, B * (size_t)H))) return rc;
  HIP_OK(c, hipMemset(c->slab_acc, 0, B * (size_t)H * 8));
  c->row_req_host.assign(B, row_req_default());
  if ((rc = dev_alloc(c, &c->row_req, B))) return rc;
  HIP_OK(c, hipMemcpy(c->row_req, c->row_req_host.data(), B * sizeof(tgx::RowReq), hipMemcpyHostToDevice));
  if ((rc = quantize_weights(c)) || (rc = pack_weights(c))) return rc;
  c->past = 0;
  c->row_host.assign(B, RowHost{});
  c->finalized = true;
  return TGX_OK;
}

void tgx_destroy(tgx_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  drop_step_graphs(c);
  c->mem.release_all();      // every device buffer of the context, by its record (dev_mem.h)
  if (c->host_ring) (void)hipHostFree(c->host_ring);
  for (auto& e : c->ticket_ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : c->prof.ev) if (e) (void)hipEventDestroy(e);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int tgx_forward(tgx_ctx* c, const int64_t* ids, int batch, int seq) {
  if (!c || !ids) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "forward before finalize");
  if (batch < 1 || batch > c->d.max_batch || seq < 1) return set_err(c, TGX_ERR_INVALID, "batch/seq out of range");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  if (seq > 1 && c->past > 0) return set_err(c, TGX_ERR_INVALID, "seq>1 with pastLength>0");
  if (finished_row(c) >= 0) return set_err(c, TGX_ERR_STATE, "row %d finished in tgx_decode_rows: tgx_reset_row it (or tgx_reset_cache) first", finished_row(c));
  if (c->past + seq > c->d.max_ctx) return set_err(c, TGX_ERR_CONTEXT, "context size exceeded: %lld + %d > %d", (long long)c->past, seq, c->d.max_ctx);
  for (int b = 0; b < batch; b++)
    if (c->row_host[(size_t)b].idle || c->row_host[(size_t)b].past != c->past) return set_err(c, TGX_ERR_STATE, "tgx_forward on a batch whose rows differ in length (row %d: %lld, longest %lld): use tgx_decode / tgx_forward_row, or tgx_reset_cache", b, (long long)c->row_host[(size_t)b].past, (long long)c->past);
  for (int64_t i = 0; i < (int64_t)batch * seq; i++)
    if (ids[i] < 0 || ids[i] >= c->d.vocab) return set_err(c, TGX_ERR_INVALID, "token id out of range");
  HIP_OK(c, hipSetDevice(c->device));
  c->batch = batch;
  for (int b = 0; b < batch; b++) { int rc = kv_ensure_blocks(c, b, c->past + seq); if (rc) return rc; }
  for (int b = 0; b < batch; b++) HIP_OK(c, hipMemcpyAsync(c->rows[(size_t)b].prompt, ids + (size_t)b * seq, (size_t)seq * 8, hipMemcpyHostToDevice, c->stream));
  // batch rows are stacked into one row block while that stays within 8192 workspace rows (the CLI's 4 short prompts cost one pass over the weights)
  const int per = std::max(1, std::min(batch, 8192 / seq));
  for (int row0 = 0; row0 < batch; row0 += per)
    if (int rc = issue_pass(c, row0, std::min(per, batch - row0), seq, (int)c->past)) return rc;      // every row at the batch's pastLength
  if (int rc = finish_pass(c)) return rc;
  c->past += seq;
  for (int b = 0; b < batch; b++) c->row_host[(size_t)b].restart(c->past, /*idle=*/false, c->row_host[(size_t)b].fin);
  c->have_logits = true;
  c->have_token = false;
  c->have_probs = false;                          // the logits are new: no sampled step belongs to them yet
  for (RowHost& r : c->row_host) r.probs_ok = false;
  return TGX_OK;
}

int tgx_read_logits(tgx_ctx* c, float* out, int rounded) {
  if (!c || !out) return TGX_ERR_INVALID;
  if (!c->have_logits) return set_err(c, TGX_ERR_STATE, "no logits: call tgx_forward/tgx_decode first");
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  const size_t V = (size_t)c->d.vocab;
  for (int b = 0; b < c->batch; b++) HIP_OK(c, hipMemcpy(out + b * V, c->rows[(size_t)b].logits, V * 4, hipMemcpyDeviceToHost));
  if (rounded && c->dt != tgx::DT_F32)
    for (size_t i = 0; i < V * (size_t)c->batch; i++)
      out[i] = c->dt == tgx::DT_BF16 ? host_bf16_to_f32(host_f32_to_bf16(out[i])) : host_half_to_f32(host_f32_to_half(out[i]));
  return TGX_OK;
}

int tgx_sample(tgx_ctx* c, const tgx_sampler_cfg* cfg, uint64_t seed, int64_t* out_ids) {
  if (!c || !cfg) return TGX_ERR_INVALID;
  if (!c->have_logits) return set_err(c, TGX_ERR_STATE, "no logits to sample from");
  REFUSE_NOLOGITS(c, "tgx_sample");
  HIP_OK(c, hipSetDevice(c->device));
  if (int rc = ensure_seed(c, *cfg, seed)) return rc;
  note_sampled(c, 0, c->batch, *cfg);
  launch_sample(c, 0, c->batch, *cfg, /*advance_pos=*/false, /*log_step=*/false);
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipStreamSynchronize(c->stream));
  for (int b = 0; b < c->batch; b++) {
    int t = 0;
    HIP_OK(c, hipMemcpy(&t, c->rows[(size_t)b].tok, 4, hipMemcpyDeviceToHost));
    if (out_ids) out_ids[b] = t;
    if (b == 0) c->last_sampled0 = t;
    c->row_host[(size_t)b].tok = 1;
  }
  c->have_token = true;
  return TGX_OK;
}

int tgx_decode(tgx_ctx* c, const tgx_sampler_cfg* cfg, uint64_t seed, int n_steps, int64_t* out_ids) {
  if (!c || !cfg || n_steps < 0) return TGX_ERR_INVALID;
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  REFUSE_NOLOGITS(c, "tgx_decode");
  if (!c->have_token) return set_err(c, TGX_ERR_STATE, "decode needs a current token: call tgx_sample after tgx_forward");
  if (finished_row(c) >= 0) return set_err(c, TGX_ERR_STATE, "row %d finished in tgx_decode_rows: tgx_reset_row it first (tgx_decode would advance it)", finished_row(c));
  if (c->past + n_steps > c->d.max_ctx) return set_err(c, TGX_ERR_CONTEXT, "context size exceeded: %lld + %d > %d", (long long)c->past, n_steps, c->d.max_ctx);
  if (n_steps > c->log_cap) return set_err(c, TGX_ERR_INVALID, "n_steps exceeds the token log capacity %d", c->log_cap);
  HIP_OK(c, hipSetDevice(c->device));
  const int64_t start = c->steps_issued;
  int rc = run_decode_steps(c, *cfg, seed, n_steps);
  if (rc) return rc;
  c->have_logits = true;
  if (out_ids && n_steps > 0) {
    const size_t B = (size_t)c->batch;
    std::vector<int> tmp((size_t)n_steps * B);
    if ((rc = read_tok_log(c, start, n_steps, tmp.data()))) return rc;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < tmp.size(); i++) out_ids[i] = tmp[i];
    c->last_sampled0 = tmp[(size_t)(n_steps - 1) * B];
  }
  return TGX_OK;
}

int tgx_step_async(tgx_ctx* c, const tgx_sampler_cfg* cfg, uint64_t seed, int64_t* out_ticket) {
  if (!c || !cfg || !out_ticket) return TGX_ERR_INVALID;
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  REFUSE_NOLOGITS(c, "tgx_step_async");
  if (!c->have_token) return set_err(c, TGX_ERR_STATE, "step needs a current token: call tgx_sample after tgx_forward");
  if (finished_row(c) >= 0) return set_err(c, TGX_ERR_STATE, "row %d finished in tgx_decode_rows: tgx_reset_row it first (tgx_step_async would advance it)", finished_row(c));
  if (c->past + 1 > c->d.max_ctx) return set_err(c, TGX_ERR_CONTEXT, "context size exceeded");
  HIP_OK(c, hipSetDevice(c->device));
  int rc = run_decode_steps(c, *cfg, seed, 1);
  if (rc) return rc;
  const int64_t ticket = c->steps_issued;
  HIP_OK(c, hipEventRecord(c->ticket_ev[ticket % MAX_TICKET_EVENTS], c->stream));
  c->have_logits = true;
  *out_ticket = ticket;
  return TGX_OK;
}

int tgx_fetch_token(tgx_ctx* c, int64_t ticket, int32_t* out_id) {
  if (!c || !out_id) return TGX_ERR_INVALID;
  if (ticket == 0) { *out_id = c->last_sampled0; return TGX_OK; }
  if (ticket < 0 || ticket > c->steps_issued || c->steps_issued - ticket >= MAX_TICKET_EVENTS)
    return set_err(c, TGX_ERR_INVALID, "ticket %lld is not outstanding", (long long)ticket);
  HIP_OK(c, hipEventSynchronize(c->ticket_ev[ticket % MAX_TICKET_EVENTS]));
  *out_id = c->host_ring[((ticket - 1) % HOST_RING) * c->batch];   // row 0 of the step that ticket names
  return TGX_OK;
}

int tgx_reset_cache(tgx_ctx* c) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "reset before finalize");
  HIP_OK(c, hipSetDevice(c->device));
  for (auto& r : c->rows) HIP_OK(c, hipMemsetAsync(r.pos, 0, 4, c->stream));
  for (int b = 0; b < c->d.max_batch; b++) kv_release_row(c, b);
  std::fill(c->row_req_host.begin(), c->row_req_host.end(), row_req_default());
  HIP_OK(c, hipMemcpyAsync(c->row_req, c->row_req_host.data(), c->row_req_host.size() * sizeof(tgx::RowReq), hipMemcpyHostToDevice, c->stream));   // (synchronised below)
  if (c->slab_acc) HIP_OK(c, hipMemsetAsync(c->slab_acc, 0, (size_t)c->d.max_batch * c->d.hidden * 8, c->stream));
  if (c->lp_rows) HIP_OK(c, hipMemsetAsync(c->lp_rows, 0, (size_t)c->d.max_batch * sizeof(tgx::LpRow), c->stream));
  if (c->proc_hist) HIP_OK(c, hipMemsetAsync(c->proc_hist, 0, (size_t)c->d.max_batch * c->d.vocab * sizeof(unsigned int), c->stream));
  if (int rc = vs_rezero(c)) return rc;      // (a sampled verify pass that failed half-way may have left its histograms)
  HIP_OK(c, hipStreamSynchronize(c->stream));
  c->vf_pass_rows = 0;
  c->past = 0;
  for (RowHost& r : c->row_host) { r.restart(0, /*idle=*/false, /*fin=*/0); r.lp_count = 0; r.auto_id = -1; }
  c->have_logits = c->have_token = false;
  c->poisoned = false;
  return TGX_OK;
}

int64_t tgx_past_length(const tgx_ctx* c) { return c ? c->past : -1; }

// ---- per-row sequence lifecycle (include/tgx.h, ABI 3).  The step kernels read every row's position from its own device word; the host keeps the
// mirror row_host[].past and `past` = the longest row of the batch (capacity checks, attention-form limits: a form chosen for the longest row is valid for
// the shorter ones — the direct form's pass count and the split form's active splits are derived on the device from each row's position).
// Retired rows (RowHost::idle) are left out of both: nothing waits for them and they bound nothing (run_decode_steps keeps them below the longest live row).
static void refresh_longest(tgx_ctx* c) {
  int64_t m = 0;
  int live = 0;
  bool all = true;
  for (int b = 0; b < c->batch; b++) {
    if (c->row_host[(size_t)b].idle || c->row_host[(size_t)b].fin) continue;      // (a finished row counts for neither, include/tgx.h tgx_decode_rows)
    live++;
    m = std::max(m, c->row_host[(size_t)b].past);
    all = all && c->row_host[(size_t)b].tok;
  }
  c->past = m;
  c->have_token = live > 0 && all;
}

int64_t tgx_past_length_row(const tgx_ctx* c, int row) {
  if (!c || !c->finalized || row < 0 || row >= c->d.max_batch) return -1;
  return c->row_host[(size_t)row].idle ? 0 : c->row_host[(size_t)row].past;        // a retired row holds no sequence, wherever its position word stands
}

int tgx_reset_row(tgx_ctx* c, int row) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "reset before finalize");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipMemsetAsync(c->rows[(size_t)row].pos, 0, 4, c->stream));     // stream-ordered behind the steps already enqueued
  kv_release_row(c, row);                                                     // paged KV: its blocks go back to the pool (a retired row rides along on the scratch block)
  row_req_reset(c, row);                                                      // tgx_decode_rows: default settings ...
  if (c->proc_hist) HIP_OK(c, hipMemsetAsync(c->proc_hist + (size_t)row * c->d.vocab, 0, (size_t)c->d.vocab * sizeof(unsigned int), c->stream));      // ... and an empty history
  c->row_host[(size_t)row].restart(0, /*idle=*/row < c->batch, /*fin=*/0);    // ... not finished; a live slot becomes a retired one: the batch keeps stepping without it
  refresh_longest(c);
  return TGX_OK;
}

// host state of a row after its prompt pass went through (the caller synchronised)
static void row_admitted(tgx_ctx* c, int row, int seq, bool keep_lp_count = false) {
  c->row_host[(size_t)row].restart(seq, /*idle=*/false, /*fin=*/0);
  // a new sequence: what the slot counted while it rode along retired is gone (its settings stay; the log-probability setting, held back while the row was retired, goes to the device)
  row_req_push(c, row, ROWQ_STATE | ROWQ_LP | ROWQ_PROC | (keep_lp_count ? 0 : ROWQ_LPCOUNT));      // (the processors' settings likewise)
  if (!keep_lp_count) c->row_host[(size_t)row].lp_count = 0;                   // ... its log-probability records as well; tgx_extend_row keeps them
  c->row_host[(size_t)row].probs_ok = false;
}

// the rows an admission (src -1, prompt lengths lens) or a fork of row src (lens nullptr) fills: each in range and named once, the new ones growing the batch in order,
// every one empty (retired, or holding no position); a fork's source a live, unfinished row that holds logits
static int check_target_rows(tgx_ctx* c, int n, const int32_t* rows, const int32_t* lens, int src) {
  const tgx_model_desc& d = c->d;
  std::vector<char> named((size_t)d.max_batch, 0);
  int n_new = 0;
  for (int i = 0; i < n; i++) {
    const int row = rows[i];
    if (row < 0 || row >= d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, d.max_batch);
    if (row == src) return set_err(c, TGX_ERR_INVALID, "row %d is the source of the fork", row);
    if (named[(size_t)row]) return set_err(c, TGX_ERR_INVALID, "row %d named twice", row);
    named[(size_t)row] = 1;
    n_new += row >= c->batch;
  }
  if (src >= 0) {
    const RowHost& s = c->row_host[(size_t)src];
    if (src >= c->batch || s.idle || s.fin || s.past < 1) return set_err(c, TGX_ERR_STATE, "source row %d is not a live, unfinished row of the batch", src);
    if (s.nologits) return set_err(c, TGX_ERR_STATE, "source row %d was truncated and holds no logits: tgx_extend_row it first", src);
  }
  for (int row = c->batch; row < c->batch + n_new; row++)
    if (row >= d.max_batch || !named[(size_t)row])
      return set_err(c, TGX_ERR_INVALID, "the new rows of a call must be %d..%d (the batch grows in order, max_batch %d)", c->batch, c->batch + n_new - 1, d.max_batch);
  for (int i = 0; i < n; i++) {
    if (lens && (lens[i] < 1 || lens[i] > d.max_ctx))
      return set_err(c, lens[i] < 1 ? TGX_ERR_INVALID : TGX_ERR_CONTEXT, "prompt %d: seq %d out of range (context size %d)", i, lens[i], d.max_ctx);
    const RowHost& r = c->row_host[(size_t)rows[i]];
    if (!r.idle && r.past != 0) return set_err(c, TGX_ERR_STATE, "row %d holds %lld positions%s: tgx_reset_row first", rows[i], (long long)r.past, r.fin ? " (finished)" : "");
  }
  return TGX_OK;
}

// ---- admission (include/tgx.h tgx_forward_row, tgx_forward_rows): n prompts, back to back in ids, into the empty rows rows[], each from position 0 whatever the other
// rows of the batch hold — `past` of every pass is the argument 0, and c->past (the longest live row) moves only through refresh_longest after the passes went through.
// may_join (tgx_forward_rows): consecutive whole prompts share ONE ragged prefill pass per group of <= max(8192, longest) workspace rows where a matrix-core route
// takes the group's rows; every other prompt, and every prompt of tgx_forward_row, runs issue_pass's one-row pass.  Only a call with a ragged pass uploads tables
// (one buffer, ONE upload: per group the tables of ragged_tables, then the call's ids) and holds the four lm_head staging rows.
// the vf_* workspace: every position's logits of a one-row verify pass (tgx_verify_row), at first use; the group form of tgx_score_row holds it as well
static int ensure_verify_ws(tgx_ctx* c) {
  if (c->vf_rec) return TGX_OK;
  const size_t R = tgx_ctx::VERIFY_ROWS, H = (size_t)c->d.hidden, V = (size_t)c->d.vocab, P = (size_t)c->lm_grid;
  int rc;
  if ((rc = dev_alloc(c, &c->vf_x, R * H)) || (rc = dev_alloc(c, &c->vf_logits, R * V)) || (rc = dev_alloc(c, &c->vf_part_val, R * P)) || (rc = dev_alloc(c, &c->vf_part_idx, R * P))) return rc;
  HIP_OK(c, hipMemset(c->vf_x, 0, R * H * 4));      // (a group of three positions rides as four through lm_head: the fourth row is read)
  return dev_alloc(c, &c->vf_rec, sizeof(tgx::VerifyRecord) / 4);
}
// tgx_score_row: the workspace of a scoring pass of seq positions on route rt, before the pass is issued; the read-back of its scores, behind it
static int score_prepare(tgx_ctx* c, ScoreCall* sc, PrefillRoute rt, int row) {
  sc->ids = c->rows[(size_t)row].prompt;
  if (sc->n_score < 1) return TGX_OK;
  if (rt != ROUTE_TILED) if (int rc = ensure_verify_ws(c)) return rc;
  return ensure_score_ws(c, sc->n_score + 1, rt == ROUTE_TILED);
}
static int score_read_back(tgx_ctx* c, const ScoreCall* sc) {
  if (sc->n_score < 1) return TGX_OK;
  HIP_OK(c, hipMemcpyAsync(sc->host, c->sc_out, sc->host_bytes, hipMemcpyDeviceToHost, c->stream));
  return TGX_OK;
}

// the four lm_head staging rows of a ragged pass, at first use
static int ensure_rg_lm_ws(tgx_ctx* c) {
  if (c->rg_x) return TGX_OK;
  const size_t V = (size_t)c->d.vocab, H = (size_t)c->d.hidden, P = (size_t)c->lm_grid;
  int rc;
  if ((rc = dev_alloc(c, &c->rg_x, 4 * H)) || (rc = dev_alloc(c, &c->rg_logits, 4 * V)) || (rc = dev_alloc(c, &c->rg_part_val, 4 * P)) || (rc = dev_alloc(c, &c->rg_part_idx, 4 * P))) return rc;
  return TGX_OK;
}
// lm_head of the batch rows rws[] whose hidden rows a ragged pass left (tgx_forward_rows, tgx_advance_rows' FEED rows): four at a time (tgx_forward's grouping where
// they are consecutive rows; else gathered into staging rows and scattered back)
static void launch_lm_head_rows(tgx_ctx* c, const std::vector<int>& rws) {
  const size_t V = (size_t)c->d.vocab, H = (size_t)c->d.hidden, P = (size_t)c->lm_grid;
  for (size_t k = 0; k < rws.size();) {
    const size_t rem = rws.size() - k, real = std::min<size_t>(rem, 4);
    const int R = rem >= 3 ? 4 : (int)rem;
    bool consec = (int)real == R;
    for (size_t j = 1; j < real; j++) consec = consec && rws[k + j] == rws[k] + (int)j;
    if (consec) {
      launch_lm_head(c, rws[k], R);
    } else {
      for (int j = 0; j < R; j++)
        (void)hipMemcpyAsync(c->rg_x + j * H, c->rows[(size_t)rws[k + std::min<size_t>(j, real - 1)]].x, H * 4, hipMemcpyDeviceToDevice, c->stream);
      launch_lm_head_at(c, c->rg_x, c->rg_logits, c->rg_part_val, c->rg_part_idx, R);
      for (size_t j = 0; j < real; j++) {
        RowState& r = c->rows[(size_t)rws[k + j]];
        (void)hipMemcpyAsync(r.logits, c->rg_logits + j * V, V * 4, hipMemcpyDeviceToDevice, c->stream);
        (void)hipMemcpyAsync(r.part_val, c->rg_part_val + j * P, P * 4, hipMemcpyDeviceToDevice, c->stream);
        (void)hipMemcpyAsync(r.part_idx, c->rg_part_idx + j * P, P * 4, hipMemcpyDeviceToDevice, c->stream);
      }
    }
    k += real;
  }
}

// sc (tgx_score_row; n == 1, may_join false): the pass also scores its positions (issue_pass)
// em (tgx_embed_rows; may_join true): the same groups, routes and passes WITHOUT any lm_head launch or lm_head staging; behind each pass the pooled partials of its texts,
// behind the last the finish launch and the read-back (kernels/embed_pool.h).  The rows end in tgx_truncate_row's no-logits state
static int admit_rows(tgx_ctx* c, int n, const int32_t* rows, const int64_t* ids, const int32_t* lens, bool may_join, ScoreCall* sc = nullptr, EmbedCall* em = nullptr) {
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "forward before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  const tgx_model_desc& d = c->d;
  if (n < 1 || n > d.max_batch) return set_err(c, TGX_ERR_INVALID, "n %d out of range [1,%d]", n, d.max_batch);
  // ---- every check before anything changes
  if (int rc = check_target_rows(c, n, rows, lens, /*src=*/-1)) return rc;
  long long total = 0;
  int longest = 0;
  for (int i = 0; i < n; i++) { total += lens[i]; longest = std::max(longest, (int)lens[i]); }
  for (long long i = 0; i < total; i++)
    if (ids[i] < 0 || ids[i] >= d.vocab) return set_err(c, TGX_ERR_INVALID, "token id out of range");
  if (c->kv_paged) {
    // the ragged prompt attention copies a row's block table into LDS (<= 1024 entries)
    if (may_join && c->kv.tbl_stride() > 1024) return set_err(c, TGX_ERR_UNSUPPORTED, "tgx_forward_rows on a paged cache of %d blocks per row (at most 1024: max_ctx <= %d)", c->kv.tbl_stride(), 1024 * tgx::KV_BLOCK);
    // all or nothing: the blocks of the whole call against the free list plus the blocks the target rows give back
    long long need = 0;
    for (int i = 0; i < n; i++) need += (lens[i] + tgx::KV_BLOCK - 1) / tgx::KV_BLOCK;
    const long long have = c->kv.available_for(rows, n);      // (a block a forked sibling still maps does not come back)
    if (need > have)
      return set_err(c, TGX_ERR_CONTEXT, "KV budget exhausted: the call needs %lld blocks of %d tokens, %lld free or held by its rows of %d (option kv.budget_tokens = %d)", need,
                     tgx::KV_BLOCK, have, c->kv.n_blocks() - 1, c->kv_budget_tokens);
  }
  HIP_OK(c, hipSetDevice(c->device));
  const PrefillRoute sc_rt = prefill_route(c, lens[0], lens[0]);
  if (sc) if (int rc = score_prepare(c, sc, sc_rt, rows[0])) return rc;
  if (em) {      // the pooled positions of every text and its rows of the partials (the workspace rows follow with the groups below)
    em->n = n; em->slices = 0;
    em->tab.assign((size_t)n * 4, 0);
    for (int i = 0; i < n; i++) {
      const int np = em->pool == TGX_POOL_MEAN ? lens[i] : 1;
      em->tab[(size_t)i * 4 + 1] = np; em->tab[(size_t)i * 4 + 2] = em->slices;
      em->slices += (np + EmbedCall::SLICE - 1) / EmbedCall::SLICE;
    }
    if (int rc = ensure_embed_ws(c, *em)) return rc;
  }
  if (c->kv_paged) {
    for (int i = 0; i < n; i++) kv_release_row(c, rows[i]);
    for (int i = 0; i < n; i++) (void)kv_ensure_blocks(c, rows[i], lens[i]);     // cannot fail: counted above
  }
  // ---- groups of whole prompts: a ragged pass (p.n prompts) where a matrix-core route takes the group's rows, else (p.n = 0) one-row passes
  const int cap = std::max(8192, longest);
  std::vector<int> first((size_t)n), g_begin;
  std::vector<long long> off((size_t)n + 1, 0);           // prompt i's ids at ids + off[i]
  for (int i = 0, M = 0; i < n; i++) {
    if (i == 0 || M + lens[i] > cap) { g_begin.push_back(i); M = 0; }
    first[(size_t)i] = M;
    M += lens[i];
    off[(size_t)i + 1] = off[(size_t)i] + lens[i];
  }
  g_begin.push_back(n);
  const int n_groups = (int)g_begin.size() - 1;
  std::vector<RaggedPass> passes((size_t)n_groups);
  std::vector<PrefillRoute> route((size_t)n_groups, ROUTE_STEPS);
  std::vector<size_t> o_tab((size_t)n_groups);
  std::vector<unsigned char> host;      // the call's buffer (lives until finish_pass has synchronised)
  size_t bytes = 0;
  for (int g = 0; g < n_groups; g++) {
    RaggedPass& p = passes[(size_t)g];
    const int i0 = g_begin[(size_t)g], i1 = g_begin[(size_t)g + 1];
    p.rows = rows + i0; p.lens = lens + i0; p.first = first.data() + i0;
    for (int i = i0; i < i1; i++) { p.M += lens[i]; p.longest = std::max(p.longest, (int)lens[i]); }
    if (may_join) route[(size_t)g] = prefill_route(c, p.M, p.M);
    if (route[(size_t)g] != ROUTE_SKINNY && route[(size_t)g] != ROUTE_TILED) continue;      // (fp32 storage has no ragged pass)
    p.n = i1 - i0;
    o_tab[(size_t)g] = bytes; bytes += ragged_tables(c, p, nullptr, nullptr);
  }
  if (bytes) {
    const size_t o_ids = bytes;
    bytes += (size_t)total * 8;
    if (int rc = dev_grow(c, &c->rg_buf, &c->rg_bytes, bytes)) return rc;
    if (!em) if (int rc = ensure_rg_lm_ws(c)) return rc;
    host.assign(bytes, 0);
    std::memcpy(host.data() + o_ids, ids, (size_t)total * 8);
    for (int g = 0; g < n_groups; g++) {
      RaggedPass& p = passes[(size_t)g];
      if (!p.n) continue;
      ragged_tables(c, p, host.data() + o_tab[(size_t)g], c->rg_buf + o_tab[(size_t)g]);
      p.ids = reinterpret_cast<const long long*>(c->rg_buf + o_ids) + off[(size_t)g_begin[(size_t)g]];
    }
    HIP_OK(c, hipMemcpyAsync(c->rg_buf, host.data(), bytes, hipMemcpyHostToDevice, c->stream));
  }
  for (int i = 0; i < n; i++)      // retired rows that rode along since their reset: position word back to 0
    if (c->row_host[(size_t)rows[i]].past != 0) { HIP_OK(c, hipMemsetAsync(c->rows[(size_t)rows[i]].pos, 0, 4, c->stream)); c->row_host[(size_t)rows[i]].past = 0; }
  if (em) {      // the workspace row of every text's first pooled position: behind its group's first row in a ragged pass, from row 0 in a one-row pass
    for (int g = 0; g < n_groups; g++)
      for (int i = g_begin[(size_t)g]; i < g_begin[(size_t)g + 1]; i++)
        em->tab[(size_t)i * 4] = (passes[(size_t)g].n ? first[(size_t)i] : 0) + (em->pool == TGX_POOL_LAST ? lens[i] - 1 : 0);
    if (int rc = embed_upload_table(c, *em)) return rc;
  }
  std::vector<int> joint;             // prompts that went through a ragged pass: their lm_head comes below, four rows per pass over the weights
  for (int g = 0; g < n_groups; g++) {
    const RaggedPass& p = passes[(size_t)g];
    const int i0 = g_begin[(size_t)g], i1 = g_begin[(size_t)g + 1];
    if (p.n) {
      if (int rc = launch_route(c, route[(size_t)g], p.M, 0, 0, 0, /*past=*/0, &p)) return rc;
      if (em) launch_embed_pool(c, *em, i0, i1 - i0);      // (the next group's pass overwrites ws_x)
      for (int i = i0; i < i1; i++) joint.push_back(i);
    } else
      for (int i = i0; i < i1; i++) {
        HIP_OK(c, hipMemcpyAsync(c->rows[(size_t)rows[i]].prompt, ids + off[(size_t)i], (size_t)lens[i] * 8, hipMemcpyHostToDevice, c->stream));
        if (em) em->cur = i;
        if (int rc = issue_pass(c, rows[i], 1, lens[i], /*past=*/0, /*verify=*/false, sc, em)) return rc;
      }
  }
  std::vector<int> joint_rows(joint.size());
  for (size_t k = 0; k < joint.size(); k++) joint_rows[k] = rows[joint[k]];
  if (!em) launch_lm_head_rows(c, joint_rows);
  for (size_t k = 0; k < joint.size(); k++) launch_add_pos(c, c->rows[(size_t)rows[joint[k]]].pos, lens[joint[k]]);
  if (sc) if (int rc = score_read_back(c, sc)) return rc;
  if (em) if (int rc = launch_embed_finish(c, *em)) return rc;
  if (int rc = finish_pass(c)) return rc;
  if (sc && sc->n_score >= 1) c->score_last_form = sc_rt == ROUTE_TILED ? 1 : 2;      // (a call of one position scored nothing: the option keeps its value)
  for (int i = 0; i < n; i++) {
    c->batch = std::max(c->batch, rows[i] + 1);
    row_admitted(c, rows[i], lens[i]);
    if (em) c->row_host[(size_t)rows[i]].nologits = true;      // no lm_head ran: the slot's logits are not this sequence's (tgx_truncate_row's state)
  }
  refresh_longest(c);
  if (!em) c->have_logits = true;
  return TGX_OK;
}

int tgx_forward_row(tgx_ctx* c, int row, const int64_t* ids, int seq) {
  if (!c || !ids) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  const int32_t r = row, s = seq;
  return admit_rows(c, 1, &r, ids, &s, /*may_join=*/false);
}

int tgx_forward_rows(tgx_ctx* c, int n, const int32_t* rows, const int64_t* ids, const int32_t* lens) {
  if (!c || !rows || !ids || !lens) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  return admit_rows(c, n, rows, ids, lens, /*may_join=*/true);
}

// ---- tgx_embed_rows (include/tgx.h): tgx_forward_rows' admission and passes without lm_head, the pooled final-norm hidden state of every text behind them
// (admit_rows' em form).  The call's own argument checks come first; release retires the rows as tgx_reset_row does, behind the pass in stream order
int tgx_embed_rows(tgx_ctx* c, int n, const int32_t* rows, const int64_t* ids, const int32_t* lens, const tgx_embed_cfg* cfg, float* out) {
  if (!c || !rows || !ids || !lens || !cfg || !out) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  if (cfg->pool != TGX_POOL_LAST && cfg->pool != TGX_POOL_MEAN && cfg->pool != TGX_POOL_FIRST) return set_err(c, TGX_ERR_INVALID, "pool %d is none of TGX_POOL_LAST / MEAN / FIRST", cfg->pool);
  if (cfg->dims < 0 || cfg->dims > c->d.hidden) return set_err(c, TGX_ERR_INVALID, "dims %d out of range [0,%d] (0: the hidden size)", cfg->dims, c->d.hidden);
  EmbedCall em;
  em.pool = cfg->pool; em.normalize = cfg->normalize != 0; em.dims = cfg->dims ? cfg->dims : c->d.hidden; em.host_out = out;
  if (int rc = admit_rows(c, n, rows, ids, lens, /*may_join=*/true, nullptr, &em)) return rc;
  if (cfg->release)
    for (int i = 0; i < n; i++) if (int rc = tgx_reset_row(c, rows[i])) return rc;
  return TGX_OK;
}

// ---- tgx_fork_row (include/tgx.h): dst_rows become copies of the live row src.  Paged cache: src's full blocks by reference (KvPool::share), one fresh block per
// destination for the partial tail; slab cache: the prefix [0, past) of every (layer, kv head).  ONE kv_fork_kernel launch carries what has to be copied for all layers,
// both caches and all destinations, and the per-row state (hidden row, logits, argmax partials, position and token words) rides in the same launch.  Every check comes
// before anything changes; the launch sequence ends in finish_pass like an admission.
static void launch_kv_fork(tgx_ctx* c, int src, int n, const int32_t* dst_rows, const int* dst_blk, int src_blk) {
  const tgx_model_desc& d = c->d;
  const long long past = c->row_host[(size_t)src].past;
  for (int i0 = 0; i0 < n; i0 += tgx::KV_FORK_MAX_DST)
    launch_kv_copy(c, c->kv_paged ? past % tgx::KV_BLOCK : past, [&](tgx::KvForkArgs& a) {
      a.n_dst = std::min(n - i0, (int)tgx::KV_FORK_MAX_DST);
      a.src_row = src; a.src_id = c->kv_paged ? src_blk : src;
      for (int k = 0; k < a.n_dst; k++) { a.dst_row[k] = dst_rows[i0 + k]; a.dst_id[k] = c->kv_paged ? dst_blk[i0 + k] : dst_rows[i0 + k]; }
      // the grid from the bytes to move.  x: workgroups inside a span, one per KV_FORK_THREADS * KV_FORK_UNROLL vectors; y: grid rows that walk the 2 * n_spans spans, as
      // many as keep the launch within eight workgroups per CU for a slab prefix (the chip filled, the rest in the rows' loops) and within 64 workgroups for a paged
      // tail (at most 127 tokens per span: x = 1 at every released head_dim)
      const long long per_wg = tgx::KV_FORK_THREADS * tgx::KV_FORK_UNROLL, cap = c->kv_paged ? 64 : 8ll * c->num_cus;
      const int gx = (int)std::max<long long>(1, std::min<long long>((a.span_vecs + per_wg - 1) / per_wg, cap));
      a.kv_rows = a.span_vecs ? (int)std::max<long long>(1, std::min<long long>(2ll * a.n_spans, cap / gx)) : 0;
      const size_t H = (size_t)d.hidden, V = (size_t)d.vocab, P = (size_t)c->lm_grid;
      a.seg[0] = {reinterpret_cast<unsigned char*>(c->slab_x), (long long)(H * 4), (int)H};
      a.seg[1] = {reinterpret_cast<unsigned char*>(c->slab_logits), (long long)(V * 4), (int)V};
      a.seg[2] = {reinterpret_cast<unsigned char*>(c->slab_part_val), (long long)(P * 4), (int)P};
      a.seg[3] = {reinterpret_cast<unsigned char*>(c->slab_part_idx), (long long)(P * 4), (int)P};
      a.seg[4] = {reinterpret_cast<unsigned char*>(c->slab_pos), 4, 1};
      a.seg[5] = {reinterpret_cast<unsigned char*>(c->slab_tok), 4, 1};
      const int st_rows = ((int)std::min<size_t>(64, (V + 1023) / 1024) + gx - 1) / gx;      // the state part: up to 64 workgroups, a dword per thread and round
      return dim3((unsigned)gx, (unsigned)(a.kv_rows + st_rows));
    });
}

int tgx_fork_row(tgx_ctx* c, int src, int n, const int32_t* dst_rows) {
  if (!c || !dst_rows) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "fork before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  const tgx_model_desc& d = c->d;
  // ---- every check before anything changes
  if (n < 1 || n > d.max_batch) return set_err(c, TGX_ERR_INVALID, "n %d out of range [1,%d]", n, d.max_batch);
  if (src < 0 || src >= d.max_batch) return set_err(c, TGX_ERR_INVALID, "source row %d out of range [0,%d)", src, d.max_batch);
  if (int rc = check_target_rows(c, n, dst_rows, /*lens=*/nullptr, src)) return rc;
  if (((long long)d.head_dim * (long long)c->esz) % 4 != 0) return set_err(c, TGX_ERR_UNSUPPORTED, "tgx_fork_row: a cache row of %d bytes", (int)(d.head_dim * c->esz));
  const long long past = c->row_host[(size_t)src].past;
  const int n_full = (int)(past / tgx::KV_BLOCK), tail = (int)(past % tgx::KV_BLOCK);
  if (c->kv_paged) {
    // all or nothing: one fresh block per destination for the partial tail, against the free list plus what the destination rows give back
    const long long need = tail ? n : 0, have = c->kv.available_for(dst_rows, n);
    if (need > have)
      return set_err(c, TGX_ERR_CONTEXT, "KV budget exhausted: the fork needs %lld blocks of %d tokens for the rows' tails, %lld free or held by its rows of %d (option kv.budget_tokens = %d)",
                     need, tgx::KV_BLOCK, have, c->kv.n_blocks() - 1, c->kv_budget_tokens);
  }
  HIP_OK(c, hipSetDevice(c->device));
  std::vector<int> dst_blk((size_t)n, 0);
  int src_blk = 0;
  if (c->kv_paged) {
    for (int i = 0; i < n; i++) kv_release_row(c, dst_rows[i]);
    KvPool::Changes ch;      // the table entries of all destinations in ONE push
    for (int i = 0; i < n; i++) {
      c->kv.share(src, dst_rows[i], n_full, past, ch);
      if (tail) dst_blk[(size_t)i] = c->kv.fork_tail(dst_rows[i], ch);            // cannot run dry: counted above
    }
    kv_tbl_push(c, ch);
    if (tail) src_blk = c->kv.block_at(src, n_full);
  }
  launch_kv_fork(c, src, n, dst_rows, dst_blk.data(), src_blk);
  if (c->proc_hist)        // the same sequence, the same history: the source's words into every destination (the destinations' settings are untouched)
    for (int i = 0; i < n; i++)
      HIP_OK(c, hipMemcpyAsync(c->proc_hist + (size_t)dst_rows[i] * d.vocab, c->proc_hist + (size_t)src * d.vocab, (size_t)d.vocab * sizeof(unsigned int), hipMemcpyDeviceToDevice, c->stream));
  if (int rc = finish_pass(c)) return rc;
  for (int i = 0; i < n; i++) {
    c->batch = std::max(c->batch, dst_rows[i] + 1);
    {      // the same sequence, the same automaton and state: like the history words (the mirror of the source's state word is exact: it moves in tgx_decode_rows alone)
      const tgx::RowReq& qs = c->row_req_host[(size_t)src];
      tgx::RowReq& qd = c->row_req_host[(size_t)dst_rows[i]];
      if (qs.auto_next || qd.auto_next) {
        qd.auto_next = qs.auto_next; qd.auto_state = qs.auto_state;
        c->row_host[(size_t)dst_rows[i]].auto_id = c->row_host[(size_t)src].auto_id;
        row_proc_refresh(qd);
        row_req_push(c, dst_rows[i], ROWQ_AUTO);
      }
    }
    row_admitted(c, dst_rows[i], (int)past);
    c->row_host[(size_t)dst_rows[i]].tok = c->row_host[(size_t)src].tok;      // the token word travelled with the copy
  }
  refresh_longest(c);
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

// ---- beam search (include/tgx.h tgx_beam_select / tgx_beam_advance; kernels/beam.h, beam_plan.h).  tgx_beam_select: every check here, the launches and the
// read-back in sampler.hip (beam_select_run).  A refused call changes nothing
static_assert(beam_plan::MAX_BEAMS == TGX_MAX_BEAMS && (int)beam_plan::INVALID == (int)TGX_ERR_INVALID && (int)beam_plan::STATE == (int)TGX_ERR_STATE, "beam_plan.h");
int tgx_beam_select(tgx_ctx* c, int n, const int32_t* rows, const float* scores, int k, const int32_t* end_ids, int n_end, tgx_beam_cand* out, int32_t* out_n) {
  if (!c) return TGX_ERR_INVALID;
  if (!rows || !scores || !out || !out_n) return set_err(c, TGX_ERR_INVALID, "tgx_beam_select: null argument");
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "beam_select before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  if (n < 1 || n > TGX_MAX_BEAMS) return set_err(c, TGX_ERR_INVALID, "tgx_beam_select: n %d out of range [1,%d]", n, TGX_MAX_BEAMS);
  if (k < 1 || k > TGX_MAX_BEAMS) return set_err(c, TGX_ERR_INVALID, "tgx_beam_select: k %d out of range [1,%d]", k, TGX_MAX_BEAMS);
  if (n_end < 0 || n_end > TGX_MAX_STOP_IDS) return set_err(c, TGX_ERR_INVALID, "tgx_beam_select: n_end %d out of range [0,%d]", n_end, TGX_MAX_STOP_IDS);
  if (n_end > 0 && !end_ids) return set_err(c, TGX_ERR_INVALID, "tgx_beam_select: null end_ids with n_end %d", n_end);
  for (int i = 0; i < n; i++) {
    if (rows[i] < 0 || rows[i] >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "tgx_beam_select: row %d out of range [0,%d)", rows[i], c->d.max_batch);
    for (int j = 0; j < i; j++)
      if (rows[j] == rows[i]) return set_err(c, TGX_ERR_INVALID, "tgx_beam_select: row %d named twice", rows[i]);
    if (!std::isfinite(scores[i])) return set_err(c, TGX_ERR_INVALID, "tgx_beam_select: scores[%d] is not finite", i);
  }
  if (!c->have_logits) return set_err(c, TGX_ERR_STATE, "tgx_beam_select: no logits to select from");
  for (int i = 0; i < n; i++) {
    const RowHost& r = c->row_host[(size_t)rows[i]];
    if (rows[i] >= c->batch || r.idle || r.past < 1) return set_err(c, TGX_ERR_STATE, "tgx_beam_select: row %d is not a live row of the batch", rows[i]);
    if (r.fin) return set_err(c, TGX_ERR_STATE, "tgx_beam_select: row %d finished on the device", rows[i]);
    if (r.nologits) return set_err(c, TGX_ERR_STATE, "tgx_beam_select: row %d was truncated and holds no logits: tgx_extend_row it first", rows[i]);
  }
  HIP_OK(c, hipSetDevice(c->device));      // (tgx_finalize refused a vocabulary of more tiles than lp_merge ranks: sampler_alloc)
  return beam_select_run(c, n, rows, scores, k, end_ids, n_end, out, out_n);
}

// tgx_beam_advance: beam_plan.h decides (validation, placement, block count) before anything changes; then the childless sources retire as by tgx_reset_row, every
// pool change of the call goes to the device table in ONE push, each parent with copied children takes ONE kv_fork_kernel launch (tgx_fork_row's, unchanged), and
// ONE publish launch gives every placed row its token and next embedding.  The launch sequence ends in finish_pass like a fork
int tgx_beam_advance(tgx_ctx* c, int n_rows, const int32_t* rows, int n_next, const int32_t* parent, const int32_t* tokens, int32_t* out_rows) {
  if (!c) return TGX_ERR_INVALID;
  if (!rows || !parent || !tokens || !out_rows) return set_err(c, TGX_ERR_INVALID, "tgx_beam_advance: null argument");
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "beam_advance before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  const tgx_model_desc& d = c->d;
  // ---- every check before anything changes
  std::vector<beam_plan::RowState> st((size_t)d.max_batch);
  for (int r = 0; r < d.max_batch; r++) { const RowHost& h = c->row_host[(size_t)r]; st[(size_t)r].past = h.past; st[(size_t)r].idle = h.idle; st[(size_t)r].fin = h.fin != 0; st[(size_t)r].nologits = h.nologits; }
  beam_plan::Plan plan;
  const char* why = "";
  if (const int rc = beam_plan::make(d.max_batch, c->batch, d.vocab, st.data(), n_rows, rows, n_next, parent, tokens, &plan, &why)) return set_err(c, rc, "tgx_beam_advance: %s", why);
  if (!c->have_logits) return set_err(c, TGX_ERR_STATE, "tgx_beam_advance: no logits");
  if (plan.n_copies && ((long long)d.head_dim * (long long)c->esz) % 4 != 0) return set_err(c, TGX_ERR_UNSUPPORTED, "tgx_beam_advance: a cache row of %d bytes", (int)(d.head_dim * c->esz));
  if (c->kv_paged) {
    const long long need = beam_plan::fresh_blocks(plan, tgx::KV_BLOCK), have = beam_plan::available(c->kv, plan);
    if (need > have)
      return set_err(c, TGX_ERR_CONTEXT, "KV budget exhausted: the beam step needs %lld blocks of %d tokens for the copied rows' tails, %lld free or held by its childless rows of %d (option kv.budget_tokens = %d)",
                     need, tgx::KV_BLOCK, have, c->kv.n_blocks() - 1, c->kv_budget_tokens);
  }
  HIP_OK(c, hipSetDevice(c->device));
  // ---- the sources without a child retire (tgx_reset_row; their blocks go back with the call's one table push below)
  for (int i = 0; i < plan.n_retire; i++) {
    const int row = plan.retire[i];
    HIP_OK(c, hipMemsetAsync(c->rows[(size_t)row].pos, 0, 4, c->stream));
    row_req_reset(c, row);
    if (c->proc_hist) HIP_OK(c, hipMemsetAsync(c->proc_hist + (size_t)row * d.vocab, 0, (size_t)d.vocab * sizeof(unsigned int), c->stream));
    c->row_host[(size_t)row].restart(0, /*idle=*/true, /*fin=*/0);
  }
  beam_plan::Blocks blk;
  if (c->kv_paged) {
    KvPool::Changes ch;
    blk = beam_plan::apply(c->kv, plan, ch);      // cannot run dry: counted above
    kv_tbl_push(c, ch);
  }
  // ---- the copied children: tgx_fork_row's destination, word for word
  for (int g = 0; g < plan.n_groups; g++) {
    const beam_plan::Group& gr = plan.group[g];
    launch_kv_fork(c, gr.src, gr.n_dst, gr.dst, blk.tail_blk[g], blk.src_blk[g]);
    if (c->proc_hist)
      for (int k = 0; k < gr.n_dst; k++)
        HIP_OK(c, hipMemcpyAsync(c->proc_hist + (size_t)gr.dst[k] * d.vocab, c->proc_hist + (size_t)gr.src * d.vocab, (size_t)d.vocab * sizeof(unsigned int), hipMemcpyDeviceToDevice, c->stream));
  }
  // ---- every placed row: its token and the next embedding at its position
  launch_beam_publish(c, n_next, plan.out_rows, tokens);
  if (int rc = finish_pass(c)) return rc;
  c->batch = std::max(c->batch, plan.new_batch);
  for (int g = 0; g < plan.n_groups; g++) {
    const beam_plan::Group& gr = plan.group[g];
    for (int k = 0; k < gr.n_dst; k++) {
      const int dst = gr.dst[k];
      const tgx::RowReq& qs = c->row_req_host[(size_t)gr.src];
      tgx::RowReq& qd = c->row_req_host[(size_t)dst];
      if (qs.auto_next || qd.auto_next) {      // the same sequence, the same automaton and state (tgx_fork_row)
        qd.auto_next = qs.auto_next; qd.auto_state = qs.auto_state;
        c->row_host[(size_t)dst].auto_id = c->row_host[(size_t)gr.src].auto_id;
        row_proc_refresh(qd);
        row_req_push(c, dst, ROWQ_AUTO);
      }
      row_admitted(c, dst, (int)gr.past);
    }
  }
  for (int j = 0; j < n_next; j++) {
    c->row_host[(size_t)plan.out_rows[j]].tok = true;
    if (plan.out_rows[j] == 0) c->last_sampled0 = tokens[j];      // ticket 0's token, as after tgx_sample
    out_rows[j] = plan.out_rows[j];
  }
  refresh_longest(c);
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

// ---- row snapshots (include/tgx.h tgx_save_row / tgx_restore_row; csrc/row_snapshot.h holds the format, kernels/kv_pack.h the copy launches).  The snapshot moves
// through ONE device staging buffer in groups of whole layers: a save runs one pack launch and one copy to the host per group, a restore one copy and one unpack
// launch.  The state section (position and token words, hidden row, logits) travels with the first group, in front of its KV bytes — the bytes [128, KV offset +
// the group's layers) of the blob are one copy.  Option snapshot.stage_kib caps the buffer (one layer is always staged); it is allocated by the first call that
// moves a snapshot: a context that never does holds none of it.
static row_snapshot::Geometry snap_geometry(const tgx_ctx* c) {
  const tgx_model_desc& d = c->d;
  return {d.family, d.hidden, d.layers, d.heads, d.kv_heads, d.head_dim, d.vocab, d.compute_dtype, d.qk_norm};
}
// the checks of a save's source, and the layout of its snapshot
static int snap_source(tgx_ctx* c, int row, row_snapshot::Layout* out) {
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "snapshot before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  const RowHost& r = c->row_host[(size_t)row];
  if (row >= c->batch || r.idle || r.fin || r.past < 1) return set_err(c, TGX_ERR_STATE, "row %d is not a live, unfinished row of the batch", row);
  const bool logits = c->have_logits && !r.nologits;
  *out = row_snapshot::layout(snap_geometry(c), r.past, (logits ? row_snapshot::FLAG_LOGITS : 0u) | (logits && r.tok ? row_snapshot::FLAG_TOKEN : 0u));
  return TGX_OK;
}
struct SnapGroups { long long layer_bytes; size_t state_area; int per_group; };
// the groups of whole layers a snapshot laid out as l moves in, and the staging buffer that holds one of them behind the state area
static int snap_stage_for(tgx_ctx* c, const row_snapshot::Layout& l, SnapGroups* g) {
  g->layer_bytes = (long long)row_snapshot::layer_bytes(snap_geometry(c), l.past);
  g->state_area = (size_t)(l.kv_off - l.state_off);
  const long long room = (long long)c->snapshot_stage_kib * 1024 - (long long)g->state_area;
  g->per_group = (int)std::max<long long>(1, std::min<long long>(c->d.layers, room / g->layer_bytes));
  return dev_grow(c, &c->snap_stage, &c->snap_stage_bytes, g->state_area + (size_t)g->per_group * (size_t)g->layer_bytes);
}
// one kv_pack_kernel launch: layers [l0, l0 + nl) of `row`, past positions each, between the cache and staging + state_area; with_state: the state section as well
static void launch_kv_pack(tgx_ctx* c, int row, long long past, int l0, int nl, size_t state_area, bool with_state, bool logits, bool unpack) {
  const tgx_model_desc& d = c->d;
  const long long tok_bytes = (long long)d.head_dim * (long long)c->esz;
  const bool v16 = tok_bytes % 16 == 0;
  const int vec = v16 ? 16 : 4;
  tgx::KvPackArgs a{};
  a.stage = c->snap_stage + state_area;
  if (c->kv_paged) {
    a.k = c->slab_k; a.v = c->slab_v; a.tbl = c->kv_tbl + (size_t)row * c->kv.tbl_stride();
    a.head_stride = tgx::KV_BLOCK * tok_bytes; a.piece_stride = d.kv_heads * a.head_stride; a.layer_stride = c->kv.n_blocks() * a.piece_stride;
  } else {
    a.k = c->rows[(size_t)row].kcache; a.v = c->rows[(size_t)row].vcache; a.tbl = nullptr;
    a.piece_stride = tgx::KV_BLOCK * tok_bytes; a.head_stride = d.max_ctx * tok_bytes; a.layer_stride = d.kv_heads * a.head_stride;
  }
  a.span_vecs = past * tok_bytes / vec; a.piece_vecs = (int)(tgx::KV_BLOCK * tok_bytes / vec);
  a.n_pieces = (int)((past + tgx::KV_BLOCK - 1) / tgx::KV_BLOCK);
  a.layer0 = l0; a.kv_heads = d.kv_heads; a.n_spans = nl * 2 * d.kv_heads;
  // the grid from the pieces to move, within eight workgroups per CU as launch_kv_fork's (the rest in the kernel's loops).  x: the pieces of a span; y: the spans
  const long long cap = 8ll * c->num_cus;
  const int gx = (int)std::max<long long>(1, std::min<long long>(a.n_pieces, cap));
  a.kv_rows = (int)std::max<long long>(1, std::min<long long>(a.n_spans, cap / gx));
  int st_rows = 0;
  if (with_state) {
    const size_t H = (size_t)d.hidden, V = (size_t)d.vocab;
    unsigned char* const st = c->snap_stage;
    a.seg[0] = {reinterpret_cast<unsigned char*>(c->slab_pos + row), st, 1};
    a.seg[1] = {reinterpret_cast<unsigned char*>(c->slab_tok + row), st + 4, 1};
    a.n_seg = 2;
    if (logits) {
      a.seg[2] = {reinterpret_cast<unsigned char*>(c->slab_x + (size_t)row * H), st + 8, (int)H};
      a.seg[3] = {reinterpret_cast<unsigned char*>(c->slab_logits + (size_t)row * V), st + 8 + 4 * H, (int)V};
      a.n_seg = 4;
    }
    st_rows = ((int)std::min<size_t>(64, logits ? (V + 1023) / 1024 : 1) + gx - 1) / gx;      // the state part: up to 64 workgroups, a dword per thread and round
  }
  const dim3 grid((unsigned)gx, (unsigned)(a.kv_rows + st_rows)), block(tgx::KV_PACK_THREADS);
  if (v16) {
    if (unpack) hipLaunchKernelGGL((tgx::kv_pack_kernel<tgx::u32x4, true>), grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL((tgx::kv_pack_kernel<tgx::u32x4, false>), grid, block, 0, c->stream, a);
  } else {
    if (unpack) hipLaunchKernelGGL((tgx::kv_pack_kernel<unsigned int, true>), grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL((tgx::kv_pack_kernel<unsigned int, false>), grid, block, 0, c->stream, a);
  }
}

int tgx_row_snapshot_bytes(const tgx_ctx* cc, int row, int64_t* out_bytes) {
  tgx_ctx* c = const_cast<tgx_ctx*>(cc);      // (the error text alone is written)
  if (!c || !out_bytes) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  row_snapshot::Layout l;
  if (int rc = snap_source(c, row, &l)) return rc;
  *out_bytes = (int64_t)l.total;
  return TGX_OK;
}

int tgx_save_row(tgx_ctx* c, int row, void* buf, int64_t cap, int64_t* out_bytes) {
  if (!c || !buf || !out_bytes) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  row_snapshot::Layout l;
  if (int rc = snap_source(c, row, &l)) return rc;
  if (cap < (int64_t)l.total) return set_err(c, TGX_ERR_INVALID, "tgx_save_row: the snapshot of row %d takes %llu bytes, the buffer holds %lld", row, (unsigned long long)l.total, (long long)cap);
  const tgx_model_desc& d = c->d;
  if (((long long)d.head_dim * (long long)c->esz) % 4 != 0) return set_err(c, TGX_ERR_UNSUPPORTED, "tgx_save_row: a cache row of %d bytes", (int)(d.head_dim * c->esz));
  HIP_OK(c, hipSetDevice(c->device));
  SnapGroups g;
  if (int rc = snap_stage_for(c, l, &g)) return rc;
  unsigned char* const out = static_cast<unsigned char*>(buf);
  const bool logits = (l.flags & row_snapshot::FLAG_LOGITS) != 0;
  for (int l0 = 0; l0 < d.layers; l0 += g.per_group) {
    const int nl = std::min(g.per_group, d.layers - l0);
    launch_kv_pack(c, row, l.past, l0, nl, g.state_area, /*with_state=*/l0 == 0, logits, /*unpack=*/false);
    const size_t kv_at = (size_t)l.kv_off + (size_t)l0 * (size_t)g.layer_bytes, kv_n = (size_t)nl * (size_t)g.layer_bytes;
    if (l0 == 0) HIP_OK(c, hipMemcpyAsync(out + l.state_off, c->snap_stage, g.state_area + kv_n, hipMemcpyDeviceToHost, c->stream));      // state | padding | the first group
    else HIP_OK(c, hipMemcpyAsync(out + kv_at, c->snap_stage + g.state_area, kv_n, hipMemcpyDeviceToHost, c->stream));
  }
  if (int rc = finish_pass(c)) return rc;
  row_snapshot::write_header(out, snap_geometry(c), l);
  if (!(l.flags & row_snapshot::FLAG_TOKEN)) row_snapshot::put32(out + l.state_off + 4, 0);      // no current token: the word reads 0, whatever the slot held
  memset(out + l.state_off + l.state_bytes, 0, (size_t)(l.kv_off - l.state_off - l.state_bytes));      // the padding in front of the KV section
  *out_bytes = (int64_t)l.total;
  return TGX_OK;
}

int tgx_restore_row(tgx_ctx* c, int row, const void* buf, int64_t bytes) {
  if (!c || !buf) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "restore before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  const tgx_model_desc& d = c->d;
  // ---- every check before anything changes
  const int32_t r32 = row;
  if (int rc = check_target_rows(c, 1, &r32, /*lens=*/nullptr, /*src=*/-1)) return rc;
  row_snapshot::Layout l;
  int32_t tok = 0;
  const char* why = "";
  if (const int v = row_snapshot::validate(buf, bytes, snap_geometry(c), d.max_ctx, &l, &tok, &why)) return set_err(c, v, "tgx_restore_row: not a snapshot this context can restore: %s", why);
  if (((long long)d.head_dim * (long long)c->esz) % 4 != 0) return set_err(c, TGX_ERR_UNSUPPORTED, "tgx_restore_row: a cache row of %d bytes", (int)(d.head_dim * c->esz));
  if (c->kv_paged) {
    const long long need = c->kv.blocks_for(l.past), have = c->kv.available_for(&row, 1);
    if (need > 1024) return set_err(c, TGX_ERR_UNSUPPORTED, "tgx_restore_row of %lld blocks into a paged cache (at most 1024 per row)", need);
    if (need > have)
      return set_err(c, TGX_ERR_CONTEXT, "KV budget exhausted: the snapshot needs %lld blocks of %d tokens, %lld free or held by row %d of %d (option kv.budget_tokens = %d)", need,
                     tgx::KV_BLOCK, have, row, c->kv.n_blocks() - 1, c->kv_budget_tokens);
  }
  HIP_OK(c, hipSetDevice(c->device));
  SnapGroups g;
  if (int rc = snap_stage_for(c, l, &g)) return rc;
  if (c->kv_paged) {       // blocks of its own for every position: nothing is shared, no shared block is written
    kv_release_row(c, row);
    (void)kv_ensure_blocks(c, row, l.past);      // cannot fail: counted above
  }
  const unsigned char* const in = static_cast<const unsigned char*>(buf);
  const bool logits = (l.flags & row_snapshot::FLAG_LOGITS) != 0, has_tok = (l.flags & row_snapshot::FLAG_TOKEN) != 0;
  for (int l0 = 0; l0 < d.layers; l0 += g.per_group) {
    const int nl = std::min(g.per_group, d.layers - l0);
    const size_t kv_at = (size_t)l.kv_off + (size_t)l0 * (size_t)g.layer_bytes, kv_n = (size_t)nl * (size_t)g.layer_bytes;
    if (l0 == 0) HIP_OK(c, hipMemcpyAsync(c->snap_stage, in + l.state_off, g.state_area + kv_n, hipMemcpyHostToDevice, c->stream));
    else HIP_OK(c, hipMemcpyAsync(c->snap_stage + g.state_area, in + kv_at, kv_n, hipMemcpyHostToDevice, c->stream));
    launch_kv_pack(c, row, l.past, l0, nl, g.state_area, /*with_state=*/l0 == 0, logits, /*unpack=*/true);
  }
  if (logits) {            // the argmax partials depend on lm_grid and are not held: from the logits, as tgx_set_logits does
    RowState& r = c->rows[(size_t)row];
    launch_argmax_partials(c, r.logits, d.vocab, r.part_val, r.part_idx);
  }
  if (int rc = finish_pass(c)) return rc;
  c->batch = std::max(c->batch, row + 1);
  row_admitted(c, row, (int)l.past);
  c->row_host[(size_t)row].tok = has_tok;
  c->row_host[(size_t)row].nologits = !logits;
  if (logits) c->have_logits = true;
  if (row == 0 && has_tok) c->last_sampled0 = tok;      // ticket 0's token, as after tgx_sample
  refresh_longest(c);
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

// ---- the continuation calls (include/tgx.h): live rows grow by several positions in one pass.  tgx_extend_row / tgx_score_row on a held row (a FEED of one row),
// tgx_verify_row / tgx_verify_row_sampled (a STEP of one row: its current token and a draft, accepted on the device), tgx_verify_rows (n STEPs), tgx_advance_rows
// (STEPs, FEEDs and admissions together).  Every call runs its own argument checks, in its own order and words, before anything changes; behind them ONE
// description of the pass (ContPass) serves the blocks the calls share: the paged cache's room (check_paged_room), the STEP launches behind a joint pass (step_tail),
// the host's bookkeeping from the device's records (follow_step_rows), the call's buffer (call_buffer), and the joint pass itself (joint_pass).
static bool row_holds(const tgx_ctx* c, int row) { return row < c->batch && !c->row_host[(size_t)row].idle && c->row_host[(size_t)row].past >= 1; }      // (row >= 0) a sequence to continue

// One continuation pass: its sequences in workspace order — the STEP sequences first, then the FEED / FEED_MORE ones, both in the caller's array order, so that the
// STEP sequences alone are the pass's first ns sequences and first Ms workspace rows.  Built once per call, behind the call's checks
struct ContPass {
  int n = 0, ns = 0, M = 0, Ms = 0;                         // sequences and workspace rows; the STEP ones among them
  // per sequence: batch row, index in the caller's arrays, TGX_ADV_*, first workspace row, positions in the pass (a STEP: n_draft + 1), the position it starts
  // at (an admission: 0), n_draft (a FEED: 0)
  std::vector<int> rows, idx, kind, first, lens, past, nd;
  std::vector<const int64_t*> ids;                          // its ids in the caller's array (a STEP: the draft)
  std::vector<char> holds, smp;                             // the row holds a sequence (0: an admission); a STEP row that does not sample greedily
  std::vector<char> prc;                                    // a STEP row with a logit processor on (option verify.processors let it through)
  bool any_processed = false;
  std::vector<tgx_sampler_cfg> cfg;                         // a STEP row's sampler settings
  std::vector<tgx::VerifyRecord> rec;                       // the STEP rows' records, read back behind the pass
  std::vector<int> adm;                                     // the admissions' rows
  bool any_sampled = false;
  void add(const tgx_ctx* c, int row, int i, int k, const int64_t* src, int len) {      // (every STEP before the first FEED)
    const bool step = k == TGX_ADV_STEP, held = step || row_holds(c, row);
    const int sl = len + (step ? 1 : 0);
    rows.push_back(row); idx.push_back(i); kind.push_back(k); ids.push_back(src); first.push_back(M); lens.push_back(sl); nd.push_back(step ? len : 0);
    past.push_back(held ? (int)c->row_host[(size_t)row].past : 0); holds.push_back(held);
    cfg.push_back(step ? row_cfg(c, row) : tgx_sampler_cfg{}); smp.push_back(step && !is_greedy(&cfg.back()));
    any_sampled = any_sampled || smp.back();
    prc.push_back(step && row_processed(c, row)); any_processed = any_processed || prc.back();
    if (!held) adm.push_back(row);
    n++; M += sl;
    if (step) { ns++; Ms += sl; rec.emplace_back(); }
  }
  // the ragged pass over all sequences, or over the STEP sequences alone
  RaggedPass view(bool steps_only) const {
    RaggedPass p;
    p.n = steps_only ? ns : n; p.M = steps_only ? Ms : M;
    p.rows = rows.data(); p.lens = lens.data(); p.first = first.data(); p.past = past.data();
    for (int j = 0; j < p.n; j++) p.longest = std::max(p.longest, lens[(size_t)j]);
    return p;
  }
};
// the pass of an n-row call: row rows[i] takes lens[i] ids, the rows' ids back to back; kinds nullptr (tgx_verify_rows): every sequence a STEP
static ContPass cont_pass(const tgx_ctx* c, int n, const int32_t* rows, const int32_t* kinds, const int64_t* ids, const int32_t* lens) {
  ContPass cp;
  for (int steps = 1; steps >= 0; steps--) {
    long long off = 0;
    for (int i = 0; i < n; off += lens[i], i++) {
      const int k = kinds ? kinds[i] : TGX_ADV_STEP;
      if ((k == TGX_ADV_STEP) == (bool)steps) cp.add(c, rows[i], i, k, ids ? ids + off : nullptr, lens[i]);
    }
  }
  return cp;
}

// A row named by an n-row call: refused the second time (a row out of range is left to the row's own checks)
static int name_row(tgx_ctx* c, std::vector<char>& named, int row) {
  if (row < 0 || row >= c->d.max_batch) return TGX_OK;
  if (named[(size_t)row]) return set_err(c, TGX_ERR_INVALID, "row %d named twice", row);
  named[(size_t)row] = 1;
  return TGX_OK;
}

// The paged cache's room for a pass, all or nothing: the blocks of all its sequences together against the free list plus what the admissions' rows give back.
// Ahead of it the refusal of more than 1024 blocks per row where the joint pass, or some sequence's own pass (the piecewise forms), takes a matrix-core route: the
// prompt attention copies the row's block table into LDS (<= 1024 entries).  The budget message keeps each call's words.
// (The block a continuation's first new position falls into is the row's own: a block forked siblings map as well is full, and tgx_truncate_row copies before it
// leaves a row inside one.)
enum RoomWords { ROOM_ROW, ROOM_CALL, ROOM_CALL_ADM };
static int check_paged_room(tgx_ctx* c, const ContPass& cp, const char* fn, RoomWords words) {
  if (!c->kv_paged) return TGX_OK;
  auto matrix_core = [&](int len) { const PrefillRoute rt = prefill_route(c, len, len); return rt == ROUTE_SKINNY || rt == ROUTE_TILED; };
  bool mfma = matrix_core(cp.M);
  for (int j = 0; j < cp.n && !mfma; j++) mfma = matrix_core(cp.lens[(size_t)j]);
  if (mfma && c->kv.tbl_stride() > 1024)
    return set_err(c, TGX_ERR_UNSUPPORTED, "%s on a paged cache of %d blocks per row (at most 1024: max_ctx <= %d)", fn, c->kv.tbl_stride(), 1024 * tgx::KV_BLOCK);
  long long need = 0;
  for (int j = 0; j < cp.n; j++)
    need += c->kv.blocks_for((long long)cp.past[(size_t)j] + cp.lens[(size_t)j]) - (cp.holds[(size_t)j] ? c->kv.row_blocks(cp.rows[(size_t)j]) : 0);
  const long long have = c->kv.available_for(cp.adm.data(), (int)cp.adm.size());
  if (need <= have) return TGX_OK;
  const std::string who = words == ROOM_ROW ? "row " + std::to_string(cp.rows[0]) : std::string("the call");
  return set_err(c, TGX_ERR_CONTEXT, "KV budget exhausted: %s needs %lld more blocks of %d tokens, %lld %s of %d (option kv.budget_tokens = %d)", who.c_str(), need, tgx::KV_BLOCK,
                 have, words == ROOM_CALL_ADM ? "free or held by its admissions' rows" : "free", c->kv.n_blocks() - 1, c->kv_budget_tokens);
}

// The host follows the device: the STEP sequences [j0, j1) of a pass that has gone through, from their records — a record outside [1, positions] poisons the
// context; else length, blocks (those assigned for the rejected tail go back to the pool), finished state, the log-probability count, the probabilities' state
// (greedy: tgx_read_probs reads zeros for the row; sampled: the pass's scratch is not the row's, no vector until its next sampled step — the rule of tgx_fork_row)
// and the caller's results.  The caller refreshes have_probs once its other rows are settled
static int follow_step_rows(tgx_ctx* c, const ContPass& cp, int j0, int j1, const char* fn, int64_t* out_ids, int32_t* out_n, int32_t* out_finish) {
  for (int j = j0; j < j1; j++)
    if (cp.rec[(size_t)j].n < 1 || cp.rec[(size_t)j].n > cp.lens[(size_t)j]) { c->poisoned = true; return set_err(c, TGX_ERR_DEVICE, "%s: the accept launch left no record for row %d", fn, cp.rows[(size_t)j]); }
  for (int j = j0; j < j1; j++) {
    const int row = cp.rows[(size_t)j], i = cp.idx[(size_t)j];
    const tgx::VerifyRecord& rec = cp.rec[(size_t)j];
    RowHost& r = c->row_host[(size_t)row];
    r.past = cp.past[(size_t)j] + rec.n;
    r.fin = (char)rec.finish;
    if (row_records(c, row)) r.lp_count += rec.n;
    kv_trim_row(c, row, r.past);
    if (cp.prc[(size_t)j] && c->row_host[(size_t)row].auto_id >= 0) c->row_req_host[(size_t)row].auto_state = rec.state;      // the mirror follows the commit
    if (!cp.smp[(size_t)j]) note_sampled(c, row, 1, cp.cfg[(size_t)j]);
    else r.probs_ok = false;
    for (int k = 0; k < rec.n; k++) out_ids[(size_t)i * (TGX_MAX_DRAFT + 1) + k] = rec.ids[k];
    out_n[i] = rec.n; out_finish[i] = rec.finish;
    if (row == 0) c->last_sampled0 = rec.ids[rec.n - 1];
  }
  return TGX_OK;
}

// ---- tgx_extend_row (include/tgx.h): a live row grows by several positions in one pass.  The pass is issue_pass's one-row pass with the row's real length as
// `past` (every route takes it); the row then stands as tgx_forward_row leaves one.
static int extend_row(tgx_ctx* c, int row, const int64_t* ids, int seq, ScoreCall* sc) {      // sc (tgx_score_row): the pass also scores its positions
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "extend before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  const tgx_model_desc& d = c->d;
  if (row < 0 || row >= d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, d.max_batch);
  if (seq < 1) return set_err(c, TGX_ERR_INVALID, "seq %d < 1", seq);
  if (!row_holds(c, row)) return set_err(c, TGX_ERR_STATE, "row %d holds no sequence to extend: use tgx_forward_row", row);
  const long long past = c->row_host[(size_t)row].past;
  if (past + seq > d.max_ctx) return set_err(c, TGX_ERR_CONTEXT, "context size exceeded: row %d holds %lld positions, + %d > %d", row, past, seq, d.max_ctx);
  for (int i = 0; i < seq; i++)
    if (ids[i] < 0 || ids[i] >= d.vocab) return set_err(c, TGX_ERR_INVALID, "token id out of range");
  ContPass cp;
  cp.add(c, row, 0, TGX_ADV_FEED, ids, seq);
  if (int rc = check_paged_room(c, cp, "tgx_extend_row", ROOM_ROW)) return rc;
  HIP_OK(c, hipSetDevice(c->device));
  if (int rc = ensure_extend_ws(c, seq, (int)past)) return rc;
  const PrefillRoute sc_rt = prefill_route(c, seq, seq);
  if (sc) if (int rc = score_prepare(c, sc, sc_rt, row)) return rc;
  (void)kv_ensure_blocks(c, row, past + seq);      // cannot fail: counted above
  HIP_OK(c, hipMemcpyAsync(c->rows[(size_t)row].prompt, ids, (size_t)seq * 8, hipMemcpyHostToDevice, c->stream));
  if (int rc = issue_pass(c, row, 1, seq, (int)past, /*verify=*/false, sc)) return rc;
  if (sc) if (int rc = score_read_back(c, sc)) return rc;
  if (int rc = finish_pass(c)) return rc;
  if (sc && sc->n_score >= 1) c->score_last_form = sc_rt == ROUTE_TILED ? 1 : 2;      // (a call of one position scored nothing: the option keeps its value)
  row_admitted(c, row, (int)(past + seq), /*keep_lp_count=*/true);         // no current token, a fresh stop state (a finished row runs again), the sampler settings kept
  refresh_longest(c);
  c->have_logits = true;
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

int tgx_extend_row(tgx_ctx* c, int row, const int64_t* ids, int seq) {
  if (!c || !ids) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  return extend_row(c, row, ids, seq, nullptr);
}

// ---- tgx_score_row (include/tgx.h): tgx_forward_row (an empty row) or tgx_extend_row (a row that holds a sequence) — the same checks in the same order, the same pass,
// the same row state afterwards — plus the log-probability of every supplied token, computed behind the pass (issue_pass) and read back once.  The call's own
// argument checks come first; nothing is recorded in the row's logprobs ring
int tgx_score_row(tgx_ctx* c, int row, const int64_t* ids, int seq, int top_n, float* out_lp, int32_t* out_top_ids, float* out_top_lp) {
  if (!c || !ids) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  if (top_n < 0 || top_n > TGX_MAX_LOGPROBS) return set_err(c, TGX_ERR_INVALID, "top_n %d out of range [0,%d]", top_n, TGX_MAX_LOGPROBS);
  if (seq > 1 && !out_lp) return set_err(c, TGX_ERR_INVALID, "null out_lp for %d scored positions", seq - 1);
  ScoreCall sc;
  sc.top_n = top_n; sc.n_score = std::max(0, seq - 1);
  const size_t n = (size_t)sc.n_score, L = TGX_MAX_LOGPROBS;
  const bool tops = out_top_ids || out_top_lp;
  std::vector<uint32_t> host;
  if (c->finalized && seq <= c->d.max_ctx) {
    host.resize(tops ? n * (1 + 2 * L) : n);
    sc.host = host.data(); sc.host_bytes = host.size() * 4;
  } else sc.n_score = 0;      // (the pass is refused below)
  const bool holds = c->finalized && row >= 0 && row_holds(c, row);
  const int32_t r = row, s = seq;
  const int rc = holds ? extend_row(c, row, ids, seq, &sc) : admit_rows(c, 1, &r, ids, &s, /*may_join=*/false, &sc);
  if (rc || !n) return rc;
  std::memcpy(out_lp, host.data(), n * 4);
  if (out_top_ids) std::memcpy(out_top_ids, host.data() + n, n * L * 4);
  if (out_top_lp) std::memcpy(out_top_lp, host.data() + n + n * L, n * L * 4);
  return TGX_OK;
}

// ---- tgx_verify_row / tgx_verify_row_sampled (include/tgx.h): speculative decoding on one row.  ONE causal pass — tgx_extend_row's, on whatever route it takes —
// over the row's current token and the draft, with the logits of every position (issue_pass's verify form); a row that does not sample greedily then draws every
// position with its own sampler; ONE accept launch (kernels/verify.h) takes the draft's matching prefix and leaves the row as that many decode steps would.
// One STEP row's checks, the same for the one-row calls (min_draft 1) and for every STEP row of tgx_verify_rows / tgx_advance_rows (min_draft 0), in this order;
// sampled_entry false (tgx_verify_row): a row that does not sample greedily is refused.  Nothing changes
// (count_name / id_name: what the call names the two arguments — tgx_verify_tree's are n_nodes and tokens)
static int verify_row_check(tgx_ctx* c, int row, const int64_t* draft, int n_draft, int min_draft, bool sampled_entry, const char* fn, const char* count_name = "n_draft",
                            const char* id_name = "draft token id") {
  const tgx_model_desc& d = c->d;
  if (row < 0 || row >= d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, d.max_batch);
  if (n_draft < min_draft || n_draft > TGX_MAX_DRAFT) return set_err(c, TGX_ERR_INVALID, "%s %d out of range [%d,%d]", count_name, n_draft, min_draft, TGX_MAX_DRAFT);
  for (int i = 0; i < n_draft; i++)
    if (draft[i] < 0 || draft[i] >= d.vocab) return set_err(c, TGX_ERR_INVALID, "%s out of range", id_name);
  const RowHost& rh = c->row_host[(size_t)row];
  if (!row_holds(c, row)) return set_err(c, TGX_ERR_STATE, "row %d holds no sequence to verify a draft on", row);
  if (rh.fin) return set_err(c, TGX_ERR_STATE, "row %d finished: tgx_extend_row / tgx_reset_row it first", row);
  if (rh.nologits) return set_err(c, TGX_ERR_STATE, "row %d was truncated and holds no logits: tgx_extend_row it first", row);
  if (!rh.tok) return set_err(c, TGX_ERR_STATE, "row %d has no current token: tgx_sample_row it first", row);
  const tgx_sampler_cfg cfg = row_cfg(c, row);
  if (!is_greedy(&cfg) && !sampled_entry) return set_err(c, TGX_ERR_UNSUPPORTED, "tgx_verify_row: row %d does not sample greedily (verification under sampling is not built)", row);
  if (row_processed(c, row) && !c->verify_processors) return set_err(c, TGX_ERR_UNSUPPORTED, "%s: row %d has a logit processor on (the accept rule compares raw argmaxes)", fn, row);
  if (rh.past + n_draft + 1 > d.max_ctx) return set_err(c, TGX_ERR_CONTEXT, "context size exceeded: row %d holds %lld positions, + %d > %d", row, (long long)rh.past, n_draft + 1, d.max_ctx);
  return TGX_OK;
}
// ... and behind the checks, STEP sequence j of a pass by itself: the one-row pass, the draws of a sampled row, the accept launch, the host's bookkeeping (the
// row-by-row form of verify_steps runs it per row: n_draft 0 is then a pass of the current token alone)
static int verify_row_run(tgx_ctx* c, ContPass& cp, int j, const char* fn, int64_t* out_ids, int32_t* out_n, int32_t* out_finish) {
  const int row = cp.rows[(size_t)j], M = cp.lens[(size_t)j], past = cp.past[(size_t)j];
  const bool sampled = cp.smp[(size_t)j];
  static_assert((int)tgx_ctx::VERIFY_ROWS == tgx::VERIFY_MAX_POS, "kernels/verify.h VerifyRecord");
  HIP_OK(c, hipSetDevice(c->device));
  if (int rc = ensure_verify_ws(c)) return rc;
  if (sampled) if (int rc = vs_alloc(c)) return rc;      // the positions' sampler workspace: only a sampled row's call ever holds it
  const bool processed = cp.prc[(size_t)j];
  if (processed) if (int rc = ensure_verify_proc_ws(c, /*joint=*/false)) return rc;      // ... and the processed slab: only a processed row's call
  if (int rc = ensure_extend_ws(c, M, past)) return rc;
  c->vf_pass_rows = 0;                             // the workspace changes hands
  (void)kv_ensure_blocks(c, row, (long long)past + M);      // the whole pass up front; cannot fail: counted above
  long long ids[tgx_ctx::VERIFY_ROWS] = {0};       // inputs 1 .. M - 1 = the draft; input 0 is written on the device from the row's token word
  for (int i = 0; i + 1 < M; i++) ids[i + 1] = cp.ids[(size_t)j][i];
  HIP_OK(c, hipMemcpyAsync(c->rows[(size_t)row].prompt, ids, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
  launch_verify_first_id(c, row);
  if (int rc = issue_pass(c, row, 1, M, past, /*verify=*/true)) return rc;
  if (processed) {      // every position as its step would have processed it (kernels/logit_proc.h): the automaton walk, then the positions launch
    const int first = 0; const char on = 1; const long long* const in = c->rows[(size_t)row].prompt;
    launch_logit_proc_positions(c, 1, &row, &first, &M, &in, &on, /*joint=*/false);
  }
  if (sampled) launch_sample_positions(c, row, M, cp.cfg[(size_t)j], -1, nullptr, processed);      // every position's draw under the row's settings, with the key its step would use
  launch_verify_accept(c, row, M, sampled ? c->vs_draws : nullptr, processed);      // (a processed row: the commit of its history and state rides behind the walk)
  if (row_records(c, row)) launch_logprobs_verify(c, row, M);      // one record per produced token, each from the logits of the position that produced it
  HIP_OK(c, hipMemcpyAsync(&cp.rec[(size_t)j], c->vf_rec, sizeof(tgx::VerifyRecord), hipMemcpyDeviceToHost, c->stream));
  if (int rc = finish_pass(c)) return rc;
  if (int rc = follow_step_rows(c, cp, j, j + 1, fn, out_ids, out_n, out_finish)) return rc;
  c->vf_pass_rows = M; c->vf_pass_joint = false;
  refresh_have_probs(c);
  refresh_longest(c);
  c->have_logits = true;
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

static int verify_row_impl(tgx_ctx* c, int row, const int64_t* draft, int n_draft, int64_t* out_ids, int32_t* out_n, int32_t* out_finish, bool sampled_entry) {
  const char* const fn = sampled_entry ? "tgx_verify_row_sampled" : "tgx_verify_row";
  if (!c || !draft || !out_ids || !out_n || !out_finish) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "verify before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  // ---- every check before anything changes
  if (int rc = verify_row_check(c, row, draft, n_draft, /*min_draft=*/1, sampled_entry, fn)) return rc;
  ContPass cp;
  cp.add(c, row, 0, TGX_ADV_STEP, draft, n_draft);
  if (int rc = check_paged_room(c, cp, fn, ROOM_ROW)) return rc;
  return verify_row_run(c, cp, 0, fn, out_ids, out_n, out_finish);
}
int tgx_verify_row(tgx_ctx* c, int row, const int64_t* draft, int n_draft, int64_t* out_ids, int32_t* out_n, int32_t* out_finish) {
  return verify_row_impl(c, row, draft, n_draft, out_ids, out_n, out_finish, /*sampled_entry=*/false);
}
int tgx_verify_row_sampled(tgx_ctx* c, int row, const int64_t* draft, int n_draft, int64_t* out_ids, int32_t* out_n, int32_t* out_finish) {
  return verify_row_impl(c, row, draft, n_draft, out_ids, out_n, out_finish, /*sampled_entry=*/true);
}

// ---- tgx_verify_tree (include/tgx.h): one more one-sequence member of the family — a STEP of one row whose n_nodes guesses form a token tree (csrc/verify_tree_plan.h)
// instead of a chain.  ONE pass on the skinny route runs the M = n_nodes + 1 positions: position p into cache slot past + p, rotated for past + depth(p), attending
// the history and its own branch (TreePass); the all-position lm_head and a sampled row's chain as for a chain (the draws keyed by depth); the accept launch walks
// the tree on the device and leaves the path; the compaction launch behind it moves the accepted K / V rows into place.  A chain-shaped tree IS
// tgx_verify_row_sampled: it takes that call's launches.
// The skinny route whatever prefill.min_rows says (a speed threshold for chains): prefill_route's conditions without the length test, for M <= 16 rows
static bool tree_route_ok(const tgx_ctx* c, int M) {
  return c->prefill_mfma && c->dt != tgx::DT_F32 && prefill_shapes_ok(c->d) && !c->gpt2 && c->prefill_skinny && c->d.vocab >= 128 && c->prefill_skinny_rows >= M &&
         (c->d.head_dim == 64 || c->d.head_dim == 128);
}
int tgx_verify_tree(tgx_ctx* c, int row, const int64_t* tokens, const int32_t* parent, int n_nodes, int64_t* out_ids, int32_t* out_n, int32_t* out_finish) {
  const char* const fn = "tgx_verify_tree";
  if (!c || !tokens || !parent || !out_ids || !out_n || !out_finish) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "verify before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  static_assert(TGX_MAX_TREE_NODES == TGX_MAX_DRAFT && TGX_MAX_TREE_NODES == verify_tree_plan::MAX_NODES && verify_tree_plan::MAX_POS == tgx::VERIFY_MAX_POS, "root + nodes <= VERIFY_MAX_POS");
  // ---- every check before anything changes.  The argument checks and the row's state, in verify_row_check's order and words ...
  if (int rc = verify_row_check(c, row, tokens, n_nodes, /*min_draft=*/1, /*sampled_entry=*/true, fn, "n_nodes", "token id")) return rc;
  // ... then the tree's shape ...
  verify_tree_plan::Plan tp;
  switch (verify_tree_plan::plan(tokens, parent, n_nodes, tp)) {
    case verify_tree_plan::OK: break;
    case verify_tree_plan::BAD_PARENT: return set_err(c, TGX_ERR_INVALID, "parent[%d] = %d outside [-1,%d): a node's parent stands before it", tp.bad, (int)parent[tp.bad], tp.bad);
    case verify_tree_plan::DUP_SIBLING: return set_err(c, TGX_ERR_INVALID, "node %d carries the token of an earlier child of the same parent", tp.bad);
    case verify_tree_plan::BAD_COUNT: return set_err(c, TGX_ERR_INVALID, "n_nodes %d out of range [1,%d]", n_nodes, TGX_MAX_TREE_NODES);      // (the planner's own check: refused above already)
  }
  if (!tp.chain && row_processed(c, row))
    return set_err(c, TGX_ERR_UNSUPPORTED, "%s: row %d has a logit processor on (not built for a tree that is no chain: a position's history and state depend on its branch)", fn, row);
  ContPass cp;
  cp.add(c, row, 0, TGX_ADV_STEP, tokens, n_nodes);
  if (tp.chain) {      // tgx_verify_row_sampled's pass, launches and bits
    if (int rc = check_paged_room(c, cp, fn, ROOM_ROW)) return rc;
    return verify_row_run(c, cp, 0, fn, out_ids, out_n, out_finish);
  }
  // ... what a tree that is no chain cannot have, the route and the room
  const int M = tp.M, past = cp.past[0];
  if (row_records(c, row)) return set_err(c, TGX_ERR_UNSUPPORTED, "%s: row %d records log-probabilities (not built for a tree that is no chain)", fn, row);
  if (!tree_route_ok(c, M))
    return set_err(c, TGX_ERR_UNSUPPORTED, "%s: a tree that is no chain needs the skinny matrix-core pass (16-bit storage, no GPT-2, prefill.mfma and prefill.skinny on, head_dim 64 or 128)", fn);
  if (c->kv_paged && c->kv.tbl_stride() > 1024)
    return set_err(c, TGX_ERR_UNSUPPORTED, "%s on a paged cache of %d blocks per row (at most 1024: max_ctx <= %d)", fn, c->kv.tbl_stride(), 1024 * tgx::KV_BLOCK);
  if (int rc = check_paged_room(c, cp, fn, ROOM_ROW)) return rc;
  // ---- the pass
  const bool sampled = cp.smp[0];
  HIP_OK(c, hipSetDevice(c->device));
  if (int rc = ensure_verify_ws(c)) return rc;
  if (!c->vt_tab) if (int rc = dev_alloc(c, &c->vt_tab, (size_t)tgx_ctx::VT_INTS)) return rc;
  if (sampled) if (int rc = vs_alloc(c)) return rc;
  if (int rc = ensure_extend_ws(c, M, past)) return rc;
  if (int rc = ensure_skinny_ws(c, M)) return rc;
  c->vf_pass_rows = 0;                             // the workspace changes hands
  (void)kv_ensure_blocks(c, row, (long long)past + M);      // the whole pass up front; cannot fail: counted above
  long long ids[tgx_ctx::VERIFY_ROWS] = {0};       // inputs 1 .. M - 1 = the nodes; input 0 is written on the device from the row's token word
  int tab[tgx_ctx::VT_INTS] = {0};                 // (both live until finish_pass has synchronised)
  for (int p = 0; p < M; p++) {
    if (p) ids[p] = tokens[p - 1];
    tab[tgx_ctx::VT_DEPTH + p] = tp.depth[p]; tab[tgx_ctx::VT_PAR + p] = tp.par[p];
  }
  static_assert(sizeof(tp.anc) == 2 * verify_tree_plan::MAX_POS && sizeof(tp.anc) <= 4 * (tgx_ctx::VT_INTS - tgx_ctx::VT_ANC), "the masks' slot");
  std::memcpy(tab + tgx_ctx::VT_ANC, tp.anc, sizeof(tp.anc));      // 16-bit words (positions >= M: zero)
  HIP_OK(c, hipMemcpyAsync(c->rows[(size_t)row].prompt, ids, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
  HIP_OK(c, hipMemcpyAsync(c->vt_tab, tab, sizeof(tab), hipMemcpyHostToDevice, c->stream));
  launch_verify_first_id(c, row);
  TreePass tree{c->vt_tab + tgx_ctx::VT_DEPTH, reinterpret_cast<const unsigned short*>(c->vt_tab + tgx_ctx::VT_ANC)};
  launch_prefill_skinny(c, row, 1, M, past, nullptr, &tree);
  launch_lm_head_all(c, ROUTE_SKINNY, M);
  if (sampled) launch_sample_positions(c, row, M, cp.cfg[0], -1, tree.depth);      // every position's draw, with the key of the token its DEPTH produces
  launch_verify_accept_tree(c, row, M, sampled ? c->vs_draws : nullptr);
  launch_kv_tree_compact(c, row, M, past);
  HIP_OK(c, hipMemcpyAsync(&cp.rec[0], c->vf_rec, sizeof(tgx::VerifyRecord), hipMemcpyDeviceToHost, c->stream));
  if (int rc = finish_pass(c)) return rc;
  if (int rc = follow_step_rows(c, cp, 0, 1, fn, out_ids, out_n, out_finish)) return rc;
  c->vf_pass_rows = M; c->vf_pass_joint = false;
  refresh_have_probs(c);
  refresh_longest(c);
  c->have_logits = true;
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

// ---- the joint pass of tgx_verify_rows and tgx_advance_rows: the pass's sequences in ONE ragged causal pass — tgx_forward_rows' with each sequence's real length as
// its `past` (RaggedPass.past) — on the skinny or tiled route rt.  Sequence j's ids stand at workspace rows [first_j, first_j + lens_j) and go into its row's cache
// from past_j; a STEP sequence's row 0 is the row's current token, written on the device.  Behind the pass: the STEP sequences' tail (step_tail), tgx_forward_rows'
// lm_head for the FEED rows' last positions (launch_lm_head_rows; FEED_MORE rows: none), ONE read-back of the records.
// The vj_* workspace of the STEP positions: hidden rows, logits and argmax partials per position, the sampled rows' draws, one record per row and the accept
// launch's argument table; sized by the first call that has a STEP
static int ensure_verify_rows_ws(tgx_ctx* c) {
  if (c->vj_args) return TGX_OK;      // the last of them
  const size_t R = tgx_ctx::VERIFY_POSITIONS, H = (size_t)c->d.hidden, V = (size_t)c->d.vocab, P = (size_t)c->lm_grid, B = (size_t)c->d.max_batch;
  int rc;
  if ((rc = dev_alloc(c, &c->vj_x, R * H)) || (rc = dev_alloc(c, &c->vj_logits, R * V)) || (rc = dev_alloc(c, &c->vj_part_val, R * P)) || (rc = dev_alloc(c, &c->vj_part_idx, R * P)) ||
      (rc = dev_alloc(c, &c->vj_draws, R)) || (rc = dev_alloc(c, &c->vj_rec, B * (sizeof(tgx::VerifyRecord) / 4)))) return rc;
  HIP_OK(c, hipMemset(c->vj_x, 0, R * H * 4));      // (a group of three positions rides as four through lm_head: the fourth row is read)
  return dev_alloc(c, &c->vj_args, B * verify_args_bytes());
}
// The call's buffer: the pass's tables, then its ids — ONE upload.  tables(host, dev): ragged_tables, or advance_tables with its target; (nullptr, nullptr) sizes
// them.  Grows rg_buf, fills `host` (it lives until finish_pass has synchronised) and scatters the caller's ids behind each sequence's first slot (input 0 of a STEP
// sequence is written on the device from the row's token word); *o_ids: where the ids stand in the buffer
typedef std::function<size_t(unsigned char* host, const unsigned char* dev)> PassTables;
static int call_buffer(tgx_ctx* c, const ContPass& cp, const RaggedPass& p, const PassTables& tables, std::vector<unsigned char>& host, size_t* o_ids) {
  *o_ids = tables(nullptr, nullptr);
  if (int rc = dev_grow(c, &c->rg_buf, &c->rg_bytes, *o_ids + (size_t)p.M * 8)) return rc;
  host.assign(*o_ids + (size_t)p.M * 8, 0);
  tables(host.data(), c->rg_buf);
  long long* const h_ids = reinterpret_cast<long long*>(host.data() + *o_ids);
  for (int j = 0; j < p.n; j++) {
    const int step = j < cp.ns ? 1 : 0;
    for (int k = 0; k < cp.lens[(size_t)j] - step; k++) h_ids[cp.first[(size_t)j] + step + k] = cp.ids[(size_t)j][k];
  }
  return TGX_OK;
}
// The STEP tail behind a joint pass: lm_head of the Ms STEP positions into the vj_* workspace; a sampled row's positions under its own settings, each with the key its
// step would use (the chains share one scratch: stream order); the accept launch with one workgroup per row (kernels/verify.h); one log-probability record per
// produced token of a recording row; the records' read-back, queued
static int step_tail(tgx_ctx* c, ContPass& cp, PrefillRoute lm_rt, const long long* d_ids) {
  launch_lm_head_all(c, lm_rt, cp.Ms, nullptr, /*joint=*/true);
  if (cp.any_processed) {      // the processed rows' positions (option verify.processors): the automaton walk, then the positions launch; the other rows get no workgroup
    std::vector<const long long*> in((size_t)cp.ns);
    for (int j = 0; j < cp.ns; j++) in[(size_t)j] = d_ids + cp.first[(size_t)j];
    launch_logit_proc_positions(c, cp.ns, cp.rows.data(), cp.first.data(), cp.lens.data(), in.data(), cp.prc.data(), /*joint=*/true);
  }
  for (int j = 0; j < cp.ns; j++)
    if (cp.smp[(size_t)j]) launch_sample_positions(c, cp.rows[(size_t)j], cp.lens[(size_t)j], cp.cfg[(size_t)j], cp.first[(size_t)j], nullptr, cp.prc[(size_t)j]);
  launch_verify_accept_rows(c, d_ids, cp.ns, cp.rows.data(), cp.first.data(), cp.nd.data(), cp.smp.data(), cp.prc.data());
  for (int j = 0; j < cp.ns; j++)
    if (row_records(c, cp.rows[(size_t)j])) launch_logprobs_verify(c, cp.rows[(size_t)j], cp.lens[(size_t)j], cp.first[(size_t)j], j);
  HIP_OK(c, hipMemcpyAsync(cp.rec.data(), c->vj_rec, (size_t)cp.ns * sizeof(tgx::VerifyRecord), hipMemcpyDeviceToHost, c->stream));
  return TGX_OK;
}
// The attention form is the routine's one switch.  ATTN_KEY_SPLIT (tgx_verify_rows): the STEP sequences alone — the pass's first ns — with the key-split attention
// (ragged_tables, ensure_extend_rg_ws; kernels/attn_extend.h), recorded in verify.last_form / last_splits.  ATTN_MIXED (tgx_advance_rows): every sequence with
// the mixed work list (advance_tables at advance_attn_target, ensure_mix_ws; kernels/attn_mixed.h), recorded in advance.last_form / last_tiles.  The two forms
// agree only up to the order of the fp32 sums: neither call takes the other's
enum ContAttn { ATTN_KEY_SPLIT, ATTN_MIXED };
static int joint_pass(tgx_ctx* c, ContPass& cp, ContAttn attn, PrefillRoute rt, const char* fn, int64_t* out_ids, int32_t* out_n, int32_t* out_finish) {
  static_assert(TGX_MAX_VERIFY_POSITIONS <= tgx::VERIFY_MAX_ROWS, "kernels/verify.h VerifyFirstIds");
  const bool mixed = attn == ATTN_MIXED;
  RaggedPass p = cp.view(/*steps_only=*/!mixed);
  const int n = p.n, ns = cp.ns;
  if (ns) if (int rc = ensure_verify_rows_ws(c)) return rc;
  if (cp.any_sampled) if (int rc = vs_alloc(c)) return rc;
  if (cp.any_processed) if (int rc = ensure_verify_proc_ws(c, /*joint=*/true)) return rc;
  // the STEP positions' lm_head: on the tiled route the GEMV form would stream the lm_head weights once per FOUR positions (32 step rows: eight passes, measured
  // +0.8 ms on Llama-3.2-1B, profiles/advance_rows.txt); where the skinny route would take Ms rows by themselves, its one-pass form serves them from ws_x
  // (a pass of STEP sequences alone: rt is that route already)
  PrefillRoute lm_rt = rt;
  if (ns && rt == ROUTE_TILED && prefill_route(c, cp.Ms, cp.Ms) == ROUTE_SKINNY) {
    if (int rc = ensure_skinny_ws(c, cp.Ms)) return rc;
    lm_rt = ROUTE_SKINNY;
  }
  std::vector<int> head_rows;     // the FEED rows: their last position's logits
  for (int j = ns; j < n; j++) if (cp.kind[(size_t)j] == TGX_ADV_FEED) head_rows.push_back(cp.rows[(size_t)j]);
  if (!head_rows.empty()) if (int rc = ensure_rg_lm_ws(c)) return rc;
  int target = 0;
  if (mixed) target = advance_attn_target(c, p);
  else if (int rc = ensure_extend_rg_ws(c, p)) return rc;
  std::vector<unsigned char> host;
  size_t o_ids = 0;
  if (int rc = call_buffer(c, cp, p, [&](unsigned char* h, const unsigned char* dev) { return mixed ? advance_tables(c, p, h, dev, target) : ragged_tables(c, p, h, dev); }, host, &o_ids)) return rc;
  if (mixed) if (int rc = ensure_mix_ws(c, p)) return rc;
  long long* const d_ids = reinterpret_cast<long long*>(c->rg_buf + o_ids);
  p.ids = d_ids;
  c->vf_pass_rows = 0;                             // the workspace changes hands
  if (c->kv_paged)                                 // the admissions' rows give their blocks back first
    for (int j = ns; j < n; j++) if (!cp.holds[(size_t)j]) kv_release_row(c, cp.rows[(size_t)j]);
  for (int j = 0; j < n; j++) (void)kv_ensure_blocks(c, cp.rows[(size_t)j], (long long)cp.past[(size_t)j] + cp.lens[(size_t)j]);      // cannot fail: counted (check_paged_room)
  for (int j = ns; j < n; j++) {                   // retired rows that rode along since their reset: position word back to 0
    const int row = cp.rows[(size_t)j];
    if (!cp.holds[(size_t)j] && c->row_host[(size_t)row].past != 0) { HIP_OK(c, hipMemsetAsync(c->rows[(size_t)row].pos, 0, 4, c->stream)); c->row_host[(size_t)row].past = 0; }
  }
  HIP_OK(c, hipMemcpyAsync(c->rg_buf, host.data(), host.size(), hipMemcpyHostToDevice, c->stream));
  if (ns) launch_verify_first_ids(c, d_ids, ns, cp.rows.data(), cp.first.data());
  if (int rc = launch_route(c, rt, p.M, 0, 0, 0, /*past=*/0, &p)) return rc;
  if (ns) if (int rc = step_tail(c, cp, lm_rt, d_ids)) return rc;
  launch_lm_head_rows(c, head_rows);
  for (int j = ns; j < n; j++) launch_add_pos(c, c->rows[(size_t)cp.rows[(size_t)j]].pos, cp.lens[(size_t)j]);
  if (int rc = finish_pass(c)) return rc;
  // ---- the host follows the device: the STEP rows from their records, the FEED rows as an admission / tgx_extend_row does
  if (int rc = follow_step_rows(c, cp, 0, ns, fn, out_ids, out_n, out_finish)) return rc;
  c->vf_pass_rows = cp.Ms; c->vf_pass_joint = true;
  if (mixed) { c->advance_last_form = 1; c->advance_last_tiles = target; }
  else { c->verify_last_form = 1; c->verify_last_splits = p.ext_ns; }
  for (int j = ns; j < n; j++) {
    const int row = cp.rows[(size_t)j];
    c->batch = std::max(c->batch, row + 1);
    row_admitted(c, row, cp.past[(size_t)j] + cp.lens[(size_t)j], /*keep_lp_count=*/(bool)cp.holds[(size_t)j]);
    if (cp.kind[(size_t)j] == TGX_ADV_FEED_MORE) c->row_host[(size_t)row].nologits = true;      // its logits slot is not the caller's to read: more of the prompt follows
  }
  refresh_have_probs(c);
  refresh_longest(c);
  c->have_logits = true;
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

// The STEP sequences of a pass behind their checks — all of tgx_verify_rows, and the STEP part of tgx_advance_rows' piecewise form.  Where a matrix-core route
// takes the Ms positions: the joint pass with the key-split attention.  Else (fp32 storage, prefill.mfma 0, shapes the tile does not cover, Ms below the routes'
// minimum) row by row: each row's own pass -> draws -> accept, bit for bit the one-row call; its positions' logits then join the call's in vj_logits:
// verify.last_form 2
static int verify_steps(tgx_ctx* c, ContPass& cp, const char* fn, int64_t* out_ids, int32_t* out_n, int32_t* out_finish) {
  const PrefillRoute rt = prefill_route(c, cp.Ms, cp.Ms);
  if (rt == ROUTE_SKINNY || rt == ROUTE_TILED) return joint_pass(c, cp, ATTN_KEY_SPLIT, rt, fn, out_ids, out_n, out_finish);
  if (int rc = ensure_verify_rows_ws(c)) return rc;
  const size_t V = (size_t)c->d.vocab;
  for (int j = 0; j < cp.ns; j++) {
    if (int rc = verify_row_run(c, cp, j, fn, out_ids, out_n, out_finish)) return rc;
    HIP_OK(c, hipMemcpyAsync(c->vj_logits + (size_t)cp.first[(size_t)j] * V, c->vf_logits, (size_t)cp.lens[(size_t)j] * V * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  if (int rc = finish_pass(c)) return rc;
  c->vf_pass_rows = cp.Ms; c->vf_pass_joint = true;
  c->verify_last_form = 2;
  return TGX_OK;
}

// ---- tgx_verify_rows (include/tgx.h): the drafts of n rows in ONE causal pass and ONE accept launch (verify_steps)
int tgx_verify_rows(tgx_ctx* c, int n, const int32_t* rows, const int64_t* drafts, const int32_t* n_draft, int64_t* out_ids, int32_t* out_n, int32_t* out_finish) {
  const char* const fn = "tgx_verify_rows";
  if (!c || !rows || !drafts || !n_draft || !out_ids || !out_n || !out_finish) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "verify before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  const tgx_model_desc& d = c->d;
  if (n < 1 || n > d.max_batch) return set_err(c, TGX_ERR_INVALID, "n %d out of range [1,%d]", n, d.max_batch);
  // ---- every check before anything changes: per row in array order, each row's in the one-row call's order; the call's position limit behind them
  std::vector<char> named((size_t)d.max_batch, 0);
  long long M = 0, off = 0;
  for (int i = 0; i < n; i++) {
    if (int rc = name_row(c, named, rows[i])) return rc;
    if (n_draft[i] < 0 || n_draft[i] > TGX_MAX_DRAFT) return set_err(c, TGX_ERR_INVALID, "n_draft %d out of range [0,%d]", (int)n_draft[i], TGX_MAX_DRAFT);      // (ahead of the read of its ids)
    if (int rc = verify_row_check(c, rows[i], drafts + off, n_draft[i], /*min_draft=*/0, /*sampled_entry=*/true, fn)) return rc;
    M += n_draft[i] + 1; off += n_draft[i];
  }
  if (M > TGX_MAX_VERIFY_POSITIONS) return set_err(c, TGX_ERR_INVALID, "%s: %lld positions in one call (at most %d)", fn, M, TGX_MAX_VERIFY_POSITIONS);
  ContPass cp = cont_pass(c, n, rows, /*kinds=*/nullptr, drafts, n_draft);
  if (int rc = check_paged_room(c, cp, fn, ROOM_CALL)) return rc;
  HIP_OK(c, hipSetDevice(c->device));
  return verify_steps(c, cp, fn, out_ids, out_n, out_finish);
}

// ---- tgx_advance_rows (include/tgx.h): STEP rows (tgx_verify_rows' sequences) and FEED / FEED_MORE rows (continuations from their row's length, admissions from 0)
// in ONE ragged pass: the joint pass with the mixed attention.  Where no matrix-core route takes the M positions the equivalent calls run one after another
// behind the joint checks — the STEP rows through verify_steps, a FEED through extend_row or admit_rows: advance.last_form 2.
int tgx_advance_rows(tgx_ctx* c, int n, const int32_t* rows, const int32_t* kinds, const int64_t* ids, const int32_t* lens, int64_t* out_ids, int32_t* out_n, int32_t* out_finish) {
  const char* const fn = "tgx_advance_rows";
  if (!c || !rows || !kinds || !lens || !out_ids || !out_n || !out_finish) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "advance before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  const tgx_model_desc& d = c->d;
  if (n < 1 || n > d.max_batch) return set_err(c, TGX_ERR_INVALID, "n %d out of range [1,%d]", n, d.max_batch);
  // ---- every check before anything changes.  The call's own first: kinds, lens, the two position limits
  long long M = 0, Ms = 0, n_ids = 0;
  for (int i = 0; i < n; i++) {
    if (kinds[i] < TGX_ADV_STEP || kinds[i] > TGX_ADV_FEED_MORE) return set_err(c, TGX_ERR_INVALID, "%s: kinds[%d] = %d (0 step, 1 feed, 2 feed, more follows)", fn, i, (int)kinds[i]);
    if (lens[i] < 0) return set_err(c, TGX_ERR_INVALID, "%s: lens[%d] = %d < 0", fn, i, (int)lens[i]);
    if (kinds[i] == TGX_ADV_STEP) Ms += (long long)lens[i] + 1;
    M += (long long)lens[i] + (kinds[i] == TGX_ADV_STEP ? 1 : 0);
    n_ids += lens[i];
  }
  if (Ms > TGX_MAX_VERIFY_POSITIONS) return set_err(c, TGX_ERR_INVALID, "%s: %lld step positions in one call (at most %d)", fn, Ms, TGX_MAX_VERIFY_POSITIONS);
  if (M > TGX_MAX_ADVANCE_POSITIONS) return set_err(c, TGX_ERR_INVALID, "%s: %lld positions in one call (at most %d)", fn, M, TGX_MAX_ADVANCE_POSITIONS);
  if (n_ids > 0 && !ids) return set_err(c, TGX_ERR_INVALID, "null argument");
  // ... then per row in array order, each row's in its equivalent call's order; the new rows' order behind them
  std::vector<char> named((size_t)d.max_batch, 0);
  int n_new = 0;
  long long off = 0;
  for (int i = 0; i < n; off += lens[i], i++) {
    const int row = rows[i], len = lens[i];
    const int64_t* const my = ids ? ids + off : nullptr;
    if (int rc = name_row(c, named, row)) return rc;
    if (kinds[i] == TGX_ADV_STEP) {
      if (len > TGX_MAX_DRAFT) return set_err(c, TGX_ERR_INVALID, "n_draft %d out of range [0,%d]", len, TGX_MAX_DRAFT);      // (ahead of the read of its ids)
      if (int rc = verify_row_check(c, row, my, len, /*min_draft=*/0, /*sampled_entry=*/true, fn)) return rc;
    } else {
      if (row < 0 || row >= d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, d.max_batch);
      if (len < 1) return set_err(c, TGX_ERR_INVALID, "seq %d < 1", len);
      const long long past = c->row_host[(size_t)row].past;
      if (row_holds(c, row) && past + len > d.max_ctx) return set_err(c, TGX_ERR_CONTEXT, "context size exceeded: row %d holds %lld positions, + %d > %d", row, past, len, d.max_ctx);
      if (!row_holds(c, row) && len > d.max_ctx) return set_err(c, TGX_ERR_CONTEXT, "prompt %d: seq %d out of range (context size %d)", i, len, d.max_ctx);
      for (int k = 0; k < len; k++)
        if (my[k] < 0 || my[k] >= d.vocab) return set_err(c, TGX_ERR_INVALID, "token id out of range");
      n_new += row >= c->batch;
    }
  }
  for (int row = c->batch; row < c->batch + n_new; row++)
    if (row >= d.max_batch || !named[(size_t)row])
      return set_err(c, TGX_ERR_INVALID, "the new rows of a call must be %d..%d (the batch grows in order, max_batch %d)", c->batch, c->batch + n_new - 1, d.max_batch);
  ContPass cp = cont_pass(c, n, rows, kinds, ids, lens);
  if (int rc = check_paged_room(c, cp, fn, ROOM_CALL_ADM)) return rc;
  HIP_OK(c, hipSetDevice(c->device));
  for (int i = 0; i < n; i++) { out_n[i] = 0; out_finish[i] = 0; }
  const PrefillRoute rt = prefill_route(c, cp.M, cp.M);
  if (rt == ROUTE_SKINNY || rt == ROUTE_TILED) return joint_pass(c, cp, ATTN_MIXED, rt, fn, out_ids, out_n, out_finish);
  // ---- piecewise: the equivalent calls behind the joint checks; the admissions' rows give their blocks back first, so that every piece's own count fits
  if (c->kv_paged) for (int row : cp.adm) kv_release_row(c, row);
  if (cp.ns) if (int rc = verify_steps(c, cp, "tgx_verify_rows", out_ids, out_n, out_finish)) return rc;      // (the call it stands for, named in a device failure's message)
  std::vector<int> feeds;      // the continuations in array order, then the admissions in row order (the batch grows in order)
  for (int j = cp.ns; j < cp.n; j++) feeds.push_back(j);
  std::stable_sort(feeds.begin(), feeds.end(), [&](int x, int y) { return cp.holds[(size_t)x] != cp.holds[(size_t)y] ? cp.holds[(size_t)x] > cp.holds[(size_t)y] : (!cp.holds[(size_t)x] && cp.rows[(size_t)x] < cp.rows[(size_t)y]); });
  for (int j : feeds) {
    const int32_t r1 = cp.rows[(size_t)j], s1 = cp.lens[(size_t)j];
    if (int rc = cp.holds[(size_t)j] ? extend_row(c, r1, cp.ids[(size_t)j], s1, nullptr) : admit_rows(c, 1, &r1, cp.ids[(size_t)j], &s1, /*may_join=*/false)) return rc;
    if (cp.kind[(size_t)j] == TGX_ADV_FEED_MORE) c->row_host[(size_t)r1].nologits = true;      // its logits slot is not the caller's to read: more of the prompt follows
  }
  refresh_longest(c);
  c->advance_last_form = 2;
  return TGX_OK;
}

// test / diagnostic use: the fp32 logits [M][V] of the last verify pass, while the workspace still holds them
int tgx_read_pass_logits(tgx_ctx* c, float* out, int cap_rows, int32_t* out_rows) {
  if (!c || !out || !out_rows) return c ? set_err(c, TGX_ERR_INVALID, "null argument") : TGX_ERR_INVALID;
  const int M = c->vf_pass_rows;
  const float* const src = c->vf_pass_joint ? c->vj_logits : c->vf_logits;      // (a tgx_verify_rows joint pass: all its positions in call order)
  if (M < 1 || !src) return set_err(c, TGX_ERR_STATE, "no verify pass to read: the workspace holds none (no call yet, or another call has used it since)");
  if (cap_rows < M) return set_err(c, TGX_ERR_INVALID, "cap_rows %d below the pass's %d positions", cap_rows, M);
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  HIP_OK(c, hipMemcpy(out, src, (size_t)M * c->d.vocab * 4, hipMemcpyDeviceToHost));
  *out_rows = M;
  return TGX_OK;
}

// paged KV: rows [0, n_tok) of every (layer, kv head) of both caches from block src_blk into block dst_blk — the cache part of the fork's copy launch alone
// (kernels/kv_fork.h: a grid without the state rows behind the cache part's)
static void launch_kv_tail_copy(tgx_ctx* c, int src_blk, int dst_blk, int n_tok) {
  launch_kv_copy(c, n_tok, [&](tgx::KvForkArgs& a) {
    a.n_dst = 1; a.src_id = src_blk; a.dst_id[0] = dst_blk;
    a.kv_rows = std::min(2 * a.n_spans, 64);
    return dim3(1, (unsigned)a.kv_rows);      // (at most 127 tokens per span: one workgroup covers it at every released head_dim)
  });
}

int tgx_truncate_row(tgx_ctx* c, int row, int64_t new_len) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "truncate before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  const tgx_model_desc& d = c->d;
  if (row < 0 || row >= d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, d.max_batch);
  if (row >= c->batch || c->row_host[(size_t)row].idle || c->row_host[(size_t)row].past < 1) return set_err(c, TGX_ERR_STATE, "row %d holds no sequence to truncate", row);
  const long long past = c->row_host[(size_t)row].past;
  if (new_len < 1) return set_err(c, TGX_ERR_INVALID, "new_len %lld < 1: tgx_reset_row empties a row", (long long)new_len);
  if (new_len > past) return set_err(c, TGX_ERR_INVALID, "new_len %lld beyond the %lld positions row %d holds", (long long)new_len, past, row);
  // nothing to roll back and the logits in the slot are those of the last position held: the row stays as it is
  if (new_len == past && !c->row_host[(size_t)row].fin && !c->row_host[(size_t)row].nologits) return TGX_OK;
  const int keep = (int)((new_len + tgx::KV_BLOCK - 1) / tgx::KV_BLOCK), tail = (int)(new_len % tgx::KV_BLOCK);
  // the block that holds the new tail, where forked siblings map it as well: the next append would write into it
  const int shared_blk = c->kv_paged && tail && c->kv.shared(row, keep - 1) ? c->kv.block_at(row, keep - 1) : 0;
  if (shared_blk && !c->kv.free_blocks())
    return set_err(c, TGX_ERR_CONTEXT, "KV budget exhausted: truncating row %d to %lld leaves it inside a block shared with %d forked row(s) and no block is free for its copy (option kv.budget_tokens = %d)",
                   row, (long long)new_len, c->kv.sharers(shared_blk) - 1, c->kv_budget_tokens);
  if (shared_blk && ((long long)d.head_dim * (long long)c->esz) % 4 != 0) return set_err(c, TGX_ERR_UNSUPPORTED, "tgx_truncate_row: a cache row of %d bytes", (int)(d.head_dim * c->esz));
  // ---- nothing above changed anything: "a refused call changes nothing" is about those checks.  From here on the host bookkeeping (blocks, table) moves ahead of the
  // launches; should one of them not issue, launches_ok poisons the context — the row's lengths then stay as they were, and only tgx_reset_cache follows
  HIP_OK(c, hipSetDevice(c->device));
  if (shared_blk) {        // copy on write, before any append can happen: rows [0, tail) into a fresh block, the table entry swapped, this row's reference dropped
    KvPool::Changes ch;
    const int fresh = c->kv.unshare_tail(row, keep - 1, ch).second;      // cannot run dry: checked above
    launch_kv_tail_copy(c, shared_blk, fresh, tail);
    kv_tbl_push(c, ch);
  }
  kv_trim_row(c, row, new_len);                                         // the blocks beyond the new length (a shared one only loses this row's reference)
  if (new_len != past) launch_add_pos(c, c->rows[(size_t)row].pos, (int)(new_len - past));      // stream-ordered behind the steps already enqueued
  if (c->row_host[(size_t)row].fin) { row_req_push(c, row, ROWQ_STATE); c->row_host[(size_t)row].fin = 0; }
  if (int rc = launches_ok(c)) return rc;
  RowHost& r = c->row_host[(size_t)row];
  r.past = new_len;
  r.tok = r.probs_ok = false; r.nologits = true;                        // the logits of position new_len - 1 no longer exist
  refresh_longest(c);
  return TGX_OK;
}

// ---- tgx_splice_row (include/tgx.h): ranges cut out of the middle of a live row.  checks -> plan (splice_plan.h) -> launches (kernels/kv_splice.h) -> bookkeeping.
// The move runs in groups of whole layers through the snapshot staging buffer (option snapshot.stage_kib caps it; one layer is always staged), allocated at first use.
// Paged cache: the scatter launches write through the row's NEW table while later groups' gathers still read through the old one, so the new table row is first
// built in the head of the staging buffer (a copy of the device row plus the pool's changes) and the device table itself is pushed behind the last scatter.
int tgx_splice_row(tgx_ctx* c, int row, int n_keep, const int64_t* starts, const int64_t* lens, int64_t* out_len) {
  if (!c) return TGX_ERR_INVALID;
  if (!starts || !lens) return set_err(c, TGX_ERR_INVALID, "null argument");
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "splice before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  const tgx_model_desc& d = c->d;
  if (row < 0 || row >= d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, d.max_batch);
  if (n_keep < 1 || n_keep > TGX_MAX_SPLICE_RANGES) return set_err(c, TGX_ERR_INVALID, "n_keep %d out of range [1,%d]", n_keep, TGX_MAX_SPLICE_RANGES);
  if (row >= c->batch || c->row_host[(size_t)row].idle || c->row_host[(size_t)row].past < 1) return set_err(c, TGX_ERR_STATE, "row %d holds no sequence to splice", row);
  if (d.family == TGX_FAMILY_GPT2) return set_err(c, TGX_ERR_UNSUPPORTED, "tgx_splice_row: GPT-2's positions are learned and added to the hidden state: there is nothing to re-rotate");
  const long long past = c->row_host[(size_t)row].past;
  splice_plan::Plan plan;
  if (const char* why = splice_plan::make(past, n_keep, starts, lens, &plan)) return set_err(c, TGX_ERR_INVALID, "tgx_splice_row: %s (row %d holds %lld positions)", why, row, past);
  const long long tok_bytes = (long long)d.head_dim * (long long)c->esz, half_bytes = tok_bytes / 2;
  if (tok_bytes % 4 != 0 || (d.head_dim & 1) || half_bytes % 4 != 0) return set_err(c, TGX_ERR_UNSUPPORTED, "tgx_splice_row: a cache row of %d bytes", (int)tok_bytes);
  if (plan.truncation()) {      // one range [0, L): tgx_truncate_row's bits and block accounting (L == past with the logits in place: its no-op)
    if (int rc = tgx_truncate_row(c, row, plan.new_len)) return rc;
    if (out_len) *out_len = plan.new_len;
    return TGX_OK;
  }
  splice_plan::Blocks blk;
  if (c->kv_paged) {
    // all or nothing: the fresh blocks of the copy on write against the FREE LIST ALONE (the blocks the row gives back are not counted: the sum errs towards refusing)
    blk = splice_plan::blocks(c->kv, row, plan);
    if (blk.fresh.size() > c->kv.free_blocks())
      return set_err(c, TGX_ERR_CONTEXT, "KV budget exhausted: splicing row %d writes %zu block(s) shared with forked rows and %zu block(s) are free for their copies (option kv.budget_tokens = %d)",
                     row, blk.fresh.size(), c->kv.free_blocks(), c->kv_budget_tokens);
  }
  HIP_OK(c, hipSetDevice(c->device));
  // the staging buffer: [the new table row | groups of whole layers].  (A failed growth fails the call before the row or the pool moved.)
  const int moved = (int)plan.moved(), stride = c->kv_paged ? c->kv.tbl_stride() : 0;
  const size_t head = ((size_t)stride * 4 + 255) / 256 * 256;
  const long long layer_bytes = 2ll * d.kv_heads * moved * tok_bytes;
  const long long room = (long long)c->snapshot_stage_kib * 1024 - (long long)head;
  const int per_group = (int)std::max<long long>(1, std::min<long long>(d.layers, room / layer_bytes));
  if (int rc = dev_grow(c, &c->snap_stage, &c->snap_stage_bytes, head + (size_t)per_group * (size_t)layer_bytes)) return rc;
  // ---- nothing above changed anything: "a refused call changes nothing" is about those checks.  From here on the host bookkeeping (blocks, table) moves ahead of the
  // launches; should one of them not issue, launches_ok poisons the context — the row's lengths then stay as they were, and only tgx_reset_cache follows
  int* const new_tbl = reinterpret_cast<int*>(c->snap_stage);
  KvPool::Changes ch;
  if (c->kv_paged) {
    hipLaunchKernelGGL(kv_tbl_copy_kernel, dim3(1), dim3(256), 0, c->stream, new_tbl, c->kv_tbl + (size_t)row * stride, stride);
    for (size_t i = 0; i < blk.fresh.size(); i++) {      // copy on write, before anything writes: cannot run dry, counted above
      const std::pair<int, int> of = c->kv.unshare(row, blk.fresh[i], ch);
      if (i == 0 && blk.carry) launch_kv_tail_copy(c, of.first, of.second, blk.carry);      // the identity rows in front of f
    }
    c->kv.trim(row, plan.new_len, ch);      // the blocks beyond the new length (a shared one only loses this row's reference)
    kv_tbl_push(c, ch, new_tbl, row * stride);
  }
  tgx::KvSpliceArgs a{};
  a.k = c->rows[(size_t)row].kcache; a.v = c->rows[(size_t)row].vcache;
  a.stage = c->snap_stage + head;
  a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin;
  a.layer_stride = c->kv_paged ? (long long)c->kv.n_blocks() * d.kv_heads * tgx::KV_BLOCK * d.head_dim : (long long)d.kv_heads * d.max_ctx * d.head_dim;
  a.kv_heads = d.kv_heads; a.hd = d.head_dim; a.max_ctx = d.max_ctx; a.moved = moved;
  const bool wide = half_bytes % 16 == 0;
  a.chunks = (int)(half_bytes / (wide ? 16 : 4));
  for (int i = plan.first_moved, m0 = 0; i < plan.n_seg; i++) {
    a.seg[a.n_seg++] = {(int)plan.seg[i].src, (int)plan.seg[i].dst, m0, (int)plan.seg[i].len};
    m0 += (int)plan.seg[i].len;
  }
  for (int l0 = 0; l0 < d.layers; l0 += per_group) {
    a.layer0 = l0; a.n_layers = std::min(per_group, d.layers - l0);
    a.tbl = c->kv_paged ? c->kv_tbl + (size_t)row * stride : nullptr;
    launch_kv_splice(c, a, wide, /*scatter=*/false);
    a.tbl = c->kv_paged ? new_tbl : nullptr;
    launch_kv_splice(c, a, wide, /*scatter=*/true);
  }
  if (c->kv_paged) kv_tbl_push(c, ch);
  launch_add_pos(c, c->rows[(size_t)row].pos, (int)(plan.new_len - past));      // stream-ordered behind the steps already enqueued
  if (c->row_host[(size_t)row].fin) { row_req_push(c, row, ROWQ_STATE); c->row_host[(size_t)row].fin = 0; }
  if (int rc = launches_ok(c)) return rc;
  RowHost& r = c->row_host[(size_t)row];
  r.past = plan.new_len;
  r.tok = r.probs_ok = false; r.nologits = true;      // the logits belong to a sequence the row no longer holds
  refresh_longest(c);
  if (out_len) *out_len = plan.new_len;
  return TGX_OK;
}

int tgx_sample_row(tgx_ctx* c, int row, const tgx_sampler_cfg* cfg, uint64_t seed, int64_t* out_id) {
  if (!c || !cfg) return TGX_ERR_INVALID;
  if (!c->have_logits) return set_err(c, TGX_ERR_STATE, "no logits to sample from");
  if (row < 0 || row >= c->batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->batch);
  if (c->row_host[(size_t)row].nologits) return set_err(c, TGX_ERR_STATE, "row %d was truncated and holds no logits: tgx_extend_row it first", row);
  HIP_OK(c, hipSetDevice(c->device));
  if (int rc = ensure_seed(c, *cfg, seed)) return rc;
  note_sampled(c, row, 1, *cfg);
  const bool processed = row_processed(c, row);      // the row's own processors, without the counting step: it has no current token yet
  if (processed) launch_logit_proc(c, row, 1, /*step=*/false);
  c->row_host[(size_t)row].probs_proc = processed;
  launch_sample(c, row, 1, *cfg, /*advance_pos=*/false, /*log_step=*/false, processed);
  const bool records = row_records(c, row);
  if (records) launch_logprobs(c, row, 1, /*force=*/true);      // the first token after an admission, tgx_extend_row or tgx_fork_row
  HIP_OK(c, hipGetLastError());
  LAUNCH_OK(c);
  HIP_OK(c, hipStreamSynchronize(c->stream));
  if (records) c->row_host[(size_t)row].lp_count++;
  int t = 0;
  HIP_OK(c, hipMemcpy(&t, c->rows[(size_t)row].tok, 4, hipMemcpyDeviceToHost));
  if (out_id) *out_id = t;
  if (row == 0) c->last_sampled0 = t;
  c->row_host[(size_t)row].tok = 1;
  refresh_longest(c);
  return TGX_OK;
}
// ---- per-row sampler settings and device-side stop (include/tgx.h tgx_decode_rows) ----------------------------------------------------------------------
int tgx_set_row_sampler(tgx_ctx* c, int row, const tgx_sampler_cfg* cfg, uint64_t seed) {
  if (!c) return TGX_ERR_INVALID;
  if (!cfg) return set_err(c, TGX_ERR_INVALID, "null sampler configuration");
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "set_row_sampler before finalize");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  HIP_OK(c, hipSetDevice(c->device));
  tgx::RowReq& q = c->row_req_host[(size_t)row];
  q.temperature = cfg->temperature; q.top_k = cfg->top_k; q.top_p = cfg->top_p; q.min_p = cfg->min_p; q.seed = seed;
  row_req_push(c, row, ROWQ_SAMPLER);
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

int tgx_set_row_stop(tgx_ctx* c, int row, int32_t max_new, const int32_t* stop_ids, int n_stop) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "set_row_stop before finalize");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  if (n_stop < 0 || n_stop > TGX_MAX_STOP_IDS) return set_err(c, TGX_ERR_INVALID, "n_stop %d out of range [0,%d]", n_stop, TGX_MAX_STOP_IDS);
  if (n_stop > 0 && !stop_ids) return set_err(c, TGX_ERR_INVALID, "null stop_ids with n_stop %d", n_stop);
  HIP_OK(c, hipSetDevice(c->device));
  tgx::RowReq& q = c->row_req_host[(size_t)row];
  q.max_new = max_new; q.n_stop = n_stop;
  for (int k = 0; k < TGX_MAX_STOP_IDS; k++) q.stop[k] = k < n_stop ? stop_ids[k] : -1;
  row_req_push(c, row, ROWQ_STOP);
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

// ---- per-token log-probabilities (include/tgx.h; kernels/logprobs.h)
int tgx_set_row_logprobs(tgx_ctx* c, int row, int top_n) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "set_row_logprobs before finalize");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  if (top_n < -1 || top_n > TGX_MAX_LOGPROBS) return set_err(c, TGX_ERR_INVALID, "top_n %d out of range [-1,%d]", top_n, TGX_MAX_LOGPROBS);
  HIP_OK(c, hipSetDevice(c->device));
  if (top_n >= 0) { if (int rc = logprobs_alloc(c)) return rc; }      // a context that never asks allocates nothing
  c->row_req_host[(size_t)row].lp = top_n + 1;
  row_req_push(c, row, ROWQ_LP);
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

// ---- per-row logit processors (include/tgx.h; kernels/logit_proc.h).  Every check comes before anything changes; the settings travel by value in stream-ordered
// launches, like the sampler settings
int tgx_set_row_penalties(tgx_ctx* c, int row, const tgx_penalty_cfg* cfg) {
  if (!c) return TGX_ERR_INVALID;
  if (!cfg) return set_err(c, TGX_ERR_INVALID, "null penalty configuration");
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "set_row_penalties before finalize");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  if (!std::isfinite(cfg->repetition) || !(cfg->repetition > 0.f)) return set_err(c, TGX_ERR_INVALID, "repetition penalty %g: a finite value > 0", (double)cfg->repetition);
  if (!std::isfinite(cfg->presence) || !std::isfinite(cfg->frequency)) return set_err(c, TGX_ERR_INVALID, "presence / frequency penalty not finite");
  const bool neutral = cfg->repetition == 1.f && cfg->presence == 0.f && cfg->frequency == 0.f;
  if (neutral && !c->proc_part_idx) return TGX_OK;      // a context that never asked: nothing to switch off, nothing allocated
  HIP_OK(c, hipSetDevice(c->device));
  if (int rc = proc_alloc(c)) return rc;
  tgx::RowReq& q = c->row_req_host[(size_t)row];
  q.repetition = cfg->repetition; q.presence = cfg->presence; q.frequency = cfg->frequency;
  row_proc_refresh(q);
  row_req_push(c, row, ROWQ_PROC);
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

struct RowBiasUpdate { int row, n; int ids[TGX_MAX_LOGIT_BIAS]; float val[TGX_MAX_LOGIT_BIAS]; };
static __global__ void row_bias_set_kernel(int* ids, float* val, RowBiasUpdate u) {
  for (int k = threadIdx.x; k < u.n; k += blockDim.x) { ids[(size_t)u.row * TGX_MAX_LOGIT_BIAS + k] = u.ids[k]; val[(size_t)u.row * TGX_MAX_LOGIT_BIAS + k] = u.val[k]; }
}

int tgx_set_row_logit_bias(tgx_ctx* c, int row, int n, const int32_t* ids, const float* bias) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "set_row_logit_bias before finalize");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  if (n < 0 || n > TGX_MAX_LOGIT_BIAS) return set_err(c, TGX_ERR_INVALID, "n %d out of range [0,%d]", n, TGX_MAX_LOGIT_BIAS);
  if (n > 0 && (!ids || !bias)) return set_err(c, TGX_ERR_INVALID, "null ids / bias with n %d", n);
  RowBiasUpdate u{};
  u.row = row; u.n = n;
  int banned = 0;
  for (int k = 0; k < n; k++) {
    if (ids[k] < 0 || ids[k] >= c->d.vocab) return set_err(c, TGX_ERR_INVALID, "bias id %d out of range [0,%d)", (int)ids[k], c->d.vocab);
    if (std::isnan(bias[k]) || bias[k] == INFINITY) return set_err(c, TGX_ERR_INVALID, "bias of id %d is NaN or +inf", (int)ids[k]);
    banned += bias[k] == -INFINITY;
    u.ids[k] = ids[k]; u.val[k] = bias[k];
  }
  if (n > 1) {
    std::vector<int32_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    for (int k = 1; k < n; k++) if (sorted[(size_t)k] == sorted[(size_t)k - 1]) return set_err(c, TGX_ERR_INVALID, "bias id %d named twice", (int)sorted[(size_t)k]);
  }
  if (banned >= c->d.vocab) return set_err(c, TGX_ERR_INVALID, "a bias of -inf on all %d ids", c->d.vocab);
  if (n == 0 && !c->proc_part_idx) return TGX_OK;       // a context that never asked: nothing to clear, nothing allocated
  HIP_OK(c, hipSetDevice(c->device));
  if (int rc = proc_alloc(c)) return rc;
  if (n > 0) hipLaunchKernelGGL(row_bias_set_kernel, dim3(1), dim3(64), 0, c->stream, c->proc_bias_ids, c->proc_bias_val, u);
  tgx::RowReq& q = c->row_req_host[(size_t)row];
  q.n_bias = n;
  row_proc_refresh(q);
  row_req_push(c, row, ROWQ_PROC);
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

int tgx_set_row_history(tgx_ctx* c, int row, const int64_t* prompt_ids, int n_prompt, const int64_t* produced_ids, int n_produced) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "set_row_history before finalize");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  if (n_prompt < 0 || n_produced < 0) return set_err(c, TGX_ERR_INVALID, "negative list length");
  if ((n_prompt > 0 && !prompt_ids) || (n_produced > 0 && !produced_ids)) return set_err(c, TGX_ERR_INVALID, "null id list with a length > 0");
  const int64_t V = c->d.vocab;
  for (int i = 0; i < n_prompt; i++) if (prompt_ids[i] < 0 || prompt_ids[i] >= V) return set_err(c, TGX_ERR_INVALID, "history id out of range");
  for (int i = 0; i < n_produced; i++) if (produced_ids[i] < 0 || produced_ids[i] >= V) return set_err(c, TGX_ERR_INVALID, "history id out of range");
  if (n_prompt + n_produced == 0 && !c->proc_part_idx) return TGX_OK;      // a context that never asked: its rows' histories are empty
  HIP_OK(c, hipSetDevice(c->device));
  if (n_prompt + n_produced == 0) {         // clearing: a stream-ordered fill, no host buffer and nothing to wait for (as tgx_reset_row)
    HIP_OK(c, hipMemsetAsync(c->proc_hist + (size_t)row * V, 0, (size_t)V * sizeof(unsigned int), c->stream));
    return TGX_OK;
  }
  if (int rc = proc_alloc(c)) return rc;
  // REPLACE: the row's words built here and copied in stream order behind the steps that still count into the old ones (the copy is waited for: the vector is this call's)
  std::vector<unsigned int> words((size_t)V, 0u);
  for (int i = 0; i < n_prompt; i++) words[(size_t)prompt_ids[i]] |= tgx::PROC_PROMPT_BIT;
  for (int i = 0; i < n_produced; i++) {
    unsigned int& w = words[(size_t)produced_ids[i]];
    if ((w & tgx::PROC_COUNT_MASK) < tgx::PROC_COUNT_MASK) w++;
  }
  HIP_OK(c, hipMemcpyAsync(c->proc_hist + (size_t)row * V, words.data(), (size_t)V * sizeof(unsigned int), hipMemcpyHostToDevice, c->stream));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  return TGX_OK;
}

// ---- token automata (include/tgx.h; automaton.h holds the checks, kernels/logit_proc.h the mask stage and the advance launch)
static_assert(automaton::NONE == TGX_AUTOMATON_NONE && automaton::MAX_STATES == TGX_MAX_AUTOMATON_STATES && automaton::MAX_TABLES == TGX_MAX_AUTOMATA && tgx::AUTO_NONE == TGX_AUTOMATON_NONE, "automaton.h");
int tgx_automaton_create(tgx_ctx* c, int32_t n_states, int32_t start, const uint16_t* next, int32_t* out_id) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "automaton_create before finalize");
  if (!next || !out_id) return set_err(c, TGX_ERR_INVALID, "null argument");
  char why[160];
  if (automaton::validate(n_states, start, next, c->d.vocab, why, sizeof(why))) return set_err(c, TGX_ERR_INVALID, "tgx_automaton_create: %s", why);
  int id = -1;
  for (int i = 0; i < TGX_MAX_AUTOMATA && id < 0; i++) if (!c->automata[i].next) id = i;
  if (id < 0) return set_err(c, TGX_ERR_INVALID, "tgx_automaton_create: %d tables are live (tgx_automaton_destroy one first)", TGX_MAX_AUTOMATA);
  HIP_OK(c, hipSetDevice(c->device));
  const size_t words = (size_t)n_states * (size_t)c->d.vocab;
  unsigned short* dev = nullptr;
  if (int rc = dev_alloc(c, &dev, words)) return rc;
  // the caller's array may be pageable and is the caller's again on return: the copy is waited for
  const hipError_t e = hipMemcpy(dev, next, words * sizeof(uint16_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) { dev_free(c, &dev); return set_err(c, TGX_ERR_DEVICE, "tgx_automaton_create: copying the table failed: %s", hipGetErrorString(e)); }
  c->automata[id].next = dev; c->automata[id].n_states = n_states; c->automata[id].start = start;
  *out_id = id;
  return TGX_OK;
}

int tgx_automaton_destroy(tgx_ctx* c, int32_t id) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "automaton_destroy before finalize");
  if (id < 0 || id >= TGX_MAX_AUTOMATA || !c->automata[id].next) return set_err(c, TGX_ERR_INVALID, "tgx_automaton_destroy: no automaton %d", (int)id);
  for (int b = 0; b < c->d.max_batch; b++)
    if (c->row_host[(size_t)b].auto_id == id) return set_err(c, TGX_ERR_STATE, "tgx_automaton_destroy: row %d still names automaton %d (tgx_set_row_automaton(row, -1, -1) or reset it first)", b, (int)id);
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));      // steps in flight may still read the table of a row that was switched off behind them
  dev_free(c, &c->automata[id].next);
  c->automata[id] = tgx_ctx::AutoTable{};
  return TGX_OK;
}

int tgx_set_row_automaton(tgx_ctx* c, int row, int32_t id, int32_t state) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "set_row_automaton before finalize");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  if (id < -1 || id >= TGX_MAX_AUTOMATA || (id >= 0 && !c->automata[id].next)) return set_err(c, TGX_ERR_INVALID, "tgx_set_row_automaton: no automaton %d", (int)id);
  if (id >= 0 && !automaton::state_ok(c->automata[id].n_states, state)) return set_err(c, TGX_ERR_INVALID, "tgx_set_row_automaton: state %d out of range [-1,%d)", (int)state, c->automata[id].n_states);
  tgx::RowReq& q = c->row_req_host[(size_t)row];
  if (id < 0 && !q.auto_next) return TGX_OK;      // nothing to switch off
  HIP_OK(c, hipSetDevice(c->device));
  if (id >= 0) { if (int rc = proc_alloc(c)) return rc; }      // the mask is a stage of the processor launch: its slab and partials
  q.auto_next = id >= 0 ? c->automata[id].next : nullptr;
  q.auto_state = id >= 0 ? (state < 0 ? c->automata[id].start : state) : 0;
  c->row_host[(size_t)row].auto_id = id;
  row_proc_refresh(q);
  row_req_push(c, row, ROWQ_PROC | ROWQ_AUTO);
  HIP_OK(c, hipGetLastError());
  return TGX_OK;
}

int tgx_read_row_automaton(tgx_ctx* c, int row, int32_t* out_id, int32_t* out_state) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "read_row_automaton before finalize");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  const int id = c->row_host[(size_t)row].auto_id;
  int state = -1;
  if (id >= 0) HIP_OK(c, hipMemcpy(&state, &c->row_req[row].auto_state, 4, hipMemcpyDeviceToHost));
  if (out_id) *out_id = id;
  if (out_state) *out_state = state;
  return TGX_OK;
}

int tgx_read_row_logprobs(tgx_ctx* c, int row, int n, float* out_lp, int32_t* out_top_ids, float* out_top_lp, int32_t* out_top_n) {
  if (!c) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "read_row_logprobs before finalize");
  if (row < 0 || row >= c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "row %d out of range [0,%d)", row, c->d.max_batch);
  if (!out_lp) return set_err(c, TGX_ERR_INVALID, "null out_lp");
  // the host mirrors the row's record counter (RowHost::lp_count follows every call that records): a refused call touches neither the device nor the caller's buffers
  const int64_t count = c->row_host[(size_t)row].lp_count;
  if (count < 1) return set_err(c, TGX_ERR_STATE, "row %d has recorded no log-probabilities (tgx_set_row_logprobs; the count restarts with the row)", row);
  const int have = (int)std::min<int64_t>(count, TGX_LOGPROB_RING);
  if (n < 1 || n > have) return set_err(c, TGX_ERR_INVALID, "n %d out of range [1,%d]: row %d holds %d record(s)", n, have, row, have);
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  std::vector<tgx::LpRecord> recs((size_t)n);
  const int s0 = (int)((count - n) % TGX_LOGPROB_RING), first = std::min(n, TGX_LOGPROB_RING - s0);
  const tgx::LpRecord* ring = c->lp_ring + (size_t)row * TGX_LOGPROB_RING;
  HIP_OK(c, hipMemcpy(recs.data(), ring + s0, (size_t)first * sizeof(tgx::LpRecord), hipMemcpyDeviceToHost));
  if (first < n) HIP_OK(c, hipMemcpy(recs.data() + first, ring, (size_t)(n - first) * sizeof(tgx::LpRecord), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) {
    const tgx::LpRecord& r = recs[(size_t)i];
    out_lp[i] = r.lp;
    if (out_top_n) out_top_n[i] = r.top_n;
    for (int k = 0; k < TGX_MAX_LOGPROBS; k++) {
      if (out_top_ids) out_top_ids[(size_t)i * TGX_MAX_LOGPROBS + k] = r.ids[k];
      if (out_top_lp) out_top_lp[(size_t)i * TGX_MAX_LOGPROBS + k] = r.lps[k];
    }
  }
  return TGX_OK;
}

int tgx_decode_rows(tgx_ctx* c, int n_steps, int64_t* out_ids, int32_t* out_new, int32_t* out_finish) {
  if (!c) return TGX_ERR_INVALID;
  if (n_steps < 0) return set_err(c, TGX_ERR_INVALID, "n_steps %d < 0", n_steps);
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "decode before finalize");
  if (c->poisoned) return set_err(c, TGX_ERR_STATE, "an earlier pass failed half-way: call tgx_reset_cache first");
  int running = 0;
  for (int b = 0; b < c->batch; b++) running += !c->row_host[(size_t)b].idle && !c->row_host[(size_t)b].fin;
  if (!running) return set_err(c, TGX_ERR_STATE, "tgx_decode_rows: no live row is unfinished (tgx_reset_row / tgx_forward_row a row first)");
  REFUSE_NOLOGITS(c, "tgx_decode_rows");
  if (!c->have_token) return set_err(c, TGX_ERR_STATE, "decode needs a current token: call tgx_sample / tgx_sample_row after the forward");
  if (c->past + n_steps > c->d.max_ctx) return set_err(c, TGX_ERR_CONTEXT, "context size exceeded: %lld + %d > %d", (long long)c->past, n_steps, c->d.max_ctx);
  for (int b = 0; b < c->batch; b++)      // a finished row rides at its own length: one that holds the whole context has no row left to ride on
    if (c->row_host[(size_t)b].fin && !c->row_host[(size_t)b].idle && c->row_host[(size_t)b].past >= c->d.max_ctx)
      return set_err(c, TGX_ERR_CONTEXT, "row %d finished at the context size %d: tgx_reset_row it first", b, c->d.max_ctx);
  if (n_steps > c->log_cap) return set_err(c, TGX_ERR_INVALID, "n_steps exceeds the token log capacity %d", c->log_cap);
  HIP_OK(c, hipSetDevice(c->device));
  const size_t B = (size_t)c->batch;
  std::vector<int64_t> before(B);
  for (size_t b = 0; b < B; b++) before[b] = c->row_host[b].past;
  const int64_t start = c->steps_issued;
  int rc = TGX_OK;
  if (n_steps > 0) {
    c->row_union = row_union_of(c);
    rc = run_decode_steps(c, tgx_sampler_cfg{0.f, 0, 1.f, 0.f}, 0, n_steps);
    c->row_union = -1;
  }
  if (rc) { refresh_longest(c); return rc; }
  c->have_logits = true;
  // one readback behind the steps: the ids of the call, every row's position and request state
  std::vector<int> ids((size_t)n_steps * B), pos(B);
  std::vector<tgx::RowReq> req(B);
  if (n_steps > 0 && (rc = read_tok_log(c, start, n_steps, ids.data()))) return rc;
  HIP_OK(c, hipMemcpyAsync(pos.data(), c->slab_pos, B * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_OK(c, hipMemcpyAsync(req.data(), c->row_req, B * sizeof(tgx::RowReq), hipMemcpyDeviceToHost, c->stream));
  bool records = false;      // the record counters travel with the readback only while some row of the batch records
  for (size_t b = 0; b < B; b++) records = records || row_records(c, (int)b);
  std::vector<tgx::LpRow> lp(records ? B : 0);
  if (records) HIP_OK(c, hipMemcpyAsync(lp.data(), c->lp_rows, B * sizeof(tgx::LpRow), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  for (size_t b = 0; b < B; b++) {
    const bool idle = c->row_host[b].idle;
    if (records) c->row_host[b].lp_count = lp[b].count;
    c->row_host[b].past = pos[b];                              // a row advanced once per token it produced (retired rows: wherever their ride took them)
    c->row_host[b].fin = idle ? 0 : (char)req[b].finished;
    c->row_req_host[b].auto_state = req[b].auto_state;         // the automaton's state word moves on the device only: the mirror follows the readback
    if (out_new) out_new[b] = idle ? 0 : (int32_t)(pos[b] - before[b]);
    if (out_finish) out_finish[b] = idle ? 0 : req[b].finished;
    if (c->row_host[b].fin) kv_trim_row(c, (int)b, c->row_host[b].past);
  }
  if (out_ids)
    for (size_t i = 0; i < ids.size(); i++) out_ids[i] = c->row_host[i % B].idle ? -1 : ids[i];
  if (n_steps > 0) c->last_sampled0 = ids[(size_t)(n_steps - 1) * B];
  refresh_longest(c);
  return TGX_OK;
}

int64_t tgx_context_size(const tgx_ctx* c) { return c ? c->d.max_ctx : -1; }
int32_t tgx_num_layers(const tgx_ctx* c) { return c ? c->d.layers : -1; }

int tgx_synchronize(tgx_ctx* c) {
  if (!c) return TGX_ERR_INVALID;
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  return TGX_OK;
}

int tgx_read_kv(tgx_ctx* c, int row, int layer, float* k_out, float* v_out) {
  if (!c || !c->finalized || row < 0 || row >= c->d.max_batch || layer < 0 || layer >= c->d.layers) return TGX_ERR_INVALID;
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  const tgx_model_desc& d = c->d;
  const size_t hd = (size_t)d.head_dim, per_head = (size_t)d.max_ctx * hd, T = (size_t)tgx_past_length_row(c, row);
  std::vector<unsigned char> tmp(per_head * c->esz);
  for (int which = 0; which < 2; which++) {
    float* out = which ? v_out : k_out;
    if (!out) continue;
    const ebyte* base = (which ? c->rows[(size_t)row].vcache : c->rows[(size_t)row].kcache) + (size_t)layer * d.kv_heads * per_head * c->esz;
    if (c->kv_paged) base = (which ? c->slab_v : c->slab_k) + (size_t)layer * c->kv.n_blocks() * d.kv_heads * tgx::KV_BLOCK * hd * c->esz;
    for (int h = 0; h < d.kv_heads; h++) {
      if (c->kv_paged) {      // the row's tokens block by block through its table
        for (size_t t0 = 0; t0 < T; t0 += tgx::KV_BLOCK) {
          const size_t n = std::min<size_t>(tgx::KV_BLOCK, T - t0);
          const size_t blk = (size_t)c->kv.block_at(row, (int)(t0 / tgx::KV_BLOCK));
          HIP_OK(c, hipMemcpy(tmp.data() + t0 * hd * c->esz, base + ((blk * d.kv_heads + h) * tgx::KV_BLOCK) * hd * c->esz, n * hd * c->esz, hipMemcpyDeviceToHost));
        }
      } else
      HIP_OK(c, hipMemcpy(tmp.data(), base + (size_t)h * per_head * c->esz, T * hd * c->esz, hipMemcpyDeviceToHost));
      for (size_t t = 0; t < T; t++)
        for (size_t k = 0; k < hd; k++) {   // BSHD view
          const size_t i = t * hd + k;
          float v;
          if (c->dt == tgx::DT_F32) memcpy(&v, tmp.data() + 4 * i, 4);
          else { uint16_t u; memcpy(&u, tmp.data() + 2 * i, 2); v = c->dt == tgx::DT_BF16 ? host_bf16_to_f32(u) : host_half_to_f32(u); }
          out[(t * d.kv_heads + h) * hd + k] = v;
        }
    }
  }
  return TGX_OK;
}

int tgx_write_kv(tgx_ctx* c, int row, int layer, const float* k_in, const float* v_in, int64_t n_rows) {
  if (!c || !c->finalized || row < 0 || row >= c->d.max_batch || layer < 0 || layer >= c->d.layers || n_rows < 0 || n_rows > tgx_past_length_row(c, row)) return c ? set_err(c, TGX_ERR_INVALID, "write_kv: row / layer / n_rows out of range") : TGX_ERR_INVALID;
  if (c->kv_paged)      // a block forked siblings map as well (tgx_fork_row) is not written through: the siblings would change with it
    for (int64_t t0 = 0; t0 < n_rows; t0 += tgx::KV_BLOCK) {
      const int idx = (int)(t0 / tgx::KV_BLOCK);
      if (c->kv.shared(row, idx))
        return set_err(c, TGX_ERR_STATE, "write_kv: positions %lld.. of row %d lie in a block shared with %d forked row(s)", (long long)t0, row, c->kv.sharers(c->kv.block_at(row, idx)) - 1);
    }
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  const tgx_model_desc& d = c->d;
  const size_t hd = (size_t)d.head_dim, per_head = (size_t)d.max_ctx * hd, T = (size_t)n_rows;
  std::vector<unsigned char> tmp(T * hd * c->esz);
  for (int which = 0; which < 2; which++) {
    const float* in = which ? v_in : k_in;
    if (!in || !T) continue;
    ebyte* base = (which ? c->rows[(size_t)row].vcache : c->rows[(size_t)row].kcache) + (size_t)layer * d.kv_heads * per_head * c->esz;
    if (c->kv_paged) base = (which ? c->slab_v : c->slab_k) + (size_t)layer * c->kv.n_blocks() * d.kv_heads * tgx::KV_BLOCK * hd * c->esz;
    for (int h = 0; h < d.kv_heads; h++) {
      for (size_t t = 0; t < T; t++)
        for (size_t k = 0; k < hd; k++) {   // BSHD view in, head-major cache out; one round-to-nearest-even into the storage dtype
          const float v = in[(t * d.kv_heads + h) * hd + k];
          const size_t i = t * hd + k;
          if (c->dt == tgx::DT_F32) memcpy(tmp.data() + 4 * i, &v, 4);
          else { const uint16_t u = c->dt == tgx::DT_BF16 ? host_f32_to_bf16(v) : host_f32_to_half(v); memcpy(tmp.data() + 2 * i, &u, 2); }
        }
      if (c->kv_paged) {
        for (size_t t0 = 0; t0 < T; t0 += tgx::KV_BLOCK) {
          const size_t n = std::min<size_t>(tgx::KV_BLOCK, T - t0);
          const size_t blk = (size_t)c->kv.block_at(row, (int)(t0 / tgx::KV_BLOCK));
          HIP_OK(c, hipMemcpy(base + ((blk * d.kv_heads + h) * tgx::KV_BLOCK) * hd * c->esz, tmp.data() + t0 * hd * c->esz, n * hd * c->esz, hipMemcpyHostToDevice));
        }
      } else
      HIP_OK(c, hipMemcpy(base + (size_t)h * per_head * c->esz, tmp.data(), T * hd * c->esz, hipMemcpyHostToDevice));
    }
  }
  return TGX_OK;
}

int tgx_profile_decode(tgx_ctx* c, int n_reps, int64_t* launches, double* total_ms) {
  if (!c || !launches || !total_ms || n_reps < 0) return TGX_ERR_INVALID;
  if (!c->have_token) return set_err(c, TGX_ERR_STATE, "profile needs a current token: call tgx_sample after tgx_forward");
  if (c->past + 1 > c->d.max_ctx) return set_err(c, TGX_ERR_CONTEXT, "context size exceeded");
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < TGX_KERNEL_COUNT; i++) { launches[i] = 0; total_ms[i] = 0.0; }
  update_attn_modes(c, c->past, 1);
  // Each class is launched back-to-back over all layers (every launch streams a different layer's weights, so
  // nothing is served from the Infinity Cache) between two events on the launch stream.  The residual
  // epilogues write to a scratch vector: the model state (x, KV cache up to pastLength, token) is untouched.
  for (int rep = 0; rep < n_reps; rep++) {
    for (int cls = 0; cls < TGX_KERNEL_COUNT; cls++) {
      HIP_OK(c, hipEventRecord(c->prof.ev[0], c->stream));
      int n = 0;
      if (cls == TGX_KERNEL_LMHEAD) { launch_lm_head(c, 0, 1); n = 1; }
      else for (int l = 0; l < c->d.layers; l++) n += launch_layer_kernel(c, &c->rows[0], 1, c->prof_same_layer ? 0 : l, cls, c->scratch_x, (long long)c->kv_row_elems);
      HIP_OK(c, hipEventRecord(c->prof.ev[1], c->stream));
      HIP_OK(c, hipEventSynchronize(c->prof.ev[1]));
      float ms = 0.f;
      HIP_OK(c, hipEventElapsedTime(&ms, c->prof.ev[0], c->prof.ev[1]));
      launches[cls] += n;
      total_ms[cls] += ms;
    }
  }
  HIP_OK(c, hipGetLastError());
  c->have_logits = false;   // the lm_head replay overwrote the logits buffer
  return TGX_OK;
}

int tgx_read_probs(tgx_ctx* c, float* out) {
  if (!c || !out) return TGX_ERR_INVALID;
  if (!c->have_probs || !c->have_logits) return set_err(c, TGX_ERR_STATE, "no probabilities: the last sample was greedy or none was taken");
  HIP_OK(c, hipSetDevice(c->device));
  // a sampled step leaves its logits, thresholds and normalisers on the device, not the vector: evaluate it now (rows whose last step was greedy read as zeros)
  const size_t V = (size_t)c->d.vocab;
  for (int b = 0; b < c->batch; b++) {
    if (c->row_host[(size_t)b].probs_ok) launch_probs(c, b, c->row_host[(size_t)b].probs_cfg, c->row_host[(size_t)b].probs_proc);
    else HIP_OK(c, hipMemsetAsync(c->rows[(size_t)b].probs, 0, V * 4, c->stream));
  }
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipStreamSynchronize(c->stream));
  for (int b = 0; b < c->batch; b++) HIP_OK(c, hipMemcpy(out + b * V, c->rows[(size_t)b].probs, V * 4, hipMemcpyDeviceToHost));
  return TGX_OK;
}

int tgx_set_logits(tgx_ctx* c, const float* logits, int batch) {
  if (!c || !logits) return TGX_ERR_INVALID;
  if (!c->finalized) return set_err(c, TGX_ERR_STATE, "set_logits before finalize");
  if (batch < 1 || batch > c->d.max_batch) return set_err(c, TGX_ERR_INVALID, "batch out of range");
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  const size_t V = (size_t)c->d.vocab;
  for (int b = 0; b < batch; b++) HIP_OK(c, hipMemcpy(c->rows[(size_t)b].logits, logits + b * V, V * 4, hipMemcpyHostToDevice));
  // the greedy path reads per-workgroup argmax partials: rebuild them from the injected logits
  for (int b = 0; b < batch; b++) {
    RowState& r = c->rows[(size_t)b];
    launch_argmax_partials(c, r.logits, (int)V, r.part_val, r.part_idx);
  }
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipStreamSynchronize(c->stream));
  c->batch = batch;
  c->have_probs = false;
  for (RowHost& r : c->row_host) r.probs_ok = false;
  c->have_logits = true;
  return TGX_OK;
}

int tgx_get_option(const tgx_ctx* c, const char* key, int* out_value) {
  if (!c || !key || !out_value) return TGX_ERR_INVALID;
  if (!strcmp(key, "attn.direct_limit")) { *out_value = (int)std::min<long long>(direct_limit(c, c->batch, true), INT_MAX); return TGX_OK; }
  if (!strcmp(key, "attn.nw4_limit")) { *out_value = (int)nw4_limit(c, c->batch, true); return TGX_OK; }
  if (!strcmp(key, "graph.steps")) { *out_value = c->graph_steps; return TGX_OK; }
  if (!strcmp(key, "act.round16")) { *out_value = c->act16; return TGX_OK; }
  if (!strcmp(key, "kv.budget_tokens")) { *out_value = c->kv_budget_tokens; return TGX_OK; }
  if (!strcmp(key, "extend.attn_splits")) { *out_value = c->extend_attn_splits; return TGX_OK; }
  if (!strcmp(key, "score.rows")) { *out_value = c->score_rows; return TGX_OK; }
  if (!strcmp(key, "score.vocab_chunk")) { *out_value = c->score_vocab_chunk; return TGX_OK; }
  if (!strcmp(key, "snapshot.stage_kib")) { *out_value = c->snapshot_stage_kib; return TGX_OK; }
  if (!strcmp(key, "verify.last_splits")) { *out_value = c->verify_last_splits; return TGX_OK; }  // read-only: the key splits of the last tgx_verify_rows joint pass's attention (0: unsplit)
  if (!strcmp(key, "verify.processors")) { *out_value = c->verify_processors; return TGX_OK; }
  if (!strcmp(key, "verify.last_form")) { *out_value = c->verify_last_form; return TGX_OK; }      // read-only: the form of the last tgx_verify_rows (0 none yet, 1 the joint pass, 2 row by row)
  if (!strcmp(key, "advance.attn_tiles")) { *out_value = c->advance_attn_tiles; return TGX_OK; }
  if (!strcmp(key, "advance.last_form")) { *out_value = c->advance_last_form; return TGX_OK; }    // read-only: the form of the last tgx_advance_rows (0 none yet, 1 the joint pass, 2 piecewise)
  if (!strcmp(key, "advance.last_tiles")) { *out_value = c->advance_last_tiles; return TGX_OK; }  // read-only: the tile target of the last joint pass's attention (0: nothing split)
  if (!strcmp(key, "embed.last_pool_launches")) { *out_value = c->embed_last_launches; return TGX_OK; }     // read-only: pooling launches (partials + finish) of the last tgx_embed_rows
  if (!strcmp(key, "score.last_form")) { *out_value = c->score_last_form; return TGX_OK; }     // read-only: the form of the last tgx_score_row that scored a position (0 none yet, 1 matrix cores, 2 by groups)
  if (!strcmp(key, "weights.packed")) { *out_value = c->weights_packed; return TGX_OK; }
  if (!strcmp(key, "weights.packed_classes")) { *out_value = c->packed_classes; return TGX_OK; }
  if (!strcmp(key, "weights.packed_matrices")) { *out_value = c->packed_matrices; return TGX_OK; }        // read-only, after tgx_finalize: matrices stored packed ...
  if (!strcmp(key, "weights.packed_fallbacks")) { *out_value = c->packed_fallbacks; return TGX_OK; }      // ... matrices that stayed plain because a row's escape record overflowed ...
  if (!strcmp(key, "weights.packed_max_row_esc")) { *out_value = c->packed_max_row_esc; return TGX_OK; }  // ... and the most escapes seen in one row
  if (!strcmp(key, "weights.fp8")) { *out_value = c->weights_fp8; return TGX_OK; }
  if (!strcmp(key, "weights.fp8_classes")) { *out_value = c->fp8_classes; return TGX_OK; }
  if (!strcmp(key, "weights.fp8_matrices")) { *out_value = c->fp8_matrices; return TGX_OK; }            // read-only, after tgx_finalize: matrices with an 8-bit stream ...
  if (!strcmp(key, "weights.fp8_fallbacks")) { *out_value = c->fp8_fallbacks; return TGX_OK; }          // ... matrices quantized but served by the plain kernel on the dequantized master
  if (!strcmp(key, "kv.free_tokens")) { *out_value = c->kv_paged ? (int)c->kv.free_blocks() * tgx::KV_BLOCK : -1; return TGX_OK; }      // paged KV: tokens' worth of unassigned blocks
  if (!strcmp(key, "mem.live_allocs")) { *out_value = (int)c->mem.live(); return TGX_OK; }                     // read-only: device buffers the context holds now ...
  if (!strcmp(key, "mem.live_kib")) { *out_value = (int)((c->mem.live_bytes() + 1023) / 1024); return TGX_OK; }  // ... and their bytes, rounded up to KiB
  return TGX_ERR_INVALID;
}

int tgx_set_option(tgx_ctx* c, const char* key, int value) {
  if (!c || !key) return TGX_ERR_INVALID;
  static const char* cls_names[TGX_KERNEL_COUNT] = {"qkv", "attn", "oproj", "gateup", "down", "lmhead"};
  drop_step_graphs(c);
  if (!strcmp(key, "graph")) { c->use_graph = value != 0; return TGX_OK; }
  if (!strcmp(key, "graph.steps")) { if (value < 1 || value > 64) return set_err(c, TGX_ERR_INVALID, "graph.steps out of range"); c->graph_steps = value; return TGX_OK; }
  if (!strcmp(key, "debug.skip")) { c->debug_skip = value; return TGX_OK; }
  if (!strcmp(key, "debug.attn")) { c->debug_attn = value; return TGX_OK; }
  if (!strcmp(key, "attn.gmax")) {   // query heads per attention workgroup: the kernel is instantiated for 1..4 (0 = default)
    if (value < 0 || value > 4) return set_err(c, TGX_ERR_INVALID, "attn.gmax must be 0 (default) or 1..4");
    c->attn_gmax = value; return TGX_OK;
  }
  if (!strcmp(key, "attn.direct_max")) { c->attn_direct_max = c->attn_fused_max = value; return TGX_OK; }      // (both forms of the limit: an explicit value forces the form)
  if (!strcmp(key, "attn.direct_nw4")) { drop_step_graphs(c); c->attn_direct_nw4 = c->attn_fused_nw4 = value; return TGX_OK; }
  if (!strcmp(key, "prefill.qkv_nosplit")) { c->qkv_nosplit = value; return TGX_OK; }
  if (!strcmp(key, "prefill.splitk_8k")) { c->splitk_8k = value; return TGX_OK; }
  if (!strcmp(key, "act.round16")) { drop_step_graphs(c); c->act16 = value != 0; return TGX_OK; }
  if (!strcmp(key, "act.one_term_kernels")) { c->act16_kernels = value != 0; return TGX_OK; }      // 0: the two-term kernels on the all-zero second term (bit-identical; tests)      // (the all-zero term buffer is allocated with the next workspace check)
  if (!strcmp(key, "oproj.fused")) { drop_step_graphs(c); c->oproj_fused = value != 0; return TGX_OK; }
  if (!strcmp(key, "attn.raw_fuse")) { drop_step_graphs(c); c->attn_raw_fuse = value; return TGX_OK; }
  if (!strcmp(key, "attn.batch_mfma")) { if (value < 0) return set_err(c, TGX_ERR_INVALID, "attn.batch_mfma is a row count (0 = off)"); drop_step_graphs(c); c->attn_batch_mfma = value; return TGX_OK; }
  if (!strcmp(key, "attn.mfma_min")) { c->attn_mfma_min = value; return TGX_OK; }
  if (!strcmp(key, "prefill.defer_reduce")) { c->defer_reduce = value != 0; return TGX_OK; }
  if (!strcmp(key, "skinny.dma")) { drop_step_graphs(c); c->skinny_dma = value != 0; return TGX_OK; }
  if (!strcmp(key, "skinny.dma_oproj")) { drop_step_graphs(c); c->skinny_dma_oproj = value; return TGX_OK; }
  if (!strcmp(key, "skinny.terms")) { drop_step_graphs(c); c->skinny_terms = value; return TGX_OK; }     // 2: the QKV and lm_head products of 17-32-row batches as well (experiment)
  if (!strcmp(key, "skinny.ksplit")) { if (value < 0 || value > 2) return set_err(c, TGX_ERR_INVALID, "skinny.ksplit must be 0, 1 (<= 16 rows) or 2 (<= 32 rows)"); c->skinny_ksplit = value; return TGX_OK; }
  if (!strcmp(key, "prefill.gemm_tm")) { c->gemm_tm = value; return TGX_OK; }
  if (!strcmp(key, "debug.gemv")) { c->debug_gemv = value; return TGX_OK; }
  if (!strcmp(key, "prefill.mfma")) { c->prefill_mfma = value != 0; return TGX_OK; }
  if (!strcmp(key, "prefill.min_rows")) { c->prefill_min_rows = value; return TGX_OK; }
  if (!strcmp(key, "prefill.f32_min_rows")) { c->prefill_f32_min_rows = value; return TGX_OK; }
  if (!strcmp(key, "prefill.splitk")) { c->gemm_splitk = value; return TGX_OK; }
  if (!strcmp(key, "decode.step_rows")) { if (value != 32 && value != 64 && value != 128) return set_err(c, TGX_ERR_INVALID, "decode.step_rows is 32, 64 or 128"); drop_step_graphs(c); c->decode_step_rows = value; return TGX_OK; }
  if (!strcmp(key, "prefill.skinny_hidden_max")) { c->prefill_skinny_hidden_max = value; return TGX_OK; }
  if (!strcmp(key, "prefill.skinny_rows")) { if (value < 0 || value > 128) return set_err(c, TGX_ERR_INVALID, "prefill.skinny_rows is 0..128"); c->prefill_skinny_rows = value; return TGX_OK; }
  if (!strcmp(key, "prefill.wide_8k_eff")) { c->wide_8k_eff = value; return TGX_OK; }
  if (!strcmp(key, "prefill.wide_n_min")) { c->wide_n_min = value; return TGX_OK; }
  if (!strcmp(key, "prefill.attn_dma")) { c->attn_dma = value; return TGX_OK; }
  if (!strcmp(key, "prefill.attn_ksplit")) { c->attn_ksplit = value; return TGX_OK; }
  if (!strcmp(key, "attn.qk_fuse")) { c->qk_fuse = value; return TGX_OK; }
  if (!strcmp(key, "prefill.skinny")) { c->prefill_skinny = value; return TGX_OK; }
  if (!strcmp(key, "decode.mfma_min_batch")) { if (value < 1) return set_err(c, TGX_ERR_INVALID, "decode.mfma_min_batch must be >= 1"); c->decode_mfma_min = value; return TGX_OK; }
  if (!strcmp(key, "debug.profile_same_layer")) { c->prof_same_layer = value; return TGX_OK; }
  if (!strcmp(key, "extend.attn_splits")) { if (value < -1) return set_err(c, TGX_ERR_INVALID, "extend.attn_splits is -1 (automatic), 0 (never) or a split count"); c->extend_attn_splits = value; return TGX_OK; }
  if (!strcmp(key, "advance.attn_tiles")) { if (value < -1) return set_err(c, TGX_ERR_INVALID, "advance.attn_tiles is -1 (automatic), 0 (never split) or a tile count"); c->advance_attn_tiles = value; return TGX_OK; }
  if (!strcmp(key, "score.rows")) { if (value < 64 || value % 64) return set_err(c, TGX_ERR_INVALID, "score.rows is a positive multiple of 64"); c->score_rows = value; return TGX_OK; }
  if (!strcmp(key, "score.vocab_chunk")) { if (value < 1024 || value % 1024) return set_err(c, TGX_ERR_INVALID, "score.vocab_chunk is a positive multiple of 1024"); c->score_vocab_chunk = value; return TGX_OK; }
  if (!strcmp(key, "snapshot.stage_kib")) { if (value < 1) return set_err(c, TGX_ERR_INVALID, "snapshot.stage_kib is a size in KiB (one layer of a row is always staged)"); c->snapshot_stage_kib = value; return TGX_OK; }
  if (!strcmp(key, "verify.processors")) {      // 1: the chain verify calls take rows with a logit processor on (include/tgx.h); read on the host at each call
    if (value != 0 && value != 1) return set_err(c, TGX_ERR_INVALID, "verify.processors is 0 or 1");
    c->verify_processors = value; return TGX_OK;
  }
  if (!strcmp(key, "oproj.sliced")) { drop_step_graphs(c); c->oproj_sliced = value != 0; return TGX_OK; }
  if (!strcmp(key, "weights.packed") || !strcmp(key, "weights.packed_classes")) {
    if (c->finalized) return set_err(c, TGX_ERR_STATE, "%s is set before tgx_finalize (the packed copies are made there)", key);
    if (key[14] == '_') { if (value < 0 || value > 7) return set_err(c, TGX_ERR_INVALID, "weights.packed_classes is a mask of gate_up (1), down (2), lm_head (4)"); c->packed_classes = value; }
    else c->weights_packed = value != 0;
    return TGX_OK;
  }
  if (!strcmp(key, "weights.fp8") || !strcmp(key, "weights.fp8_classes")) {
    if (c->finalized) return set_err(c, TGX_ERR_STATE, "%s is set before tgx_finalize (the weights are quantized there)", key);
    if (key[11] == '_') { if (value < 0 || value > 7) return set_err(c, TGX_ERR_INVALID, "weights.fp8_classes is a mask of gate_up (1), down (2), lm_head (4)"); c->fp8_classes = value; }
    else { if (value != 0 && value != 1) return set_err(c, TGX_ERR_INVALID, "weights.fp8 is 0 or 1"); c->weights_fp8 = value; }
    return TGX_OK;
  }
  if (!strcmp(key, "kv.budget_tokens")) {
    if (c->finalized) return set_err(c, TGX_ERR_STATE, "kv.budget_tokens is set before tgx_finalize (it sizes the caches)");
    if (value < 0) return set_err(c, TGX_ERR_INVALID, "kv.budget_tokens >= 0 (0 = one max_ctx slab per row)");
    c->kv_budget_tokens = value; return TGX_OK;
  }
  if (!strcmp(key, "attn.nsplit")) {
    if (c->finalized) return set_err(c, TGX_ERR_STATE, "attn.nsplit must be set before tgx_finalize");
    if (value < 1 || value > 32) return set_err(c, TGX_ERR_INVALID, "attn.nsplit out of range");
    c->attn_nsplit_opt = value;
    return TGX_OK;
  }
  for (int i = 0; i < TGX_KERNEL_COUNT; i++) {
    const size_t n = strlen(cls_names[i]);
    if (strncmp(key, cls_names[i], n) || key[n] != '.') continue;
    if (!strcmp(key + n + 1, "ks")) {
      if (value != 1 && value != 2 && value != 4) return set_err(c, TGX_ERR_INVALID, "ks must be 1, 2 or 4");
      c->tune[i].ks = value;
      return TGX_OK;
    }
    if (!strcmp(key + n + 1, "bpc")) {
      if (value < 1 || value > 16) return set_err(c, TGX_ERR_INVALID, "bpc out of range");
      if (i == TGX_KERNEL_LMHEAD && c->finalized) return set_err(c, TGX_ERR_STATE, "lmhead.bpc must be set before tgx_finalize");
      c->tune[i].bpc = value;
      return TGX_OK;
    }
    if (!strcmp(key + n + 1, "packed_bpc") && (i == TGX_KERNEL_GATEUP || i == TGX_KERNEL_DOWN || i == TGX_KERNEL_LMHEAD)) {      // the classes with a packed form
      if (value < 1 || value > 16) return set_err(c, TGX_ERR_INVALID, "packed_bpc out of range");
      if (i == TGX_KERNEL_LMHEAD && c->finalized) return set_err(c, TGX_ERR_STATE, "lmhead.packed_bpc must be set before tgx_finalize");
      c->tune[i].packed_bpc = value;
      return TGX_OK;
    }
  }
  return set_err(c, TGX_ERR_INVALID, "unknown option %s", key);
}

int64_t tgx_bytes_per_token(const tgx_ctx* c, int64_t T) {
  if (!c) return -1;
  const tgx_model_desc& d = c->d;
  const int64_t H = d.hidden, I = d.inter, V = d.vocab, L = d.layers, q = (int64_t)d.heads * d.head_dim, kv = (int64_t)d.kv_heads * d.head_dim;
  const int64_t b = (int64_t)c->esz;   // bytes per stored parameter / cache element
  if (c->gpt2) {   // c_attn, c_proj, c_fc, mlp.c_proj with their biases, two LayerNorms (weight + bias); ln_f, one wpe row, the wte head
    const int64_t per_layer = 3 * H * H + 3 * H + H * H + H + I * H + I + H * I + H + 4 * H;
    return b * (L * per_layer + 2 * H + H + V * H) + b * 2 * L * kv * T;
  }
  const int64_t per_layer = (q + 2 * kv) * H + (d.qkv_bias ? (q + 2 * kv) : 0) + H * q + 2 * I * H + H * I + 2 * H;
  // exponent-packed matrices (option weights.packed) stream their planes and escape records instead of 2 bytes per weight
  int64_t saved = 0;
  auto packed_saving = [&](const PackedMat& m, int64_t rows, int64_t cols) { if (m.P) saved += b * rows * cols - rows * (m.row_bytes + 16 * m.ks); };      // (one 16-byte record per row and K-part)
  for (const LayerW& w : c->L) { packed_saving(w.pgu, 2 * I, H); packed_saving(w.pdown, H, I); }
  packed_saving(c->plm, V, H);
  // matrices quantized by option weights.fp8 stream their code planes and one 4-byte scale per row
  auto fp8_saving = [&](const Fp8Mat& m, int64_t rows, int64_t cols) { if (m.Q) saved += b * rows * cols - rows * (m.row_bytes + 4); };
  for (const LayerW& w : c->L) { fp8_saving(w.qgu, 2 * I, H); fp8_saving(w.qdown, H, I); }
  fp8_saving(c->qlm, V, H);
  return b * (L * per_layer + H + V * H) + b * 2 * L * kv * T - saved;
}

}  // extern "C"
