// decode.hip — the batch-1..4 decode step of the MI355X shim: one launch per kernel class and layer (kernels/gemv.h), the K-sliced o_proj behind
// split-form attention (kernels/oproj_sliced.h), lm_head + per-workgroup argmax, the greedy finalize.
// == for (auto& layer : layers_) x = layer->forward(x); norm; lm_head  (GPTModel.h:51-58, DecoderLayer.h:38-43, Attention.h:71-91, GatedMLP.h:37-41)
#include "ctx.h"
#include "gemv_grid.h"
#include "kernels/attn_decode.h"
#include "kernels/gemv.h"
#include "kernels/gemv_packed.h"
#include "kernels/gemv_fp8.h"
#include "kernels/oproj_sliced.h"
#include "kernels/verify.h"
#include "kernels/kv_tree.h"

int gemv_grid(const tgx_ctx* c, int units, int ks, int bpc) { return tgx::gemv_grid_plan(units, 4 / ks, c->num_cus * bpc).grid; }

// 16-byte slices per lane per row for a K range split over ks waves (the kernel's NX template parameter)
static int gemv_nx(int K, int ks) { return ((K / 8) + ks * 64 - 1) / (ks * 64); }

// smallest K split that keeps a wave's slice within 8 x 512 elements; norm-fused launches must use 1
static int gemv_auto_ks(int K, int want) {
  int ks = want;
  while (ks < 4 && gemv_nx(K, ks) > 8) ks *= 2;
  return ks;
}

// the argument block of batch row `r` alone (every slab pointer advanced by r row strides)
static tgx::GemvArgs gemv_row(const tgx_ctx* c, tgx::GemvArgs a, int r) {
  a.x += (size_t)r * a.x_stride;
  if (a.out) a.out += (size_t)r * a.out_stride;
  if (a.q_out) a.q_out += (size_t)r * a.q_stride;
  if (a.k_raw) a.k_raw += (size_t)r * a.kraw_stride;
  if (a.k_cache) a.k_cache = (ebyte*)a.k_cache + (size_t)r * a.kv_stride * c->esz;
  if (a.v_cache) a.v_cache = (ebyte*)a.v_cache + (size_t)r * a.kv_stride * c->esz;
  if (a.pos) a.pos += r;
  if (a.blk_tbl) a.blk_tbl += (size_t)r * a.tbl_stride;
  if (a.logits) a.logits += (size_t)r * a.logits_stride;
  if (a.part_val) a.part_val += (size_t)r * a.part_stride;
  if (a.part_idx) a.part_idx += (size_t)r * a.part_stride;
  return a;
}

template <int DT, int PRO, int EPI, int NX>
static void launch_gemv_nx(tgx_ctx* c, const tgx::GemvArgs& a, int grid, int R) {
  const dim3 g(grid), b(256);
  // rows share the weight pass; R x NX activation slices of 8 floats stay in registers (4 x 8 x 8 = 256 of the 512 a wave
  // of a 256-thread workgroup may use)
  if (R == 4) { hipLaunchKernelGGL((tgx::gemv_kernel<DT, PRO, EPI, NX, 4>), g, b, 0, c->stream, a); return; }
  if (R == 2) { hipLaunchKernelGGL((tgx::gemv_kernel<DT, PRO, EPI, NX, 2>), g, b, 0, c->stream, a); return; }
  // the fixed-point residual stream behind the K-sliced o_proj (batch 1, 16-bit storage, RMSNorm families): gate_up reads it, down adds to it
  if constexpr (DT != tgx::DT_F32 && ((PRO == tgx::PRO_RMSNORM && EPI == tgx::EPI_SILU_MUL) || (PRO == tgx::PRO_PLAIN && EPI == tgx::EPI_RESIDUAL))) {
    if (R == 1 && (a.x_acc || a.res_acc)) { hipLaunchKernelGGL((tgx::gemv_kernel<DT, PRO, EPI, NX, 1, true>), g, b, a.x_acc ? (size_t)a.K * 4 : 0, c->stream, a); return; }
  }
  for (int r = 0; r < R; r++) hipLaunchKernelGGL((tgx::gemv_kernel<DT, PRO, EPI, NX, 1>), g, b, 0, c->stream, gemv_row(c, a, r));
}

// ---- exponent-packed weights (kernels/gemv_packed.h; option weights.packed) ----
template <int PRO, int EPI, int NX>
static void launch_gemv_packed_nx(tgx_ctx* c, const tgx::GemvPackedArgs& p, int grid) {
  const dim3 g(grid), b(256);
  if constexpr (EPI != tgx::EPI_LOGITS) {      // the fixed-point residual stream behind the K-sliced o_proj (launch_gemv_nx)
    if (p.g.x_acc || p.g.res_acc) { hipLaunchKernelGGL((tgx::gemv_packed_kernel<PRO, EPI, NX, true>), g, b, p.g.x_acc ? (size_t)p.g.K * 4 : 0, c->stream, p); return; }
  }
  hipLaunchKernelGGL((tgx::gemv_packed_kernel<PRO, EPI, NX, false>), g, b, 0, c->stream, p);
}

template <int PRO, int EPI>
static void launch_gemv_packed(tgx_ctx* c, const tgx::GemvArgs& a, const PackedMat& pk, int grid, int nx) {
  tgx::GemvPackedArgs p{};
  p.g = a; p.P = pk.P; p.rec = pk.rec; p.row_bytes = pk.row_bytes; p.e0h4 = pk.e0h4;
  switch (nx) {
    case 1: launch_gemv_packed_nx<PRO, EPI, 1>(c, p, grid); break;
    case 2: launch_gemv_packed_nx<PRO, EPI, 2>(c, p, grid); break;
    case 3: launch_gemv_packed_nx<PRO, EPI, 3>(c, p, grid); break;
    case 4: launch_gemv_packed_nx<PRO, EPI, 4>(c, p, grid); break;
    case 5: launch_gemv_packed_nx<PRO, EPI, 5>(c, p, grid); break;
    case 6: launch_gemv_packed_nx<PRO, EPI, 6>(c, p, grid); break;
    case 7: launch_gemv_packed_nx<PRO, EPI, 7>(c, p, grid); break;
    default: launch_gemv_packed_nx<PRO, EPI, 8>(c, p, grid); break;
  }
}

// One matrix of class `cls` into the packed form, laid out for the K split its batch-1 launch uses now.  Leaves `out` empty (the plain kernel serves the
// matrix) when the shape is outside the format or a row has more escapes than its record holds.
static int pack_matrix(tgx_ctx* c, const ebyte* W, int N, int K, int cls, int* stat_dev, PackedMat* out) {
  const int ks = gemv_auto_ks(K, c->tune[cls].ks), nx = gemv_nx(K, ks);
  if (K % 8 || K > tgx::PACKED_K_MAX || nx > 8) return TGX_OK;
  PackedMat m;
  m.ks = ks; m.row_bytes = (long long)ks * ((nx + 3) / 4) * 3072;
  int rc;
  if ((rc = dev_alloc(c, &m.P, (size_t)N * (size_t)m.row_bytes)) || (rc = dev_alloc(c, &m.rec, (size_t)N * (size_t)ks))) { dev_free(c, &m.P); return rc; }
  HIP_OK(c, hipMemsetAsync(stat_dev, 0, 4 * sizeof(int), c->stream));
  const size_t n8 = (size_t)N * K / 8;
  hipLaunchKernelGGL(tgx::packed_maxexp_kernel, dim3((unsigned)std::min<size_t>((n8 + 255) / 256, 4096)), dim3(256), 0, c->stream, reinterpret_cast<const bf16_t*>(W), n8, stat_dev);
  tgx::PackRowsArgs a{};
  a.W = reinterpret_cast<const bf16_t*>(W); a.N = N; a.K = K; a.ks = ks; a.nx = nx; a.P = m.P; a.rec = m.rec; a.row_bytes = m.row_bytes; a.stat = stat_dev;
  hipLaunchKernelGGL(tgx::pack_rows_kernel, dim3(N), dim3(64), 0, c->stream, a);
  int stat[4] = {0, 0, 0, 0};
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipMemcpyAsync(stat, stat_dev, sizeof(stat), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  c->packed_max_row_esc = std::max(c->packed_max_row_esc, stat[3]);
  if (stat[1] > 0) {       // a (row, K-part)'s escapes do not fit its record: this matrix stays plain
    dev_free(c, &m.P); dev_free(c, &m.rec);
    c->packed_fallbacks++;
    return TGX_OK;
  }
  const unsigned int E0h = (unsigned int)std::max((stat[0] >> 1) - 7, 0);
  m.e0h4 = E0h * 0x01010101u; m.n_esc = stat[2]; m.max_row_esc = stat[3];
  *out = m;
  c->packed_matrices++;
  return TGX_OK;
}

int pack_weights(tgx_ctx* c) {
  const tgx_model_desc& d = c->d;
  if (!c->weights_packed || c->dt != tgx::DT_BF16 || c->gpt2) return TGX_OK;      // (GPT-2's LayerNorm / GELU launches have no packed form)
  const int classes = c->packed_classes & ~(c->weights_fp8 ? c->fp8_classes : 0);      // a class quantized by weights.fp8 streams its codes: a packed copy would never be read
  int* stat_dev = nullptr;
  int rc = dev_alloc(c, &stat_dev, 4);
  for (size_t l = 0; l < c->L.size() && !rc; l++) {
    LayerW& w = c->L[l];
    if (classes & 1) rc = pack_matrix(c, w.wgu, 2 * d.inter, d.hidden, TGX_KERNEL_GATEUP, stat_dev, &w.pgu);
    if (!rc && (classes & 2) && d.inter <= 16384) rc = pack_matrix(c, w.wdown, d.hidden, d.inter, TGX_KERNEL_DOWN, stat_dev, &w.pdown);
  }
  if (!rc && (classes & 4)) rc = pack_matrix(c, d.tied ? c->embed : c->lm_head, d.vocab, d.hidden, TGX_KERNEL_LMHEAD, stat_dev, &c->plm);
  dev_free(c, &stat_dev);
  return rc;
}

// ---- FP8 weights (kernels/gemv_fp8.h; option weights.fp8) ----
template <int PRO, int EPI, int NX>
static void launch_gemv_fp8_nx(tgx_ctx* c, const tgx::GemvFp8Args& p, int grid) {
  const dim3 g(grid), b(256);
  if constexpr (EPI != tgx::EPI_LOGITS) {      // the fixed-point residual stream behind the K-sliced o_proj (launch_gemv_nx)
    if (p.g.x_acc || p.g.res_acc) { hipLaunchKernelGGL((tgx::gemv_fp8_kernel<PRO, EPI, NX, true>), g, b, p.g.x_acc ? (size_t)p.g.K * 4 : 0, c->stream, p); return; }
  }
  hipLaunchKernelGGL((tgx::gemv_fp8_kernel<PRO, EPI, NX, false>), g, b, 0, c->stream, p);
}

template <int PRO, int EPI>
static void launch_gemv_fp8(tgx_ctx* c, const tgx::GemvArgs& a, const Fp8Mat& q, int grid, int nx) {
  tgx::GemvFp8Args p{};
  p.g = a; p.Q = q.Q; p.scale = q.scale; p.row_bytes = q.row_bytes;
  switch (nx) {
    case 1: launch_gemv_fp8_nx<PRO, EPI, 1>(c, p, grid); break;
    case 2: launch_gemv_fp8_nx<PRO, EPI, 2>(c, p, grid); break;
    case 3: launch_gemv_fp8_nx<PRO, EPI, 3>(c, p, grid); break;
    case 4: launch_gemv_fp8_nx<PRO, EPI, 4>(c, p, grid); break;
    case 5: launch_gemv_fp8_nx<PRO, EPI, 5>(c, p, grid); break;
    case 6: launch_gemv_fp8_nx<PRO, EPI, 6>(c, p, grid); break;
    case 7: launch_gemv_fp8_nx<PRO, EPI, 7>(c, p, grid); break;
    default: launch_gemv_fp8_nx<PRO, EPI, 8>(c, p, grid); break;
  }
}

// The matrices of the classes in weights.fp8_classes, quantized where they lie (the rule: include/tgx.h).  Two launches per matrix: the row scales and the
// check for weights the rule refuses — all matrices first, so that nothing is overwritten when one is refused — then the dequantized master, the codes in the
// layout of the class's batch-1 launch and nothing else.  A matrix whose shape the layout does not cover is quantized all the same and keeps no stream.
int quantize_weights(tgx_ctx* c) {
  const tgx_model_desc& d = c->d;
  if (!c->weights_fp8) return TGX_OK;
  struct Job { ebyte* W; int N, K, cls, layer; Fp8Mat* out; };
  std::vector<Job> jobs;
  for (size_t l = 0; l < c->L.size(); l++) {
    LayerW& w = c->L[l];
    if (c->fp8_classes & 1) jobs.push_back({w.wgu, 2 * d.inter, d.hidden, TGX_KERNEL_GATEUP, (int)l, &w.qgu});
    if (c->fp8_classes & 2) jobs.push_back({w.wdown, d.hidden, d.inter, TGX_KERNEL_DOWN, (int)l, &w.qdown});
  }
  if (c->fp8_classes & 4) jobs.push_back({d.tied ? c->embed : c->lm_head, d.vocab, d.hidden, TGX_KERNEL_LMHEAD, -1, &c->qlm});
  if (jobs.empty()) return TGX_OK;
  int* stat_dev = nullptr;
  int rc = dev_alloc(c, &stat_dev, jobs.size());
  if (rc) return rc;
  std::vector<float*> scale(jobs.size(), nullptr);
  std::vector<int> stat(jobs.size(), INT_MAX);
  auto drop = [&]() { for (float*& s : scale) if (s) dev_free(c, &s); dev_free(c, &stat_dev); };
  if (hipMemcpyAsync(stat_dev, stat.data(), stat.size() * sizeof(int), hipMemcpyHostToDevice, c->stream) != hipSuccess) { drop(); return set_err(c, TGX_ERR_DEVICE, "weights.fp8: the status upload failed"); }
  for (size_t i = 0; i < jobs.size(); i++) {
    if ((rc = dev_alloc(c, &scale[i], (size_t)jobs[i].N))) { drop(); return rc; }
    hipLaunchKernelGGL(tgx::fp8_row_scale_kernel, dim3(jobs[i].N), dim3(64), 0, c->stream, reinterpret_cast<const bf16_t*>(jobs[i].W), jobs[i].K, scale[i], stat_dev + i);
  }
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(stat.data(), stat_dev, stat.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) { drop(); return set_err(c, TGX_ERR_DEVICE, "weights.fp8: the scan of the weights failed"); }
  for (size_t i = 0; i < jobs.size(); i++) {
    if (stat[i] >= jobs[i].N) continue;
    const Job& j = jobs[i];
    char name[96];
    if (j.cls == TGX_KERNEL_LMHEAD) snprintf(name, sizeof name, "%s", d.tied ? "model.embed_tokens.weight" : "lm_head.weight");
    else snprintf(name, sizeof name, "model.layers.%d.mlp.%s_proj.weight", j.layer, j.cls == TGX_KERNEL_DOWN ? "down" : (stat[i] < d.inter ? "gate" : "up"));
    drop();
    return set_err(c, TGX_ERR_UNSUPPORTED, "weights.fp8: %s holds a non-finite weight or one of magnitude 2^100 or more (row %d)", name, stat[i]);
  }
  for (size_t i = 0; i < jobs.size(); i++) {
    const Job& j = jobs[i];
    const int ks = gemv_auto_ks(j.K, c->tune[j.cls].ks), nx = gemv_nx(j.K, ks);
    const bool stream = j.K % 8 == 0 && nx <= 8;
    Fp8Mat m;
    tgx::Fp8QuantArgs a{};
    a.W = reinterpret_cast<bf16_t*>(j.W); a.K = j.K; a.ks = ks; a.nx = nx; a.scale = scale[i];
    if (stream) {
      m.ks = ks; m.row_bytes = (long long)ks * ((nx + 1) / 2) * 1024; m.scale = scale[i];
      if ((rc = dev_alloc(c, &m.Q, (size_t)j.N * (size_t)m.row_bytes))) { drop(); return rc; }
      if (hipMemsetAsync(m.Q, 0, (size_t)j.N * (size_t)m.row_bytes, c->stream) != hipSuccess) { dev_free(c, &m.Q); drop(); return set_err(c, TGX_ERR_DEVICE, "weights.fp8: clearing the code planes failed"); }
      a.Q = m.Q; a.row_bytes = m.row_bytes;
    }
    hipLaunchKernelGGL(tgx::fp8_quant_rows_kernel, dim3(j.N), dim3(64), 0, c->stream, a);
    if (stream) { *j.out = m; scale[i] = nullptr; c->fp8_matrices++; }      // (the stream keeps its scales)
    else c->fp8_fallbacks++;
  }
  const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
  drop();
  return ok ? TGX_OK : set_err(c, TGX_ERR_DEVICE, "weights.fp8: quantizing the weights failed");
}

template <int PRO, int EPI>
static void launch_gemv(tgx_ctx* c, tgx::GemvArgs a, int cls, int R, const PackedMat* pk = nullptr, const Fp8Mat* q8 = nullptr) {
  const Tune& tn = c->tune[cls];
  a.dbg = ((c->debug_gemv >> (8 + cls)) & 1) ? (c->debug_gemv & 15) : 0;
  if (!a.ldw) a.ldw = a.K;
  a.ks = gemv_auto_ks(a.K, tn.ks);   // norm-fused launches K-split too (their waves exchange the sums of squares through LDS)
  while (R > 1 && a.ks < 4 && gemv_nx(a.K, a.ks) > 4) a.ks *= 2;   // batch rows: at most 4 slices per row and lane (measured: B = 2 and 4 on the 1B / 3B / 7B shapes)
  // two rows on the gate_up launch: 2 slices per row and lane leave room for the double-buffered weight registers (R x NX <= 4):
  // Llama-3.2-1B B = 2: 2394 -> 2506 tok/s; the same split loses 2-6 % at B = 4 and on the other launches (tools/batch_bench.py --opts)
  if (R == 2 && cls == TGX_KERNEL_GATEUP && a.ks == 1 && gemv_nx(a.K, 1) == 4) a.ks = 2;
  const int grid = (EPI == tgx::EPI_LOGITS) ? c->lm_grid : gemv_grid(c, a.units, a.ks, tn.bpc);
  const int nx = gemv_nx(a.K, a.ks);
  if constexpr ((PRO == tgx::PRO_RMSNORM && (EPI == tgx::EPI_SILU_MUL || EPI == tgx::EPI_LOGITS)) || (PRO == tgx::PRO_PLAIN && EPI == tgx::EPI_RESIDUAL)) {
    // batch 1 over a matrix quantized by option weights.fp8 with a stream laid out for this K split: half the bytes, bit-identical to the plain kernel over the
    // dequantized master (workgroups per CU: the class's packed_bpc — no other value has been measured yet, profiles/weights_fp8.txt)
    if (q8 && q8->Q && R == 1 && q8->ks == a.ks && a.ldw == a.K && !a.dbg) {
      launch_gemv_fp8<PRO, EPI>(c, a, *q8, (EPI == tgx::EPI_LOGITS) ? grid : gemv_grid(c, a.units, a.ks, tn.packed_bpc), nx);
      return;
    }
    // batch 1 over an exponent-packed matrix laid out for this K split: 25 % fewer bytes, bit-identical results
    // (its own workgroups per CU, Tune::packed_bpc; the lm_head's grid is lm_grid in both forms: it sizes the argmax partials)
    if (pk && pk->P && R == 1 && pk->ks == a.ks && a.ldw == a.K && !a.dbg) {
      launch_gemv_packed<PRO, EPI>(c, a, *pk, (EPI == tgx::EPI_LOGITS) ? grid : gemv_grid(c, a.units, a.ks, tn.packed_bpc), nx);
      return;
    }
  }
  if constexpr (PRO == tgx::PRO_LAYERNORM || EPI == tgx::EPI_GELU) {   // GPT-2 (hidden <= 2048, checked in tgx_create): at most 4 slices per lane
    TGX_DT_SWITCH(c->dt, switch (nx) {
      case 1: launch_gemv_nx<DT, PRO, EPI, 1>(c, a, grid, R); break;
      case 2: launch_gemv_nx<DT, PRO, EPI, 2>(c, a, grid, R); break;
      case 3: launch_gemv_nx<DT, PRO, EPI, 3>(c, a, grid, R); break;
      default: launch_gemv_nx<DT, PRO, EPI, 4>(c, a, grid, R); break;
    })
  } else {
    TGX_DT_SWITCH(c->dt, switch (nx) {
      case 1: launch_gemv_nx<DT, PRO, EPI, 1>(c, a, grid, R); break;
      case 2: launch_gemv_nx<DT, PRO, EPI, 2>(c, a, grid, R); break;
      case 3: launch_gemv_nx<DT, PRO, EPI, 3>(c, a, grid, R); break;
      case 4: launch_gemv_nx<DT, PRO, EPI, 4>(c, a, grid, R); break;
      case 5: launch_gemv_nx<DT, PRO, EPI, 5>(c, a, grid, R); break;
      case 6: launch_gemv_nx<DT, PRO, EPI, 6>(c, a, grid, R); break;
      case 7: launch_gemv_nx<DT, PRO, EPI, 7>(c, a, grid, R); break;
      default: launch_gemv_nx<DT, PRO, EPI, 8>(c, a, grid, R); break;
    })
  }
}

static void fill_strides(const tgx_ctx* c, tgx::GemvArgs& a) {
  const tgx_model_desc& d = c->d;
  a.x_stride = 0; a.out_stride = 0;       // set per call site (x and out come from different slabs)
  a.q_stride = (long long)d.heads * d.head_dim; a.kraw_stride = (long long)d.kv_heads * d.head_dim;
  a.kv_stride = (long long)c->kv_row_elems; a.logits_stride = d.vocab; a.part_stride = c->lm_grid;
  a.act16 = c->act16;
}

// Qwen3: independent batch rows (each its own cache) take the q/k norm inside the attention launch; the positions of one sequence that a
// prefill-by-steps pass handles together (kv_stride 0) need each other's finished keys, so they keep the separate norm launch
static bool qk_fused(const tgx_ctx* c, long long kv_stride) { return c->d.qk_norm && c->d.head_dim == 128 && kv_stride != 0 && c->qk_fuse; }

// The K-sliced o_proj with the attention merge in its prologue (kernels/oproj_sliced.h; no attn_combine launch, fixed-point residual stream between o_proj
// and down) serves batch-1 steps on the VALU split attention form: head_dim 64 (a slice of 2-4 heads reads 9-35 KB of records; at head_dim 128 the records
// outweigh the launch it removes: Llama-3.2-3B -0.2 us per layer, Mistral-7B +3.4, tools/probes/layer_lab.hip), 16-bit storage, RMSNorm families
// without an o_proj bias, one down launch (intermediate <= 16384), row blocks that tile hidden.  Measured on Llama-3.2-1B at context 2064:
// {attention, combine, o_proj} 12.9 -> {attention, sliced o_proj} 10.2 us per layer; Qwen2.5-0.5B 10.1 -> 8.4 (profiles/r04_oproj_sliced.txt).
bool oproj_sliced_ok(const tgx_ctx* c, int R, long long kv_stride) {
  const tgx_model_desc& d = c->d;
  if (!c->oproj_sliced || R != 1 || kv_stride == 0 || c->attn_direct || c->attn_mfma || c->gpt2 || c->dt == tgx::DT_F32 || !c->slab_acc) return false;
  if (d.head_dim != 64 || d.qk_norm || d.inter > 16384 || c->attn_nsplit > 32) return false;
  if (d.hidden > tgx::XACC_HIDDEN_MAX) return false;     // the fixed-point gate_up hands the converted residual to its waves through hidden * 4 bytes of LDS
  const int qd = d.heads * d.head_dim;
  if (qd % 256 == 0) return d.hidden % tgx::oproj_sliced_rows<32>() == 0;
  return qd % 128 == 0 && d.hidden % tgx::oproj_sliced_rows<16>() == 0;
}

// The direct attention form with the o_proj product in its epilogue (attn_decode_kernel template OPJ, kernels/attn_decode.h): batch-1 steps at short
// contexts run {qkv, attention + o_proj, gate_up, down}.  Each query head's workgroups (oj_rsplit of them, each repeating the head's attention over the few
// hundred keys) multiply the normalised head output by their rows of W_o[:, head columns] and add into the fixed-point residual accumulators that gate_up
// and down already read (see above).  Measured per layer (tools/probes/layer_lab.hip, profiles/r04_attn_oproj_fused.txt): Qwen2.5-0.5B at context 30 / 270 /
// 600 20.2 / 21.0 / 21.8 -> 18.8 / 19.9 / 21.4 us, Llama-3.2-1B 33.3 / 34.2 / 35.5 -> 30.9 / 32.9 / 34.3; the split form is ahead from ~700 / ~900 keys.
bool oproj_fused_capable(const tgx_ctx* c) {
  const tgx_model_desc& d = c->d;
  if (!c->oproj_fused || c->gpt2 || c->dt == tgx::DT_F32 || !c->slab_acc) return false;
  return d.head_dim == 64 && !d.qk_norm && d.inter <= 16384 && d.hidden % 8 == 0 && d.hidden <= tgx::XACC_HIDDEN_MAX;
}
bool oproj_fused_ok(const tgx_ctx* c, int R, long long kv_stride) {
  return R == 1 && c->batch == 1 && kv_stride != 0 && c->attn_direct && oproj_fused_capable(c);
}
// the residual stream between o_proj and down lives in the fixed-point accumulators (either o_proj form above)
static bool resid_fixed(const tgx_ctx* c, int R, long long kv_stride) { return oproj_sliced_ok(c, R, kv_stride) || oproj_fused_ok(c, R, kv_stride); }

// One kernel class of one decoder layer for R rows (batch rows of the slabs, or the chunk rows of a prefill-by-steps pass).  `resid` is the residual stream of row0 that the
// o_proj/down epilogues update (slab_x in the real pass; a scratch vector when tgx_profile_decode replays a class).
int launch_layer_kernel(tgx_ctx* c, RowState* rv, int R, int l, int cls, float* resid, long long kv_stride) {
  const tgx_model_desc& d = c->d;
  RowState& r = rv[0];   // R consecutive row views with the slabs' row strides; kv_stride = 0 when the rows are positions of ONE sequence
  const int H = d.hidden, I = d.inter, hd = d.head_dim, qd = d.heads * hd, kvd = d.kv_heads * hd;
  // bytes between a layer's caches (ebyte pointers): a row's slab [kv_heads][max_ctx][hd], or — paged KV — the layer's pool of KV_BLOCK-token blocks
  const size_t kv_layer = (c->kv_paged ? (size_t)c->kv.n_blocks() * d.kv_heads * tgx::KV_BLOCK : (size_t)d.kv_heads * d.max_ctx) * hd * c->esz;
  // paged: the rows share the pools (no row stride) and differ by their block tables; rows that are positions of ONE sequence (kv_stride 0) share one table
  const long long kvs = c->kv_paged ? 0 : kv_stride, tbs = (c->kv_paged && kv_stride != 0) ? c->kv.tbl_stride() : 0;
  const LayerW& w = c->L[(size_t)l];
  switch (cls) {
    case TGX_KERNEL_QKV: {   // input_layernorm -> qkv_proj -> RoPE -> cache append   (DecoderLayer.h:40, Attention.h:94-106)
      tgx::GemvArgs a{};
      fill_strides(c, a);
      a.W = w.wqkv; a.bias = w.bqkv; a.x = r.x; a.x_stride = H; a.norm_w = w.in_norm; a.eps = d.norm_eps;
      a.N = qd + 2 * kvd; a.K = H; a.units = a.N / 2;
      a.q_out = r.q; a.k_cache = r.kcache + (size_t)l * kv_layer; a.v_cache = r.vcache + (size_t)l * kv_layer; a.kv_stride = kvs;
      a.blk_tbl = r.tbl; a.tbl_stride = tbs;
      a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin; a.pos = r.pos;
      a.heads = d.heads; a.kv_heads = d.kv_heads; a.hd = hd; a.max_ctx = d.max_ctx;
      a.raw_qk = d.qk_norm ? 1 : 0; a.k_raw = r.k_raw;
      if (c->gpt2) {   // ln_1 -> c_attn (+bias) -> split into heads -> cache append; no rotation: the tables hold cos = 1, sin = 0 (ModelGPT2.h:60-75)
        a.norm_b = w.in_norm_b;
        launch_gemv<tgx::PRO_LAYERNORM, tgx::EPI_QKV_ROPE>(c, a, TGX_KERNEL_QKV, R);
        break;
      }
      launch_gemv<tgx::PRO_RMSNORM, tgx::EPI_QKV_ROPE>(c, a, TGX_KERNEL_QKV, R);
      if (d.qk_norm && !qk_fused(c, kv_stride)) {   // q_norm / k_norm -> RoPE -> cache append (Attention.h:156-163); batch rows on blockIdx.y
        tgx::QkNormArgs n{};
        n.q = r.q; n.k_raw = r.k_raw; n.k_cache = r.kcache + (size_t)l * kv_layer; n.q_norm_w = w.q_norm; n.k_norm_w = w.k_norm;
        n.rope_cos = c->rope_cos; n.rope_sin = c->rope_sin; n.pos = r.pos;
        n.heads = d.heads; n.kv_heads = d.kv_heads; n.hd = hd; n.max_ctx = d.max_ctx; n.eps = d.norm_eps;
        n.q_stride = qd; n.kraw_stride = kvd; n.kv_stride = kvs; n.blk_tbl = r.tbl; n.tbl_stride = tbs;
        TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL(tgx::qk_norm_rope_kernel<DT>, dim3(d.heads + d.kv_heads, R), dim3(64), 0, c->stream, n))
      }
      break;
    }
    case TGX_KERNEL_ATTN: {  // flashAttention(q, Kall, Vall) over keys [0, pos[row]]; blockIdx.y = batch row (own cache, own length)
      tgx::AttnArgs a{};
      a.q = r.q; a.k_cache = r.kcache + (size_t)l * kv_layer; a.v_cache = r.vcache + (size_t)l * kv_layer;
      a.pos = r.pos; a.part = r.attn_part; a.out = r.attn;
      a.heads = d.heads; a.kv_heads = d.kv_heads; a.max_ctx = d.max_ctx; a.nsplit = c->attn_nsplit;
      a.scale = 1.0f / sqrtf((float)hd);
      a.q_stride = qd; a.kv_stride = kvs; a.part_stride = (long long)c->attn_part_row; a.dbg = c->debug_attn;
      a.blk_tbl = r.tbl; a.tbl_stride = tbs;
      a.act16 = c->act16 ? (c->dt == tgx::DT_BF16 ? 1 : (c->dt == tgx::DT_F16 ? 2 : 0)) : 0;
      if (qk_fused(c, kv_stride)) {
        a.k_raw = r.k_raw; a.kraw_stride = kvd; a.q_norm_w = w.q_norm; a.k_norm_w = w.k_norm;
        a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin; a.eps = d.norm_eps;
      }
      if (oproj_fused_ok(c, R, kv_stride)) {      // + o_proj and the residual add in the same launch (Attention.h:111-112, DecoderLayer.h:40)
        a.oj_w = w.wo; a.oj_x = r.x; a.oj_acc = c->slab_acc + (size_t)(&r - c->rows.data()) * H; a.oj_H = H; a.oj_ldw = qd;
      }
      launch_attn(c, a, R, /*combine=*/!oproj_sliced_ok(c, R, kv_stride));
      break;
    }
    case TGX_KERNEL_OPROJ: { // o_proj + residual                                     (Attention.h:90, DecoderLayer.h:40)
      if (oproj_fused_ok(c, R, kv_stride)) return 0;       // done by the attention launch
      tgx::GemvArgs a{};
      fill_strides(c, a);
      a.W = w.wo; a.bias = w.bo; a.x = r.attn; a.x_stride = qd; a.N = H; a.K = qd; a.units = (H + 1) / 2; a.out = resid; a.out_stride = H; a.hd = 2;
      if (oproj_sliced_ok(c, R, kv_stride)) {   // split-form attention, batch 1: K-sliced product, the split records merged in its prologue, partial sums into
        // the row's fixed-point accumulators (kernels/oproj_sliced.h); the residual x is added by K slice 0; gate_up reads the accumulators, down empties them
        tgx::OprojSlicedArgs o{};
        o.W = w.wo; o.ldw = qd; o.part = r.attn_part; o.nsplit = c->attn_nsplit; o.x = r.x; o.acc = c->slab_acc + (size_t)(&r - c->rows.data()) * H; o.H = H; o.act16 = c->act16;
        const dim3 blk(256);
        TGX_DT16_SWITCH(c->dt,
          if (qd % 256 == 0) hipLaunchKernelGGL((tgx::oproj_sliced_kernel<DT, 64, 32>), dim3(H / tgx::oproj_sliced_rows<32>(), qd / 256), blk, 0, c->stream, o);
          else hipLaunchKernelGGL((tgx::oproj_sliced_kernel<DT, 64, 16>), dim3(H / tgx::oproj_sliced_rows<16>(), qd / 128), blk, 0, c->stream, o);)
        break;
      }
      launch_gemv<tgx::PRO_PLAIN, tgx::EPI_RESIDUAL>(c, a, TGX_KERNEL_OPROJ, R);
      break;
    }
    case TGX_KERNEL_GATEUP: { // post_attention_layernorm -> gate_up_proj -> siluMul  (DecoderLayer.h:41, GatedMLP.h:37-39)
      tgx::GemvArgs a{};
      fill_strides(c, a);
      a.W = w.wgu; a.x = r.x; a.x_stride = H; a.norm_w = w.post_norm; a.eps = d.norm_eps;
      if (c->gpt2) {   // ln_2 -> c_fc (+bias) -> gelu_new   (ModelGPT2.h:96-107,131-134)
        a.norm_b = w.post_norm_b; a.bias = w.bfc;
        a.N = I; a.K = H; a.units = (I + 1) / 2; a.out = r.h; a.out_stride = I; a.hd = 2;
        launch_gemv<tgx::PRO_LAYERNORM, tgx::EPI_GELU>(c, a, TGX_KERNEL_GATEUP, R);
        break;
      }
      a.N = 2 * I; a.K = H; a.units = I; a.out = r.h; a.out_stride = I; a.hd = 2;
      if (resid_fixed(c, R, kv_stride)) a.x_acc = c->slab_acc + (size_t)(&r - c->rows.data()) * H;     // x' = fp32(acc)
      launch_gemv<tgx::PRO_RMSNORM, tgx::EPI_SILU_MUL>(c, a, TGX_KERNEL_GATEUP, R, &w.pgu, &w.qgu);
      break;
    }
    case TGX_KERNEL_DOWN: {  // down_proj + residual                                  (GatedMLP.h:40, DecoderLayer.h:41)
      tgx::GemvArgs a{};
      fill_strides(c, a);
      a.W = w.wdown; a.bias = w.bdown; a.x = r.h; a.x_stride = I; a.N = H; a.K = I; a.units = (H + 1) / 2; a.out = resid; a.out_stride = H; a.hd = 2;
      if (I > 16384) {   // 32B/70B-class intermediate sizes: one launch keeps at most 16384 elements of x in registers — the K range is
        // covered by 2-4 launches that accumulate into the residual stream in order (x += W[:, k0:k1] . h[k0:k1])
        const int parts = (I + 16383) / 16384, per = ((I / 8 + parts - 1) / parts) * 8;
        for (int k0 = 0; k0 < I; k0 += per) {
          tgx::GemvArgs p = a;
          p.W = w.wdown + (size_t)k0 * c->esz; p.x = r.h + k0; p.K = std::min(per, I - k0); p.ldw = I;
          if (k0) p.bias = nullptr;
          launch_gemv<tgx::PRO_PLAIN, tgx::EPI_RESIDUAL>(c, p, TGX_KERNEL_DOWN, R);
        }
        break;
      }
      if (resid_fixed(c, R, kv_stride)) a.res_acc = c->slab_acc + (size_t)(&r - c->rows.data()) * H;   // x = fp32(acc) + down(h); acc <- 0
      launch_gemv<tgx::PRO_PLAIN, tgx::EPI_RESIDUAL>(c, a, TGX_KERNEL_DOWN, R, &w.pdown, &w.qdown);
      break;
    }
    default: return 0;
  }
  return 1;
}

// All decoder layers for R rows: their current tokens' embeddings sit in the x slab, positions in the pos slab.
// == for (auto& layer : layers_) x = layer->forward(x)  (GPTModel.h:53-55)
void launch_layers(tgx_ctx* c, RowState* rv, int R, long long kv_stride) {
  for (int l = 0; l < c->d.layers; l++)
    for (int cls = TGX_KERNEL_QKV; cls <= TGX_KERNEL_DOWN; cls++) launch_layer_kernel(c, rv, R, l, cls, rv[0].x, kv_stride);
}
void launch_layers(tgx_ctx* c, int row0, int R) { launch_layers(c, &c->rows[(size_t)row0], R, (long long)c->kv_row_elems); }

// model.norm -> lm_head on the current position + per-workgroup argmax partials   (GPTModel.h:56-57)
void launch_lm_head(tgx_ctx* c, int row0, int R) {
  RowState& r = c->rows[(size_t)row0];
  launch_lm_head_at(c, r.x, r.logits, r.part_val, r.part_idx, R);
}

void launch_lm_head_at(tgx_ctx* c, const float* x, float* logits, float* part_val, int* part_idx, int R) {
  const tgx_model_desc& d = c->d;
  tgx::GemvArgs a{};
  fill_strides(c, a);
  a.W = d.tied ? c->embed : c->lm_head; a.x = x; a.x_stride = d.hidden; a.norm_w = c->final_norm; a.eps = d.norm_eps;
  a.N = d.vocab; a.K = d.hidden; a.units = (d.vocab + 1) / 2; a.hd = 2;
  a.logits = logits; a.part_val = part_val; a.part_idx = part_idx;
  if (c->gpt2) {   // ln_f -> wte^T (tied head, ModelGPT2.h:170-176)
    a.norm_b = c->final_norm_b;
    launch_gemv<tgx::PRO_LAYERNORM, tgx::EPI_LOGITS>(c, a, TGX_KERNEL_LMHEAD, R);
    return;
  }
  launch_gemv<tgx::PRO_RMSNORM, tgx::EPI_LOGITS>(c, a, TGX_KERNEL_LMHEAD, R, &c->plm, &c->qlm);
}

tgx::FinalizeArgs make_finalize_args(tgx_ctx* c, int row, bool advance_pos, bool log_step) {
  RowState& r = c->rows[(size_t)row];
  tgx::FinalizeArgs a{};
  a.part_val = r.part_val; a.part_idx = r.part_idx; a.n_part = c->lm_grid;
  a.tok = r.tok; a.pos = r.pos; a.step = c->step; a.tok_log = c->tok_log; a.host_ring = c->mirror_to_host ? c->host_ring_dev : nullptr;
  a.log_cap = c->log_cap; a.ring_cap = HOST_RING;
  a.row = row; a.rows = c->batch;
  a.log = log_step ? 1 : 0; a.bump_step = (row == c->batch - 1) ? 1 : 0;
  if (log_step && c->batch > 1) { a.done = c->step_done; a.done_total = c->batch; a.bump_step = 0; }      // rows of a batch may be finalized concurrently: the last to count itself moves the step
  a.embed = c->embed; a.x = r.x; a.H = c->d.hidden; a.V = c->d.vocab; a.advance_pos = advance_pos ? 1 : 0;
  a.wpe = c->gpt2 ? c->wpe : nullptr; a.n_pos = c->d.n_positions > 0 ? c->d.n_positions : 1;
  return a;
}

// == argmax (Sampler.cpp:26-29) + token publish / pastLength / next embedding: one finalize launch per row
void launch_finalize_greedy(tgx_ctx* c, int row0, int R, bool advance_pos, bool log_step) {
  for (int b = row0; b < row0 + R; b++) {
    const tgx::FinalizeArgs a = make_finalize_args(c, b, advance_pos, log_step);
    TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL(tgx::finalize_greedy_kernel<DT>, dim3(1), dim3(256), 0, c->stream, a))
  }
}

// the batched step: rows are finalized concurrently; the row that completes the batch's count moves the step counter (FinalizeArgs.done)
void launch_finalize_rows(tgx_ctx* c, int row0, int M) {
  tgx::FinalizeRowsArgs fa{};
  fa.f = make_finalize_args(c, row0, /*advance_pos=*/true, /*log_step=*/true);
  fa.part_stride = c->lm_grid; fa.x_stride = c->d.hidden;
  TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL(tgx::finalize_rows_kernel<DT>, dim3(M), dim3(256), 0, c->stream, fa))
}

// prefill by steps: chunk row r <- embedding of prompt token r at position pos0 + r
void launch_embed_chunk(tgx_ctx* c, const long long* ids, int R, int pos0) {
  tgx::EmbedChunkArgs e{};
  e.ids = ids; e.embed = c->embed; e.x = c->ch_x; e.H = c->d.hidden; e.pos = c->ch_pos; e.pos0 = pos0; e.wpe = c->gpt2 ? c->wpe : nullptr;
  TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL(tgx::embed_chunk_kernel<DT>, dim3(R), dim3(256), 0, c->stream, e))
}
void launch_add_pos(tgx_ctx* c, int* pos, int n) { hipLaunchKernelGGL(tgx::add_pos_kernel, dim3(1), dim3(64), 0, c->stream, pos, n); }
void launch_argmax_partials(tgx_ctx* c, const float* logits, int V, float* part_val, int* part_idx) {
  hipLaunchKernelGGL(tgx::argmax_partials_kernel, dim3(c->lm_grid), dim3(256), 0, c->stream, logits, V, part_val, part_idx);
}

// ---- tgx_verify_row (kernels/verify.h).  The pass's first input is the row's device-resident current token ...
void launch_verify_first_id(tgx_ctx* c, int row) {
  hipLaunchKernelGGL(tgx::verify_first_id_kernel, dim3(1), dim3(64), 0, c->stream, c->rows[(size_t)row].prompt, (const int*)c->rows[(size_t)row].tok);
}
// ... and behind the pass and the M positions' lm_head, ONE launch accepts the draft's matching prefix and leaves the row as that many decode steps would
// (draws: the positions' sampled ids, launch_sample_positions; nullptr: greedy)
// what g[i] is chosen from, and the commit: the raw pair again and nothing; a processed row (option verify.processors): the processed slab's per-tile partials
// from workspace row `first`, the row's history words and — with an automaton on — its slice of the positions' states
static void verify_select(tgx_ctx* c, tgx::VerifyArgs& a, int row, bool processed, bool joint, size_t first) {
  a.sel_part_val = a.part_val; a.sel_part_idx = a.part_idx; a.sel_part_stride = a.part_stride; a.sel_n_part = a.n_part;
  if (!processed) return;
  const size_t T = (size_t)((c->d.vocab + 1023) / 1024);
  a.sel_part_val = (joint ? c->vpj_part_val : c->vp_part_val) + first * T; a.sel_part_idx = (joint ? c->vpj_part_idx : c->vp_part_idx) + first * T;
  a.sel_part_stride = (long long)T; a.sel_n_part = (int)T;
  a.hist = c->proc_hist + (size_t)row * c->d.vocab;
  a.states = (c->row_req_host[(size_t)row].proc & tgx::PROC_AUTOMATON) ? (joint ? c->vpj_states : c->vp_states) + first : nullptr;
}
void launch_verify_accept(tgx_ctx* c, int row, int M, const int* draws, bool processed) {
  if (processed && (!c->vp_states || !c->proc_hist)) { c->launch_fault = "processed verification requested before its buffers exist"; return; }
  RowState& r = c->rows[(size_t)row];
  tgx::VerifyArgs a{};
  a.part_val = c->vf_part_val; a.part_idx = c->vf_part_idx; a.part_stride = c->lm_grid; a.n_part = c->lm_grid; a.M = M;
  verify_select(c, a, row, processed, /*joint=*/false, 0);
  a.logits = c->vf_logits; a.draft = r.prompt + 1; a.draws = draws;
  a.tok = r.tok; a.pos = r.pos; a.req = c->row_req + row;
  a.row_logits = r.logits; a.row_part_val = r.part_val; a.row_part_idx = r.part_idx; a.x = r.x;
  a.embed = c->embed; a.wpe = c->gpt2 ? c->wpe : nullptr; a.H = c->d.hidden; a.V = c->d.vocab; a.n_pos = c->d.n_positions > 0 ? c->d.n_positions : 1;
  a.rec = reinterpret_cast<tgx::VerifyRecord*>(c->vf_rec);
  TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL(tgx::verify_accept_kernel<DT>, dim3(1), dim3(256), 0, c->stream, a))
}
// ---- tgx_verify_tree: the walk over the token tree whose tables vt_tab holds (parent positions in, the accepted path out) ...
void launch_verify_accept_tree(tgx_ctx* c, int row, int M, const int* draws) {
  if (!c->vt_tab || !c->vf_rec || M > tgx::VERIFY_MAX_POS) { c->launch_fault = "tree verification requested before its buffers exist"; return; }
  RowState& r = c->rows[(size_t)row];
  tgx::VerifyTreeArgs t{};
  tgx::VerifyArgs& a = t.v;
  a.part_val = c->vf_part_val; a.part_idx = c->vf_part_idx; a.part_stride = c->lm_grid; a.n_part = c->lm_grid; a.M = M;
  verify_select(c, a, row, /*processed=*/false, /*joint=*/false, 0);
  a.logits = c->vf_logits; a.draft = r.prompt + 1; a.draws = draws;
  a.tok = r.tok; a.pos = r.pos; a.req = c->row_req + row;
  a.row_logits = r.logits; a.row_part_val = r.part_val; a.row_part_idx = r.part_idx; a.x = r.x;
  a.embed = c->embed; a.wpe = nullptr; a.H = c->d.hidden; a.V = c->d.vocab; a.n_pos = c->d.n_positions > 0 ? c->d.n_positions : 1;
  a.rec = reinterpret_cast<tgx::VerifyRecord*>(c->vf_rec);
  t.par = c->vt_tab + tgx_ctx::VT_PAR; t.path = c->vt_tab + tgx_ctx::VT_PATH;
  TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::verify_accept_tree_kernel<DT>, dim3(1), dim3(256), 0, c->stream, t))
}
// ... and behind it the accepted branch's K / V rows into place (kernels/kv_tree.h): one workgroup per (layer, kv head, K | V)
void launch_kv_tree_compact(tgx_ctx* c, int row, int M, int past) {
  const tgx_model_desc& d = c->d;
  if (!c->vt_tab || !c->vf_rec || M > tgx::VERIFY_MAX_POS || d.head_dim % 8 != 0 || (tgx::VERIFY_MAX_POS - 1) * (d.head_dim / 8) > 256 || past + M > d.max_ctx) {
    c->launch_fault = "kv_tree_compact: the pass does not fit the launch (at most 16 positions, head_dim <= 128)"; return;
  }
  RowState& r = c->rows[(size_t)row];
  tgx::KvTreeArgs a{};
  a.k = reinterpret_cast<bf16_t*>(r.kcache); a.v = reinterpret_cast<bf16_t*>(r.vcache);
  a.layer_stride = (long long)(c->kv_paged ? (size_t)c->kv.n_blocks() * d.kv_heads * tgx::KV_BLOCK : (size_t)d.kv_heads * d.max_ctx) * d.head_dim;
  a.tbl = c->kv_paged ? r.tbl : nullptr;
  a.path = c->vt_tab + tgx_ctx::VT_PATH; a.rec = reinterpret_cast<const tgx::VerifyRecord*>(c->vf_rec);
  a.kv_heads = d.kv_heads; a.hd = d.head_dim; a.max_ctx = d.max_ctx; a.past = past; a.M = M;
  hipLaunchKernelGGL(tgx::kv_tree_compact_kernel, dim3(d.layers * d.kv_heads, 2), dim3(256), 0, c->stream, a);
}
// ---- tgx_verify_rows: both launches for the n rows of a joint pass (ids: the pass's ids on the device, row i's M_i = n_draft[i] + 1 inputs from first[i])
void launch_verify_first_ids(tgx_ctx* c, long long* ids, int n, const int* rows, const int* first) {
  tgx::VerifyFirstIds f{};
  for (int i = 0; i < n; i++) { f.tok[i] = c->rows[(size_t)rows[i]].tok; f.first[i] = first[i]; }
  hipLaunchKernelGGL(tgx::verify_first_ids_kernel, dim3(1), dim3(tgx::VERIFY_MAX_ROWS), 0, c->stream, ids, f, n);
}
void launch_verify_accept_rows(tgx_ctx* c, const long long* ids, int n, const int* rows, const int* first, const int* n_draft, const char* sampled, const char* processed) {
  static_assert(sizeof(tgx::VerifyArgs) % 8 == 0, "the table's entries hold pointers");
  if (!c->vj_args || !c->vj_rec || n > tgx::VERIFY_MAX_ROWS) { c->launch_fault = "joint verification requested before its buffers exist"; return; }
  const size_t V = (size_t)c->d.vocab, P = (size_t)c->lm_grid;
  c->vj_args_host.resize((size_t)n * sizeof(tgx::VerifyArgs));      // (the context's: it outlives the upload)
  tgx::VerifyArgs* tab = reinterpret_cast<tgx::VerifyArgs*>(c->vj_args_host.data());
  for (int i = 0; i < n; i++) {
    RowState& r = c->rows[(size_t)rows[i]];
    const size_t f = (size_t)first[i];
    tgx::VerifyArgs a{};
    a.part_val = c->vj_part_val + f * P; a.part_idx = c->vj_part_idx + f * P; a.part_stride = c->lm_grid; a.n_part = c->lm_grid; a.M = n_draft[i] + 1;
    const bool proc = processed && processed[i];
    if (proc && (!c->vpj_states || !c->proc_hist)) { c->launch_fault = "processed verification requested before its buffers exist"; return; }
    verify_select(c, a, rows[i], proc, /*joint=*/true, f);
    a.logits = c->vj_logits + f * V; a.draft = ids + f + 1; a.draws = sampled[i] ? c->vj_draws + f : nullptr;
    a.tok = r.tok; a.pos = r.pos; a.req = c->row_req + rows[i];
    a.row_logits = r.logits; a.row_part_val = r.part_val; a.row_part_idx = r.part_idx; a.x = r.x;
    a.embed = c->embed; a.wpe = c->gpt2 ? c->wpe : nullptr; a.H = c->d.hidden; a.V = c->d.vocab; a.n_pos = c->d.n_positions > 0 ? c->d.n_positions : 1;
    a.rec = reinterpret_cast<tgx::VerifyRecord*>(c->vj_rec) + i;
    tab[i] = a;
  }
  if (hipMemcpyAsync(c->vj_args, tab, (size_t)n * sizeof(tgx::VerifyArgs), hipMemcpyHostToDevice, c->stream) != hipSuccess) { c->launch_fault = "joint verification: the argument table's upload failed"; return; }
  TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL(tgx::verify_accept_rows_kernel<DT>, dim3(n), dim3(256), 0, c->stream, reinterpret_cast<const tgx::VerifyArgs*>(c->vj_args)))
}
// the size of one entry of the accept launch's table, for the workspace (abi.hip ensure_verify_rows_ws)
size_t verify_args_bytes() { return sizeof(tgx::VerifyArgs); }
