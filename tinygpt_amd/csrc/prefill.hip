// prefill.hip — the batched prefill of the MI355X shim for 16-bit storage (kernels/prefill.h, gemm_dma.h): every product of S prompt positions on the
// matrix cores, causal flash attention, RoPE + cache append.  == CausalLM::forward on [B,S] ids with an empty cache (GPTModel.h:51-56)
#include "ctx.h"
#include <type_traits>
#include "kernels/prefill.h"
#include "kernels/gemm_dma.h"
#include "kernels/gemm_dma_qkv.h"
#include "kernels/attn_prefill_dma.h"
#include "kernels/attn_extend.h"
#include "kernels/attn_mixed.h"
#include "attn_worklist.h"
#include "kernels/gemm_f32.h"
#include "kernels/score.h"
#include "kernels/embed_pool.h"

bool prefill_shapes_ok(const tgx_model_desc& d) {
  return d.hidden % 64 == 0 && (d.heads * d.head_dim) % 64 == 0 && d.inter % 64 == 0;
}

int ensure_prefill_ws(tgx_ctx* c, int S) {
  if (S <= c->ws_rows && (!c->act16 || c->ws_zero || c->dt == tgx::DT_F32)) return TGX_OK;
  S = std::max(S, c->ws_rows);
  const tgx_model_desc& d = c->d;
  const size_t H = (size_t)d.hidden, qd = (size_t)d.heads * d.head_dim, kvd = (size_t)d.kv_heads * d.head_dim, I = (size_t)d.inter;
  const size_t wout = qd + 2 * kvd, wa = std::max(H, qd);   // the gate_up product leaves no fp32 intermediate (GEMM_SILU)
  drop_step_graphs(c);                                       // a captured batched decode step holds pointers into the old workspace
  HIP_OK(c, hipStreamSynchronize(c->stream));
  // fp32 storage: ws_ah / ws_qh / ws_hh hold fp32 rows (the fp32 GEMM's A operands, the rotated queries); the lo terms are unused
  const size_t rows = (size_t)S, te = c->dt == tgx::DT_F32 ? 4 : 2, lo = c->dt == tgx::DT_F32 ? 0 : 1;
  const size_t zero_bytes = c->act16 && lo ? (rows * std::max(wa, I) + 8) * 2 : 0;      // option act.round16: the all-zero "lo term" of every stored-term product (any A operand fits: rows x max(H, qd, I))
  const struct { void* p; size_t bytes; } ws[] = {      // p: the context's pointer field.  0 bytes: released, not allocated (ws_pos: the fp32 prefill alone)
    {&c->ws_x, rows * H * 4}, {&c->ws_out, rows * wout * 4}, {&c->ws_ah, rows * wa * te}, {&c->ws_al, rows * wa * 2 * lo + 16}, {&c->ws_al2, rows * H * 2 * lo + 16},
    {&c->ws_qh, rows * qd * te}, {&c->ws_ql, rows * qd * 2 * lo + 16}, {&c->ws_hh, rows * I * te}, {&c->ws_hl, rows * I * 2 * lo + 16},
    {&c->ws_zero, zero_bytes}, {&c->ws_pos, c->dt == tgx::DT_F32 ? rows * 4 : 0}};
  for (const auto& w : ws) dev_free(c, (ebyte**)w.p);
  c->ws_rows = 0;      // (a failure below leaves it so: the next call starts over)
  for (const auto& w : ws) if (int rc = w.bytes ? dev_alloc(c, (ebyte**)w.p, w.bytes) : TGX_OK) return rc;
  if (c->ws_zero) HIP_OK(c, hipMemset(c->ws_zero, 0, zero_bytes));
  c->ws_rows = S;
  return TGX_OK;
}

int ensure_ws_part(tgx_ctx* c, size_t need) {
  if (need > c->ws_part_bytes) drop_step_graphs(c);
  return dev_grow(c, &c->ws_part, &c->ws_part_bytes, need);
}

// defer (optional, RESIDUAL / STORE products): when the product is split over K, leave the slabs in ws_part for the consumer kernel to sum
// (rmsnorm_split_kernel / rope_kv_split_kernel: same z order, one launch and one pass over the rows less) and report the slab count; 1 = done here.
// -1 (round 5): the UNSPLIT eight-wave N = hidden product stored its result as ONE slab instead of adding it to the residual
// stream in its epilogue — a read-modify-write of M x N floats by four waves per CU at the end of a launch that has one tile per CU (nothing left to overlap
// it: 18-19 of o_proj's 52 us, tools/probes/gemm_lab.hip); the row-wise norm kernel that reads the stream next adds the slab while it streams.
// The gate_up product on full 128-byte lines (kernels/gemm_dma.h gemm_dma8i_kernel): taken where the 256 x 256 kernel would be, on the
// default contract; the producing norm launch then writes the two terms interleaved per k32 block (rmsnorm_split_kernel `inter`) into ws_out, which is idle
// between the RoPE / cache-append launch and the next layer's QKV product.
// split-K slabs wait for their row-wise consumer from this many rows on (192 until the row-wise norm launch loaded its slabs eight at a time: Llama-3.2-1B
// S = 160 2.51 -> 2.41 ms, 191 2.54 -> 2.46; Mistral-7B S = 160 9.90 -> 9.65)
constexpr int DEFER_MIN_ROWS = 129;
// the eight-wave 128 x 128 gate_up kernel while its tiles number at most this many half-chips (8 = 4 tiles per CU: everything below the 256 x 256 kernel's range;
// 3 / 8: Llama-3.2-1B S = 512 3.62 / 3.44 ms, 768 5.06 / 4.94; Mistral-7B S = 256 11.16 / 10.81, 512 22.5 / 21.4)
constexpr int WIDE_8K_MAX = 8;
static bool gemm_full_lines(const tgx_ctx* c, int epi, int M, int N, int K) {
  if (epi != tgx::GEMM_SILU || c->gpt2 || (c->act16 && c->ws_zero) || K % 64 != 0 || N % 256 != 0) return false;
  const tgx_model_desc& d = c->d;
  if ((size_t)d.heads * d.head_dim + 2 * (size_t)d.kv_heads * d.head_dim < (size_t)K) return false;      // ws_out holds [M][2 K] 16-bit terms
  const int t256 = ((N + 255) / 256) * ((M + 255) / 256), r256 = (t256 + c->num_cus - 1) / c->num_cus;
  const bool ragged256 = c->wide_8k_eff > 0 && t256 >= c->num_cus && 100 * t256 < c->wide_8k_eff * r256 * c->num_cus;
  return t256 >= c->num_cus && !ragged256;
}

static void launch_gemm(tgx_ctx* c, int epi, const ebyte* B_, const ebyte* bias_, float* C, int M, int N, int K, int ldc, bool three_terms = false,
                 const bf16_t* a_hi = nullptr, const bf16_t* a_lo = nullptr, int three_from = 0, int* defer = nullptr, bool a_inter = false) {
  if (defer) *defer = 1;
  // every kernel below steps K by 64 (tgx::GBK); prefill_shapes_ok admits only models whose hidden, heads * head_dim and inter — the K of every caller — are such
  if (K % 64 != 0) { c->launch_fault = "internal: launch_gemm with K not a multiple of 64"; return; }
  if (a_inter) {       // A arrives interleaved in a_hi (the caller asked gemm_full_lines first)
    tgx::GemmArgs g{};
    g.A_hi = a_hi; g.A_lo = nullptr; g.A_lo2 = nullptr; g.inter = N / 2; g.out_hi = c->ws_hh; g.out_lo = c->ws_hl;
    g.B = reinterpret_cast<const bf16_t*>(B_); g.bias = nullptr; g.C = C; g.M = M; g.N = N; g.K = K; g.ldc = ldc; g.three_from = 1 << 30;
    const dim3 g8((N + 255) / 256, (M + 255) / 256), b8(512);
    TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL((tgx::gemm_dma8i_kernel<DT, tgx::GEMM_SILU>), g8, b8, (size_t)5 * 256 * 128, c->stream, g))
    return;
  }
  const bool one = c->act16 && c->ws_zero;       // option act.round16: A_hi is the (rounded) activation; every other term reads zeros, the eight-wave kernels skip it
  if (one) { three_terms = false; three_from = 0; }
  const bool one_k = one && c->act16_kernels;    // ... in kernels that have a one-term form
  const bf16_t* B = reinterpret_cast<const bf16_t*>(B_);   // 16-bit storage (bf16 or fp16 bit patterns); fp32 storage never gets here
  const bf16_t* bias = reinterpret_cast<const bf16_t*>(bias_);
  tgx::GemmArgs g{};
  g.A_hi = a_hi ? a_hi : c->ws_ah; g.A_lo = one ? c->ws_zero : (a_lo ? a_lo : c->ws_al); g.A_lo2 = three_terms ? c->ws_al2 : nullptr;
  g.inter = N / 2; g.out_hi = c->ws_hh; g.out_lo = c->ws_hl;
  g.B = B; g.bias = bias; g.C = C; g.M = M; g.N = N; g.K = K; g.ldc = ldc; g.three_from = three_from;
  // few column tiles (N = hidden) -> 64-row tiles, so that at least two workgroups share a CU
  const bool few = ((N + tgx::GBN - 1) / tgx::GBN) * ((M + tgx::GBM - 1) / tgx::GBM) < 2 * c->num_cus;
  // measured (tools/prefill_bench.py --gemm-tm, Llama-3.2-1B, S = 2048): this policy 15.0 ms, 64-row tiles also for the three-term
  // QKV product 15.3, 128-row tiles everywhere 15.85, 64-row tiles everywhere 15.9
  const bool small = (epi == tgx::GEMM_SILU || epi == tgx::GEMM_GELU) ? false : (c->gemm_tm ? c->gemm_tm == 64 : (few && !three_terms));
  const int tm = small ? 64 : tgx::GBM;
  const dim3 grid((N + tgx::GBN - 1) / tgx::GBN, (M + tm - 1) / tm), blk(256);
  const size_t dyn = three_terms ? (size_t)tm * tgx::GLD * 2 : 0;      // LDS tile of the third term
  // few row tiles (a short prompt): the tiles alone cannot stream the weights at rate (S <= 96 cost a flat 4.7 ms on Llama-3.2-1B) —
  // split K over blockIdx.z until ~2 workgroups per CU exist; the slabs are summed in z order by a second launch (deterministic)
  const int ntiles = (int)(grid.x * grid.y), ktiles = K / tgx::GBK;
  int nsplit = 1;
  // (the balanced QKV launch below fills the chip by itself from 1024 rows on at hidden 2048: 128 + 128 workgroups of equal work; Llama-3.2-1B S = 1024 5.16 -> 5.06 ms — no slabs then; option prefill.qkv_nosplit)
  const bool qkv_bal = three_terms && epi == tgx::GEMM_STORE && three_from > 0 && three_from % tgx::GBN == 0 && N > three_from && M >= 128;
  const int qkv_wgs = qkv_bal ? (three_from / tgx::GBN) * ((M + 127) / 128) + ((N - three_from + tgx::GBN - 1) / tgx::GBN) * ((M + 63) / 64) : 0;
  const bool qkv_nosplit = qkv_bal && c->qkv_nosplit && qkv_wgs >= c->num_cus;
  if (c->gemm_splitk && ntiles < c->num_cus && !qkv_nosplit) nsplit = std::min(std::min(16, ktiles), (2 * c->num_cus + ntiles - 1) / ntiles);
  // N = hidden products of a 129-1500-row prompt (round 4, option prefill.splitk_8k): their 128 x 128 tiles number less than a chip (Llama-3.2-1B S = 1024: 128 tiles on 256
  // CUs, 84 us per product against 104 at twice the rows) — the eight-wave LDS-DMA kernel over 2-4 K slabs instead of 64-row register-staged slabs or a half-empty chip
  bool part_8k = false;
  if (c->gemm_splitk && c->splitk_8k && !three_terms && (epi == tgx::GEMM_RESIDUAL || epi == tgx::GEMM_STORE) && M > 128) {
    const int t128 = ((N + 127) / 128) * ((M + 127) / 128);
    // slabs z = 2..4 that shorten the critical path: rounds of workgroups x 1 / z of the K loop against one round of whole tiles (160 tiles on 256 CUs: z = 3 -> 2 rounds of a
    // third = 0.67; 128 tiles: z = 2 -> 0.5); taken from 0.8 down (the slabs cost a pass over z x M x N floats)
    int z = 1; double best = 0.8001;
    for (int zz = 2; zz <= 4; zz++) {
      const double cost = (double)((zz * t128 + c->num_cus - 1) / c->num_cus) / zz;
      if (t128 < c->num_cus && cost < best - 1e-9 && K / 64 >= 4 * zz) { best = cost; z = zz; }
    }
    if (z >= 2) { part_8k = true; nsplit = z; }
  }
  // K >> N (`down`) on 128 x 256 tiles x 2 K slabs: a third fewer operand lines per output than the 128 x 128 kernel, which waits for them (kernels/gemm_dma.h
  // gemm_dma8n_kernel).  Needs a consumer that sums pending slabs (`defer`) and two rounds of workgroups (prefill.wide_n_min, in chips): at one
  // round (Llama-3.2-1B S = 2048: 256 workgroups) it ties with the one-slab 128 x 128 launch (141 vs 140-146 us) and costs a second slab; Mistral-7B S = 2048 56.1 -> 54.1 ms
  if (nsplit == 1 && defer && c->defer_reduce && epi == tgx::GEMM_RESIDUAL && !three_terms && !one && K >= 2 * N && K % 128 == 0 && N % 256 == 0 &&
      2 * (N / 256) * ((M + 127) / 128) >= c->wide_n_min * c->num_cus) {
    if (!ensure_ws_part(c, (size_t)2 * M * N * 4)) {      // (no slabs: the paths below)
      g.part = c->ws_part; g.nsplit = 2; g.interleave = 0; g.k_per = K / 2;
      const dim3 g8(N / 256, (M + 127) / 128, 2), b8(512);
      TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL((tgx::gemm_dma8n_kernel<DT>), g8, b8, (size_t)2 * (2 * 128 + 256) * 64 * 2, c->stream, g))
      *defer = 2;
      return;
    }
  }
  // one tile per CU on the eight-wave 128 x 128 kernel, a consumer that can take a pending slab: store the product, let the consumer add it (see `defer` above)
  const int t128u = ((N + 127) / 128) * ((M + 127) / 128);
  const bool store_slab = nsplit == 1 && defer && c->defer_reduce && epi == tgx::GEMM_RESIDUAL && !three_terms &&
                          2 * t128u >= c->num_cus && 2 * t128u <= 3 * c->num_cus &&
                          ((N + 255) / 256) * ((M + 255) / 256) < c->num_cus;
  if ((nsplit > 1 || store_slab) && ensure_ws_part(c, (size_t)nsplit * M * N * 4)) nsplit = 1;
  if (store_slab && c->ws_part_bytes >= (size_t)M * N * 4) {
    g.part = c->ws_part; g.nsplit = 1; g.interleave = 0; g.k_per = K;
    const dim3 g8((N + 127) / 128, (M + 127) / 128, 1), b8(512);
    const size_t lds8 = (size_t)3 * 3 * 128 * 64 * 2;
    TGX_DT16_SWITCH(c->dt, if (one_k) hipLaunchKernelGGL((tgx::gemm_dma8k_kernel<DT, tgx::GEMM_PARTIAL, false>), g8, b8, lds8, c->stream, g); else hipLaunchKernelGGL((tgx::gemm_dma8k_kernel<DT, tgx::GEMM_PARTIAL>), g8, b8, lds8, c->stream, g);)
    *defer = -1;
    return;
  }
  if (nsplit > 1) {
    g.part = c->ws_part; g.nsplit = nsplit; g.interleave = epi == tgx::GEMM_SILU ? 1 : 0;
    g.k_per = part_8k ? ((K / 64 + nsplit - 1) / nsplit) * 64 : ((ktiles + nsplit - 1) / nsplit) * tgx::GBK;
    const dim3 gz(grid.x, grid.y, nsplit);
    const size_t nout = (size_t)M * (epi == tgx::GEMM_SILU ? N / 2 : N);
    const dim3 rg((unsigned)((nout + 255) / 256));
    // the slabs' GEMM: operand tiles by LDS-DMA (round 3) — the register-staged kernel streamed a short prompt's weights at
    // 1-2 TB/s (S = 48: gate_up 32 us for 67 MB); 64-row tiles whenever the prompt fits them, k = 64 per stage (32 for the 128-row three-term tile)
    // measured (Llama-3.2-1B, ms per prompt, DMA vs register-staged slabs): S = 40 1.61 / 1.79, 48 1.65 / 1.76, 64 1.71 / 1.87; 96 2.08 / 1.99, 128 2.12 / 2.09,
    // 256 2.65 / 2.68; Mistral-7B S = 48 5.40 / 6.23 — the 64-row tile wins, the 128-row one does not: prompts of <= 64 rows only (value 2 = always)
    if (part_8k) {
      const dim3 g8((N + 127) / 128, (M + 127) / 128, nsplit), b8(512);
      const size_t lds8 = (size_t)3 * 3 * 128 * 64 * 2;
      TGX_DT16_SWITCH(c->dt, if (one_k) hipLaunchKernelGGL((tgx::gemm_dma8k_kernel<DT, tgx::GEMM_PARTIAL, false>), g8, b8, lds8, c->stream, g); else hipLaunchKernelGGL((tgx::gemm_dma8k_kernel<DT, tgx::GEMM_PARTIAL>), g8, b8, lds8, c->stream, g);)
    }
    const bool dma_part = !part_8k && M <= 64 && g.k_per % 64 == 0;
    if (dma_part) {
      const int mi = (small || M <= 64) ? 1 : 2;
      const int dbk = (mi == 2 && three_terms) ? 32 : 64;
      const dim3 gd((N + tgx::GBN - 1) / tgx::GBN, (M + 64 * mi - 1) / (64 * mi), nsplit);
      const size_t lds = tgx::gemm_dma_lds_bytes(mi, three_terms, dbk, 2);
      TGX_DT16_SWITCH(c->dt,
        if (mi == 1) hipLaunchKernelGGL((tgx::gemm_dma_kernel<DT, tgx::GEMM_PARTIAL, 1, 64, 2>), gd, blk, lds, c->stream, g);
        else if (dbk == 64) hipLaunchKernelGGL((tgx::gemm_dma_kernel<DT, tgx::GEMM_PARTIAL, 2, 64, 2>), gd, blk, lds, c->stream, g);
        else hipLaunchKernelGGL((tgx::gemm_dma_kernel<DT, tgx::GEMM_PARTIAL, 2, 32, 2>), gd, blk, lds, c->stream, g);)
    }
    TGX_DT16_SWITCH(c->dt,
      if (dma_part || part_8k) {}
      else if (small) hipLaunchKernelGGL((tgx::gemm_x2_kernel<DT, tgx::GEMM_PARTIAL, 1>), gz, blk, dyn, c->stream, g);
      else hipLaunchKernelGGL((tgx::gemm_x2_kernel<DT, tgx::GEMM_PARTIAL, 2>), gz, blk, dyn, c->stream, g);
      if (defer && c->defer_reduce && M >= DEFER_MIN_ROWS && (epi == tgx::GEMM_RESIDUAL || epi == tgx::GEMM_STORE)) { *defer = nsplit; }   // with few rows the row-wise consumers are too few workgroups to sum 16 slabs quickly (round 2, S = 64: 1.82 -> 1.87 ms; S = 256: 2.80 -> 2.70)
      else if (epi == tgx::GEMM_SILU) hipLaunchKernelGGL((tgx::gemm_splitk_reduce_kernel<DT, tgx::GEMM_SILU>), rg, blk, 0, c->stream, g);
      else if (epi == tgx::GEMM_GELU) hipLaunchKernelGGL((tgx::gemm_splitk_reduce_kernel<DT, tgx::GEMM_GELU>), rg, blk, 0, c->stream, g);
      else if (epi == tgx::GEMM_RESIDUAL) hipLaunchKernelGGL((tgx::gemm_splitk_reduce_kernel<DT, tgx::GEMM_RESIDUAL>), rg, blk, 0, c->stream, g);
      else hipLaunchKernelGGL((tgx::gemm_splitk_reduce_kernel<DT, tgx::GEMM_STORE>), rg, blk, 0, c->stream, g);)
    return;
  }
  // (a prompt whose 256 x 256 tiles leave the last round of workgroups mostly empty — 1152 rows at intermediate 8192: 320 tiles = 1.25 rounds, the time of 2048 rows — takes the
  //  128 x 128 kernel below instead: 1152 tiles = 4.5 rounds; option prefill.wide_8k_eff = per cent of the last round's fill below which that happens)
  const int t256 = ((N + 255) / 256) * ((M + 255) / 256), r256 = (t256 + c->num_cus - 1) / c->num_cus;
  const bool ragged256 = c->wide_8k_eff > 0 && epi == tgx::GEMM_SILU && t256 >= c->num_cus && 100 * t256 < c->wide_8k_eff * r256 * c->num_cus;
  if (!three_terms && (epi == tgx::GEMM_SILU || epi == tgx::GEMM_GELU) && t256 >= c->num_cus && !ragged256) {
    // the wide product (gate_up / c_fc) with enough 256 x 256 tiles to fill the chip: 8 waves, three-stage LDS-DMA ring
    const dim3 g8((N + 255) / 256, (M + 255) / 256), b8(512);
    const size_t lds8 = (size_t)3 * 3 * 256 * 32 * 2;
    TGX_DT16_SWITCH(c->dt,
      if (epi == tgx::GEMM_SILU) { if (one_k) hipLaunchKernelGGL((tgx::gemm_dma8_kernel<DT, tgx::GEMM_SILU, false>), g8, b8, lds8, c->stream, g); else hipLaunchKernelGGL((tgx::gemm_dma8_kernel<DT, tgx::GEMM_SILU>), g8, b8, lds8, c->stream, g); }
      else hipLaunchKernelGGL((tgx::gemm_dma8_kernel<DT, tgx::GEMM_GELU>), g8, b8, lds8, c->stream, g);)
    return;
  }
  if (!three_terms && (epi == tgx::GEMM_RESIDUAL || epi == tgx::GEMM_STORE) &&
      ((N + 255) / 256) * ((M + 255) / 256) >= c->num_cus) {
    // the N = hidden products of a prompt long enough to give every CU a 256 x 256 tile (Llama-3.2-1B from 8192 rows, Mistral-7B from 4096): the wide
    // product's kernel with the plain fp32 epilogue 
    const dim3 g8((N + 255) / 256, (M + 255) / 256), b8(512);
    const size_t lds8 = (size_t)3 * 3 * 256 * 32 * 2;
    TGX_DT16_SWITCH(c->dt,
      if (epi == tgx::GEMM_RESIDUAL) { if (one_k) hipLaunchKernelGGL((tgx::gemm_dma8_kernel<DT, tgx::GEMM_RESIDUAL, false>), g8, b8, lds8, c->stream, g); else hipLaunchKernelGGL((tgx::gemm_dma8_kernel<DT, tgx::GEMM_RESIDUAL>), g8, b8, lds8, c->stream, g); }
      else { if (one_k) hipLaunchKernelGGL((tgx::gemm_dma8_kernel<DT, tgx::GEMM_STORE, false>), g8, b8, lds8, c->stream, g); else hipLaunchKernelGGL((tgx::gemm_dma8_kernel<DT, tgx::GEMM_STORE>), g8, b8, lds8, c->stream, g); })
    return;
  }
  if (!three_terms && epi == tgx::GEMM_SILU) {
    // the wide product of a prompt too short for 256 x 256 tiles (129-384 rows: 128-384 tiles of 128 x 128): the eight-wave kernel with the K step split between
    // wave pairs instead of the four-wave one (option prefill.wide_8k: Llama-3.2-1B S = 256 gate_up 61 us per layer)
    const int t128 = ((N + 127) / 128) * ((M + 127) / 128);
    if (2 * t128 >= c->num_cus && (2 * t128 <= WIDE_8K_MAX * c->num_cus || ragged256)) {
      const dim3 g8((N + 127) / 128, (M + 127) / 128), b8(512);
      const size_t lds8 = (size_t)3 * 3 * 128 * 64 * 2;
      TGX_DT16_SWITCH(c->dt, if (one_k) hipLaunchKernelGGL((tgx::gemm_dma8k_kernel<DT, tgx::GEMM_SILU, false>), g8, b8, lds8, c->stream, g); else hipLaunchKernelGGL((tgx::gemm_dma8k_kernel<DT, tgx::GEMM_SILU>), g8, b8, lds8, c->stream, g);)
      return;
    }
  }
  if (!three_terms && (epi == tgx::GEMM_RESIDUAL || epi == tgx::GEMM_STORE)) {
    // N = hidden products whose 128 x 128 tiles number between half a chip and a chip and a half: eight waves per tile, K step split between wave pairs
    const int t128 = ((N + 127) / 128) * ((M + 127) / 128);
    if (2 * t128 >= c->num_cus && 2 * t128 <= 3 * c->num_cus) {
      const dim3 g8((N + 127) / 128, (M + 127) / 128), b8(512);
      const size_t lds8 = (size_t)3 * 3 * 128 * 64 * 2;
      TGX_DT16_SWITCH(c->dt,
        if (epi == tgx::GEMM_RESIDUAL) { if (one_k) hipLaunchKernelGGL((tgx::gemm_dma8k_kernel<DT, tgx::GEMM_RESIDUAL, false>), g8, b8, lds8, c->stream, g); else hipLaunchKernelGGL((tgx::gemm_dma8k_kernel<DT, tgx::GEMM_RESIDUAL>), g8, b8, lds8, c->stream, g); }
        else { if (one_k) hipLaunchKernelGGL((tgx::gemm_dma8k_kernel<DT, tgx::GEMM_STORE, false>), g8, b8, lds8, c->stream, g); else hipLaunchKernelGGL((tgx::gemm_dma8k_kernel<DT, tgx::GEMM_STORE>), g8, b8, lds8, c->stream, g); })
      return;
    }
  }
  if (three_terms && epi == tgx::GEMM_STORE && three_from > 0 && three_from % tgx::GBN == 0 && N > three_from &&
      (N - three_from) % 64 == 0 && three_from / tgx::GBN == (N - three_from) / 64 && 2 * (three_from / tgx::GBN) * ((M + 127) / 128) >= c->num_cus) {
    // ... with as many 128-column Q tiles as 64-column K | V tiles (q_dim = 4 kv_dim) and at least half a chip of workgroups: eight waves per workgroup, the Q tile and the
    // K | V tile of a row block on ONE staging of the activation lines (kernels/gemm_dma.h gemm_dma_qkv8_kernel)
    const int nwg = (three_from / tgx::GBN) * ((M + 127) / 128);
    if (c->qkv_epi.q_hi && c->d.head_dim == 64 && !c->d.qk_norm && defer) {
      // ... and RoPE + cache append + the q split in its epilogue (one sequence, head_dim 64): no fp32 QKV matrix, no rope_kv_split launch
      g.rope_q_hi = c->qkv_epi.q_hi; g.rope_q_lo = c->qkv_epi.q_lo; g.rope_k = c->qkv_epi.k; g.rope_v = c->qkv_epi.v;
      g.rope_cos = c->rope_cos; g.rope_sin = c->rope_sin; g.rope_past = c->qkv_epi.past; g.rope_max_ctx = c->d.max_ctx; g.rope_kv_heads = c->d.kv_heads; g.rope_tbl = c->qkv_epi.tbl;
      TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL((tgx::gemm_dma_qkv8_kernel<DT, true>), dim3(nwg), dim3(512), (size_t)2 * (3 * 128 + 128 + 64) * 64 * 2, c->stream, g))
      *defer = 0;         // the rows are finished: the caller skips its RoPE / cache-append launch
      return;
    }
    TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL((tgx::gemm_dma_qkv8_kernel<DT>), dim3(nwg), dim3(512), (size_t)2 * (3 * 128 + 128 + 64) * 64 * 2, c->stream, g))
    return;
  }
  if (three_terms && epi == tgx::GEMM_STORE && three_from > 0 && three_from % tgx::GBN == 0 && N > three_from && M >= 128) {
    // the QKV product of a bf16 prompt: Q columns as two-term 128-row tiles, K / V columns as three-term 64-row tiles, ONE launch with
    // equal work per workgroup pair (kernels/gemm_dma.h gemm_dma_qkv_kernel)
    const int nq = (three_from / tgx::GBN) * ((M + 127) / 128), nkv = ((N - three_from + tgx::GBN - 1) / tgx::GBN) * ((M + 63) / 64);
    const size_t ldsq = std::max(tgx::gemm_dma_lds_bytes(2, false, 32, 2), tgx::gemm_dma_lds_bytes(1, true, 32, 2));
    TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL((tgx::gemm_dma_qkv_kernel<DT, 32, 2>), dim3(nq + nkv), blk, ldsq, c->stream, g))
    return;
  }
  // every other product: operand tiles by LDS-DMA into a two-stage ring (kernels/gemm_dma.h), one barrier per K step
  // geometry per tile height: 128-row tiles k = 32, 64-row tiles k = 64 (round 2's sweep, profiles/r02_prefill_dma_sweep.txt: deeper rings lose 4-20 % to occupancy
  // here — the eight-wave kernels are where they pay; the other geometries went with the option bits that selected them in round 6, the unsplit register-staged
  // gemm_x2_kernel of round 1 with the family mask itself: Llama-3.2-1B 2048 tokens 11.4-11.7 -> 10.0-10.3 ms)
  static_assert(tgx::gemm_dma_lds_bytes(1, true, 64, 2) <= 160 * 1024 && tgx::gemm_dma_lds_bytes(2, true, 32, 2) <= 160 * 1024, "the two-stage rings fit the LDS of a CU");
  const size_t lds = small ? tgx::gemm_dma_lds_bytes(1, three_terms, 64, 2) : tgx::gemm_dma_lds_bytes(2, three_terms, 32, 2);
#define TGX_DMA(EPI_, MI_) do { if ((MI_) == 1) hipLaunchKernelGGL((tgx::gemm_dma_kernel<DT, EPI_, 1, 64, 2>), grid, blk, lds, c->stream, g); \
                                else hipLaunchKernelGGL((tgx::gemm_dma_kernel<DT, EPI_, 2, 32, 2>), grid, blk, lds, c->stream, g); } while (0)
  TGX_DT16_SWITCH(c->dt,
    if (epi == tgx::GEMM_SILU) TGX_DMA(tgx::GEMM_SILU, 2);
    else if (epi == tgx::GEMM_GELU) TGX_DMA(tgx::GEMM_GELU, 2);
    else if (epi == tgx::GEMM_RESIDUAL) { if (small) TGX_DMA(tgx::GEMM_RESIDUAL, 1); else TGX_DMA(tgx::GEMM_RESIDUAL, 2); }
    else { if (small) TGX_DMA(tgx::GEMM_STORE, 1); else TGX_DMA(tgx::GEMM_STORE, 2); })
#undef TGX_DMA
}

// ---- the key-split attention of a continuation (kernels/attn_extend.h; option extend.attn_splits).  Splits of a pass of S positions from `past`: 0 = the per-row
// prompt attention (a pass from position 0, more than one query block, the option at 0, a context below the measured threshold)
int extend_attn_splits(const tgx_ctx* c, int S, int past) {
  if (c->extend_attn_splits == 0 || past <= 0 || S > tgx::ATTN_QBLK || c->dt == tgx::DT_F32) return 0;
  const int tiles = (past + S - 1) / tgx::ATTN_KTILE + 1;
  int ns = c->extend_attn_splits;
  if (ns < 0) {      // automatic: heads x splits ~ the CUs, at most 32, from the context where the split form wins (ctx.h extend_attn_min)
    if (past + S <= (c->d.head_dim == 64 ? c->extend_attn_min64 : c->extend_attn_min128)) return 0;
    ns = std::min(32, c->num_cus / std::max(1, c->d.heads));
    if (ns < 2) return 0;
  }
  return std::min(ns, tiles);
}
// bytes of the partials of ns splits: attn_extend_part_vals values of 256 lanes per (split, head) (kernels/attn_extend.h)
static size_t extend_part_bytes(const tgx_ctx* c, int ns) {
  const int vals = c->d.head_dim == 64 ? tgx::attn_extend_part_vals<64>() : tgx::attn_extend_part_vals<128>();
  return (size_t)ns * c->d.heads * vals * 256 * sizeof(float);
}
int ensure_extend_ws(tgx_ctx* c, int S, int past) {
  const int ns = extend_attn_splits(c, S, past);
  if (!ns) return TGX_OK;
  return dev_grow(c, &c->ext_part, &c->ext_part_bytes, extend_part_bytes(c, ns));
}
static void launch_attn_extend(tgx_ctx* c, const tgx::AttnPrefillArgs& a, int ns, const unsigned short* anc = nullptr) {      // anc: a token tree's masks (tgx_verify_tree)
  const int hd = c->d.head_dim;
  tgx::AttnExtendArgs e{};
  e.a = a; e.part = c->ext_part; e.ns = ns; e.n_tiles = (a.past + a.S - 1) / tgx::ATTN_KTILE + 1;
  if (!c->ext_part || extend_part_bytes(c, ns) > c->ext_part_bytes) { c->launch_fault = "attn_extend: the partials' workspace was not sized for this pass"; return; }
  const size_t lds1 = (size_t)tgx::ATTN_KTILE * ((hd + 8) + (hd + 32)) * 2;
  const dim3 grid(a.heads, ns), blk(256);
  if (anc) {
    tgx::AttnExtendTreeArgs t{};
    t.e = e; t.anc = anc;
    auto go_tree = [&](auto paged) {
      constexpr bool P = decltype(paged)::value;
      TGX_DT16_SWITCH(c->dt,
        if (hd == 64) { hipLaunchKernelGGL((tgx::attn_extend_tree_kernel<DT, 64, P>), grid, blk, lds1, c->stream, t); hipLaunchKernelGGL((tgx::attn_extend_merge_kernel<DT, 64>), dim3(a.heads), blk, 0, c->stream, e); }
        else { hipLaunchKernelGGL((tgx::attn_extend_tree_kernel<DT, 128, P>), grid, blk, lds1, c->stream, t); hipLaunchKernelGGL((tgx::attn_extend_merge_kernel<DT, 128>), dim3(a.heads), blk, 0, c->stream, e); })
    };
    if (a.blk_tbl) go_tree(std::true_type{}); else go_tree(std::false_type{});
    return;
  }
  auto go = [&](auto paged) {
    constexpr bool P = decltype(paged)::value;
    TGX_DT16_SWITCH(c->dt,
      if (hd == 64) { hipLaunchKernelGGL((tgx::attn_extend_kernel<DT, 64, P>), grid, blk, lds1, c->stream, e); hipLaunchKernelGGL((tgx::attn_extend_merge_kernel<DT, 64>), dim3(a.heads), blk, 0, c->stream, e); }
      else { hipLaunchKernelGGL((tgx::attn_extend_kernel<DT, 128, P>), grid, blk, lds1, c->stream, e); hipLaunchKernelGGL((tgx::attn_extend_merge_kernel<DT, 128>), dim3(a.heads), blk, 0, c->stream, e); })
  };
  if (a.blk_tbl) go(std::true_type{}); else go(std::false_type{});
}
// ---- the ragged key-split form (tgx_verify_rows; kernels/attn_extend.h attn_extend_rg_kernel).  Option extend.attn_splits: 0 never, N >= 1 N splits, -1 automatic:
// split when the longest past_i + S_i of the pass exceeds extend_attn_min{64,128}, with min(32, 2 * CUs / (n * heads)) splits, unsplit when that is below 2.
// The split count is measured (tools/spec_bench.py --rows, profiles/verify_rows.txt; Llama-3.2-1B bf16, 32 heads, context 2048, ms per tgx_verify_rows call of
// 4 positions per row, greedy; spread of a figure ~0.05): two workgroups per CU win at every batch size tried —
//   n = 2: unsplit 1.95, 2 splits 1.53, 4 1.34, 8 1.30      n = 4: unsplit 2.05, 2 1.63, 4 1.47, 8 1.55      n = 8: unsplit 2.23, 2 1.88, 4 1.95, 8 2.04
// (one workgroup per CU, the one-row call's rule taken to n rows, gave 1.34 / 1.63 / unsplit 2.23).  The THRESHOLD is still the one measured for ONE row (ctx.h
// extend_attn_min); for n > 1 sequences, for contexts other than 2048 and for head_dim 128 it is unmeasured.
static size_t extend_rg_part_bytes(const tgx_ctx* c, int n, int ns) { return (size_t)n * extend_part_bytes(c, ns); }
int ensure_extend_rg_ws(tgx_ctx* c, RaggedPass& p) {
  p.ext_ns = 0;
  if (c->extend_attn_splits == 0 || !p.past || p.longest > tgx::ATTN_QBLK || c->dt == tgx::DT_F32) return TGX_OK;
  int reach = 0;       // the longest past_i + S_i
  for (int i = 0; i < p.n; i++) reach = std::max(reach, p.past[i] + p.lens[i]);
  int ns = c->extend_attn_splits;
  if (ns < 0) {
    if (reach <= (c->d.head_dim == 64 ? c->extend_attn_min64 : c->extend_attn_min128)) return TGX_OK;
    ns = std::min(32, 2 * c->num_cus / std::max(1, p.n * c->d.heads));
    if (ns < 2) return TGX_OK;
  }
  p.ext_ns = std::min(ns, (reach - 1) / tgx::ATTN_KTILE + 1);
  return dev_grow(c, &c->ext_part, &c->ext_part_bytes, extend_rg_part_bytes(c, p.n, p.ext_ns));
}
static void launch_attn_extend_rg(tgx_ctx* c, const tgx::AttnRgArgs& r, const RaggedPass& rg) {
  const int hd = c->d.head_dim;
  tgx::AttnExtendRgArgs e{};
  e.r = r; e.part = c->ext_part; e.ns = rg.ext_ns;
  if (!c->ext_part || extend_rg_part_bytes(c, rg.n, rg.ext_ns) > c->ext_part_bytes) { c->launch_fault = "attn_extend_rg: the partials' workspace was not sized for this pass"; return; }
  const size_t lds1 = (size_t)tgx::ATTN_KTILE * ((hd + 8) + (hd + 32)) * 2;
  const dim3 grid(r.a.heads, rg.ext_ns, rg.n), mgrid(r.a.heads, rg.n), blk(256);
  auto go = [&](auto paged) {
    constexpr bool P = decltype(paged)::value;
    TGX_DT16_SWITCH(c->dt,
      if (hd == 64) { hipLaunchKernelGGL((tgx::attn_extend_rg_kernel<DT, 64, P>), grid, blk, lds1, c->stream, e); hipLaunchKernelGGL((tgx::attn_extend_rg_merge_kernel<DT, 64>), mgrid, blk, 0, c->stream, e); }
      else { hipLaunchKernelGGL((tgx::attn_extend_rg_kernel<DT, 128, P>), grid, blk, lds1, c->stream, e); hipLaunchKernelGGL((tgx::attn_extend_rg_merge_kernel<DT, 128>), mgrid, blk, 0, c->stream, e); })
  };
  if (c->kv_paged) go(std::true_type{}); else go(std::false_type{});
}

// ---- the mixed attention of tgx_advance_rows (kernels/attn_mixed.h; the lists: attn_worklist.h through advance_tables below).  Option advance.attn_tiles -> the
// tile target of a pass; -1 is attn_worklist.h's auto_target at two workgroups per CU; the default is a fixed 16 (ctx.h advance_attn_tiles: the sweep, and what it left unmeasured).
// A target whose partials would exceed MIX_PART_MAX is doubled until they fit (a pass of 8192 positions at target 1 would ask for gigabytes)
static_assert(attn_worklist::QBLK == tgx::ATTN_QBLK && attn_worklist::KTILE == tgx::ATTN_KTILE, "attn_worklist.h restates the prompt attention's blocking");
static_assert(sizeof(attn_worklist::Item) == sizeof(tgx::MixItem), "kernels/attn_mixed.h MixItem is attn_worklist.h Item");
constexpr size_t MIX_PART_MAX = (size_t)512 << 20;
static size_t mix_slot_bytes(const tgx_ctx* c) {
  return (size_t)(c->d.head_dim == 64 ? tgx::attn_extend_part_vals<64>() : tgx::attn_extend_part_vals<128>()) * 256 * sizeof(float);
}
static std::vector<attn_worklist::Seq> mix_seqs(const RaggedPass& p) {
  std::vector<attn_worklist::Seq> s((size_t)p.n);
  for (int j = 0; j < p.n; j++) s[(size_t)j] = attn_worklist::Seq{p.lens[j], p.past ? p.past[j] : 0};
  return s;
}
int advance_attn_target(const tgx_ctx* c, const RaggedPass& p) {
  if (c->dt == tgx::DT_F32 || c->advance_attn_tiles == 0) return 0;
  const std::vector<attn_worklist::Seq> s = mix_seqs(p);
  int t = c->advance_attn_tiles > 0 ? c->advance_attn_tiles : attn_worklist::auto_target(s.data(), p.n, c->d.heads, 2 * c->num_cus);
  while (t > 0 && (size_t)attn_worklist::count(s.data(), p.n, c->d.heads, t).slots * mix_slot_bytes(c) > MIX_PART_MAX) t *= 2;
  return t;
}
int ensure_mix_ws(tgx_ctx* c, const RaggedPass& p) {
  if (!p.mix_slots) return TGX_OK;
  return dev_grow(c, &c->mix_part, &c->mix_part_bytes, (size_t)p.mix_slots * mix_slot_bytes(c));
}
static void launch_attn_mixed(tgx_ctx* c, const tgx::AttnRgArgs& r, const RaggedPass& rg) {
  const int hd = c->d.head_dim;
  if (!c->mix_part || (size_t)rg.mix_slots * mix_slot_bytes(c) > c->mix_part_bytes) { c->launch_fault = "attn_mixed: the partials' workspace was not sized for this pass"; return; }
  tgx::AttnMixArgs e{};
  e.r = r; e.part = c->mix_part; e.items = rg.mix_split;
  tgx::AttnMixArgs m = e;
  m.items = rg.mix_merge;
  const size_t lds1 = (size_t)tgx::ATTN_KTILE * ((hd + 8) + (hd + 32)) * 2;
  const dim3 grid(rg.n_mix_split), mgrid(rg.n_mix_merge), blk(256);
  auto go = [&](auto paged) {
    constexpr bool P = decltype(paged)::value;
    TGX_DT16_SWITCH(c->dt,
      if (hd == 64) { hipLaunchKernelGGL((tgx::attn_mixed_split_kernel<DT, 64, P>), grid, blk, lds1, c->stream, e); hipLaunchKernelGGL((tgx::attn_mixed_merge_kernel<DT, 64>), mgrid, blk, 0, c->stream, m); }
      else { hipLaunchKernelGGL((tgx::attn_mixed_split_kernel<DT, 128, P>), grid, blk, lds1, c->stream, e); hipLaunchKernelGGL((tgx::attn_mixed_merge_kernel<DT, 128>), mgrid, blk, 0, c->stream, m); })
  };
  if (c->kv_paged) go(std::true_type{}); else go(std::false_type{});
}

// causal GQA flash attention of S prompt positions of one batch row (grid = ceil(S / 128) query blocks x heads)
// anc (tgx_verify_tree): the S <= 16 positions are a token tree's, masked by its ancestor words — the key-split form by the same rule as a chain of S positions, else
// one workgroup per head of the one query block
void launch_attn_prefill(tgx_ctx* c, const tgx::AttnPrefillArgs& a_, bool allow_lean, const unsigned short* anc) {
  tgx::AttnPrefillArgs a = a_;
  const int hd = c->d.head_dim;
  if (const int ns = extend_attn_splits(c, a.S, a.past)) { launch_attn_extend(c, a, ns, anc); return; }
  if (anc) {
    if (a.S > 16 || (hd != 64 && hd != 128)) { c->launch_fault = "attn_prefill_tree: a token tree has at most 16 positions, head_dim 64 or 128"; return; }
    tgx::AttnTreeArgs t{};
    t.a = a; t.anc = anc;
    const size_t lds = (size_t)tgx::ATTN_KTILE * ((hd + 8) + (hd + 32)) * 2;
    const dim3 grid(a.heads), blk(256);
    auto go_tree = [&](auto paged) {
      constexpr bool P = decltype(paged)::value;
      TGX_DT16_SWITCH(c->dt,
        if (hd == 64) hipLaunchKernelGGL((tgx::attn_prefill_tree_kernel<DT, 64, P>), grid, blk, lds, c->stream, t);
        else hipLaunchKernelGGL((tgx::attn_prefill_tree_kernel<DT, 128, P>), grid, blk, lds, c->stream, t))
    };
    if (a.blk_tbl) go_tree(std::true_type{}); else go_tree(std::false_type{});
    return;
  }
  const int nqb = (a.S + tgx::ATTN_QBLK - 1) / tgx::ATTN_QBLK, nwg = nqb * a.heads;
  const size_t lds1 = (size_t)tgx::ATTN_KTILE * ((hd + 8) + (hd + 32)) * 2;      // one K tile | V tile pair (kernels/prefill.h)
  // head_dim 64, three or more workgroups per CU (prompts from ~3k tokens at 32 heads): K / V tiles by LDS-DMA, the next tile's scores under the current tile's
  // softmax (kernels/attn_prefill_dma.h; bit-identical to attn_prefill_kernel): S = 4096 203 -> 177 us per layer, 8192 730 -> 632; at S = 2048 (one round of 512
  // workgroups) the launch lasts as long as its heaviest workgroup's chain of tiles in either form (62-63 us).  Option prefill.attn_dma: 0 never, 1 auto, 2 always
  if (hd == 64 && (c->attn_dma == 2 || (c->attn_dma == 1 && allow_lean && nwg >= 3 * c->num_cus))) {
    a.heavy_first = 1;
    const dim3 grid(a.heads, nqb), blk(256);
    TGX_DT16_SWITCH(c->dt, if (a.blk_tbl) hipLaunchKernelGGL((tgx::attn_prefill_dma_kernel<DT, true>), grid, blk, (size_t)2 * 3 * 64 * 64 * 2, c->stream, a);
                           else hipLaunchKernelGGL((tgx::attn_prefill_dma_kernel<DT, false>), grid, blk, (size_t)2 * 3 * 64 * 64 * 2, c->stream, a))
    return;
  }
  // key split inside the workgroup (attn_prefill_kernel KP = 2; option prefill.attn_ksplit: 0 never, 1 auto, 2 always): eight waves, the odd tiles on waves 4-7,
  // one merge at the end — half the chain of tiles per wave.  head_dim 128: S = 2048 94 -> 91 us per layer, 4096 401 -> 305, 8192 1284 -> 1086 (always);
  // head_dim 64 below three workgroups per CU: S = 2048 62 -> 55-56 us in isolation, 68.1 -> 61.3 in the model's trace (profiles/r05_prefill.txt section 5)
  const bool ksplit = nqb >= 2 && (c->attn_ksplit == 2 || (c->attn_ksplit == 1 && (hd == 128 || nwg < 3 * c->num_cus)));
  // head_dim 64 with three or more workgroups per CU: the one-tile look-ahead form at three waves per SIMD (prefill.h)
  const bool lean = allow_lean && hd == 64 && nwg >= 3 * c->num_cus;
  a.heavy_first = ksplit ? 1 : 0;
  const dim3 gridk(a.heads, nqb), blkk(512), grid(nqb, a.heads), blk(256);
  auto go = [&](auto paged) {        // (paged KV: the same forms through the sequence's block table)
    constexpr bool P = decltype(paged)::value;
    TGX_DT16_SWITCH(c->dt,
      if (ksplit) {
        if (hd == 64) hipLaunchKernelGGL((tgx::attn_prefill_kernel<DT, 64, 2, 2, P>), gridk, blkk, 2 * lds1, c->stream, a);
        else hipLaunchKernelGGL((tgx::attn_prefill_kernel<DT, 128, 1, 2, P>), gridk, blkk, 2 * lds1, c->stream, a);
      } else if (lean) hipLaunchKernelGGL((tgx::attn_prefill_kernel<DT, 64, 1, 1, P>), grid, blk, lds1, c->stream, a);
      else if (hd == 64) hipLaunchKernelGGL((tgx::attn_prefill_kernel<DT, 64, 2, 1, P>), grid, blk, lds1, c->stream, a);
      else hipLaunchKernelGGL((tgx::attn_prefill_kernel<DT, 128, 1, 1, P>), grid, blk, lds1, c->stream, a))     // head_dim 128: two waves per SIMD only in this form (95 vs 138 µs per layer at S = 2048)
  };
  if (a.blk_tbl) go(std::true_type{}); else go(std::false_type{});
}
// the prompt attention of a ragged pass: ONE launch over rg's work list (kernels/prefill.h attn_prefill_rg_kernel).  The form is launch_attn_prefill's rule with the
// longest prompt in the place of the row: the key split (another fp32 summation order) as that rule gives it for the longest prompt's workgroups, so that equal-length
// prompts take the form tgx_forward takes for each of their rows; among the one-group forms, which compute the same bits (tests/test_hip_prefill.py), the launch's
// total workgroup count picks the occupancy form (LDS-DMA or the lean look-ahead from three workgroups per CU)
void launch_attn_prefill_ragged(tgx_ctx* c, const tgx::AttnPrefillArgs& a, const RaggedPass& rg, long long layer_off, bool allow_lean) {
  tgx::AttnRgArgs r{};
  r.a = a; r.seq = rg.seq; r.item = rg.items; r.layer_off = layer_off;
  if (rg.ext_ns > 0) { launch_attn_extend_rg(c, r, rg); return; }      // continuations (tgx_verify_rows): the key-split form
  if (rg.n_mix_split > 0) launch_attn_mixed(c, r, rg);                  // tgx_advance_rows: the query blocks cut into key ranges, and their merge (two launches) ...
  if (rg.n_items == 0) return;                                          // ... beside the whole blocks below (an empty list launches nothing)
  const int hd = c->d.head_dim;
  const int nqb = (rg.longest + tgx::ATTN_QBLK - 1) / tgx::ATTN_QBLK, nwg = nqb * a.heads, total = rg.n_items;
  const size_t lds1 = (size_t)tgx::ATTN_KTILE * ((hd + 8) + (hd + 32)) * 2;
  const bool dma_row = hd == 64 && (c->attn_dma == 2 || (c->attn_dma == 1 && allow_lean && nwg >= 3 * c->num_cus));
  const bool ksplit = !dma_row && nqb >= 2 && (c->attn_ksplit == 2 || (c->attn_ksplit == 1 && (hd == 128 || nwg < 3 * c->num_cus)));
  const bool wide = !ksplit && allow_lean && hd == 64 && total >= 3 * c->num_cus;
  const bool dma = dma_row || (wide && c->attn_dma == 1);
  const bool lean = !dma && wide;
  const dim3 grid(total), blk(256), blkk(512);
  auto go = [&](auto paged) {
    constexpr bool P = decltype(paged)::value;
    TGX_DT16_SWITCH(c->dt,
      if (dma) hipLaunchKernelGGL((tgx::attn_prefill_dma_rg_kernel<DT, P>), grid, blk, (size_t)2 * 3 * 64 * 64 * 2, c->stream, r);
      else if (ksplit) {
        if (hd == 64) hipLaunchKernelGGL((tgx::attn_prefill_rg_kernel<DT, 64, 2, 2, P>), grid, blkk, 2 * lds1, c->stream, r);
        else hipLaunchKernelGGL((tgx::attn_prefill_rg_kernel<DT, 128, 1, 2, P>), grid, blkk, 2 * lds1, c->stream, r);
      } else if (lean) hipLaunchKernelGGL((tgx::attn_prefill_rg_kernel<DT, 64, 1, 1, P>), grid, blk, lds1, c->stream, r);
      else if (hd == 64) hipLaunchKernelGGL((tgx::attn_prefill_rg_kernel<DT, 64, 2, 1, P>), grid, blk, lds1, c->stream, r);
      else hipLaunchKernelGGL((tgx::attn_prefill_rg_kernel<DT, 128, 1, 1, P>), grid, blk, lds1, c->stream, r))
  };
  if (c->kv_paged) go(std::true_type{}); else go(std::false_type{});
}
// the device tables of a ragged pass (ctx.h): built here because the work list's blocking is attn_prefill_rg_kernel's
size_t ragged_tables(const tgx_ctx* c, RaggedPass& p, unsigned char* host, const unsigned char* dev) {
  constexpr int QB = tgx::ATTN_QBLK, KT = tgx::ATTN_KTILE;
  auto align = [](size_t o) { return (o + 15) & ~(size_t)15; };
  p.n_items = 0;
  for (int j = 0; j < p.n; j++) p.n_items += ((p.lens[j] + QB - 1) / QB) * c->d.heads;
  const size_t o_tok = align((size_t)p.n * sizeof(tgx::RgSeq)), o_item = align(o_tok + (size_t)p.M * 4), bytes = align(o_item + (size_t)p.n_items * sizeof(tgx::RgItem));
  if (!host) return bytes;
  tgx::RgSeq* sq = reinterpret_cast<tgx::RgSeq*>(host);
  int* tok = reinterpret_cast<int*>(host + o_tok);
  tgx::RgItem* it = reinterpret_cast<tgx::RgItem*>(host + o_item);
  std::vector<std::pair<int, int>> blocks;             // (prompt, query block), heaviest first: key tiles descending, ties in prompt order
  for (int j = 0; j < p.n; j++) {
    const RowState& r = c->rows[(size_t)p.rows[j]];
    sq[j].row0 = p.first[j]; sq[j].S = p.lens[j];
    sq[j].k = reinterpret_cast<bf16_t*>(r.kcache); sq[j].v = reinterpret_cast<bf16_t*>(r.vcache); sq[j].tbl = r.tbl; sq[j].past = p.past ? p.past[j] : 0; sq[j].pad = 0;
    for (int s = 0; s < p.lens[j]; s++) tok[p.first[j] + s] = j;
    for (int qb = 0; qb < (p.lens[j] + QB - 1) / QB; qb++) blocks.emplace_back(j, qb);
  }
  auto tiles = [&](const std::pair<int, int>& b) { return ((p.past ? p.past[b.first] : 0) + std::min(b.second * QB + QB - 1, p.lens[b.first] - 1)) / KT + 1; };      // its real key tiles
  std::stable_sort(blocks.begin(), blocks.end(), [&](const std::pair<int, int>& x, const std::pair<int, int>& y) { return tiles(x) > tiles(y); });
  int k = 0;
  for (const auto& b : blocks)
    for (int h = 0; h < c->d.heads; h++) it[k++] = tgx::RgItem{b.first, b.second, h, 0};
  p.seq = reinterpret_cast<const tgx::RgSeq*>(dev);
  p.tok_seq = reinterpret_cast<const int*>(dev + o_tok);
  p.items = reinterpret_cast<const tgx::RgItem*>(dev + o_item);
  return bytes;
}
// ... of tgx_advance_rows: ragged_tables' block (the sequences, the token map, the whole query blocks as its work list) with the mixed attention's two lists behind
// it.  The lists, their order and the partial slots are attn_worklist.h's (checked on a CPU: tests/attn_worklist_check.cpp); at target 0 both lists are empty
size_t advance_tables(const tgx_ctx* c, RaggedPass& p, unsigned char* host, const unsigned char* dev, int target) {
  auto align = [](size_t o) { return (o + 15) & ~(size_t)15; };
  const std::vector<attn_worklist::Seq> s = mix_seqs(p);
  const attn_worklist::Counts n = attn_worklist::count(s.data(), p.n, c->d.heads, target);
  p.n_items = n.unsplit; p.n_mix_split = n.split; p.n_mix_merge = n.merge; p.mix_slots = n.slots;
  const size_t o_tok = align((size_t)p.n * sizeof(tgx::RgSeq)), o_item = align(o_tok + (size_t)p.M * 4), o_split = align(o_item + (size_t)n.unsplit * sizeof(tgx::RgItem)),
               o_merge = align(o_split + (size_t)n.split * sizeof(tgx::MixItem)), bytes = align(o_merge + (size_t)n.merge * sizeof(tgx::MixItem));
  if (!host) return bytes;
  tgx::RgSeq* sq = reinterpret_cast<tgx::RgSeq*>(host);
  int* tok = reinterpret_cast<int*>(host + o_tok);
  for (int j = 0; j < p.n; j++) {
    const RowState& r = c->rows[(size_t)p.rows[j]];
    sq[j].row0 = p.first[j]; sq[j].S = p.lens[j];
    sq[j].k = reinterpret_cast<bf16_t*>(r.kcache); sq[j].v = reinterpret_cast<bf16_t*>(r.vcache); sq[j].tbl = r.tbl; sq[j].past = p.past ? p.past[j] : 0; sq[j].pad = 0;
    for (int k = 0; k < p.lens[j]; k++) tok[p.first[j] + k] = j;
  }
  const attn_worklist::Lists L = attn_worklist::build(s.data(), p.n, c->d.heads, target);
  tgx::RgItem* it = reinterpret_cast<tgx::RgItem*>(host + o_item);
  for (size_t k = 0; k < L.unsplit.size(); k++) it[k] = tgx::RgItem{L.unsplit[k].seq, L.unsplit[k].qblk, L.unsplit[k].h, 0};
  if (!L.split.empty()) std::memcpy(host + o_split, L.split.data(), L.split.size() * sizeof(tgx::MixItem));
  if (!L.merge.empty()) std::memcpy(host + o_merge, L.merge.data(), L.merge.size() * sizeof(tgx::MixItem));
  p.seq = reinterpret_cast<const tgx::RgSeq*>(dev);
  p.tok_seq = reinterpret_cast<const int*>(dev + o_tok);
  p.items = reinterpret_cast<const tgx::RgItem*>(dev + o_item);
  p.mix_split = reinterpret_cast<const tgx::MixItem*>(dev + o_split);
  p.mix_merge = reinterpret_cast<const tgx::MixItem*>(dev + o_merge);
  return bytes;
}
// RoPE + cache append + q split of S prompt rows of one batch row
// (depth: a token tree's device depth table, tgx_verify_tree — row s into slot past + s, rotated for past + depth[s])
void launch_rope_kv_split(tgx_ctx* c, const tgx::RopeKvArgs& a, int S, const int* depth) {
  if (depth) {
    tgx::RopeTreeArgs r{};
    r.a = a; r.depth = depth;
    TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::rope_kv_split_tree_kernel<DT>, dim3(S), dim3(256), 0, c->stream, r))
    return;
  }
  TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::rope_kv_split_kernel<DT>, dim3(S), dim3(256), 0, c->stream, a))
}
// ... of every row of a ragged pass, each into its own prompt's row: ONE launch
void launch_rope_kv_split_ragged(tgx_ctx* c, const tgx::RopeKvArgs& a, const RaggedPass& rg, long long layer_off) {
  tgx::RopeRgArgs r{};
  r.a = a; r.seq = rg.seq; r.tok_seq = rg.tok_seq; r.layer_off = layer_off;
  TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::rope_kv_split_rg_kernel<DT>, dim3(rg.M), dim3(256), 0, c->stream, r))
}
// the ids of a ragged pass -> ws_x (GPT-2: + the learned position of each row within its prompt, one launch per prompt)
void launch_embed_ragged(tgx_ctx* c, const RaggedPass& rg) {
  const int H = c->d.hidden;
  if (!c->gpt2) {
    TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::embed_rows_any_kernel<DT>, dim3(rg.M), dim3(256), 0, c->stream, rg.ids, (const void*)c->embed, (const void*)nullptr, c->ws_x, H, rg.M, 0LL, 0))
    return;
  }
  for (int i = 0; i < rg.n; i++)
    TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::embed_rows_any_kernel<DT>, dim3(rg.lens[i]), dim3(256), 0, c->stream, rg.ids + rg.first[i], (const void*)c->embed, (const void*)c->wpe,
                                              c->ws_x + (size_t)rg.first[i] * H, H, rg.lens[i], 0LL, rg.past ? rg.past[i] : 0))
}
// RMSNorm of the rows of x into 16-bit terms (ws_ah / ws_al), first adding a pending split-K residual (nsplit > 1: the slabs in ws_part)
void launch_norm_terms(tgx_ctx* c, float* x, const ebyte* norm_w, int M, int H, int nsplit, bool third) {
  TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::rmsnorm_split_kernel<DT>, dim3(M), dim3(256), 0, c->stream, x, reinterpret_cast<const bf16_t*>(norm_w), c->d.norm_eps, H,
                                          c->ws_ah, c->ws_al, third ? c->ws_al2 : (bf16_t*)nullptr, (const float*)(nsplit > 1 ? c->ws_part : nullptr), nsplit, (long long)M * H, (const bf16_t*)nullptr))
}
void launch_embed_rows(tgx_ctx* c, const long long* ids, float* X, int M, int S) {
  TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::embed_rows_kernel<DT>, dim3(M), dim3(256), 0, c->stream, ids, (const bf16_t*)c->embed, X, c->d.hidden, S, (long long)c->d.max_ctx))
}

// All layers for S prompt positions of one row at once; leaves the last position's hidden state in row.x.
// == CausalLM::forward on [1,S] ids with an empty cache (GPTModel.h:51-56)
// NB batch rows [row0, row0 + NB) are stacked into ONE [NB*S] row block for the row-wise kernels and the GEMMs (the weights stream
// once for all of them); RoPE / cache append and attention run per batch row on its slice and its own cache.
// rg (tgx_forward_rows): a ragged pass of rg->M rows instead — RoPE / cache append and attention then run as ONE launch each for all its prompts
static void prefill_pass(tgx_ctx* c, int row0, int NB, int S, int past, const RaggedPass* rg) {
  const tgx_model_desc& d = c->d;
  const int H = d.hidden, I = d.inter, hd = d.head_dim, qd = d.heads * hd, kvd = d.kv_heads * hd;
  const size_t kv_layer = c->kv_paged ? (size_t)c->kv.n_blocks() * d.kv_heads * tgx::KV_BLOCK * hd : (size_t)d.kv_heads * d.max_ctx * hd;      // elements (paged KV: a layer's pool)
  const int M = rg ? rg->M : NB * S;
  const size_t wout = (size_t)qd + 2 * kvd;
  // GPT-2 (ModelGPT2.h:23-208): wte + wpe rows, LayerNorm with bias ahead of both products, a bias on every Conv1D, c_fc -> gelu_new;
  // its rotation tables are the identity, so the RoPE / cache-append kernel and the attention are the Llama family's
  if (rg) launch_embed_ragged(c, *rg);
  else TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::embed_rows_any_kernel<DT>, dim3(M), dim3(256), 0, c->stream, (const long long*)c->rows[(size_t)row0].prompt, (const void*)c->embed, (const void*)(c->gpt2 ? c->wpe : nullptr), c->ws_x, H, S, (long long)d.max_ctx, past))
  int pend = 1;                     // slabs of the previous layer's down product still to be added to ws_x (1: none; -1: one whole-K slab, see launch_gemm)
  const bf16_t* pend_bias = nullptr;
  for (int l = 0; l < d.layers; l++) {
    const LayerW& w = c->L[(size_t)l];
    // the QKV product feeds a second rounding (the KV cache): bf16 needs three split terms to reproduce the step path's cache
    // entries (two leave 1-8 % of them one ulp off); fp16's two terms already carry 22 bits
    const bool three = c->dt == tgx::DT_BF16;
    if (c->gpt2) { TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL((tgx::norm_rows_kernel<DT, 1, 1>), dim3(M), dim3(256), 0, c->stream, (const float*)c->ws_x, (const void*)w.in_norm, (const void*)w.in_norm_b, d.norm_eps, H, (float*)nullptr, c->ws_ah, c->ws_al, three ? c->ws_al2 : (bf16_t*)nullptr)) }
    else { TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::rmsnorm_split_kernel<DT>, dim3(M), dim3(256), 0, c->stream, c->ws_x, (const bf16_t*)w.in_norm, d.norm_eps, H, c->ws_ah, c->ws_al, three ? c->ws_al2 : (bf16_t*)nullptr,
                                                  (const float*)(pend != 1 ? c->ws_part : nullptr), std::abs(pend), (long long)M * H, pend_bias)) }
    pend = 1;
    int qsl = 1;
    c->qkv_epi = QkvEpi{};
    if (NB == 1 && !rg) {      // one sequence: the QKV product may finish its rows itself (launch_gemm: gemm_dma_qkv8_kernel<.., ROPE>)
      RowState& r0 = c->rows[(size_t)row0];
      c->qkv_epi.q_hi = c->ws_qh; c->qkv_epi.q_lo = c->ws_ql; c->qkv_epi.past = past; c->qkv_epi.tbl = r0.tbl;
      c->qkv_epi.k = reinterpret_cast<bf16_t*>(r0.kcache) + (size_t)l * kv_layer; c->qkv_epi.v = reinterpret_cast<bf16_t*>(r0.vcache) + (size_t)l * kv_layer;
    }
    launch_gemm(c, tgx::GEMM_STORE, w.wqkv, w.bqkv, c->ws_out, M, qd + 2 * kvd, H, qd + 2 * kvd, /*three_terms=*/three, nullptr, nullptr, /*three_from=*/qd, &qsl);   // Q columns: two terms
    c->qkv_epi = QkvEpi{};
    if (rg) {
      tgx::RopeKvArgs a{};
      a.QKV = c->ws_out; a.q_hi = c->ws_qh; a.q_lo = c->ws_ql;
      if (qsl > 1) { a.QKV = nullptr; a.part = c->ws_part; a.nsplit = qsl; a.slab = (long long)M * (long long)wout; a.bias = reinterpret_cast<const bf16_t*>(w.bqkv); }
      a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin;
      a.heads = d.heads; a.kv_heads = d.kv_heads; a.hd = hd; a.max_ctx = d.max_ctx;
      a.q_norm_w = d.qk_norm ? (const bf16_t*)w.q_norm : nullptr; a.k_norm_w = d.qk_norm ? (const bf16_t*)w.k_norm : nullptr; a.eps = d.norm_eps;
      launch_rope_kv_split_ragged(c, a, *rg, (long long)((size_t)l * kv_layer));
      tgx::AttnPrefillArgs at{};
      at.q_hi = c->ws_qh; at.q_lo = c->ws_ql; at.o_hi = c->ws_ah; at.o_lo = c->ws_al;
      at.heads = d.heads; at.kv_heads = d.kv_heads; at.max_ctx = d.max_ctx; at.scale = 1.0f / sqrtf((float)hd);
      launch_attn_prefill_ragged(c, at, *rg, (long long)((size_t)l * kv_layer), /*allow_lean=*/true);
    }
    for (int b = 0; b < NB && qsl != 0 && !rg; b++) {
      RowState& r = c->rows[(size_t)(row0 + b)];
      bf16_t* kc = reinterpret_cast<bf16_t*>(r.kcache);
      bf16_t* vc = reinterpret_cast<bf16_t*>(r.vcache);
      const size_t ro = (size_t)b * S;             // first workspace row of this batch row
      tgx::RopeKvArgs a{};
      a.QKV = c->ws_out + ro * wout; a.q_hi = c->ws_qh + ro * qd; a.q_lo = c->ws_ql + ro * qd;
      if (qsl > 1) { a.QKV = nullptr; a.part = c->ws_part + ro * wout; a.nsplit = qsl; a.slab = (long long)M * (long long)wout; a.bias = reinterpret_cast<const bf16_t*>(w.bqkv); }
      a.k_cache = kc + (size_t)l * kv_layer; a.v_cache = vc + (size_t)l * kv_layer;
      a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin;
      a.heads = d.heads; a.kv_heads = d.kv_heads; a.hd = hd; a.max_ctx = d.max_ctx; a.past = past; a.blk_tbl = r.tbl;
      a.q_norm_w = d.qk_norm ? (const bf16_t*)w.q_norm : nullptr; a.k_norm_w = d.qk_norm ? (const bf16_t*)w.k_norm : nullptr; a.eps = d.norm_eps;
      launch_rope_kv_split(c, a, S);
    }
    for (int b = 0; b < NB && !rg; b++) {
      RowState& r = c->rows[(size_t)(row0 + b)];
      bf16_t* kc = reinterpret_cast<bf16_t*>(r.kcache);
      bf16_t* vc = reinterpret_cast<bf16_t*>(r.vcache);
      const size_t ro = (size_t)b * S;
      tgx::AttnPrefillArgs a{};
      a.q_hi = c->ws_qh + ro * qd; a.q_lo = c->ws_ql + ro * qd; a.k_cache = kc + (size_t)l * kv_layer; a.v_cache = vc + (size_t)l * kv_layer;
      a.o_hi = c->ws_ah + ro * qd; a.o_lo = c->ws_al + ro * qd; a.S = S; a.heads = d.heads; a.kv_heads = d.kv_heads; a.max_ctx = d.max_ctx; a.past = past;
      a.scale = 1.0f / sqrtf((float)hd); a.qblk_mirror = 1; a.blk_tbl = r.tbl;
      launch_attn_prefill(c, a, /*allow_lean=*/true);
    }
    int osl = 1;
    launch_gemm(c, tgx::GEMM_RESIDUAL, w.wo, w.bo, c->ws_x, M, H, qd, H, false, nullptr, nullptr, 0, c->gpt2 ? nullptr : &osl);
    if (c->gpt2) {
      TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL((tgx::norm_rows_kernel<DT, 1, 1>), dim3(M), dim3(256), 0, c->stream, (const float*)c->ws_x, (const void*)w.post_norm, (const void*)w.post_norm_b, d.norm_eps, H, (float*)nullptr, c->ws_ah, c->ws_al, (bf16_t*)nullptr))
      launch_gemm(c, tgx::GEMM_GELU, w.wgu, w.bfc, nullptr, M, I, H, I);             // c_fc + bias + gelu_new -> ws_hh / ws_hl
    } else {
      const bool fl = gemm_full_lines(c, tgx::GEMM_SILU, M, 2 * I, H);
      bf16_t* const ai = reinterpret_cast<bf16_t*>(c->ws_out);
      TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::rmsnorm_split_kernel<DT>, dim3(M), dim3(256), 0, c->stream, c->ws_x, (const bf16_t*)w.post_norm, d.norm_eps, H, fl ? ai : c->ws_ah, c->ws_al, (bf16_t*)nullptr,
                                                (const float*)(osl != 1 ? c->ws_part : nullptr), std::abs(osl), (long long)M * H, reinterpret_cast<const bf16_t*>(w.bo), fl ? 1 : 0))
      if (fl) launch_gemm(c, tgx::GEMM_SILU, w.wgu, nullptr, nullptr, M, 2 * I, H, 2 * I, false, ai, nullptr, 0, nullptr, true);
      else launch_gemm(c, tgx::GEMM_SILU, w.wgu, nullptr, nullptr, M, 2 * I, H, 2 * I);      // gate_up + siluMul -> ws_hh / ws_hl
    }
    // the down product's slabs wait for the next layer's input norm (the last layer, and GPT-2's LayerNorm path, finish them here)
    const bool can_defer = !c->gpt2 && l + 1 < d.layers;
    launch_gemm(c, tgx::GEMM_RESIDUAL, w.wdown, w.bdown, c->ws_x, M, H, I, H, false, c->ws_hh, c->ws_hl, 0, can_defer ? &pend : nullptr);
    pend_bias = reinterpret_cast<const bf16_t*>(w.bdown);
  }
  if (rg) {
    for (int i = 0; i < rg->n; i++)
      (void)hipMemcpyAsync(c->rows[(size_t)rg->rows[i]].x, c->ws_x + ((size_t)rg->first[i] + rg->lens[i] - 1) * H, (size_t)H * 4, hipMemcpyDeviceToDevice, c->stream);
    return;
  }
  for (int b = 0; b < NB; b++)     // the last position of every batch row feeds lm_head
    (void)hipMemcpyAsync(c->rows[(size_t)(row0 + b)].x, c->ws_x + ((size_t)(b + 1) * S - 1) * H, (size_t)H * 4, hipMemcpyDeviceToDevice, c->stream);
}
void launch_prefill(tgx_ctx* c, int row0, int NB, int S, int past) { prefill_pass(c, row0, NB, S, past, nullptr); }
void launch_prefill_ragged(tgx_ctx* c, const RaggedPass& rg) { prefill_pass(c, 0, 0, 0, 0, &rg); }

// ---- tgx_score_row (include/tgx.h; kernels/score.h): every position's log-probability behind a prompt pass.
// Workspace, all of it through dev_grow and none of it seq x V: the tile partials and target values of one group of positions, the call's output arrays
// (lp | top ids | top lps: ONE read-back) and, for the matrix-core form, the [group rows][vocabulary chunk] fp32 product
static int score_tiles(const tgx_ctx* c) { return (c->d.vocab + tgx::SAMP_TILE - 1) / tgx::SAMP_TILE; }
static int score_chunk(const tgx_ctx* c) { return std::min(c->score_vocab_chunk, score_tiles(c) * tgx::SAMP_TILE); }
int ensure_score_ws(tgx_ctx* c, int seq, bool tiled) {
  const size_t n = (size_t)std::max(0, seq - 1), T = (size_t)score_tiles(c);
  if (!n) return TGX_OK;
  if (T > (size_t)tgx::SAMP_MAX_WG) return set_err(c, TGX_ERR_UNSUPPORTED, "vocabulary %d exceeds the sampler's %d entries", c->d.vocab, tgx::SAMP_MAX_WG * tgx::SAMP_TILE);
  const size_t rows = tiled ? std::min<size_t>((size_t)c->score_rows, n) : (size_t)tgx_ctx::VERIFY_ROWS;
  int rc;
  if ((rc = dev_grow(c, &c->sc_part, &c->sc_part_bytes, rows * T * (8 + 8 * tgx::LP_MAX + 4) + rows * 4))) return rc;
  if ((rc = dev_grow(c, &c->sc_out, &c->sc_out_bytes, n * (1 + 2 * (size_t)tgx::LP_MAX) * 4))) return rc;
  if (tiled && (rc = dev_grow(c, &c->sc_logits, &c->sc_logits_bytes, rows * (size_t)score_chunk(c) * 4))) return rc;
  c->sc_part_rows = (int)rows;
  return TGX_OK;
}
static tgx::ScoreArgs score_args(tgx_ctx* c, const ScoreCall& sc, int pos0) {
  const size_t R = (size_t)c->sc_part_rows, T = (size_t)score_tiles(c), n = (size_t)sc.n_score;
  tgx::ScoreArgs a{};
  a.V = c->d.vocab; a.nwg = (int)T; a.top_n = sc.top_n; a.ids = sc.ids; a.pos0 = pos0; a.n_score = sc.n_score;
  a.tile_sum = reinterpret_cast<double*>(c->sc_part);
  a.tile_keys = reinterpret_cast<unsigned long long*>(c->sc_part + R * T * 8);
  a.tile_max = reinterpret_cast<float*>(c->sc_part + R * T * (8 + 8 * tgx::LP_MAX));
  a.tgt = a.tile_max + R * T;
  a.out_lp = reinterpret_cast<float*>(c->sc_out); a.out_ids = reinterpret_cast<int*>(a.out_lp + n); a.out_top_lp = a.out_lp + n + n * tgx::LP_MAX;
  return a;
}
// the tile launch over a block of R positions from pos0: `width` vocabulary entries from col0 (a multiple of the tile) per position, `stride` floats apart
void launch_score_tiles(tgx_ctx* c, const ScoreCall& sc, const float* logits, long long stride, int col0, int width, int R, int pos0) {
  if (R > c->sc_part_rows || col0 % tgx::SAMP_TILE) { c->launch_fault = "score: a block the workspace was not sized for"; return; }
  tgx::ScoreArgs a = score_args(c, sc, pos0);
  a.logits = logits; a.stride = stride; a.col0 = col0;
  hipLaunchKernelGGL(tgx::score_tile_kernel, dim3((width + tgx::SAMP_TILE - 1) / tgx::SAMP_TILE, R), dim3(tgx::SAMP_WG), 0, c->stream, a);
}
// ... and, behind the tile launches of all the vocabulary, the group's records
void launch_score_record(tgx_ctx* c, const ScoreCall& sc, int R, int pos0) {
  if (R > c->sc_part_rows) { c->launch_fault = "score: a block the workspace was not sized for"; return; }
  const tgx::ScoreArgs a = score_args(c, sc, pos0);
  hipLaunchKernelGGL(tgx::score_record_kernel, dim3(1, R), dim3(tgx::SAMP_WG), 0, c->stream, a);
}
// The matrix-core form, behind prefill_pass over ws_x (one sequence): groups of <= score.rows positions; per group the final norm into 16-bit terms, then per
// vocabulary chunk ONE product against that slice of the lm_head rows (the plain matrix; `embed` when tied) and the tile launch over it.  The product is pinned to
// ONE kernel form — gemm_dma_kernel, 128-row tiles, unsplit K — called directly, not through launch_gemm's tile-count heuristics: a logit is the same K-ordered
// sum (per k16 step the lo term, then the hi term) whatever the group and chunk sizes, so the scores are the same bits for every legal option value.
// The weights stream once per group.
void launch_score_tiled(tgx_ctx* c, const ScoreCall& sc) {
  const tgx_model_desc& d = c->d;
  const int H = d.hidden, V = d.vocab, chunk = score_chunk(c);
  const bf16_t* W = reinterpret_cast<const bf16_t*>(d.tied ? c->embed : c->lm_head);
  if (H % 64 != 0 || !c->sc_logits) { c->launch_fault = "score: the matrix-core form needs hidden % 64 == 0 and its workspace"; return; }
  const bool one = c->act16 && c->ws_zero;
  const size_t lds = tgx::gemm_dma_lds_bytes(2, false, 32, 2);
  for (int g0 = 0; g0 < sc.n_score; g0 += c->sc_part_rows) {
    const int R = std::min(c->sc_part_rows, sc.n_score - g0);
    float* x = c->ws_x + (size_t)g0 * H;
    if (c->gpt2) { TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL((tgx::norm_rows_kernel<DT, 1, 1>), dim3(R), dim3(256), 0, c->stream, (const float*)x, (const void*)c->final_norm, (const void*)c->final_norm_b, d.norm_eps, H, (float*)nullptr, c->ws_ah, c->ws_al, (bf16_t*)nullptr)) }
    else { TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL(tgx::rmsnorm_split_kernel<DT>, dim3(R), dim3(256), 0, c->stream, x, (const bf16_t*)c->final_norm, d.norm_eps, H, c->ws_ah, c->ws_al, (bf16_t*)nullptr, (const float*)nullptr, 0, 0LL, (const bf16_t*)nullptr, 0)) }
    for (int n0 = 0; n0 < V; n0 += chunk) {
      const int N = std::min(chunk, V - n0);
      tgx::GemmArgs g{};
      g.A_hi = c->ws_ah; g.A_lo = one ? c->ws_zero : c->ws_al; g.A_lo2 = nullptr;
      g.B = W + (size_t)n0 * H; g.bias = nullptr; g.C = c->sc_logits; g.M = R; g.N = N; g.K = H; g.ldc = chunk; g.three_from = 0;
      const dim3 grid((N + tgx::GBN - 1) / tgx::GBN, (R + 127) / 128), blk(256);
      TGX_DT16_SWITCH(c->dt, hipLaunchKernelGGL((tgx::gemm_dma_kernel<DT, tgx::GEMM_STORE, 2, 32, 2>), grid, blk, lds, c->stream, g))
      launch_score_tiles(c, sc, c->sc_logits, chunk, n0, N, R, g0);
    }
    launch_score_record(c, sc, R, g0);
  }
}

// dynamic LDS sizes of the tiled GEMMs
int prefill_set_attrs(tgx_ctx* c) {
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_x2_kernel<tgx::DT_BF16, tgx::GEMM_PARTIAL, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, tgx::GBM * tgx::GLD * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_x2_kernel<tgx::DT_F16, tgx::GEMM_PARTIAL, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, tgx::GBM * tgx::GLD * 2));
#define TGX_DMA_ATTR1(DT_, EPI_, MI_, BK_, NS_) HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma_kernel<DT_, EPI_, MI_, BK_, NS_>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::min<size_t>(160 * 1024, tgx::gemm_dma_lds_bytes(MI_, true, BK_, NS_))));
#define TGX_DMA_ATTR(DT_, EPI_, MI_) TGX_DMA_ATTR1(DT_, EPI_, MI_, ((MI_) == 1 ? 64 : 32), 2)
#define TGX_DMA_ATTR_D(DT_) TGX_DMA_ATTR(DT_, tgx::GEMM_SILU, 2) TGX_DMA_ATTR(DT_, tgx::GEMM_GELU, 2) TGX_DMA_ATTR(DT_, tgx::GEMM_RESIDUAL, 1) TGX_DMA_ATTR(DT_, tgx::GEMM_RESIDUAL, 2) TGX_DMA_ATTR(DT_, tgx::GEMM_STORE, 1) TGX_DMA_ATTR(DT_, tgx::GEMM_STORE, 2)
  TGX_DMA_ATTR_D(tgx::DT_BF16) TGX_DMA_ATTR_D(tgx::DT_F16)
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8n_kernel<tgx::DT_BF16>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (2 * 128 + 256) * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8n_kernel<tgx::DT_F16>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (2 * 128 + 256) * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma_qkv8_kernel<tgx::DT_BF16, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (3 * 128 + 128 + 64) * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma_qkv8_kernel<tgx::DT_F16, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (3 * 128 + 128 + 64) * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma_qkv8_kernel<tgx::DT_BF16>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (3 * 128 + 128 + 64) * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma_qkv8_kernel<tgx::DT_F16>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (3 * 128 + 128 + 64) * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8i_kernel<tgx::DT_BF16, tgx::GEMM_SILU>), hipFuncAttributeMaxDynamicSharedMemorySize, 5 * 256 * 128));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8i_kernel<tgx::DT_F16, tgx::GEMM_SILU>), hipFuncAttributeMaxDynamicSharedMemorySize, 5 * 256 * 128));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::attn_prefill_kernel<tgx::DT_BF16, 128, 1, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (64 * 136 + 64 * 160) * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::attn_prefill_kernel<tgx::DT_BF16, 128, 1, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (64 * 136 + 64 * 160) * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::attn_prefill_kernel<tgx::DT_F16, 128, 1, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (64 * 136 + 64 * 160) * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::attn_prefill_kernel<tgx::DT_F16, 128, 1, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (64 * 136 + 64 * 160) * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::attn_prefill_rg_kernel<tgx::DT_BF16, 128, 1, 2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (64 * 136 + 64 * 160) * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::attn_prefill_rg_kernel<tgx::DT_BF16, 128, 1, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (64 * 136 + 64 * 160) * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::attn_prefill_rg_kernel<tgx::DT_F16, 128, 1, 2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (64 * 136 + 64 * 160) * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::attn_prefill_rg_kernel<tgx::DT_F16, 128, 1, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (64 * 136 + 64 * 160) * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_BF16, tgx::GEMM_SILU>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_F16, tgx::GEMM_SILU>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_BF16, tgx::GEMM_RESIDUAL>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_BF16, tgx::GEMM_STORE>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_F16, tgx::GEMM_RESIDUAL>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_F16, tgx::GEMM_STORE>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_BF16, tgx::GEMM_RESIDUAL>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_BF16, tgx::GEMM_STORE>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_F16, tgx::GEMM_RESIDUAL>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_F16, tgx::GEMM_STORE>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_BF16, tgx::GEMM_SILU>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_BF16, tgx::GEMM_GELU>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_F16, tgx::GEMM_SILU>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_F16, tgx::GEMM_GELU>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  // split-K slabs on the eight-wave kernel
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_BF16, tgx::GEMM_PARTIAL, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_BF16, tgx::GEMM_PARTIAL, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_F16, tgx::GEMM_PARTIAL, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_F16, tgx::GEMM_PARTIAL, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  // option act.round16: the one-term forms
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_BF16, tgx::GEMM_SILU, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_BF16, tgx::GEMM_SILU, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_BF16, tgx::GEMM_RESIDUAL, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_BF16, tgx::GEMM_RESIDUAL, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_BF16, tgx::GEMM_STORE, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_BF16, tgx::GEMM_STORE, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_F16, tgx::GEMM_SILU, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_F16, tgx::GEMM_SILU, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_F16, tgx::GEMM_RESIDUAL, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_F16, tgx::GEMM_RESIDUAL, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8k_kernel<tgx::DT_F16, tgx::GEMM_STORE, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 128 * 64 * 2));
  HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::gemm_dma8_kernel<tgx::DT_F16, tgx::GEMM_STORE, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 256 * 32 * 2));
#define TGX_DMA_ATTR_P(DT_) TGX_DMA_ATTR1(DT_, tgx::GEMM_PARTIAL, 1, 64, 2) TGX_DMA_ATTR1(DT_, tgx::GEMM_PARTIAL, 2, 64, 2) TGX_DMA_ATTR1(DT_, tgx::GEMM_PARTIAL, 2, 32, 2)
  TGX_DMA_ATTR_P(tgx::DT_BF16) TGX_DMA_ATTR_P(tgx::DT_F16)
#undef TGX_DMA_ATTR_P
#undef TGX_DMA_ATTR_D
#undef TGX_DMA_ATTR
#undef TGX_DMA_ATTR1
  return TGX_OK;
}

// ---- tgx_embed_rows (include/tgx.h; kernels/embed_pool.h): the pooled final-norm hidden state of every text behind its prompt pass.
// Workspace, all of it through dev_grow: em_buf = the text table | out [n][dims] | partials [slices][H]; em_stage = one slice of rows for prefill by steps
int ensure_embed_ws(tgx_ctx* c, EmbedCall& em) {
  const size_t H = (size_t)c->d.hidden, al = 32;
  const size_t tab = ((size_t)em.n * sizeof(tgx::EmbedText) + al - 1) / al * al, out = ((size_t)em.n * (size_t)em.dims * 4 + al - 1) / al * al;
  if (int rc = dev_grow(c, &c->em_buf, &c->em_bytes, tab + out + (size_t)em.slices * H * 4)) return rc;
  if (int rc = dev_grow(c, &c->em_stage, &c->em_stage_bytes, (size_t)tgx::EMB_SLICE * H * 4)) return rc;
  c->em_off_out = tab; c->em_off_part = tab + out;
  c->embed_last_launches = 0;
  return TGX_OK;
}
int embed_upload_table(tgx_ctx* c, const EmbedCall& em) {
  static_assert(sizeof(tgx::EmbedText) == 16, "EmbedCall::tab holds four ints per text");
  static_assert(EmbedCall::SLICE == tgx::EMB_SLICE, "the host lays the partials out by the kernel's slice");
  HIP_OK(c, hipMemcpyAsync(c->em_buf, em.tab.data(), (size_t)em.n * sizeof(tgx::EmbedText), hipMemcpyHostToDevice, c->stream));
  return TGX_OK;
}
static tgx::EmbedPoolArgs embed_pool_args(tgx_ctx* c, int t0) {
  tgx::EmbedPoolArgs a{};
  a.x = c->ws_x; a.tab = reinterpret_cast<const tgx::EmbedText*>(c->em_buf); a.part = reinterpret_cast<float*>(c->em_buf + c->em_off_part);
  a.norm_w = c->final_norm; a.norm_b = c->gpt2 ? c->final_norm_b : nullptr; a.eps = c->d.norm_eps; a.H = c->d.hidden;
  a.act16 = c->act16 && c->dt != tgx::DT_F32 ? 1 : 0;
  a.t0 = t0; a.stage_slice = -1; a.stage_cnt = 0;
  return a;
}
static void launch_embed_pool_grid(tgx_ctx* c, const tgx::EmbedPoolArgs& a, dim3 grid) {
  if (c->gpt2) { TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL((tgx::embed_pool_kernel<DT, 1>), grid, dim3(tgx::EMB_WG), 0, c->stream, a)) }
  else { TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL((tgx::embed_pool_kernel<DT, 0>), grid, dim3(tgx::EMB_WG), 0, c->stream, a)) }
  c->embed_last_launches++;
}
void launch_embed_pool(tgx_ctx* c, const EmbedCall& em, int t0, int nt) {
  if (!c->em_buf || !c->ws_x || t0 < 0 || nt < 1 || t0 + nt > em.n) { c->launch_fault = "embed: a pass the workspace was not sized for"; return; }
  int most = 1;
  for (int t = t0; t < t0 + nt; t++) most = std::max(most, em.np(t));
  launch_embed_pool_grid(c, embed_pool_args(c, t0), dim3((unsigned)((most + tgx::EMB_SLICE - 1) / tgx::EMB_SLICE), (unsigned)nt));
}
void launch_embed_pool_stage(tgx_ctx* c, const EmbedCall& em, int t, int slice, int cnt) {
  if (!c->em_buf || !c->em_stage || t < 0 || t >= em.n || cnt < 1 || cnt > tgx::EMB_SLICE || slice < 0 || slice * tgx::EMB_SLICE + cnt > em.np(t)) {
    c->launch_fault = "embed: a slice the workspace was not sized for"; return;
  }
  tgx::EmbedPoolArgs a = embed_pool_args(c, t);
  a.x = c->em_stage; a.stage_slice = slice; a.stage_cnt = cnt;
  launch_embed_pool_grid(c, a, dim3(1, 1));
}
int launch_embed_finish(tgx_ctx* c, const EmbedCall& em) {
  tgx::EmbedFinishArgs a{};
  a.tab = reinterpret_cast<const tgx::EmbedText*>(c->em_buf); a.part = reinterpret_cast<const float*>(c->em_buf + c->em_off_part);
  a.out = reinterpret_cast<float*>(c->em_buf + c->em_off_out); a.H = c->d.hidden; a.dims = em.dims; a.normalize = em.normalize;
  hipLaunchKernelGGL(tgx::embed_finish_kernel, dim3((unsigned)em.n), dim3(tgx::EMB_WG), 0, c->stream, a);
  c->embed_last_launches++;
  HIP_OK(c, hipMemcpyAsync(em.host_out, a.out, (size_t)em.n * (size_t)em.dims * 4, hipMemcpyDeviceToHost, c->stream));
  return TGX_OK;
}
