// attn_extend.h — key-split attention of a continuation (tgx_extend_row): ONE query block (S <= 128 new positions of one sequence) against the keys [0, past + S).
//
// The prompt attention (prefill.h attn_prefill_kernel) gives such a pass one workgroup per head, which walks every key tile in sequence: 30 tokens over a 4096-token
// history on 32 heads are 32 workgroups of 65 tiles each on a 256-CU chip.  Here the grid is (heads, NS): workgroup (h, s) runs the SAME tile pipeline
// (attn_prefill_wg<.., SPLIT>: S^T = K.Q^T on the matrix cores, lane-local online softmax, transposing LDS read for V, Q as hi / lo terms, causal mask by index
// against past + qi) over its own contiguous range of 64-key tiles and leaves an unnormalised fp32 partial (O[hd], m, l) per query.  Split boundaries are tile
// boundaries, so a tile never straddles a 128-token page.  A second launch merges the NS partials of every (query, head) IN SPLIT ORDER — the result does not depend
// on which workgroup finished first, so it is bit-reproducible from run to run — and emits the rows through the prompt attention's own epilogue (attn_emit_rows):
// the same o_hi / o_lo terms in the same layout, so the o_proj product behind it is unchanged.
//
// A split may hold no visible key for a query (an early query whose causal range ends before the split begins): its partial is (0, -inf, 0), whose merge factor is
// exp2(-inf) = 0 — it contributes exactly nothing.  Waves whose 32 queries all lie beyond S write and merge nothing.
//
// Partials: part[split][head][value][256 lanes], value = attn_extend_part_vals<HD>() floats (the O registers in register order, m, l); a lane of the merge kernel
// reads what the same lane of the split workgroup wrote, 256 contiguous bytes per wave and value.
#pragma once
#include "prefill.h"

namespace tgx {

struct AttnExtendArgs {
  AttnPrefillArgs a;
  float* part;
  int ns, n_tiles;      // 1 <= ns <= n_tiles = (past + S - 1) / 64 + 1
};

// tiles [t0, t1) of split s: contiguous, the first n_tiles % ns splits hold one more
template <int DT, int HD, bool PAGED>
__global__ __launch_bounds__(256, HD == 64 ? 1 : 2) void attn_extend_kernel(const AttnExtendArgs e) {
  constexpr int LA = HD == 64 ? 2 : 1;      // the look-ahead of the prompt attention's default forms
  const int h = blockIdx.x, s = blockIdx.y;
  const int base = e.n_tiles / e.ns, rem = e.n_tiles - base * e.ns;
  const int t0 = s * base + min(s, rem), t1 = t0 + base + (s < rem ? 1 : 0);
  float* const part = e.part + ((size_t)s * e.a.heads + h) * (size_t)(attn_extend_part_vals<HD>() * 256);
  attn_prefill_wg<DT, HD, LA, 1, PAGED, true>(e.a, h, 0, t0, t1, part);
}

// ... of a token tree (tgx_verify_tree): the same splits under the tree mask (prefill.h TREE); attn_extend_merge_kernel merges them as they are
struct AttnExtendTreeArgs { AttnExtendArgs e; const unsigned short* anc; };
template <int DT, int HD, bool PAGED>
__global__ __launch_bounds__(256, HD == 64 ? 1 : 2) void attn_extend_tree_kernel(const AttnExtendTreeArgs t) {
  constexpr int LA = HD == 64 ? 2 : 1;
  const AttnExtendArgs& e = t.e;
  const int h = blockIdx.x, s = blockIdx.y;
  const int base = e.n_tiles / e.ns, rem = e.n_tiles - base * e.ns;
  const int t0 = s * base + min(s, rem), t1 = t0 + base + (s < rem ? 1 : 0);
  float* const part = e.part + ((size_t)s * e.a.heads + h) * (size_t)(attn_extend_part_vals<HD>() * 256);
  attn_prefill_wg<DT, HD, LA, 1, PAGED, true, true>(e.a, h, 0, t0, t1, part, t.anc);
}

template <int DT, int HD>
__global__ __launch_bounds__(256) void attn_extend_merge_kernel(const AttnExtendArgs e) {
  constexpr int NB = HD / 32, NV = attn_extend_part_vals<HD>();
  __shared__ __attribute__((aligned(16))) bf16_t stage[4 * 32 * (HD + 4)];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = blockIdx.x;
  const int q0 = wv * 32;
  if (q0 >= e.a.S) return;                   // wave-uniform; no barrier below
  const bool qvalid = q0 + (lane & 31) < e.a.S;
  const float* pi = e.part + (size_t)h * (NV * 256) + tid;
  const size_t split_stride = (size_t)e.a.heads * (NV * 256);
  f32x16 oacc[NB];
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int r = 0; r < 16; r++) oacc[b][r] = pi[(b * 16 + r) * 256];
  float m_run = pi[(NB * 16) * 256], l_run = pi[(NB * 16 + 1) * 256];
  for (int s = 1; s < e.ns; s++) {
    pi += split_stride;
    const float m_b = pi[(NB * 16) * 256], l_b = pi[(NB * 16 + 1) * 256];
    const float m_new = fmaxf(m_run, m_b);
    const bool dead = m_new == -INFINITY;      // nothing attended in either part (a padded query)
    const float fa = dead ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new), fb = dead ? 1.f : __builtin_amdgcn_exp2f(m_b - m_new);
    l_run = l_run * fa + l_b * fb;
    m_run = m_new;
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) oacc[b][r] = oacc[b][r] * fa + pi[(b * 16 + r) * 256] * fb;
  }
  attn_emit_rows<DT, HD>(e.a, h, q0, qvalid, oacc, l_run, stage + wv * 32 * (HD + 4), lane);
}

// ---- the ragged form (tgx_verify_rows): the continuations of SEVERAL sequences (each one query block, S_i <= 128, from its own past_i) in one launch pair.
// Grid (heads, NS, sequences).  Sequence i has n_tiles_i = (past_i + S_i - 1) / 64 + 1 key tiles and uses ns_i = min(NS, n_tiles_i) splits with attn_extend_kernel's
// contiguous partition; a workgroup whose split >= ns_i leaves before any barrier.  Partials: part[seq][split][head][value][256].  The merge walks the ns_i partials
// of its sequence in split order (the same bits from run to run) and emits at the sequence's workspace rows.
struct AttnExtendRgArgs {
  AttnRgArgs r;          // the pass's q / o terms from its first workspace row; the sequences' table (item unused)
  float* part;
  int ns;                // NS >= 1
};
// the sequence's arguments, its split count and (split kernel) this split's tiles
template <int HD>
__device__ __forceinline__ AttnPrefillArgs attn_extend_rg_seq(const AttnExtendRgArgs& e, const int j, const int h, int& ns_j, int& n_tiles) {
  const RgItem it{j, 0, h, 0};
  const AttnPrefillArgs a = attn_rg_args<HD>(e.r, it);
  n_tiles = (a.past + a.S - 1) / ATTN_KTILE + 1;
  ns_j = min(e.ns, n_tiles);
  return a;
}
template <int DT, int HD, bool PAGED>
__global__ __launch_bounds__(256, HD == 64 ? 1 : 2) void attn_extend_rg_kernel(const AttnExtendRgArgs e) {
  constexpr int LA = HD == 64 ? 2 : 1;
  const int h = blockIdx.x, s = blockIdx.y, j = blockIdx.z;
  int ns_j, n_tiles;
  const AttnPrefillArgs a = attn_extend_rg_seq<HD>(e, j, h, ns_j, n_tiles);
  if (s >= ns_j) return;                     // workgroup-uniform; no barrier above
  const int base = n_tiles / ns_j, rem = n_tiles - base * ns_j;
  const int t0 = s * base + min(s, rem), t1 = t0 + base + (s < rem ? 1 : 0);
  float* const part = e.part + (((size_t)j * e.ns + s) * a.heads + h) * (size_t)(attn_extend_part_vals<HD>() * 256);
  attn_prefill_wg<DT, HD, LA, 1, PAGED, true>(a, h, 0, t0, t1, part);
}

template <int DT, int HD>
__global__ __launch_bounds__(256) void attn_extend_rg_merge_kernel(const AttnExtendRgArgs e) {
  constexpr int NB = HD / 32, NV = attn_extend_part_vals<HD>();
  __shared__ __attribute__((aligned(16))) bf16_t stage[4 * 32 * (HD + 4)];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = blockIdx.x, j = blockIdx.y;
  int ns_j, n_tiles;
  const AttnPrefillArgs a = attn_extend_rg_seq<HD>(e, j, h, ns_j, n_tiles);
  const int q0 = wv * 32;
  if (q0 >= a.S) return;                     // wave-uniform; no barrier below
  const bool qvalid = q0 + (lane & 31) < a.S;
  const size_t split_stride = (size_t)a.heads * (NV * 256);
  const float* pi = e.part + (size_t)j * e.ns * split_stride + (size_t)h * (NV * 256) + tid;
  f32x16 oacc[NB];
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int r = 0; r < 16; r++) oacc[b][r] = pi[(b * 16 + r) * 256];
  float m_run = pi[(NB * 16) * 256], l_run = pi[(NB * 16 + 1) * 256];
  for (int s = 1; s < ns_j; s++) {
    pi += split_stride;
    const float m_b = pi[(NB * 16) * 256], l_b = pi[(NB * 16 + 1) * 256];
    const float m_new = fmaxf(m_run, m_b);
    const bool dead = m_new == -INFINITY;      // nothing attended in either part (a padded query)
    const float fa = dead ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new), fb = dead ? 1.f : __builtin_amdgcn_exp2f(m_b - m_new);
    l_run = l_run * fa + l_b * fb;
    m_run = m_new;
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) oacc[b][r] = oacc[b][r] * fa + pi[(b * 16 + r) * 256] * fb;
  }
  attn_emit_rows<DT, HD>(a, h, q0, qvalid, oacc, l_run, stage + wv * 32 * (HD + 4), lane);
}

}  // namespace tgx
