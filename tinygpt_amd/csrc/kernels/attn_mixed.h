// attn_mixed.h — the attention of a MIXED ragged pass (tgx_advance_rows): prompt chunks of several query blocks and one-token steps over long contexts in one
// work list whose items carry a key range.
//
// A ragged pass so far was either all work-list (prefill.h attn_prefill_rg_kernel: one workgroup walks every key tile of its query block) or all key-split
// (attn_extend.h attn_extend_rg_kernel: every sequence one query block).  In a mix the first form makes a one-token row over a 4096-token context one workgroup of
// 65 serial tiles, and the second does not take a 200-token chunk at all.  Here the host (csrc/attn_worklist.h) cuts every query block whose causal key range
// exceeds a tile target into <= 32 contiguous ranges of 64-key tiles:
//   whole blocks   stay items of attn_prefill_rg_kernel (prefill.hip launches it over them unchanged: the same per-workgroup code, the same bits)
//   ranges         attn_mixed_split_kernel: one workgroup per (sequence, query block, head, range) runs attn_prefill_wg<.., SPLIT> over its tiles [t0, t1) and
//                  leaves attn_extend.h's unnormalised partial (O, m, l) per query in ITS slot of the partial area — the area is per (sequence, query block),
//                  not per sequence as in attn_extend_rg_kernel
//   merge          attn_mixed_merge_kernel: one workgroup per (split block, head) walks the block's partials IN SPLIT ORDER (slot, slot + heads, ..) — the result
//                  does not depend on which workgroup finished first: the same bits from run to run — and emits through attn_emit_rows
// Range boundaries are tile boundaries, so a tile never straddles a 128-token page.  A range may hold no visible key for an early query of its block: its partial
// is (0, -inf, 0) and merges to nothing (attn_extend.h).  Waves whose 32 queries lie beyond the sequence write and merge nothing.
#pragma once
#include "attn_extend.h"

namespace tgx {

struct MixItem { int seq, qblk, h, t0, t1, split, nsplit, slot; };      // csrc/attn_worklist.h Item, field for field
struct AttnMixArgs {
  AttnRgArgs r;               // the pass's q / o terms from its first workspace row; the sequences' table (r.item unused)
  const MixItem* items;       // this launch's list
  float* part;                // [slots][attn_extend_part_vals][256]
};

template <int HD>
__device__ __forceinline__ AttnPrefillArgs attn_mixed_seq(const AttnMixArgs& e, const MixItem& it) {
  const RgItem ri{it.seq, it.qblk, it.h, 0};
  return attn_rg_args<HD>(e.r, ri);
}

template <int DT, int HD, bool PAGED>
__global__ __launch_bounds__(256, HD == 64 ? 1 : 2) void attn_mixed_split_kernel(const AttnMixArgs e) {
  constexpr int LA = HD == 64 ? 2 : 1;      // the look-ahead of the prompt attention's default forms
  const MixItem it = e.items[blockIdx.x];
  const AttnPrefillArgs a = attn_mixed_seq<HD>(e, it);
  float* const part = e.part + (size_t)it.slot * (size_t)(attn_extend_part_vals<HD>() * 256);
  attn_prefill_wg<DT, HD, LA, 1, PAGED, true>(a, it.h, it.qblk, it.t0, it.t1, part);
}

template <int DT, int HD>
__global__ __launch_bounds__(256) void attn_mixed_merge_kernel(const AttnMixArgs e) {
  constexpr int NB = HD / 32, NV = attn_extend_part_vals<HD>();
  __shared__ __attribute__((aligned(16))) bf16_t stage[4 * 32 * (HD + 4)];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const MixItem it = e.items[blockIdx.x];
  const AttnPrefillArgs a = attn_mixed_seq<HD>(e, it);
  const int q0 = it.qblk * ATTN_QBLK + wv * 32;
  if (q0 >= a.S) return;                     // wave-uniform; no barrier below
  const bool qvalid = q0 + (lane & 31) < a.S;
  const size_t split_stride = (size_t)a.heads * (NV * 256);
  const float* pi = e.part + (size_t)it.slot * (NV * 256) + tid;
  f32x16 oacc[NB];
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int r = 0; r < 16; r++) oacc[b][r] = pi[(b * 16 + r) * 256];
  float m_run = pi[(NB * 16) * 256], l_run = pi[(NB * 16 + 1) * 256];
  for (int s = 1; s < it.nsplit; s++) {
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
  attn_emit_rows<DT, HD>(a, it.h, q0, qvalid, oacc, l_run, stage + wv * 32 * (HD + 4), lane);
}

}  // namespace tgx
