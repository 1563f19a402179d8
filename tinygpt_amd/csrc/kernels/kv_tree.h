// kv_tree.h — the compaction behind tgx_verify_tree (include/tgx.h).  The pass wrote position p of the token tree to cache slot past + p; the accept launch
// (kernels/verify.h) took the branch path[0 .. n), path[0] = 0 < path[1] < .. .  This launch, stream-ordered behind it, moves the accepted inputs' K / V rows of every
// layer from slot past + path[j] to slot past + j, bit for bit: the row then holds positions [0, past + n) contiguously, as n decode steps leave it.  K needs no
// second rotation: position path[j] stands at depth j of its branch and was rotated for past + j when it was appended (prefill.h rope_kv_split_tree_kernel).
//
// path and n are read from the device: the host does not know them when it enqueues the launch.  path[j] >= j, and the moves overlap (path 0, 2, 3 moves 2 -> 1 and
// 3 -> 2), so nothing may be stored before everything is loaded.  A workgroup owns one (layer, kv head, K | V) span: each thread loads at most one 16-byte chunk of one
// moved row into a register, the workgroup passes a barrier, then the chunks are stored.  No other workgroup touches the span, nothing is handed between workgroups.
// n <= 1, or a path already in place (path[j] == j), moves nothing.
#pragma once
#include "common.h"

namespace tgx {

struct KvTreeArgs {
  bf16_t *k, *v;               // layer 0 of the row's cache (slab KV) or of the pools (paged KV)
  long long layer_stride;      // elements from one layer to the next
  const int* tbl;              // paged KV: the row's block table, else nullptr
  const int* path;             // [VERIFY_MAX_POS] the accept launch's path (device)
  const VerifyRecord* rec;     // its record: n
  int kv_heads, hd, max_ctx, past, M;
};

// grid (layers * kv_heads, 2): blockIdx.y 0 = K, 1 = V.  256 threads >= 15 rows x hd / 8 chunks (hd <= 128)
__global__ __launch_bounds__(256) void kv_tree_compact_kernel(const KvTreeArgs a) {
  const int n = min(a.rec->n, a.M);
  if (n <= 1) return;                                  // (workgroup-uniform: ahead of the barrier)
  const int ch = a.hd >> 3;                            // 16-byte chunks per row
  const int layer = blockIdx.x / a.kv_heads, kvh = blockIdx.x - layer * a.kv_heads;
  bf16_t* const base = (blockIdx.y ? a.v : a.k) + (size_t)layer * a.layer_stride;
  const int j = 1 + (int)threadIdx.x / ch, cc = (int)threadIdx.x - (j - 1) * ch;
  bool mine = false;
  int src = 0;
  if (j < n) {
    src = min(max(a.path[j], j), a.M - 1);             // (the walk's positions ascend: path[j] >= j; the clamp keeps a damaged table inside the pass's slots)
    mine = src != j;
  }
  auto slot_off = [&](int t) -> size_t { return a.tbl ? kv_paged_off(a.tbl, a.kv_heads, kvh, t, a.hd) : ((size_t)kvh * a.max_ctx + t) * (size_t)a.hd; };
  u32x4 val = u32x4{0u, 0u, 0u, 0u};
  if (mine) val = *reinterpret_cast<const u32x4*>(base + slot_off(a.past + src) + cc * 8);
  __syncthreads();                                     // every moved row is in registers before the first store
  if (mine) *reinterpret_cast<u32x4*>(base + slot_off(a.past + j) + cc * 8) = val;
}

}  // namespace tgx
