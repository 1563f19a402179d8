// kv_fork.h — the copy launch of tgx_fork_row (include/tgx.h): ONE launch carries, for all layers, both caches and all destinations of a call, the cache
// positions a fork cannot share, and beside them the per-row state that makes a destination row equal its source.
//
// The cache part is typeless bytes.  A cache is made of SPANS, one per (layer, kv head): span_vecs vectors of contiguous bytes that hold the positions [0, n_tok) of that head
//   slab cache   [layer][kv_head][max_ctx][hd] inside a row's slab:          id = the batch row,      n_tok = past          (the whole prefix)
//   paged cache  [layer][block][kv_head][KV_BLOCK][hd] inside the layer pool: id = the physical block, n_tok = past % KV_BLOCK (the partial tail block; the full
//                blocks are shared by reference, abi.hip)
// and the byte offset of span s of `id` is id * id_stride + (s / kv_heads) * layer_stride + (s % kv_heads) * head_stride.  Every thread loads UNROLL vectors of the
// source (16 bytes each; 4 where head_dim * element size is no multiple of 16) before it stores them to each of the n destinations: the source is read once, the loads
// of a wave are contiguous 1 KiB runs, and the destination ids arrive by value in the kernel arguments.  Positions >= n_tok are not carried.  The grid is 2-D: a grid
// row (blockIdx.y) walks whole spans, so a span's address is worked out once per span and the inner loop is adds only; blockIdx.x strides inside the span.
//
// The state part moves six words-or-vectors per destination row in 4-byte units (a vocabulary need not be a multiple of four floats): hidden row, logits, argmax
// partials, position word, token word.  It runs in the grid rows behind the cache part's.
#pragma once
#include "common.h"

namespace tgx {

constexpr int KV_FORK_MAX_DST = 128;   // destinations one launch carries by value (a call with more takes one launch per 128)
constexpr int KV_FORK_THREADS = 256;
constexpr int KV_FORK_UNROLL = 4;      // loads in flight per thread before the first store
constexpr int KV_FORK_SEGS = 6;

struct KvForkSeg { unsigned char* base; long long row_stride; int words; };   // a per-row array: `words` dwords at base + row * row_stride (bytes)

struct KvForkArgs {
  unsigned char *k, *v;                   // slab cache: slab_k / slab_v; paged: the pools
  long long id_stride, layer_stride, head_stride;   // bytes
  long long span_vecs;                    // vectors per span that hold positions [0, n_tok)
  int n_spans, kv_heads;                  // spans per cache = layers * kv_heads
  int kv_rows;                            // grid rows (blockIdx.y) of the cache part; 0: nothing to copy.  The rows behind them carry the per-row state
  int n_dst, src_id, src_row;
  int dst_id[KV_FORK_MAX_DST];            // slab: rows; paged: tail blocks
  int dst_row[KV_FORK_MAX_DST];
  KvForkSeg seg[KV_FORK_SEGS];
};

template <typename VEC>
__global__ __launch_bounds__(KV_FORK_THREADS) void kv_fork_kernel(const KvForkArgs a) {
  if ((int)blockIdx.y < a.kv_rows) {
    const long long step = (long long)gridDim.x * KV_FORK_THREADS;      // vectors one round of the row's workgroups covers
    for (int s = (int)blockIdx.y; s < 2 * a.n_spans; s += a.kv_rows) {    // K spans, then V spans
      const bool isv = s >= a.n_spans;
      const int sp = isv ? s - a.n_spans : s, l = sp / a.kv_heads, h = sp - l * a.kv_heads;
      unsigned char* const cache = (isv ? a.v : a.k) + l * a.layer_stride + h * a.head_stride;
      const VEC* const src = reinterpret_cast<const VEC*>(cache + a.src_id * a.id_stride);
      // block-strided: in one round a workgroup's threads cover KV_FORK_THREADS consecutive vectors, the UNROLL loads of a thread lie `step` vectors apart
      for (long long i0 = (long long)blockIdx.x * KV_FORK_THREADS + threadIdx.x; i0 < a.span_vecs; i0 += step * KV_FORK_UNROLL) {
        VEC val[KV_FORK_UNROLL];
#pragma unroll
        for (int u = 0; u < KV_FORK_UNROLL; u++)
          if (i0 + u * step < a.span_vecs) val[u] = src[i0 + u * step];
        for (int d = 0; d < a.n_dst; d++) {
          VEC* const dst = reinterpret_cast<VEC*>(cache + a.dst_id[d] * a.id_stride);
#pragma unroll
          for (int u = 0; u < KV_FORK_UNROLL; u++)
            if (i0 + u * step < a.span_vecs) dst[i0 + u * step] = val[u];
        }
      }
    }
    return;
  }
  // ---- per-row state: segment by segment, the workgroups of the rows behind the cache part's stride over its dwords
  const int nb = ((int)gridDim.y - a.kv_rows) * (int)gridDim.x, b = ((int)blockIdx.y - a.kv_rows) * (int)gridDim.x + (int)blockIdx.x;
#pragma unroll 1
  for (int g = 0; g < KV_FORK_SEGS; g++) {
    const KvForkSeg sg = a.seg[g];
    const unsigned int* src = reinterpret_cast<const unsigned int*>(sg.base + a.src_row * sg.row_stride);
    for (int i = b * KV_FORK_THREADS + (int)threadIdx.x; i < sg.words; i += nb * KV_FORK_THREADS) {
      const unsigned int w = src[i];
      for (int d = 0; d < a.n_dst; d++) reinterpret_cast<unsigned int*>(sg.base + a.dst_row[d] * sg.row_stride)[i] = w;
    }
  }
}

}   // namespace tgx
