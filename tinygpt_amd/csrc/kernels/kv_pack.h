// kv_pack.h — the copy launches of tgx_save_row / tgx_restore_row (include/tgx.h): a group of whole layers of ONE row's cache between the cache and a staging buffer
// that holds them in the snapshot's order [layer][K, V][kv_head][past][head_dim] (csrc/row_snapshot.h).  PACK reads the cache and writes staging, UNPACK the reverse.
//
// Typeless bytes.  A SPAN is (layer, K or V, kv head): positions [0, past) of one head, contiguous in the snapshot.  A PIECE is at most KV_BLOCK positions of a span;
// it is contiguous in the cache as well, in both layouts:
//   slab cache   [layer][kv_head][max_ctx][hd] inside the row's slab:            piece p of a span starts p * KV_BLOCK positions into the head's run
//   paged cache  [layer][block][kv_head][KV_BLOCK][hd] inside the layer pool:    piece p lies in physical block tbl[p] of the row's device-resident table — one read
//                per piece, the same address for every thread of the workgroup (a uniform load); the table is written in stream order (abi.hip kv_tbl_push), so a restore's launch sees the blocks just assigned to the row
// The grid is 2-D: blockIdx.x walks the pieces of a span, blockIdx.y the spans of the launch; both loop when the grid was capped.  One workgroup moves one piece: every
// thread loads KV_PACK_UNROLL vectors (16 bytes each; 4 where head_dim * element size is no multiple of 16) before its first store, a wave's loads are contiguous 1 KiB
// runs.  The tail piece of a span holds past % KV_BLOCK positions: nothing at or beyond `past` is read or written, on either side.  No LDS.
//
// The state section (position word, token word, hidden row, logits) rides in the grid rows behind the cache part's, in 4-byte units, as in kernels/kv_fork.h.
#pragma once
#include "common.h"

namespace tgx {

constexpr int KV_PACK_THREADS = 256;
constexpr int KV_PACK_UNROLL = 4;      // loads in flight per thread before the first store
constexpr int KV_PACK_SEGS = 4;

struct KvPackSeg { unsigned char *dev, *stage; int words; };      // `words` dwords of the row's state on the device and their place in staging

struct KvPackArgs {
  unsigned char *k, *v;                   // slab cache: the ROW's K / V slab; paged: the pools
  unsigned char* stage;                   // the group's KV bytes: [n_layers][2][kv_heads][past][hd]
  const int* tbl;                         // paged: the row's block table on the device; nullptr: slab
  long long layer_stride, head_stride, piece_stride;      // bytes in the cache.  piece_stride — slab: KV_BLOCK positions; paged: one physical block (all heads)
  long long span_vecs;                    // vectors of a span = past positions
  int piece_vecs;                         // vectors of a full piece = KV_BLOCK positions
  int n_pieces;                           // ceil(past / KV_BLOCK)
  int layer0, n_spans, kv_heads;          // the launch's first layer; its spans = layers of the group * 2 * kv_heads
  int kv_rows;                            // grid rows (blockIdx.y) of the cache part; the rows behind them carry the state segments (n_seg may be 0)
  int n_seg;
  KvPackSeg seg[KV_PACK_SEGS];
};

template <typename VEC, bool UNPACK>
__global__ __launch_bounds__(KV_PACK_THREADS) void kv_pack_kernel(const KvPackArgs a) {
  if ((int)blockIdx.y < a.kv_rows) {
    for (int s = (int)blockIdx.y; s < a.n_spans; s += a.kv_rows) {      // span s of the group: [layer][K, V][kv_head]
      const int h = s % a.kv_heads, lw = s / a.kv_heads, isv = lw & 1, l = a.layer0 + (lw >> 1);
      unsigned char* const cache_span = (isv ? a.v : a.k) + l * a.layer_stride + h * a.head_stride;
      VEC* const stage_span = reinterpret_cast<VEC*>(a.stage) + (long long)s * a.span_vecs;
      for (int p = (int)blockIdx.x; p < a.n_pieces; p += (int)gridDim.x) {
        const long long v0 = (long long)p * a.piece_vecs;
        const int n = (int)(a.span_vecs - v0 < a.piece_vecs ? a.span_vecs - v0 : a.piece_vecs);      // the tail piece stops at `past`
        const long long id = a.tbl ? a.tbl[p] : p;
        VEC* const cache = reinterpret_cast<VEC*>(cache_span + id * a.piece_stride);
        VEC* const stage = stage_span + v0;
        const VEC* const src = UNPACK ? stage : cache;
        VEC* const dst = UNPACK ? cache : stage;
        for (int i0 = (int)threadIdx.x; i0 < n; i0 += KV_PACK_THREADS * KV_PACK_UNROLL) {
          VEC val[KV_PACK_UNROLL];
#pragma unroll
          for (int u = 0; u < KV_PACK_UNROLL; u++)
            if (i0 + u * KV_PACK_THREADS < n) val[u] = src[i0 + u * KV_PACK_THREADS];
#pragma unroll
          for (int u = 0; u < KV_PACK_UNROLL; u++)
            if (i0 + u * KV_PACK_THREADS < n) dst[i0 + u * KV_PACK_THREADS] = val[u];
        }
      }
    }
    return;
  }
  // ---- the state section: segment by segment, the workgroups of the rows behind the cache part's stride over its dwords
  const int nb = ((int)gridDim.y - a.kv_rows) * (int)gridDim.x, b = ((int)blockIdx.y - a.kv_rows) * (int)gridDim.x + (int)blockIdx.x;
#pragma unroll 1
  for (int g = 0; g < a.n_seg; g++) {
    const KvPackSeg sg = a.seg[g];
    const unsigned int* const src = reinterpret_cast<const unsigned int*>(UNPACK ? sg.stage : sg.dev);
    unsigned int* const dst = reinterpret_cast<unsigned int*>(UNPACK ? sg.dev : sg.stage);
    for (int i = b * KV_PACK_THREADS + (int)threadIdx.x; i < sg.words; i += nb * KV_PACK_THREADS) dst[i] = src[i];
  }
}

}   // namespace tgx
