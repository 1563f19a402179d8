// kv_splice.h — the move of tgx_splice_row (include/tgx.h; csrc/splice_plan.h plans it): ranges are cut out of the middle of a row's cache, the positions behind
// them slide down, and their keys — stored post-RoPE at the position they were appended at — are re-rotated to the position they land on.
//
// The move is down-only and overlaps itself (dst < src, and one position's destination is another's source), so it runs in TWO launches through a device staging
// buffer, in groups of whole layers: no launch reads a cache position that another workgroup of the same launch writes.
//   gather   reads the moved positions through the OLD block table (or the slab), rotates K, copies V, writes stage[layer][K|V][kv_head][moved token][hd]
//   scatter  (behind it on the stream) copies the staged rows to their destinations through the NEW block table
// A launch of one group touches its own layers' bytes only, so the next group's gather may follow the previous group's scatter.
//
// The rotation, pinned: with (c_o, s_o) = rope_cos / rope_sin[s][p] and (c_n, s_n) = rope_cos / rope_sin[d][p] of source s and destination d
//   c = fmaf(c_n, c_o, __fmul_rn(s_n, s_o))          cos(table(d) - table(s))
//   s = fmaf(s_n, c_o, -__fmul_rn(c_n, s_o))         sin(table(d) - table(s))
// then rope_rotate_pair (common.h) on the stored pair (K[s][p], K[s][p + hd/2]) converted to fp32, rounded once to the storage dtype.  Both table rows are used,
// not the row of d - s: the tables hold cosf(fl32(inv * pos)), whose angles are not additive at large positions.
//
// Thread map: a thread owns one moved token and one chunk of p — 16 bytes of the low half of a row (8 entries at 16-bit storage, 4 at fp32; 4 bytes where half a row
// is no multiple of 16) and the same chunk of the high half.  It forms (c, s) for its chunk once, then walks the (layer, kv head) spans of the group (blockIdx.y
// strides over them): four loads — K low, K high, V low, V high — are in flight before the first store.  Consecutive threads own consecutive chunks, then consecutive
// tokens: a wave's low-half loads and its high-half loads together cover whole rows.  Vector stores and plain C++ only.  Every workgroup along blockIdx.y forms the
// (c, s) of its items again from the four table rows: 4 * hd/2 floats per moved token and grid row, small against the 2 * spans * hd entries it then moves.
#pragma once
#include "common.h"

namespace tgx {

constexpr int KV_SPLICE_THREADS = 256;
constexpr int KV_SPLICE_MAX_SEG = 16;      // == TGX_MAX_SPLICE_RANGES

struct KvSpliceSeg { int src, dst, m0, len; };      // `len` positions from src to dst < src; m0: the moved-token index of the first

struct KvSpliceArgs {
  void *k, *v;                    // layer 0 of the row's slab caches, or of the pools (paged)
  void* stage;                    // [n_layers][K|V][kv_heads][moved][hd]
  const int* tbl;                 // paged: the row's block table — the old one for a gather, the new one for a scatter; nullptr: slab
  const float *rope_cos, *rope_sin;      // [max_ctx][hd / 2]
  long long layer_stride;         // elements between two layers of the cache
  int layer0, n_layers, kv_heads, hd, max_ctx;
  int moved, chunks;              // moved tokens; chunks per half row
  int n_seg;
  KvSpliceSeg seg[KV_SPLICE_MAX_SEG];
};

// a chunk of W dwords <-> fp32: two entries per dword at 16-bit storage, one at fp32
template <int W> struct SpliceVec { typedef unsigned int type; };
template <> struct SpliceVec<4> { typedef u32x4 type; };
template <int W> __device__ __forceinline__ unsigned int splice_word(const typename SpliceVec<W>::type& v, int i) {
  if constexpr (W == 4) return v[i]; else return v;
}
template <int W> __device__ __forceinline__ void splice_set_word(typename SpliceVec<W>::type& v, int i, unsigned int w) {
  if constexpr (W == 4) v[i] = w; else v = w;
}
template <int DT, int W> __device__ __forceinline__ void splice_unpack(const typename SpliceVec<W>::type& v, float* f) {
#pragma unroll
  for (int i = 0; i < W; i++) {
    const unsigned int w = splice_word<W>(v, i);
    if constexpr (DT == DT_F32) f[i] = __uint_as_float(w);
    else { f[2 * i] = pair_lo<DT>(w); f[2 * i + 1] = pair_hi<DT>(w); }
  }
}
template <int DT, int W> __device__ __forceinline__ typename SpliceVec<W>::type splice_pack(const float* f) {
  typename SpliceVec<W>::type v;
#pragma unroll
  for (int i = 0; i < W; i++) {
    if constexpr (DT == DT_F32) splice_set_word<W>(v, i, __float_as_uint(f[i]));
    else splice_set_word<W>(v, i, (unsigned int)f32_to_elem<DT>(f[2 * i]) | ((unsigned int)f32_to_elem<DT>(f[2 * i + 1]) << 16));
  }
  return v;
}

template <int DT, int W, bool SCATTER>
__global__ __launch_bounds__(KV_SPLICE_THREADS) void kv_splice_kernel(const KvSpliceArgs a) {
  typedef elem_t<DT> E;
  typedef typename SpliceVec<W>::type VEC;
  constexpr int N = W * (DT == DT_F32 ? 1 : 2);      // entries per chunk
  const long long item = (long long)blockIdx.x * KV_SPLICE_THREADS + threadIdx.x;
  if (item >= (long long)a.moved * a.chunks) return;
  const int m = (int)(item / a.chunks), p0 = (int)(item - (long long)m * a.chunks) * N, half = a.hd >> 1;
  int s = 0, d = 0;
#pragma unroll 1
  for (int i = 0; i < a.n_seg; i++)
    if (m >= a.seg[i].m0 && m < a.seg[i].m0 + a.seg[i].len) { s = a.seg[i].src + (m - a.seg[i].m0); d = a.seg[i].dst + (m - a.seg[i].m0); }
  float cs[N], sn[N];
  if constexpr (!SCATTER) {
    const size_t o = (size_t)s * half + p0, n = (size_t)d * half + p0;
#pragma unroll
    for (int i = 0; i < N; i++) {
      const float c_o = a.rope_cos[o + i], s_o = a.rope_sin[o + i], c_n = a.rope_cos[n + i], s_n = a.rope_sin[n + i];
      cs[i] = fmaf(c_n, c_o, __fmul_rn(s_n, s_o));
      sn[i] = fmaf(s_n, c_o, -__fmul_rn(c_n, s_o));
    }
  }
  const int pos = SCATTER ? d : s;
  const size_t stage_v = (size_t)a.kv_heads * a.moved * a.hd;      // from a layer's staged K to its staged V
#pragma unroll 1
  for (int sp = (int)blockIdx.y; sp < a.n_layers * a.kv_heads; sp += (int)gridDim.y) {
    const int l = sp / a.kv_heads, h = sp - l * a.kv_heads;
    const size_t in_layer = a.tbl ? kv_paged_off(a.tbl, a.kv_heads, h, pos, a.hd) : ((size_t)h * a.max_ctx + pos) * (size_t)a.hd;
    const size_t coff = (size_t)(a.layer0 + l) * (size_t)a.layer_stride + in_layer + p0;
    const size_t soff = (((size_t)l * 2 * a.kv_heads + h) * a.moved + m) * (size_t)a.hd + p0;
    E* const kc = static_cast<E*>(a.k) + coff;
    E* const vc = static_cast<E*>(a.v) + coff;
    E* const ks = static_cast<E*>(a.stage) + soff;
    E* const vs = ks + stage_v;
    if constexpr (SCATTER) {
      const VEC k0 = *reinterpret_cast<const VEC*>(ks), k1 = *reinterpret_cast<const VEC*>(ks + half);
      const VEC v0 = *reinterpret_cast<const VEC*>(vs), v1 = *reinterpret_cast<const VEC*>(vs + half);
      *reinterpret_cast<VEC*>(kc) = k0; *reinterpret_cast<VEC*>(kc + half) = k1;
      *reinterpret_cast<VEC*>(vc) = v0; *reinterpret_cast<VEC*>(vc + half) = v1;
    } else {
      const VEC k0 = *reinterpret_cast<const VEC*>(kc), k1 = *reinterpret_cast<const VEC*>(kc + half);
      const VEC v0 = *reinterpret_cast<const VEC*>(vc), v1 = *reinterpret_cast<const VEC*>(vc + half);
      float x0[N], x1[N];
      splice_unpack<DT, W>(k0, x0); splice_unpack<DT, W>(k1, x1);
#pragma unroll
      for (int i = 0; i < N; i++) rope_rotate_pair(x0[i], x1[i], cs[i], sn[i]);
      *reinterpret_cast<VEC*>(ks) = splice_pack<DT, W>(x0); *reinterpret_cast<VEC*>(ks + half) = splice_pack<DT, W>(x1);
      *reinterpret_cast<VEC*>(vs) = v0; *reinterpret_cast<VEC*>(vs + half) = v1;
    }
  }
}

}   // namespace tgx
