// embed_pool.h — tgx_embed_rows (include/tgx.h): the pooled final-norm hidden state of every text of a prompt pass.
//
// A pass leaves the fp32 final residual of all its positions in the workspace (ws_x on the matrix-core routes; prefill by steps stages its chunks, see below).
// embed_pool_kernel: one workgroup per (text, slice of EMB_SLICE consecutive pooled positions).
//   1. statistics: a wave takes a position at a time and forms the norm's row statistic exactly as the lm_head launch does (gemv.h, one wave per row): lane l holds
//      the 8-element slices l, l + 64, ..., one fp32 FMA chain per lane in slice order, then the DPP wave_sum.  The slice's (mean, 1 / rms) pairs go through LDS.
//   2. accumulation: a thread owns column slices tid, tid + 256, ... and adds the normed rows of the slice's positions IN POSITION ORDER — model.norm's
//      w * (x * inv), GPT-2's ln_f ((x - mean) * inv) * w + b, every operation rounded once, rounded to the storage dtype under act.round16 like lm_head's input.
//      The slice's sum is one row of the [text][slice][H] partials.
// embed_finish_kernel: one workgroup per text merges its slices in slice order, divides by the number of pooled positions, keeps the first `dims` components and
// divides by their L2 norm (sum of squares in fp64, merged in a fixed tree; a zero vector stays zero).
// The order of every sum depends on the text's length alone — no atomics, no arrival order — so a call gives the same bits run to run, on every route: prefill by
// steps copies its chunks' rows into a staging slice and launches the SAME kernel per completed slice (stage form), so its slices hold the same sums.
// LAST and FIRST pooling are the one-position case (one slice of one position, divided by 1).
#pragma once
#include "common.h"

namespace tgx {

constexpr int EMB_SLICE = 32;      // positions per slice: 4 x 2048 tokens give 256 workgroups, and the partials are 1/32 of the residual rows
constexpr int EMB_WG = 256;

struct EmbedText {
  int row0;       // workspace row of the first pooled position
  int np;         // pooled positions: the text's length (MEAN) or 1 (LAST, FIRST)
  int slice0;     // the text's first row of the partials
  int pad;
};

struct EmbedPoolArgs {
  const float* x;             // the residual rows [..][H]: the pass's workspace, or the staging slice (stage form)
  const EmbedText* tab;       // the call's texts
  float* part;                // [slices of the call][H]
  const void *norm_w, *norm_b;
  float eps;
  int H, act16;
  int t0;                     // the launch's first text: blockIdx.y counts from it
  int stage_slice, stage_cnt; // stage form (stage_slice >= 0): x holds stage_cnt positions of that slice of text t0; grid (1, 1)
};

struct EmbedFinishArgs {
  const EmbedText* tab;
  const float* part;
  float* out;                 // [texts][dims]
  int H, dims, normalize;
};

// (mean, 1 / sqrt(var + eps)) of LayerNorm or (0, 1 / sqrt(mean(x^2) + eps)) of RMSNorm over one row, by one whole wave: gemv_kernel's prologue at KS == 1
template <int LN>
__device__ __forceinline__ void embed_row_stat(const float* x, int H, float eps, int lane, float& mean, float& inv) {
  const f32x4* xg = reinterpret_cast<const f32x4*>(x);
  const int nchunk = H >> 3;
  mean = 0.f;
  if (LN) {
    float sm = 0.f;
    for (int c = lane; c < nchunk; c += 64) {
      const f32x4 v0 = xg[2 * c], v1 = xg[2 * c + 1];
#pragma unroll
      for (int t = 0; t < 4; t++) sm += v0[t];
#pragma unroll
      for (int t = 0; t < 4; t++) sm += v1[t];
    }
    mean = wave_sum(sm) / (float)H;
    float sq = 0.f;
    for (int c = lane; c < nchunk; c += 64) {
      const f32x4 v0 = xg[2 * c], v1 = xg[2 * c + 1];
#pragma unroll
      for (int t = 0; t < 4; t++) { const float dlt = v0[t] - mean; sq = fmaf(dlt, dlt, sq); }
#pragma unroll
      for (int t = 0; t < 4; t++) { const float dlt = v1[t] - mean; sq = fmaf(dlt, dlt, sq); }
    }
    inv = 1.0f / sqrtf(wave_sum(sq) / (float)H + eps);
  } else {
    float ss = 0.f;
    for (int c = lane; c < nchunk; c += 64) {
      const f32x4 v0 = xg[2 * c], v1 = xg[2 * c + 1];
#pragma unroll
      for (int t = 0; t < 4; t++) ss = fmaf(v0[t], v0[t], ss);
#pragma unroll
      for (int t = 0; t < 4; t++) ss = fmaf(v1[t], v1[t], ss);
    }
    inv = 1.0f / sqrtf(wave_sum(ss) / (float)H + eps);
  }
}

template <int DT, int LN>
__global__ __launch_bounds__(EMB_WG) void embed_pool_kernel(const EmbedPoolArgs a) {
  typedef elem_t<DT> E;
  __shared__ float s_mean[EMB_SLICE], s_inv[EMB_SLICE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const EmbedText e = a.tab[a.t0 + blockIdx.y];
  int slice, cnt;
  const float* rows;
  if (a.stage_slice >= 0) {          // (kernel-uniform)
    slice = a.stage_slice; cnt = a.stage_cnt; rows = a.x;
  } else {
    slice = blockIdx.x;
    const int start = slice * EMB_SLICE;
    if (start >= e.np) return;       // (workgroup-uniform: a shorter text of the launch)
    cnt = min(EMB_SLICE, e.np - start);
    rows = a.x + (size_t)(e.row0 + start) * a.H;
  }
  for (int p = wv; p < cnt; p += EMB_WG / 64) {      // (wave-uniform trip count: wave_sum runs with every lane on)
    float mean, inv;
    embed_row_stat<LN>(rows + (size_t)p * a.H, a.H, a.eps, lane, mean, inv);
    if (lane == 0) { s_mean[p] = mean; s_inv[p] = inv; }
  }
  __syncthreads();
  float* out = a.part + (size_t)(e.slice0 + slice) * a.H;
  const int nchunk = a.H >> 3;
  for (int c = tid; c < nchunk; c += EMB_WG) {
    float w[8], b[8], acc[8];
    slice_unpack<DT>(load_slice<DT>(static_cast<const E*>(a.norm_w), c), w);
    if (LN) slice_unpack<DT>(load_slice<DT>(static_cast<const E*>(a.norm_b), c), b);
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] = 0.f;
#pragma unroll 4
    for (int p = 0; p < cnt; p++) {
      const f32x4* xg = reinterpret_cast<const f32x4*>(rows + (size_t)p * a.H) + 2 * c;
      const f32x4 v0 = xg[0], v1 = xg[1];
      const float x[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      const float mean = s_mean[p], inv = s_inv[p];
#pragma unroll
      for (int t = 0; t < 8; t++) {
        const float n = LN ? __fadd_rn(__fmul_rn(__fmul_rn(x[t] - mean, inv), w[t]), b[t]) : __fmul_rn(w[t], __fmul_rn(x[t], inv));
        acc[t] = __fadd_rn(acc[t], round_storage_if<DT>(n, a.act16));
      }
    }
    f32x4* o = reinterpret_cast<f32x4*>(out) + 2 * c;
    o[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
    o[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
  }
}

__global__ __launch_bounds__(EMB_WG) void embed_finish_kernel(const EmbedFinishArgs a) {
  __shared__ double s_sq[EMB_WG];
  const int tid = threadIdx.x;
  const EmbedText e = a.tab[blockIdx.x];
  const int ns = (e.np + EMB_SLICE - 1) / EMB_SLICE;
  const float* part = a.part + (size_t)e.slice0 * a.H;
  float* out = a.out + (size_t)blockIdx.x * a.dims;
  double sq = 0.0;
  for (int col = tid; col < a.dims; col += EMB_WG) {
    float s = 0.f;
    for (int k0 = 0; k0 < ns; k0 += 8) {          // eight loads in flight, then their adds in slice order
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = part[(size_t)min(k0 + j, ns - 1) * a.H + col];
#pragma unroll
      for (int j = 0; j < 8; j++) if (k0 + j < ns) s = __fadd_rn(s, v[j]);
    }
    s = __fdiv_rn(s, (float)e.np);
    out[col] = s;
    sq += (double)s * (double)s;
  }
  if (!a.normalize) return;          // (kernel-uniform)
  s_sq[tid] = sq;
  __syncthreads();
  for (int o = EMB_WG / 2; o > 0; o >>= 1) {      // a fixed tree
    if (tid < o) s_sq[tid] += s_sq[tid + o];
    __syncthreads();
  }
  const double tot = s_sq[0];
  if (!(tot > 0.0)) return;          // a zero vector stays zero
  const float nrm = (float)sqrt(tot);
  for (int col = tid; col < a.dims; col += EMB_WG) out[col] = __fdiv_rn(out[col], nrm);      // (the thread's own stores above)
}

}  // namespace tgx
