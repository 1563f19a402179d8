// score.h — tgx_score_row (include/tgx.h): the log-probability of every SUPPLIED token of a prompt pass.  Position p of the pass (p < seq - 1) scores the id
// the caller put at p + 1: lp = v_p[ids[p + 1]] - lse(v_p) under the model's distribution, and the first top_n entries of v_p in the sampler's order, exactly as
// logprobs.h defines them for produced tokens — the tile and merge bodies are that header's (lp_tile_body, lp_merge).
//
// The logits of a GROUP of positions arrive as a [rows][width] fp32 block that holds vocabulary entries [col0, col0 + width) of each position: the whole row of the
// verify workspace (col0 = 0, stride V), or one vocabulary chunk of the matrix-core lm_head (prefill.hip launch_score_tiled), so that no [seq][V] buffer exists.
//
//   score_tile_kernel     behind each block: per (position, 1024-entry tile of V) the tile max, the double sum of exp(v - max), the tile's first top_n composite
//                         keys, and the target's value when it lies in the tile.  The tile partition is the global one — tile t = entries [1024 t, 1024 t + 1024) —
//                         whatever the chunking: col0 is a multiple of SAMP_TILE
//   score_record_kernel   behind the last block of a group: the tiles merged (fixed association, double, rounded once) into the call's output arrays
//
// A position that scores nothing (p >= n_score: the last of the pass) leaves at once.
#pragma once
#include "logprobs.h"

namespace tgx {

struct ScoreArgs {
  const float* logits; long long stride;      // [rows][stride]: column j of row y = entry col0 + j of position pos0 + y
  int col0, V, nwg;                           // nwg: tiles of the whole vocabulary
  int top_n;
  const long long* ids;                       // the pass's ids on the device: ids[p + 1] is position p's target
  int pos0, n_score;                          // the group's first position; positions >= n_score score nothing
  float* tile_max;                            // [rows][nwg]
  double* tile_sum;                           // [rows][nwg]
  unsigned long long* tile_keys;              // [rows][nwg][LP_MAX]
  float* tgt;                                 // [rows] the target's logit
  float* out_lp;                              // [n_score]
  int* out_ids;                               // [n_score][LP_MAX]
  float* out_top_lp;                          // [n_score][LP_MAX]
};

static __global__ __launch_bounds__(SAMP_WG) void score_tile_kernel(const ScoreArgs a) {
  const int y = blockIdx.y, p = a.pos0 + y;
  if (p >= a.n_score) return;
  const int wg = a.col0 / SAMP_TILE + (int)blockIdx.x;      // the global tile
  if (wg >= a.nwg) return;
  // lg[i] = entry i of the position for the entries of this block (the pointer is only dereferenced inside [col0, col0 + width))
  const float* lg = a.logits + (long long)y * a.stride - a.col0;
  const size_t t = (size_t)y * a.nwg + wg;
  const int tok = (int)a.ids[p + 1];
  if (threadIdx.x == 0 && tok >= wg * SAMP_TILE && tok < min(a.V, (wg + 1) * SAMP_TILE)) a.tgt[y] = lg[tok];
  lp_tile_body(lg, a.V, wg, a.top_n, a.tile_max + t, a.tile_sum + t, a.tile_keys + t * LP_MAX);
}

static __global__ __launch_bounds__(SAMP_WG) void score_record_kernel(const ScoreArgs a) {
  const int y = blockIdx.y, p = a.pos0 + y, tid = threadIdx.x, nwg = a.nwg, top_n = a.top_n;
  if (p >= a.n_score) return;
  const float vt = a.tgt[y];
  double lse;
  const unsigned long long* s_out = lp_merge(a.tile_max + (size_t)y * nwg, a.tile_sum + (size_t)y * nwg, a.tile_keys + (size_t)y * nwg * LP_MAX, nwg, top_n, lse);
  if (tid < LP_MAX) {
    const unsigned long long k = tid < top_n ? s_out[tid] : 0ull;
    a.out_ids[(size_t)p * LP_MAX + tid] = k ? lp_key_index(k) : -1;
    a.out_top_lp[(size_t)p * LP_MAX + tid] = k ? (float)((double)lp_key_value(k) - lse) : -INFINITY;
  }
  if (tid == 0) a.out_lp[p] = (float)((double)vt - lse);
}

}  // namespace tgx
