// logprobs.h — per-token log-probabilities on the device (include/tgx.h tgx_set_row_logprobs / tgx_read_row_logprobs): for a row that produced token t
// from fp32 logits v[0..V), lp(t) = v[t] - lse(v) under the MODEL's distribution (temperature 1, before top-k / top-p / min-p), and the first top_n entries
// of v in the sampler's order (value descending, index ascending) with their lp.  Opt-in per row (RowReq.lp); two launches behind the step's publish:
//
//   lp_tile_kernel     ceil(V / SAMP_TILE) workgroups per row (rows on blockIdx.y), four consecutive entries per thread as in the sampler's vocabulary passes:
//                      per tile (max, sum of exp(v - tile max) in double) and, with top_n > 0, the tile's first top_n entries as composite keys
//   lp_record_kernel   one workgroup per row: the tile sums rescaled to the row maximum and added in tile order in double (the sampler's rule for its
//                      normaliser, sampler.h wg_z), the tiles' candidates merged, v[token] read, the record written into the row's ring and its counter moved
//
// No float atomics and no sort of the vocabulary: every sum has a fixed association, so a record is the same bits from run to run.  A workgroup whose row is off
// or produced nothing in this step leaves at once.  tgx_verify_row runs the same two kernels over the pass's [M][V] workspace logits with the POSITION on
// blockIdx.y: the produced ids come from the accept launch's VerifyRecord, positions >= rec->n leave at once.
#pragma once
#include "sampler.h"

namespace tgx {

struct LpArgs {
  const float* logits; long long logits_stride;       // [rows][V] (verify form: [positions][V])
  int V, nwg;
  const RowReq* req;                  // the launch's first row's request state (verify form: the row's)
  LpRow* st;                          // ... and its logprob state
  const int* tok;                     // [rows] the just-published token words (unused in the verify form)
  const VerifyRecord* rec;            // verify form: the accept launch's record; nullptr: a step / tgx_sample_row
  int force;                          // tgx_sample_row: the row produced a token whatever its counters say
  float* tile_max;                    // [rows][nwg]
  double* tile_sum;                   // [rows][nwg]
  unsigned long long* tile_keys;      // [rows][nwg][LP_MAX]; all three from the launch's first row (verify form: position 0)
  LpRecord* ring;                     // [rows][LP_RING] from the launch's first row (verify form: the row's)
};

// composite key of entry (v, idx): larger = earlier in (value descending, index ascending).  0 is no entry's key
__device__ __forceinline__ unsigned long long lp_key(float v, int idx) {
  return ((unsigned long long)float_key(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)idx);
}
__device__ __forceinline__ float lp_key_value(unsigned long long k) {
  const unsigned int u = (unsigned int)(k >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}
__device__ __forceinline__ int lp_key_index(unsigned long long k) { return (int)(0xFFFFFFFFu - (unsigned int)k); }

// does workgroup row y record in this launch, with how many alternatives and for which token
__device__ __forceinline__ bool lp_active(const LpArgs& a, int y, int& top_n, int& tok) {
  const RowReq& q = a.rec ? a.req[0] : a.req[y];
  const int mode = q.lp;
  if (mode <= 0) return false;
  top_n = min(mode - 1, LP_MAX);
  if (a.rec) {
    if (y >= a.rec->n) return false;
    tok = a.rec->ids[y];
  } else {
    if (!a.force && q.produced == a.st[y].seen) return false;
    tok = a.tok[y];
  }
  return true;
}

// one tile of one row of logits: lg[i] is entry i of the row, `wg` the tile (entries [SAMP_TILE wg, SAMP_TILE wg + SAMP_TILE) of V), the results into the tile's slots.
// Shared by lp_tile_kernel and the scoring pass (score.h score_tile_kernel, where the row is a slice of a [rows][chunk] product)
__device__ __forceinline__ void lp_tile_body(const float* lg, const int V, const int wg, const int top_n, float* out_max, double* out_sum, unsigned long long* out_keys) {
  __shared__ float shf[4];
  __shared__ double shd[4];
  __shared__ unsigned long long s_keys[4 * LP_MAX], s_out[LP_MAX];
  const int tid = threadIdx.x;
  const int base = (wg * SAMP_WG + tid) * SAMP_EPT;
  float v[SAMP_EPT];
  if (base + SAMP_EPT <= V && ((reinterpret_cast<size_t>(lg + base) & 15) == 0)) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(lg + base);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
#pragma unroll
    for (int j = 0; j < SAMP_EPT; j++) v[j] = base + j < V ? lg[base + j] : -INFINITY;
  }
  unsigned long long key[SAMP_EPT];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < SAMP_EPT; j++) {
    const bool in = base + j < V;
    key[j] = in ? lp_key(v[j], base + j) : 0ull;
    if (in) m = fmaxf(m, v[j]);
  }
  const float tmax = samp_block_max(m, shf);
  double s = 0.0;
  if (tmax > -INFINITY) {                 // (a tile of -inf alone contributes nothing)
#pragma unroll
    for (int j = 0; j < SAMP_EPT; j++) s += base + j < V ? (double)expf(v[j] - tmax) : 0.0;
  }
  s = samp_block_sum_d(s, shd);
  if (tid == 0) { *out_max = tmax; *out_sum = s; }
  if (top_n == 0) return;                 // (block-uniform)
  // the tile's first top_n entries: every wave takes the first top_n of its 256 by repeated maxima over the lanes (no barrier), the four lists are merged
  // by rank (the keys are distinct: they carry the index)
  const int lane = tid & 63, wv = tid >> 6;
  for (int r = 0; r < top_n; r++) {
    unsigned long long best = key[0];
#pragma unroll
    for (int j = 1; j < SAMP_EPT; j++) best = key[j] > best ? key[j] : best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long other = __shfl_xor(best, o, 64); best = other > best ? other : best; }
    if (lane == 0) s_keys[wv * LP_MAX + r] = best;
#pragma unroll
    for (int j = 0; j < SAMP_EPT; j++) if (key[j] == best) key[j] = 0ull;
  }
  if (tid < LP_MAX) s_out[tid] = 0ull;
  __syncthreads();
  if (tid < 4 * top_n) {
    const unsigned long long k = s_keys[(tid / top_n) * LP_MAX + tid % top_n];
    if (k) {
      int rank = 0;
      for (int w = 0; w < 4; w++)
        for (int r = 0; r < top_n; r++) rank += s_keys[w * LP_MAX + r] > k ? 1 : 0;
      if (rank < top_n) s_out[rank] = k;
    }
  }
  __syncthreads();
  if (tid < top_n) out_keys[tid] = s_out[tid];
}

static __global__ __launch_bounds__(SAMP_WG) void lp_tile_kernel(const LpArgs a) {
  const int y = blockIdx.y, wg = blockIdx.x;
  int top_n, tok;
  if (!lp_active(a, y, top_n, tok)) return;
  const size_t t = (size_t)y * a.nwg + wg;
  lp_tile_body(a.logits + (size_t)y * a.logits_stride, a.V, wg, top_n, a.tile_max + t, a.tile_sum + t, a.tile_keys + t * LP_MAX);
}

// the tiles of one row merged: lse = max + log sum exp(v - max), and (top_n > 0) the row's first top_n composite keys, returned in shared memory (entries
// [0, top_n); 0 = none).  Shared by lp_record_kernel and the scoring pass (score.h score_record_kernel)
__device__ __forceinline__ const unsigned long long* lp_merge(const float* tmaxs, const double* tsums, const unsigned long long* tkeys, const int nwg, const int top_n, double& lse) {
  __shared__ float shf[4];
  __shared__ double shd[4];
  __shared__ unsigned long long s_head[SAMP_MAX_WG], s_cand[LP_MAX * LP_MAX], s_out[LP_MAX];
  __shared__ int s_tile[LP_MAX];
  const int tid = threadIdx.x;
  // the row maximum: the maximum of the tile maxima (the same value the lm_head's argmax partials hold)
  float m = -INFINITY;
  for (int t = tid; t < nwg; t += SAMP_WG) m = fmaxf(m, tmaxs[t]);
  const float mx = samp_block_max(m, shf);
  // lse = max + log sum exp(v - max): the tile sums rescaled and added in double in a fixed association, rounded once
  double s = 0.0;
  for (int t = tid; t < nwg; t += SAMP_WG) {
    const float tm = tmaxs[t];
    if (tm > -INFINITY) s += tsums[t] * exp((double)tm - (double)mx);
  }
  s = samp_block_sum_d(s, shd);
  lse = (double)mx + log(s);
  // the first top_n entries of the row lie in the top_n tiles with the largest heads, among those tiles' own first top_n: rank the heads, gather the
  // candidates of these tiles (<= top_n^2), rank them
  if (top_n > 0) {
    for (int t = tid; t < nwg; t += SAMP_WG) s_head[t] = tkeys[(size_t)t * LP_MAX];
    if (tid < LP_MAX) { s_out[tid] = 0ull; s_tile[tid] = 0; }
    __syncthreads();
    for (int t = tid; t < nwg; t += SAMP_WG) {
      const unsigned long long k = s_head[t];
      int rank = 0;
      for (int u = 0; u < nwg && rank < top_n; u++) rank += s_head[u] > k ? 1 : 0;
      if (rank < top_n) s_tile[rank] = t;
    }
    __syncthreads();
    const int nq = min(top_n, nwg), nc = nq * top_n;
    for (int i = tid; i < nc; i += SAMP_WG) s_cand[i] = tkeys[(size_t)s_tile[i / top_n] * LP_MAX + i % top_n];
    __syncthreads();
    for (int i = tid; i < nc; i += SAMP_WG) {
      const unsigned long long k = s_cand[i];
      if (!k) continue;
      int rank = 0;
      for (int u = 0; u < nc; u++) rank += s_cand[u] > k ? 1 : 0;
      if (rank < top_n) s_out[rank] = k;
    }
    __syncthreads();
  }
  return s_out;
}

static __global__ __launch_bounds__(SAMP_WG) void lp_record_kernel(const LpArgs a) {
  const int y = blockIdx.y, tid = threadIdx.x, nwg = a.nwg;
  int top_n, tok;
  if (!lp_active(a, y, top_n, tok)) return;
  LpRow* st = a.rec ? a.st : a.st + y;
  const int count0 = __atomic_load_n(&st->count, __ATOMIC_RELAXED);       // (verify form: the last position to arrive moves it, behind every read)
  const float* lg = a.logits + (size_t)y * a.logits_stride;
  const float vt = (unsigned)tok < (unsigned)a.V ? lg[tok] : -INFINITY;
  double lse;
  const unsigned long long* s_out = lp_merge(a.tile_max + (size_t)y * nwg, a.tile_sum + (size_t)y * nwg, a.tile_keys + (size_t)y * nwg * LP_MAX, nwg, top_n, lse);
  LpRecord* out = a.ring + (a.rec ? (size_t)0 : (size_t)y * LP_RING) + (size_t)((unsigned)(count0 + (a.rec ? y : 0)) % (unsigned)LP_RING);
  if (tid < LP_MAX) {
    const unsigned long long k = tid < top_n ? s_out[tid] : 0ull;
    out->ids[tid] = k ? lp_key_index(k) : -1;
    out->lps[tid] = k ? (float)((double)lp_key_value(k) - lse) : -INFINITY;
  }
  if (tid == 0) {
    out->lp = (float)((double)vt - lse);
    out->tok = tok; out->top_n = top_n; out->pad = 0;
    const int produced = (a.rec ? a.req[0] : a.req[y]).produced;
    if (!a.rec) { st->count = count0 + 1; st->seen = produced; }
    else {
      const int n = a.rec->n;
      __threadfence();
      if (atomicAdd(&st->arrive, 1) == n - 1) { st->arrive = 0; st->seen = produced; __atomic_store_n(&st->count, count0 + n, __ATOMIC_RELAXED); }
    }
  }
}

}  // namespace tgx
