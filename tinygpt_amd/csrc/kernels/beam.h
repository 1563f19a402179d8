// beam.h — beam search on the device (include/tgx.h tgx_beam_select / tgx_beam_advance): the JOINT ranking of several rows' next-token distributions plus their
// running scores, and the publish launch that re-seats a group of rows on their chosen tokens.
//
// tgx_beam_select ranks key(i, t) = (double)score[i] + ((double)v_i[t] - lse_i) over the n <= BEAM_MAX_ROWS rows of a call (v_i: the row's fp32 logits, or its
// processed logits when a logit processor is on; lse_i: exactly logprobs.h's quantity) in the order (key descending, array index i ascending, rank within the row
// ascending) and returns the prefix that ends at the k-th candidate whose token is no end id.  Three launches, stream-ordered — no workgroup hands anything to
// another inside a launch, no flag, no arrive counter, no float atomics, every sum in a fixed association: the same call returns the same bits from run to run.
//
//   beam_tile_kernel   ceil(V / SAMP_TILE) workgroups per row, rows on blockIdx.y: logprobs.h lp_tile_body with top_n = k + n_end over the row's own pointer
//                      (16-byte loads, four consecutive entries per thread) -> per tile (max, sum of exp in double, the first top_n composite keys)
//   beam_row_kernel    one workgroup per row: logprobs.h lp_merge -> the row's lse and its first top_n keys, in the row order (value descending, index ascending)
//   beam_rank_kernel   one workgroup: the <= BEAM_MAX_ROWS * BEAM_ROW_CAND candidates ranked by counting, the prefix cut, the call's one record written
//
// WHY top_n = k + n_end PER ROW SUFFICES.  key(i, .) is a non-decreasing function of v_i[.], and equal keys of one row are ordered by their rank in the row, so the
// joint order restricted to one row IS that row's order: the entries of row i inside any prefix of the joint order are the first entries of row i.  The returned
// prefix holds at most k candidates that are no end id, and a row holds each end id once, so the prefix holds at most k + n_end entries of any one row — its first
// k + n_end.  Conversely every row brings at least k candidates that are no end id among those (or all its finite entries, if it has fewer), so the walk runs out
// of candidates only when the rows do.  k <= TGX_MAX_BEAMS = 8 and n_end <= TGX_MAX_STOP_IDS = 8: k + n_end <= 16 = BEAM_ROW_CAND <= LP_MAX.
//
// beam_publish_kernel: one workgroup per placed row of tgx_beam_advance — the token word and the next embedding at the row's position (GPT-2: + wpe), what the
// publishing thread of a step leaves; position, counters and rings are not touched.
#pragma once
#include "logprobs.h"

namespace tgx {

constexpr int BEAM_MAX_ROWS = 8;        // == TGX_MAX_BEAMS
constexpr int BEAM_ROW_CAND = 16;       // TGX_MAX_BEAMS + TGX_MAX_STOP_IDS
constexpr int BEAM_MAX_CAND = 32;       // == TGX_MAX_BEAM_CAND
static_assert(BEAM_ROW_CAND <= LP_MAX && BEAM_MAX_ROWS + ROW_MAX_STOP == BEAM_ROW_CAND, "a row's candidates are lp_tile_body's");

struct BeamCand { int beam, token; float score, lp; };      // == tgx_beam_cand
struct BeamRecord { int n, pad[3]; BeamCand cand[BEAM_MAX_CAND]; };      // what the call reads back

struct BeamSelArgs {
  const float* lg[BEAM_MAX_ROWS];       // row i's vector [V]: its logits, or its processed logits
  float score[BEAM_MAX_ROWS];
  int end_id[ROW_MAX_STOP];
  int n, k, n_end, top_n;               // top_n = k + n_end
  int V, nwg;
  float* tile_max;                      // [n][nwg]
  double* tile_sum;                     // [n][nwg]
  unsigned long long* tile_keys;        // [n][nwg][LP_MAX]
  double* row_lse;                      // [n]
  unsigned long long* row_keys;         // [n][BEAM_ROW_CAND]; 0 = no entry
  BeamRecord* rec;
};

static __global__ __launch_bounds__(SAMP_WG) void beam_tile_kernel(const BeamSelArgs a) {
  const int y = blockIdx.y, wg = blockIdx.x;
  const size_t t = (size_t)y * a.nwg + wg;
  lp_tile_body(a.lg[y], a.V, wg, a.top_n, a.tile_max + t, a.tile_sum + t, a.tile_keys + t * LP_MAX);
}

static __global__ __launch_bounds__(SAMP_WG) void beam_row_kernel(const BeamSelArgs a) {
  const int y = blockIdx.x, tid = threadIdx.x;
  double lse;
  const unsigned long long* s_out = lp_merge(a.tile_max + (size_t)y * a.nwg, a.tile_sum + (size_t)y * a.nwg, a.tile_keys + (size_t)y * a.nwg * LP_MAX, a.nwg, a.top_n, lse);
  if (tid < BEAM_ROW_CAND) a.row_keys[y * BEAM_ROW_CAND + tid] = tid < a.top_n ? s_out[tid] : 0ull;
  if (tid == 0) a.row_lse[y] = lse;
}

// thread c = i * BEAM_ROW_CAND + r holds candidate (row i, rank r).  Its place is the number of candidates ahead of it in (key descending, i ascending, r ascending)
// — a total order, so the places are distinct; thread 0 then walks the ordered list
static __global__ __launch_bounds__(BEAM_MAX_ROWS * BEAM_ROW_CAND) void beam_rank_kernel(const BeamSelArgs a) {
  constexpr int NC = BEAM_MAX_ROWS * BEAM_ROW_CAND;
  __shared__ double s_key[NC], s_lp[NC];
  __shared__ int s_tok[NC], s_order[NC];
  __shared__ int s_n;
  const int c = threadIdx.x, i = c / BEAM_ROW_CAND, r = c % BEAM_ROW_CAND;
  double key = -INFINITY, lp = -INFINITY;
  int tok = -1;
  if (i < a.n && r < a.top_n) {
    const unsigned long long k = a.row_keys[c];
    if (k) {
      tok = lp_key_index(k);
      lp = (double)lp_key_value(k) - a.row_lse[i];
      key = (double)a.score[i] + lp;
    }
  }
  const bool cand = tok >= 0 && key > -INFINITY;      // (a NaN key is no candidate either)
  s_key[c] = cand ? key : -INFINITY; s_lp[c] = lp; s_tok[c] = cand ? tok : -1;
  s_order[c] = -1;
  if (c == 0) s_n = 0;
  __syncthreads();
  if (cand) {
    int place = 0;
    for (int u = 0; u < NC; u++) {
      if (s_tok[u] < 0) continue;
      const double ku = s_key[u];
      place += (ku > key || (ku == key && u < c)) ? 1 : 0;      // (u < c: row ascending, then rank ascending)
    }
    s_order[place] = c;
    atomicAdd(&s_n, 1);      // (an integer count in shared memory)
  }
  __syncthreads();
  if (c == 0) {
    int n_out = 0, live = 0;
    for (int p = 0; p < s_n && n_out < BEAM_MAX_CAND && live < a.k; p++) {
      const int u = s_order[p], t = s_tok[u];
      bool end = false;
      for (int e = 0; e < a.n_end; e++) end = end || a.end_id[e] == t;
      BeamCand& o = a.rec->cand[n_out++];
      o.beam = u / BEAM_ROW_CAND; o.token = t; o.score = (float)s_key[u]; o.lp = (float)s_lp[u];
      live += end ? 0 : 1;
    }
    a.rec->n = n_out;
  }
}

struct BeamPublishArgs {
  int* tok[BEAM_MAX_ROWS];              // the placed rows' token words ...
  const int* pos[BEAM_MAX_ROWS];        // ... position words (read only) ...
  float* x[BEAM_MAX_ROWS];              // ... and residual streams [H]
  int token[BEAM_MAX_ROWS];
  const void* embed;                    // [V][H] storage dtype
  const void* wpe;                      // GPT-2 learned positions or nullptr
  int H, n_pos;
};
template <int DT>
__global__ __launch_bounds__(256) void beam_publish_kernel(const BeamPublishArgs a) {
  const int j = blockIdx.x;
  const int t = a.token[j];
  if (threadIdx.x == 0) *a.tok[j] = t;
  const int p = *a.pos[j];
  gather_embedding<DT>(a.embed, t, a.x[j], a.H, a.wpe, a.wpe ? (p < a.n_pos ? p : a.n_pos - 1) : 0);
}

}  // namespace tgx
