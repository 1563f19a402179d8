// verify.h — the accept step of tgx_verify_row / tgx_verify_row_sampled (include/tgx.h): speculative decoding.  One causal pass ran the row's current token and its n_draft draft
// tokens (M = n_draft + 1 positions) and left the logits and the per-workgroup argmax partials of EVERY position in the call's workspace; this launch decides on
// the device how many of them the row takes and leaves the row as that many decode steps would: nothing here depends on the host knowing the count.  Under
// sampling the staged sampler's positions mode (kernels/sampler.h) ran in between and left every position's draw; the walk is the same.
#pragma once
#include "gemv.h"

namespace tgx {

struct VerifyArgs {
  const float* part_val;     // [M][part_stride] argmax partials of the M positions (the lm_head epilogue's, or argmax_partials_rows_kernel's)
  const int* part_idx;
  long long part_stride;
  int n_part, M;
  const float* logits;       // [M][V]
  const int* draws;          // [M] the row's sampler's draw of every position (tgx_verify_row_sampled on a sampled row), or nullptr: the merged argmax partials
  const long long* draft;    // [M - 1] the draft ids on the device (the pass's inputs 1 .. M - 1)
  int* tok;                  // the row's current token / position words
  int* pos;                  // (the pass did NOT advance it: it still holds `past`)
  RowReq* req;               // the row's request state: every produced token is counted against its stop set / max_new
  float* row_logits;         // the row's slots: logits [V], argmax partials [n_part], residual stream [H]
  float* row_part_val;
  int* row_part_idx;
  float* x;
  const void* embed;         // [V][H] storage dtype
  const void* wpe;           // GPT-2 learned positions or nullptr
  int H, V, n_pos;
  VerifyRecord* rec;
  // a row with a logit processor on (option verify.processors; kernels/logit_proc.h logit_proc_pos_kernel): g[i] is chosen from the PROCESSED partials of the
  // positions, while `logits` / `part_val` / `part_idx` above stay the raw ones — they are what the row's slots receive.  Every other row: the raw pair again
  const float* sel_part_val;
  const int* sel_part_idx;
  long long sel_part_stride;
  int sel_n_part, pad0;
  // ... and the commit behind the walk, by thread 0: the row's history words [V] counted by the inputs that produced a token, its state word set to that of the
  // last producing position (states: the row's slice of automaton_walk_kernel's, or nullptr without an automaton).  hist nullptr: nothing to commit
  unsigned int* hist;
  const int* states;
};

// the pass's first input is the row's device-resident current token: the host need not know it
static __global__ void verify_first_id_kernel(long long* ids, const int* tok) { if (threadIdx.x == 0) ids[0] = *tok; }

// One workgroup of 256 threads.  g[i] = the token the row's settings choose at position i: the greedy token (highest value, lowest index on a tie, the
// (unsigned)idx < V guard of finalize_row), or the sampler's draw a.draws[i].
// The row produces g[0], then g[1] if g[0] == draft[0], ... : draft[0 .. a - 1] followed by g[a]; a produced token that finishes the row (stop id, max_new)
// ends the walk.  The position that produced the last token hands the row its logits row and partials; the next embedding is gathered at the advanced position.
// TREE (tgx_verify_tree): the M positions are a token tree's (position 0 the row's current token; par[q] = the parent POSITION of position q, below q).  The walk
// starts at position 0; the position it stands on produces g, and it moves to THE child that carries g as its input (siblings carry distinct tokens: at most one)
// or ends.  path[j] = the position that produced token j: the cache slots past + path[j] hold the accepted inputs (kernels/kv_tree.h moves them into place).
template <int DT, bool TREE = false>
__device__ __forceinline__ void verify_accept_body(const VerifyArgs& a, const int* const par = nullptr, int* const path = nullptr) {
  __shared__ int s_g[VERIFY_MAX_POS];
  __shared__ int s_win, s_tok, s_pos;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = wv; i < a.M; i += 4) {      // a wave per position: its draw, or the merge of its partials
    if (a.draws) {                         // (workgroup-uniform)
      if (lane == 0) { const int t = a.draws[i]; s_g[i] = (unsigned)t < (unsigned)a.V ? t : 0; }
      continue;
    }
    const float* pv = a.sel_part_val + (size_t)i * a.sel_part_stride;
    const int* pi = a.sel_part_idx + (size_t)i * a.sel_part_stride;
    float bv = -INFINITY; int bi = 0x7fffffff;
    for (int p = lane; p < a.sel_n_part; p += 64) {
      const float v = pv[p]; const int ix = pi[p];
      if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v = __shfl_xor(bv, o, 64); const int ix = __shfl_xor(bi, o, 64);
      if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
    }
    if (lane == 0) s_g[i] = (unsigned)bi < (unsigned)a.V ? bi : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    RowStopWords w = row_stop_words(a.req, a.tok);
    const int in0 = *a.tok;      // the pass's input 0
    int n = 0, win = 0;
    if constexpr (TREE) {
      for (int cur = 0; n < a.M;) {                 // (a parent stands below its child: the walk ends within M positions whatever the tables hold)
        const int t = s_g[cur];
        row_count_and_stop(a.req, w, t);
        w.produced++;
        path[n] = cur; a.rec->ids[n++] = t; win = cur;
        if (a.req->finished) break;
        int nxt = -1;
        for (int q = cur + 1; q < a.M; q++)
          if (par[q] == cur && a.draft[q - 1] == (long long)t) { nxt = q; break; }
        if (nxt < 0) break;
        cur = nxt;
      }
    } else
    for (int i = 0; i < a.M; i++) {
      const int t = s_g[i];
      row_count_and_stop(a.req, w, t);
      w.produced++;
      a.rec->ids[n++] = t; win = i;
      if (a.req->finished || i + 1 == a.M || a.draft[i] != (long long)t) break;
    }
    a.rec->n = n; a.rec->finish = a.req->finished;
    if constexpr (!TREE)
      if (a.hist) {      // a processed row: inputs 0 .. n - 1 are the tokens its n steps consumed — one thread, one after another (an id may occur twice)
        for (int j = 0; j < n; j++) {
          const int t = j ? (int)a.draft[j - 1] : in0;
          if ((unsigned)t >= (unsigned)a.V) continue;
          const unsigned int h = a.hist[t], c = h & PROC_COUNT_MASK;
          a.hist[t] = (h & PROC_PROMPT_BIT) | (c < PROC_COUNT_MASK ? c + 1u : c);
        }
        if (a.states) a.req->auto_state = a.states[n - 1];
        a.rec->state = a.req->auto_state;
      }
    const int np = *a.pos + n;      // the n inputs that produced tokens are in the cache; the rows behind them are dead
    *a.pos = np; *a.tok = s_g[win];
    s_win = win; s_tok = s_g[win]; s_pos = np < a.n_pos ? np : a.n_pos - 1;
    __threadfence();
  }
  __syncthreads();
  const float* src = a.logits + (size_t)s_win * a.V;
  if ((a.V & 3) == 0) {
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
    f32x4* d4 = reinterpret_cast<f32x4*>(a.row_logits);
    for (int i = threadIdx.x; i < (a.V >> 2); i += 256) d4[i] = s4[i];
  } else {
    for (int i = threadIdx.x; i < a.V; i += 256) a.row_logits[i] = src[i];
  }
  for (int p = threadIdx.x; p < a.n_part; p += 256) {
    a.row_part_val[p] = a.part_val[(size_t)s_win * a.part_stride + p];
    a.row_part_idx[p] = a.part_idx[(size_t)s_win * a.part_stride + p];
  }
  gather_embedding<DT>(a.embed, s_tok, a.x, a.H, a.wpe, a.wpe ? s_pos : 0);
}
template <int DT>
__global__ __launch_bounds__(256) void verify_accept_kernel(const VerifyArgs a) { verify_accept_body<DT>(a); }
struct VerifyTreeArgs { VerifyArgs v; const int* par; int* path; };      // device tables of VERIFY_MAX_POS ints each
template <int DT>
__global__ __launch_bounds__(256) void verify_accept_tree_kernel(const VerifyTreeArgs t) { verify_accept_body<DT, true>(t.v, t.par, t.path); }

// ---- tgx_verify_rows: the same two launches for the n rows of a joint pass.  tab[i] = row i's arguments over ITS slice of the pass's workspace (logits, partials,
// draws or nullptr, the draft ids behind its first input) and its own record; one workgroup per row runs the walk above, so a row ends as its own one-row call leaves it
struct VerifyFirstIds { int* tok[VERIFY_MAX_ROWS]; int first[VERIFY_MAX_ROWS]; };
static __global__ void verify_first_ids_kernel(long long* ids, const VerifyFirstIds f, int n) {
  const int i = threadIdx.x;
  if (i < n) ids[f.first[i]] = *f.tok[i];
}
template <int DT>
__global__ __launch_bounds__(256) void verify_accept_rows_kernel(const VerifyArgs* tab) { verify_accept_body<DT>(tab[blockIdx.x]); }

}  // namespace tgx
