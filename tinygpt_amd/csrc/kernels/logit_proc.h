// logit_proc.h — per-row logit processors (include/tgx.h tgx_set_row_penalties / tgx_set_row_logit_bias / tgx_set_row_history): repetition, presence and
// frequency penalties over a row's token history, an additive logit bias and the mask of a token automaton (tgx_set_row_automaton), applied on the device ahead of
// a step's publish.
// One launch per launch_sample_rows call (sampler.hip) while some row of the batch has a processor on: grid (ceil(V / 1024), rows), 256 threads; workgroup t of
// row y owns entries [1024 t, 1024 t + 1024), four consecutive ones per thread.  It reads the raw logits and the row's history words (16-byte loads when
// V % 4 == 0: every row of both slabs then starts on a 16-byte boundary; entry by entry otherwise), counts the row's current token (the owner of that entry reads,
// increments and stores the word and goes on with the new value: no other thread looks at it), applies the penalties, stages the tile in LDS, adds the bias entries
// that fall into the tile (the list's ids are distinct), and writes the tile into the processed-logits slab together with its (max, lowest index) partial.
// The RAW logits are never written: tgx_read_logits and the logprobs ring keep reading the model's distribution.
// A row with every processor off, or finished, is copied through with its partials recomputed, so that the consumers of the launch take ONE base pointer.
//
// The pinned formula (every operation rounded once to fp32, no contraction; tests/logit_proc_ref.py restates it in float32 numpy), per entry with raw logit v and
// word w = prompt bit << 31 | n:
//   1. w != 0:  v = v > 0 ? v / repetition : v * repetition
//   2. v = v - frequency * (float)n;  v = v - (n > 0 ? presence : 0)
//   3. the entry is in the bias list:  v = v + bias
//   4. the row has an automaton on and next[state][entry] == NONE:  v = -INFINITY
//
// The automaton (include/tgx.h tgx_set_row_automaton).  Stage 4 reads the row's table pointer and state word once per workgroup and the four 16-bit entries of
// the thread's four logits (one 8-byte load when V % 4 == 0: the table comes from the device allocator and a table row is then a multiple of 8 bytes; entry by
// entry otherwise), after the bias stage and before the tile is written, so the tile's (max, lowest index) partial sees the mask: 2 V more bytes read per
// constrained row and step.  The STATE moves in a launch of its own ahead of this one (automaton_advance_kernel: one workgroup, one thread per row of the step,
// state = next[state][current token] for rows that are on and unfinished), issued only under the union bit ROWU_AUTO: every tile of a row needs the NEW state, and
// a fold into this kernel would have the tile that owns the current token move a word the other tiles of the row read in no defined order.  A consumed token that
// the state does not allow (only a caller that switched the automaton on mid-stream can feed one) leaves the state where it is.
#pragma once
#include "common.h"

namespace tgx {

constexpr int PROC_WG = 256, PROC_EPT = 4, PROC_TILE = PROC_WG * PROC_EPT;
constexpr int PROC_MAX_BIAS = 320;                  // == TGX_MAX_LOGIT_BIAS

struct LogitProcArgs {           // every pointer: the launch's first row
  const float* logits; long long logits_stride;     // raw [rows][V]
  const RowReq* req;
  const int* tok;                // [rows] current-token words
  unsigned int* hist;            // [rows][V] history words
  const int* bias_ids;           // [rows][PROC_MAX_BIAS]
  const float* bias_val;
  float* out;                    // processed logits [rows][V]
  float* part_val; int* part_idx;   // processed partials [rows][n_tile]
  int V, n_tile;
  int step;                      // 1: a tgx_decode_rows step (the current token is counted, a finished row passes through); 0: tgx_sample_row (no current token)
};

// One rounding per operation: the products, differences and sums are written out under `fp contract(off)` — the header forms __fmul_rn / __fsub_rn / __fadd_rn
// are plain operators compiled under the default contraction mode, and `v - frequency * n` written with them becomes one v_fma_f32 (seen in the disassembly).
// The division is IEEE-rounded (hipcc's default for fp32).
__device__ __forceinline__ float proc_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float proc_sub(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}
__device__ __forceinline__ float proc_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ float proc_penalise(float v, unsigned int w, float rep, float pres, float freq) {
  const unsigned int n = w & PROC_COUNT_MASK;
  if (w) v = v > 0.f ? __fdiv_rn(v, rep) : proc_mul(v, rep);
  v = proc_sub(v, proc_mul(freq, (float)n));
  v = proc_sub(v, n > 0 ? pres : 0.f);
  return v;
}

// rows [0, rows) of a tgx_decode_rows step: an unfinished row whose automaton is on consumes its current token.  One workgroup; the only writer of the state words
struct AutoAdvanceArgs { RowReq* req; const int* tok; int rows, V; };
__global__ __launch_bounds__(WAVE) void automaton_advance_kernel(const AutoAdvanceArgs a) {
  for (int y = threadIdx.x; y < a.rows; y += WAVE) {
    RowReq& q = a.req[y];
    if (!(q.proc & PROC_AUTOMATON) || q.finished) continue;
    const int t = a.tok[y];
    if (t < 0 || t >= a.V) continue;
    const unsigned short n = q.auto_next[(size_t)q.auto_state * a.V + t];
    if (n != AUTO_NONE) q.auto_state = n;
  }
}

__global__ __launch_bounds__(PROC_WG) void logit_proc_kernel(const LogitProcArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[PROC_TILE];
  __shared__ float sv[PROC_WG / WAVE];
  __shared__ int si[PROC_WG / WAVE];
  const int y = blockIdx.y, t0 = blockIdx.x * PROC_TILE, tid = threadIdx.x, base = t0 + tid * PROC_EPT, V = a.V;
  const RowReq& q = a.req[y];
  const int proc = q.proc;
  const bool on = proc != 0 && !(a.step && q.finished);      // (workgroup-uniform)
  const bool vec = (V & 3) == 0;                              // then base < V covers the thread's four entries
  const float* lg = a.logits + (size_t)y * a.logits_stride;
  float v[PROC_EPT];
  if (vec && base < V) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(lg + base);
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++) v[j] = r[j];
  } else {
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++) v[j] = !vec && base + j < V ? lg[base + j] : 0.f;
  }
  if (on) {
    unsigned int* hw = a.hist + (size_t)y * V;
    unsigned int w[PROC_EPT];
    if (vec && base < V) {
      const u32x4 r = *reinterpret_cast<const u32x4*>(hw + base);
#pragma unroll
      for (int j = 0; j < PROC_EPT; j++) w[j] = r[j];
    } else {
#pragma unroll
      for (int j = 0; j < PROC_EPT; j++) w[j] = !vec && base + j < V ? hw[base + j] : 0u;
    }
    const bool pen = (proc & PROC_PENALTY) != 0;
    const float rep = pen ? q.repetition : 1.f, pres = pen ? q.presence : 0.f, freq = pen ? q.frequency : 0.f;
    const int tok = a.step ? a.tok[y] : -1;
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++) {
      if (base + j == tok && base + j < V) {      // the counting step: this thread owns the current token's word
        const unsigned int n = w[j] & PROC_COUNT_MASK;
        w[j] = (w[j] & PROC_PROMPT_BIT) | (n < PROC_COUNT_MASK ? n + 1u : n);
        hw[base + j] = w[j];
      }
      v[j] = proc_penalise(v[j], w[j], rep, pres, freq);
    }
    const int n_bias = (proc & PROC_BIAS) ? min(q.n_bias, PROC_MAX_BIAS) : 0;
    if (n_bias > 0) {
      *reinterpret_cast<f32x4*>(tile + tid * PROC_EPT) = f32x4{v[0], v[1], v[2], v[3]};
      __syncthreads();
      const int* ids = a.bias_ids + (size_t)y * PROC_MAX_BIAS;
      const float* bv = a.bias_val + (size_t)y * PROC_MAX_BIAS;
      for (int k = tid; k < n_bias; k += PROC_WG) {
        const int e = ids[k] - t0;
        if (e >= 0 && e < PROC_TILE) tile[e] = proc_add(tile[e], bv[k]);
      }
      __syncthreads();
      const f32x4 r = *reinterpret_cast<const f32x4*>(tile + tid * PROC_EPT);
#pragma unroll
      for (int j = 0; j < PROC_EPT; j++) v[j] = r[j];
    }
    if (proc & PROC_AUTOMATON) {      // stage 4: the entries the row's state does not allow
      const unsigned short* nx = q.auto_next + (size_t)q.auto_state * V;
      unsigned int e[PROC_EPT];
      if (vec && base < V) {
        const u32x2 r = *reinterpret_cast<const u32x2*>(nx + base);
        e[0] = r[0] & 0xffffu; e[1] = r[0] >> 16; e[2] = r[1] & 0xffffu; e[3] = r[1] >> 16;
      } else {
#pragma unroll
        for (int j = 0; j < PROC_EPT; j++) e[j] = !vec && base + j < V ? nx[base + j] : 0u;
      }
#pragma unroll
      for (int j = 0; j < PROC_EPT; j++) if (e[j] == AUTO_NONE) v[j] = -INFINITY;
    }
  }
  float* out = a.out + (size_t)y * V;
  if (vec) {
    if (base < V) *reinterpret_cast<f32x4*>(out + base) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++) if (base + j < V) out[base + j] = v[j];
  }
  // the tile's (max, lowest index): per thread in index order, across the wave by butterfly, across the four waves through LDS — ties -> the lowest index
  float best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < PROC_EPT; j++)
    if (base + j < V && (v[j] > best || (v[j] == best && base + j < bi))) { best = v[j]; bi = base + j; }
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, WAVE); const int oi = __shfl_xor(bi, o, WAVE);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if ((tid & (WAVE - 1)) == 0) { sv[tid / WAVE] = best; si[tid / WAVE] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < PROC_WG / WAVE; k++)
      if (sv[k] > best || (sv[k] == best && si[k] < bi)) { best = sv[k]; bi = si[k]; }
    a.part_val[(size_t)y * a.n_tile + blockIdx.x] = best;
    a.part_idx[(size_t)y * a.n_tile + blockIdx.x] = bi;
  }
}

}  // namespace tgx
