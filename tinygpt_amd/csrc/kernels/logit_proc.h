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

// ---- the pieces logit_proc_kernel and logit_proc_pos_kernel share: a thread's four entries of its workgroup's tile, in registers
// the thread's raw logits: one 16-byte load when V % 4 == 0 (then base < V covers all four), entry by entry otherwise
__device__ __forceinline__ void proc_load_raw(const float* lg, int base, int V, float (&v)[PROC_EPT]) {
  const bool vec = (V & 3) == 0;
  if (vec && base < V) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(lg + base);
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++) v[j] = r[j];
  } else {
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++) v[j] = !vec && base + j < V ? lg[base + j] : 0.f;
  }
}
// ... and its history words
__device__ __forceinline__ void proc_load_words(const unsigned int* hw, int base, int V, unsigned int (&w)[PROC_EPT]) {
  const bool vec = (V & 3) == 0;
  if (vec && base < V) {
    const u32x4 r = *reinterpret_cast<const u32x4*>(hw + base);
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++) w[j] = r[j];
  } else {
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++) w[j] = !vec && base + j < V ? hw[base + j] : 0u;
  }
}
// one more occurrence of the word's token: the count saturates, the prompt bit stays
__device__ __forceinline__ unsigned int proc_count(unsigned int w) {
  const unsigned int n = w & PROC_COUNT_MASK;
  return (w & PROC_PROMPT_BIT) | (n < PROC_COUNT_MASK ? n + 1u : n);
}
// stages 1-3 of the pinned formula on the thread's entries, with the words w as the position sees them: the penalties, then the row's bias entries that fall into
// the tile, through LDS (`tile`: the workgroup's PROC_TILE floats).  Every thread of the workgroup calls it (q and proc are workgroup-uniform)
__device__ __forceinline__ void proc_stages_1_3(float (&v)[PROC_EPT], const unsigned int (&w)[PROC_EPT], const RowReq& q, int proc, const int* bias_ids, const float* bias_val,
                                                float* tile, int t0, int tid) {
  const bool pen = (proc & PROC_PENALTY) != 0;
  const float rep = pen ? q.repetition : 1.f, pres = pen ? q.presence : 0.f, freq = pen ? q.frequency : 0.f;
#pragma unroll
  for (int j = 0; j < PROC_EPT; j++) v[j] = proc_penalise(v[j], w[j], rep, pres, freq);
  const int n_bias = (proc & PROC_BIAS) ? min(q.n_bias, PROC_MAX_BIAS) : 0;
  if (n_bias > 0) {
    *reinterpret_cast<f32x4*>(tile + tid * PROC_EPT) = f32x4{v[0], v[1], v[2], v[3]};
    __syncthreads();
    for (int k = tid; k < n_bias; k += PROC_WG) {
      const int e = bias_ids[k] - t0;
      if (e >= 0 && e < PROC_TILE) tile[e] = proc_add(tile[e], bias_val[k]);
    }
    __syncthreads();
    const f32x4 r = *reinterpret_cast<const f32x4*>(tile + tid * PROC_EPT);
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++) v[j] = r[j];
  }
}
// stage 4: the entries that row `nx` of the automaton's table (the state's) does not allow
__device__ __forceinline__ void proc_mask(float (&v)[PROC_EPT], const unsigned short* nx, int base, int V) {
  const bool vec = (V & 3) == 0;
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
// the thread's entries into `out` [V], and the tile's (max, lowest index) into *pv / *pi: per thread in index order, across the wave by butterfly, across the four
// waves through LDS (sv, si: PROC_WG / WAVE words each) — ties -> the lowest index
__device__ __forceinline__ void proc_store(const float (&v)[PROC_EPT], float* out, int base, int V, float* sv, int* si, float* pv, int* pi) {
  const int tid = threadIdx.x;
  if ((V & 3) == 0) {
    if (base < V) *reinterpret_cast<f32x4*>(out + base) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++) if (base + j < V) out[base + j] = v[j];
  }
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
    *pv = best; *pi = bi;
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
  float v[PROC_EPT];
  proc_load_raw(a.logits + (size_t)y * a.logits_stride, base, V, v);
  if (on) {
    unsigned int* hw = a.hist + (size_t)y * V;
    unsigned int w[PROC_EPT];
    proc_load_words(hw, base, V, w);
    const int tok = a.step ? a.tok[y] : -1;
#pragma unroll
    for (int j = 0; j < PROC_EPT; j++)
      if (base + j == tok && base + j < V) {      // the counting step: this thread owns the current token's word
        w[j] = proc_count(w[j]);
        hw[base + j] = w[j];
      }
    proc_stages_1_3(v, w, q, proc, a.bias_ids + (size_t)y * PROC_MAX_BIAS, a.bias_val + (size_t)y * PROC_MAX_BIAS, tile, t0, tid);
    if (proc & PROC_AUTOMATON) proc_mask(v, q.auto_next + (size_t)q.auto_state * V, base, V);      // stage 4
  }
  proc_store(v, a.out + (size_t)y * V, base, V, sv, si, a.part_val + (size_t)y * a.n_tile + blockIdx.x, a.part_idx + (size_t)y * a.n_tile + blockIdx.x);
}

// ---- the processors over the positions of a verify pass (include/tgx.h option verify.processors; csrc/abi.hip verify_row_run / step_tail).  Position i of a
// row's pass is processed as the row's step i would have been, without running the steps one after another:
//   the words    w_i[e] = the row's word for e, counted once more per pass input 0 .. i that equals e (at most 16 comparisons per word; proc_count per hit)
//   the state    s_i = the row's state moved by inputs 0 .. i under automaton_advance_kernel's rule — automaton_walk_kernel, a launch ahead of this one, leaves
//                every position's state in states[]: one thread per row walks its <= 16 inputs
//   the vector   stages 1-3 by proc_stages_1_3 (the code logit_proc_kernel runs), stage 4 with s_i
// Grid (ceil(V / 1024), positions), 256 threads: logit_proc_kernel's tile ownership and 16-byte paths (the pass's slabs come from the device allocator and a
// position starts at a multiple of V floats: 16-byte aligned when V % 4 == 0).  Only the positions of processed rows are listed: the consumers of an unprocessed
// row's positions keep the raw pointers.  Nothing of the row is written here — neither its words nor its state: the pass's raw logits in, the processed slab and
// its per-tile (max, lowest index) partials out.
// THE COMMIT is the accept workgroup's (kernels/verify.h verify_accept_body, thread 0 behind the walk) and not a launch of its own: the count n stands in that
// thread's registers, the work is at most 16 read-modify-writes and one state word by ONE thread (an id that occurs twice among the inputs is counted twice, in
// order, without atomics), and a launch more would cost the call several microseconds for it.  Every reader of the words and the state in this call stands ahead
// of the accept launch in stream order.
struct ProcPos { int row, i, slot, pad; const long long* ids; };      // batch row; index within its pass; workspace row; the row's pass inputs on the device [i + 1 read]
constexpr int PROC_MAX_POS = 64;                                       // == TGX_MAX_VERIFY_POSITIONS
struct LogitProcPosArgs {
  const float* logits;           // the pass's raw logits [slots][V]
  const RowReq* req;             // [max_batch]
  const unsigned int* hist;      // [max_batch][V]   (read only)
  const int* bias_ids;           // [max_batch][PROC_MAX_BIAS]
  const float* bias_val;
  const int* states;             // [slots] (automaton_walk_kernel)
  float* out;                    // processed [slots][V]
  float* part_val; int* part_idx;   // [slots][n_tile]
  int V, n_tile;
  ProcPos pos[PROC_MAX_POS];
};
struct AutoWalkRow { const RowReq* req; const long long* ids; int first, M; };
struct AutoWalkArgs { int* states; int n, V; AutoWalkRow r[PROC_MAX_POS]; };
// states[first_j + i] for the positions of the call's processed rows (rows without an automaton: nothing).  One workgroup, one thread per row; no row state is written
__global__ __launch_bounds__(PROC_MAX_POS) void automaton_walk_kernel(const AutoWalkArgs a) {
  const int j = threadIdx.x;
  if (j >= a.n) return;
  const AutoWalkRow& r = a.r[j];
  if (!(r.req->proc & PROC_AUTOMATON)) return;
  int s = r.req->auto_state;
  const unsigned short* next = r.req->auto_next;
  for (int i = 0; i < r.M; i++) {
    const long long t = r.ids[i];
    if (t >= 0 && t < a.V) {
      const unsigned short n = next[(size_t)s * a.V + (size_t)t];
      if (n != AUTO_NONE) s = n;
    }
    a.states[r.first + i] = s;
  }
}

__global__ __launch_bounds__(PROC_WG) void logit_proc_pos_kernel(const LogitProcPosArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[PROC_TILE];
  __shared__ float sv[PROC_WG / WAVE];
  __shared__ int si[PROC_WG / WAVE];
  __shared__ int s_in[VERIFY_MAX_POS];
  const ProcPos& p = a.pos[blockIdx.y];
  const int t0 = blockIdx.x * PROC_TILE, tid = threadIdx.x, base = t0 + tid * PROC_EPT, V = a.V;
  const int n_in = min(p.i + 1, VERIFY_MAX_POS);
  if (tid < n_in) s_in[tid] = (int)p.ids[tid];      // the inputs 0 .. i, once per workgroup
  __syncthreads();
  const RowReq& q = a.req[p.row];
  const int proc = q.proc;
  float v[PROC_EPT];
  proc_load_raw(a.logits + (size_t)p.slot * V, base, V, v);
  unsigned int w[PROC_EPT];
  proc_load_words(a.hist + (size_t)p.row * V, base, V, w);
  for (int k = 0; k < n_in; k++) {
    const unsigned int d = (unsigned int)(s_in[k] - base);      // (an input outside the thread's four entries: d >= PROC_EPT)
    if (d < (unsigned int)PROC_EPT) {
#pragma unroll
      for (int j = 0; j < PROC_EPT; j++) if (d == (unsigned int)j) w[j] = proc_count(w[j]);
    }
  }
  proc_stages_1_3(v, w, q, proc, a.bias_ids + (size_t)p.row * PROC_MAX_BIAS, a.bias_val + (size_t)p.row * PROC_MAX_BIAS, tile, t0, tid);
  if (proc & PROC_AUTOMATON) proc_mask(v, q.auto_next + (size_t)a.states[p.slot] * V, base, V);
  proc_store(v, a.out + (size_t)p.slot * V, base, V, sv, si, a.part_val + (size_t)p.slot * a.n_tile + blockIdx.x, a.part_idx + (size_t)p.slot * a.n_tile + blockIdx.x);
}

}  // namespace tgx
