// gemv_fp8.h — the batch-1 weight stream of gate_up, down and lm_head over weights QUANTIZED to 8 bits: OCP E4M3 codes with one power-of-two scale per output
// row, half the bytes of the bf16 stream.  Opt-in and lossy (option weights.fp8, default 0; DESIGN.md §5 "FP8 weights"); the rule is in include/tgx.h.
//
// The model is defined by the option, not by this kernel: tgx_finalize overwrites the bf16 master of every selected matrix with the dequantized values
// dq = code * 2^e_r (fp8_quant_rows_kernel below), so every path that reads the master (prefill, batched steps, verify, score, embed) computes the same model.
// Every dq is exactly a bf16 value, and this kernel multiplies exactly dq: its results are bit-identical to gemv_kernel over the dequantized master.
//
// Stream layout of a matrix [N][K], K % 8 == 0, for the thread -> (row, k) map of gemv_kernel launched with `ks` waves per row pair and
// NX = ceil(K / 8 / (64 ks)) chunks per lane: a CHUNK is the 8 codes of 8 consecutive k (8 bytes, k order); lane l of k-part p owns chunks
// c = p * per + l + 64 j (per = 64 NX), j = 0..NX-1.  Its chunks go in PAIRS h = j / 2 of one 1 KiB plane each:
//   plane h: lane l's 16 bytes = chunk 2h (dwords 0, 1: k 0..3, 4..7) then chunk 2h + 1 (dwords 2, 3)
//   row r, k-part p, plane h starts at byte r * row_bytes + (p * NH + h) * 1024, NH = ceil(NX / 2), row_bytes = ks * NH * 1024.
//   Chunks past the row's end (j >= NX, c >= the k-part's end) are padding: code 0 (its activation is zero).
//   At the 1B / 3B / 7B shapes NX is 4 or 8 and there is no padding: 1 byte per weight.
// The row scales are scale[N], 2^e_r as fp32: one 4-byte load per row, the same address in every lane, issued with the unit's weight loads.
//
// Decode: v_cvt_f32_fp8 makes the code's own value (exact for all 254 finite codes, subnormals included), one multiply by the row's 2^e_r makes dq — exact,
// because the scale is a power of two and 2^-126 <= |dq| < 2^102 is a normal fp32 (e_r >= -117).  The two rows of a unit have different scales: each
// 2-vector {w_a[t], w_b[t]} is scaled by {2^e_a, 2^e_b} in one packed multiply and enters the same v_pk_fma_f32 chain as in gemv_packed.h.  The scale is NOT
// applied to the finished row sum: that is exact only while no partial sum is subnormal.  FMA order (elements 0..7, even / odd-j accumulators), the wave
// reduction and the K-part sums are gemv_kernel's.
//
// Out of scope here: qkv / o_proj, multi-row steps and prefill reading the codes, dropping the bf16 masters, pre-quantized checkpoints, per-group scales.
#pragma once
#include "gemv_packed.h"      // f32x2, pk_fma_x0 / pk_fma_x1

namespace tgx {

constexpr int FP8_E_MIN = -117;          // the smallest row exponent: the smallest non-zero dq, 2^-9 * 2^-117, is still a normal bf16
constexpr int FP8_EXP_BAD = 227;         // bf16 exponent field of 2^100: a weight that large (or inf / NaN) is refused

struct GemvFp8Args {
  GemvArgs g;               // g.W is not read
  const unsigned char* Q;   // code planes
  const float* scale;       // [N] 2^e_r
  long long row_bytes;
};

// byte T of a dword of four codes as fp32 (v_cvt_f32_fp8 with a byte select)
template <int T> __device__ __forceinline__ float fp8_code_value(unsigned int d) { return __builtin_amdgcn_cvt_f32_fp8((int)d, T); }
__device__ __forceinline__ void fp8_chunk_values(unsigned int d0, unsigned int d1, float f[8]) {
  f[0] = fp8_code_value<0>(d0); f[1] = fp8_code_value<1>(d0); f[2] = fp8_code_value<2>(d0); f[3] = fp8_code_value<3>(d0);
  f[4] = fp8_code_value<0>(d1); f[5] = fp8_code_value<1>(d1); f[6] = fp8_code_value<2>(d1); f[7] = fp8_code_value<3>(d1);
}

// R = 1, bf16.  The three forms: (PRO_RMSNORM, EPI_SILU_MUL), (PRO_PLAIN, EPI_RESIDUAL), (PRO_RMSNORM, EPI_LOGITS).  Everything outside load_unit and the
// decode + dot block is gemv_kernel's text for R = 1.
template <int PRO, int EPI, int NX, bool XACC = false>
__global__ __launch_bounds__(256, NX <= 4 ? 4 : 1) void gemv_fp8_kernel(const GemvFp8Args pa) {
  constexpr int DT = DT_BF16;
  constexpr int NH = (NX + 1) / 2;
  typedef elem_t<DT> E;
  static_assert(PRO == PRO_PLAIN || PRO == PRO_RMSNORM, "fp8 forms: plain or RMSNorm prologue");
  static_assert(EPI == EPI_SILU_MUL || EPI == EPI_RESIDUAL || EPI == EPI_LOGITS, "fp8 forms: gate_up, down, lm_head");
  const GemvArgs& a = pa.g;
  const int n_wg = (int)gridDim.x;
  __shared__ float ps[4][2];
  __shared__ float sv[1][4];
  __shared__ int si[1][4];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int KS = a.ks, UPB = 4 / KS;
  const int slot = wv / KS, kpart = wv - slot * KS;
  const int nchunk = a.K >> 3;                                         // chunks per row
  const int per = ((nchunk + KS * 64 - 1) / (KS * 64)) * 64;           // chunks per k-part (multiple of 64)
  const int c_begin = min(kpart * per, nchunk), c_end = min(c_begin + per, nchunk);
  const int stride = n_wg * UPB;

  int cidx[NX];
  bool cok[NX];
#pragma unroll
  for (int j = 0; j < NX; j++) {
    const int c = c_begin + lane + 64 * j;
    cok[j] = c < c_end;
    cidx[j] = cok[j] ? c : max(c_end - 1, 0);    // clamped: always a legal slice of the activation vector
  }

  const size_t lane_off = (size_t)kpart * NH * 1024 + (size_t)lane * 16;      // this lane's 16 bytes of its k-part's first plane
  u32x4 wa[NH], wb[NH], na[NH], nb[NH];
  f32x2 sc = {0.f, 0.f}, nsc = {0.f, 0.f};      // {2^e of row a, 2^e of row b}: loaded with the unit's planes
  auto load_unit = [&](int ub, u32x4* ta, u32x4* tb, f32x2& s) {
    const int u = min(ub + slot, a.units - 1);
    int ra, rb; bool v;
    unit_rows<EPI>(a, u, ra, rb, v);
    s = f32x2{pa.scale[ra], pa.scale[rb]};
    const unsigned char* pra = pa.Q + (size_t)ra * pa.row_bytes + lane_off;
    const unsigned char* prb = pa.Q + (size_t)rb * pa.row_bytes + lane_off;
#pragma unroll
    for (int h = 0; h < NH; h++) {
      ta[h] = load_nt(reinterpret_cast<const u32x4*>(pra + (size_t)h * 1024));
      tb[h] = load_nt(reinterpret_cast<const u32x4*>(prb + (size_t)h * 1024));
    }
  };

  float xr[NX][8];
  auto load_x = [&]() {
    const f32x4* xg = reinterpret_cast<const f32x4*>(a.x);
#pragma unroll
    for (int j = 0; j < NX; j++) {
      f32x4 v0 = xg[2 * cidx[j]], v1 = xg[2 * cidx[j] + 1];
      if (!cok[j]) { v0 = f32x4{0.f, 0.f, 0.f, 0.f}; v1 = v0; }
#pragma unroll
      for (int t = 0; t < 4; t++) { xr[j][t] = v0[t]; xr[j][4 + t] = v1[t]; }
    }
  };
  // 0. XACC: this thread's eight accumulators of the residual stream leave first (gemv_kernel, step 0)
  ulonglong2 xacc0[(XACC && PRO == PRO_RMSNORM) ? 4 : 1];
  if constexpr (XACC && PRO == PRO_RMSNORM) {
    const ulonglong2* ag = reinterpret_cast<const ulonglong2*>(a.x_acc + (size_t)min((int)threadIdx.x, nchunk - 1) * 8);
#pragma unroll
    for (int q = 0; q < 4; q++) xacc0[q] = ag[q];
    __builtin_amdgcn_sched_barrier(0);
  }
  // 1. the first unit's weights are in flight before anything else is touched
  int ub = blockIdx.x * UPB;
  if (ub < a.units) load_unit(ub, wa, wb, sc);
  Slice8<DT> nw_x[(XACC && PRO == PRO_RMSNORM) ? NX : 1];
  if constexpr (XACC && PRO == PRO_RMSNORM) {
#pragma unroll
    for (int j = 0; j < NX; j++) nw_x[j] = load_slice<DT>(static_cast<const E*>(a.norm_w), cidx[j]);
    __builtin_amdgcn_sched_barrier(0);
  }

  // 2. this wave's slice of the activation vector -> registers (zero outside the range)
  if constexpr (XACC && PRO == PRO_RMSNORM) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    for (int cs = threadIdx.x; cs < nchunk; cs += 256) {
      ulonglong2 t[4];
      if (cs == (int)threadIdx.x) {
#pragma unroll
        for (int q = 0; q < 4; q++) t[q] = xacc0[q];
      } else {       // hidden sizes beyond 2048: the later chunks
        const ulonglong2* ag = reinterpret_cast<const ulonglong2*>(a.x_acc + (size_t)cs * 8);
#pragma unroll
        for (int q = 0; q < 4; q++) t[q] = ag[q];
      }
      float f[8];
#pragma unroll
      for (int q = 0; q < 4; q++) { f[2 * q] = fix_to_f32((long long)t[q].x); f[2 * q + 1] = fix_to_f32((long long)t[q].y); }
      f32x4* dst = reinterpret_cast<f32x4*>(xs + (size_t)cs * 8);
      dst[0] = f32x4{f[0], f[1], f[2], f[3]}; dst[1] = f32x4{f[4], f[5], f[6], f[7]};
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NX; j++) {
      const f32x4* xl = reinterpret_cast<const f32x4*>(xs + (size_t)cidx[j] * 8);
      f32x4 v0 = xl[0], v1 = xl[1];
      if (!cok[j]) { v0 = f32x4{0.f, 0.f, 0.f, 0.f}; v1 = v0; }
#pragma unroll
      for (int t = 0; t < 4; t++) { xr[j][t] = v0[t]; xr[j][4 + t] = v1[t]; }
    }
  } else {
    load_x();
  }
  // sum of one value over the KS waves that share a unit, in wave order (every wave of the workgroup takes part)
  auto ks_sum = [&](float& v) {
    if (lane == 0) ps[wv][0] = v;
    __syncthreads();
    float t = ps[slot * KS][0];
    for (int k = 1; k < KS; k++) t += ps[slot * KS + k][0];
    v = t;
    __syncthreads();               // ps is reused (unit loop)
  };
  if (PRO == PRO_RMSNORM) {   // HF order: weight * (x * rsqrt(mean(x^2)+eps))
    const E* wg = static_cast<const E*>(a.norm_w);
    Slice8<DT> nw[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) { if constexpr (XACC) nw[j] = nw_x[j]; else nw[j] = load_slice<DT>(wg, cidx[j]); }       // in flight together with x
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NX; j++)
#pragma unroll
      for (int t = 0; t < 8; t++) ss = fmaf(xr[j][t], xr[j][t], ss);
    float ssq = wave_sum(ss);
    if (KS > 1) ks_sum(ssq);
    const float inv = 1.0f / sqrtf(ssq / (float)a.K + a.eps);
#pragma unroll
    for (int j = 0; j < NX; j++) {
      float w[8];
      slice_unpack<DT>(nw[j], w);
#pragma unroll
      for (int t = 0; t < 8; t++) xr[j][t] = w[t] * (xr[j][t] * inv);
    }
  }

  if constexpr (PRO != PRO_PLAIN) {     // option act.round16 (gemv_kernel)
    if (a.act16) {          // (kernel-uniform)
#pragma unroll
      for (int j = 0; j < NX; j++)
#pragma unroll
        for (int t = 0; t < 8; t++) xr[j][t] = elem_to_f32<DT>(f32_to_elem<DT>(xr[j][t]));
    }
  }

  float best_val = -INFINITY;
  int best_idx = 0x7fffffff;

  for (; ub < a.units; ub += stride) {   // trip count uniform per workgroup
    const bool has_next = ub + stride < a.units;
    if (has_next) load_unit(ub + stride, na, nb, nsc);

    // epilogue operands are fetched now so that their latency hides under the dot products
    const int u = ub + slot;
    const bool writer = u < a.units && kpart == 0 && lane == 0;
    int ra = 0, rb = 0; bool rb_valid = false;
    float e0 = 0.f, e1 = 0.f;                // RESIDUAL: x[ra], x[rb]
    if (writer) {
      unit_rows<EPI>(a, u, ra, rb, rb_valid);
      if (EPI == EPI_RESIDUAL) {
        if constexpr (XACC) { e0 = fix_to_f32(a.res_acc[ra]); e1 = fix_to_f32(a.res_acc[rb]); }
        else { e0 = a.out[ra]; e1 = a.out[rb]; }
      }
    }

    // (acc_a, acc_b) of the unit's two rows as one 2-vector: the even-j and the odd-j chain, elements 0..7 in order (gemv_kernel's dot8 per row)
    f32x2 acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NX; j++) {
      const int h = j >> 1, o = (j & 1) * 2;
      float fa[8], fb[8];
      fp8_chunk_values(wa[h][o], wa[h][o + 1], fa);
      fp8_chunk_values(wb[h][o], wb[h][o + 1], fb);
      f32x2 acc = (j & 1) ? acc1 : acc0;
#pragma unroll
      for (int t = 0; t < 8; t += 2) {
        const f32x2 x2 = f32x2{xr[j][t], xr[j][t + 1]};
        acc = pk_fma_x0(f32x2{fa[t], fb[t]} * sc, x2, acc);               // the weights entering the FMA are dq = code * 2^e of their own row
        acc = pk_fma_x1(f32x2{fa[t + 1], fb[t + 1]} * sc, x2, acc);
      }
      if (j & 1) acc1 = acc; else acc0 = acc;
    }
    float sa = wave_sum(acc0[0] + acc1[0]);
    float sb = wave_sum(acc0[1] + acc1[1]);

    if (KS > 1) {   // fixed-order sum of the KS k-part partials through LDS
      __syncthreads();             // previous iteration's readers are done
      if (lane == 0) { ps[wv][0] = sa; ps[wv][1] = sb; }
      __syncthreads();
      if (kpart == 0) {
        sa = ps[slot * KS][0]; sb = ps[slot * KS][1];
        for (int k = 1; k < KS; k++) { sa += ps[slot * KS + k][0]; sb += ps[slot * KS + k][1]; }
      }
    }

    if (writer) {
      float va = sa, vb = sb;
      if (EPI == EPI_LOGITS) {
        a.logits[ra] = va;
        if (va > best_val) { best_val = va; best_idx = ra; }     // rows ascend within a wave: '>' keeps the first
        if (rb_valid) {
          a.logits[rb] = vb;
          if (vb > best_val) { best_val = vb; best_idx = rb; }
        }
      } else {
        if (a.bias) { const E* bias = static_cast<const E*>(a.bias); va += elem_to_f32<DT>(bias[ra]); vb += elem_to_f32<DT>(bias[rb]); }
        if (EPI == EPI_RESIDUAL) {
          a.out[ra] = e0 + va;
          if (rb_valid) a.out[rb] = e1 + vb;
          if constexpr (XACC) { a.res_acc[ra] = 0; if (rb_valid) a.res_acc[rb] = 0; }     // this lane is the only reader / writer of its rows' accumulators
        } else if (EPI == EPI_SILU_MUL) {
          a.out[u] = round_storage_if<DT>((va / (1.0f + expf(-va))) * vb, a.act16);        // (the down product's input)
        }
      }
    }

#pragma unroll
    for (int h = 0; h < NH; h++) { wa[h] = na[h]; wb[h] = nb[h]; }
    sc = nsc;
  }

  if (EPI == EPI_LOGITS) {
    // workgroup argmax, ties -> lowest index (== argmax(logits, -1), Sampler.cpp:28)
    if (lane == 0) { sv[0][wv] = best_val; si[0][wv] = best_idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float bv = sv[0][0]; int bi = si[0][0];
      for (int w = 1; w < 4; w++)
        if (sv[0][w] > bv || (sv[0][w] == bv && si[0][w] < bi)) { bv = sv[0][w]; bi = si[0][w]; }
      a.part_val[blockIdx.x] = bv;
      a.part_idx[blockIdx.x] = bi;
    }
  }
}

// ---- the quantizer (tgx_finalize) ------------------------------------------------------------------------------------------------------------------
// All of it is integer arithmetic on the bf16 patterns: no rounding mode, no denormal mode and no conversion instruction decides a code.

// the row exponent e_r of a row whose largest magnitude has the 15-bit pattern `amax` (rule 1-4 of include/tgx.h)
__device__ __forceinline__ int fp8_row_exp(unsigned int amax) {
  const int Ef = (int)(amax >> 7), M = (int)(amax & 0x7fu);
  if (amax == 0) return 0;
  if (Ef == 0) return FP8_E_MIN;                        // a row of bf16 subnormals only: far below the clamp
  const int x = Ef - 126;                               // amax = m * 2^x, m = 1.M / 2 in [0.5, 1)
  return max(M <= 0x60 ? x - 9 : x - 8, FP8_E_MIN);     // m <= 0.875  <=>  M <= 96
}
// the E4M3 code of the bf16 pattern `bits` under the row exponent e: round-to-nearest-even of the exact quotient, sign kept
__device__ __forceinline__ unsigned int fp8_code(unsigned int bits, int e) {
  const unsigned int s = (bits >> 8) & 0x80u, Ef = (bits >> 7) & 0xffu, M = bits & 0x7fu;
  const unsigned int sig = Ef ? (0x80u | M) : M;
  if (!sig) return s;
  const int t9 = (int)(Ef ? Ef : 1u) - 134 - e + 9;     // |w| / 2^e = sig * 2^t9 in units of 2^-9, the subnormal codes' step
  const int b = (31 - __clz((int)sig)) + t9;            // floor(log2) of that
  const int g = max(b - 3, 0);                          // the grid's step there is 2^g units: four significant bits, never finer than one unit
  const int sh = g - t9;                                // bits of sig below the grid
  unsigned int r;
  if (sh <= 0) r = sig << (-sh);
  else if (sh > 9) r = 0;
  else {
    const unsigned int q = sig >> sh, rem = sig & ((1u << sh) - 1u), half = 1u << (sh - 1);
    r = q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u);
  }
  return s | (((unsigned int)g << 3) + r);              // r in [8, 16] of a normal code, [0, 8] of a subnormal one: a carry moves into the exponent field by itself
}
// code * 2^e as a bf16 pattern (always exact, always a normal bf16 or a zero)
__device__ __forceinline__ unsigned int fp8_dq_bits(unsigned int code, int e) {
  const unsigned int s = (code & 0x80u) << 8, ef = (code >> 3) & 0xfu, mm = code & 7u;
  const unsigned int r = ef ? 8u + mm : mm;
  if (!r) return s;
  const int g = ef ? (int)ef - 1 : 0;
  const int mb = 31 - __clz((int)r);
  return s | ((unsigned int)(mb + g - 9 + e + 127) << 7) | ((r << (7 - mb)) & 0x7fu);
}

// one wave per row: scale[row] = 2^e_r; stat[0] = the lowest row that holds a non-finite weight or a |w| >= 2^100 (untouched where there is none)
__global__ __launch_bounds__(64) void fp8_row_scale_kernel(const bf16_t* W, int K, float* scale, int* stat) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const u32x4* w = reinterpret_cast<const u32x4*>(W + (size_t)row * K);
  unsigned int m = 0;
  for (int c = lane; c < (K >> 3); c += 64) {
    const u32x4 v = w[c];
#pragma unroll
    for (int t = 0; t < 4; t++) m = max(m, max(v[t] & 0x7fffu, (v[t] >> 16) & 0x7fffu));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, o, 64));
  if (lane == 0) {
    if ((m >> 7) >= (unsigned int)FP8_EXP_BAD) atomicMin(stat, row);
    scale[row] = __uint_as_float((unsigned int)(fp8_row_exp(m) + 127) << 23);
  }
}

struct Fp8QuantArgs {
  bf16_t* W;                // [N][K]: overwritten with the dequantized values
  int K, ks, nx;
  const float* scale;       // [N] from fp8_row_scale_kernel
  unsigned char* Q;         // code planes (zeroed by the caller: the padding), or nullptr: the matrix has no stream
  long long row_bytes;
};

// one wave per row: every chunk of the row is quantized, written back dequantized and — where the matrix has a stream — stored at its place in the planes
__global__ __launch_bounds__(64) void fp8_quant_rows_kernel(const Fp8QuantArgs a) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const int e = (int)(__float_as_uint(a.scale[row]) >> 23) - 127;
  u32x4* w = reinterpret_cast<u32x4*>(a.W + (size_t)row * a.K);
  const int nchunk = a.K >> 3, nh = (a.nx + 1) / 2, per = 64 * a.nx;
  for (int c = lane; c < nchunk; c += 64) {
    const u32x4 v = w[c];
    u32x4 dq;
    unsigned int code[2] = {0u, 0u};
#pragma unroll
    for (int t = 0; t < 8; t++) {
      const unsigned int bits = (v[t >> 1] >> (16 * (t & 1))) & 0xffffu;
      const unsigned int q = fp8_code(bits, e);
      code[t >> 2] |= q << (8 * (t & 3));
      const unsigned int d = fp8_dq_bits(q, e) << (16 * (t & 1));
      if (t & 1) dq[t >> 1] |= d; else dq[t >> 1] = d;
    }
    w[c] = dq;
    if (a.Q) {
      const int p = c / per, j = (c - p * per) >> 6;      // (c - p * per) & 63 == lane: per is a multiple of 64
      unsigned char* dst = a.Q + (size_t)row * a.row_bytes + ((size_t)p * nh + (j >> 1)) * 1024 + (size_t)lane * 16 + (size_t)(j & 1) * 8;
      *reinterpret_cast<u32x2*>(dst) = u32x2{code[0], code[1]};
    }
  }
}

}  // namespace tgx
