// gemv_fp4.h — the batch-1 weight stream of gate_up, down and lm_head over weights QUANTIZED to MXFP4: OCP E2M1 codes with one E8M0 scale byte per block
// of 32 consecutive k of a row, 4.25 bits per weight.  Opt-in and lossy (option weights.fp4, default 0; DESIGN.md §5 "FP4 weights"); the rule is in
// include/tgx.h.
//
// The model is defined by the option, not by this kernel: tgx_finalize overwrites the bf16 master of every selected matrix with the dequantized values
// dq = code * 2^e_block (fp4_quant_rows_kernel below), so every path that reads the master computes the same model.  Every dq is exactly a bf16 value, and
// this kernel multiplies exactly dq: its results are bit-identical to gemv_kernel over the dequantized master.
//
// Stream layout of a matrix [N][K], K % 32 == 0, for the thread -> (row, k) map of gemv_kernel launched with `ks` waves per row pair and
// NX = ceil(K / 8 / (64 ks)) chunks per lane: a CHUNK is the 8 codes of 8 consecutive k — one dword, element t in nibble t (byte t / 2, even t low).  Lane l
// of k-part p owns chunks c = p * per + l + 64 j (per = 64 NX), j = 0..NX-1, so a block of 32 k is the chunks of four neighbouring lanes at one j.  Nothing
// is padded to a power of two: a k-part of a row is 272 NX bytes, 256 NX of codes and then 16 NX of scales —
//   codes    the lane's chunks in QUADS h = j / 4: quad h < NX / 4 is 1 KiB, lane l's 16 bytes are its chunks 4h .. 4h + 3, one dword each; the last
//            NX % 4 chunks form a short quad of 4 (NX % 4) bytes per lane, lane after lane
//   scales   lane group g = l / 4: for a whole quad the dword at 64 h + 4 g, whose byte i is the E8M0 scale of the group's block at j = 4h + i; for the short
//            quad NX % 4 single bytes at 64 (NX / 4) + (NX % 4) g
//   row r, k-part p starts at byte r * row_bytes + p * 272 NX; row_bytes = ks * 272 NX.
//   Lanes past the row's end (c >= the k-part's end) are padding: code 0 under scale byte 127 (its activation is zero).
//   Wherever K is a multiple of 512 ks — the 1B / 3B / 7B / 70B shapes — there is none: 0.53125 bytes per weight, 4.25 bits.
// A matrix whose launch is split over K ranges (down at an intermediate size beyond 16384: decode.hip) is laid out range after range, each range as a
// matrix [N][K range] of its own.
// A lane fetches a unit (two rows) with one 16-byte non-temporal load and one 4-byte load per row and whole quad (dword and byte loads for the short
// one), issued together; the four lanes of a group read the same scale bytes.
//
// Decode: v_cvt_scalef32_pk_f32_fp4 turns one byte — two consecutive k of one row — into the two fp32 values code * 2^e, taking the block's scale as its
// second operand.  The instruction reads only the exponent field of that operand and is exact for all 16 codes under every scale byte 2..227
// (tools/probes/fp4_cvt_probe.hip, profiles/weights_fp4.txt), so the operand is the scale dword moved by ONE shift that puts byte i into bits 30:23; what
// the shift leaves in the sign and mantissa bits is not read.  The scale thus reaches the weight inside the convert: never a partial sum, never the
// activation.  Per 16 weights (a chunk of both rows): 8 converts, 2 shifts and 16 v_fma_f32 — the FP8 kernel spends 32 on half as many bytes' worth.
// The FMAs are scalar fp32 (this unit is built without packed fp32 arithmetic): elements 0..7 in order, the even-j / odd-j accumulators, the wave
// reduction and the K-part sums are gemv_kernel's for R = 1.
//
// Out of scope here: qkv / o_proj, multi-row steps and prefill reading the codes, dropping the bf16 masters, pre-quantized checkpoints.
#pragma once
#include "gemv.h"

namespace tgx {

constexpr int FP4_E_MIN = -125;          // the smallest block exponent: the smallest non-zero dq, 0.5 * 2^-125, is still a normal bf16
constexpr int FP4_EXP_BAD = 227;         // bf16 exponent field of 2^100: a weight that large (or inf / NaN) is refused
constexpr int FP4_SLOT = 272;            // bytes of one chunk slot of a k-part: 64 lanes x 4 code bytes + 16 groups x 1 scale byte
// byte offsets, within a k-part of NX slots, of lane `lane`'s code dword and of its group's scale byte for chunk slot js
__host__ __device__ __forceinline__ int fp4_code_off(int nx, int lane, int js) {
  const int full = nx >> 2, rem = nx & 3, h = js >> 2, i = js & 3;
  return h < full ? h * 1024 + lane * 16 + i * 4 : full * 1024 + lane * 4 * rem + i * 4;
}
__host__ __device__ __forceinline__ int fp4_scale_off(int nx, int lane, int js) {
  const int full = nx >> 2, rem = nx & 3, h = js >> 2, i = js & 3;
  return 256 * nx + (h < full ? h * 64 + (lane >> 2) * 4 + i : full * 64 + (lane >> 2) * rem + i);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct GemvFp4Args {
  GemvArgs g;               // g.W is not read
  const unsigned char* Q;   // planes (codes and block scales)
  long long row_bytes;
};

// acc += the chunk `d` (8 codes) under the scale operand `s` times the activations x[0..7], elements in order
__device__ __forceinline__ float fp4_dot8(float acc, unsigned int d, float s, const float* x) {
  const f32x2 v0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, s, 0), v1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, s, 1);
  const f32x2 v2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, s, 2), v3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, s, 3);
  acc = fmaf(v0[0], x[0], acc); acc = fmaf(v0[1], x[1], acc); acc = fmaf(v1[0], x[2], acc); acc = fmaf(v1[1], x[3], acc);
  acc = fmaf(v2[0], x[4], acc); acc = fmaf(v2[1], x[5], acc); acc = fmaf(v3[0], x[6], acc); acc = fmaf(v3[1], x[7], acc);
  return acc;
}
// byte I of the scale dword in the exponent field of an fp32 (the other bits are whatever the shift leaves: the convert does not read them)
template <int I> __device__ __forceinline__ float fp4_scale_operand(unsigned int sd) { return __uint_as_float(I < 3 ? sd << (23 - 8 * I) : sd >> 1); }

// R = 1, bf16.  The three forms: (PRO_RMSNORM, EPI_SILU_MUL), (PRO_PLAIN, EPI_RESIDUAL), (PRO_RMSNORM, EPI_LOGITS).  Everything outside load_unit and the
// decode + dot block is gemv_kernel's text for R = 1.
template <int PRO, int EPI, int NX, bool XACC = false>
__global__ __launch_bounds__(256, NX <= 4 ? 4 : 1) void gemv_fp4_kernel(const GemvFp4Args pa) {
  constexpr int DT = DT_BF16;
  constexpr int NF = NX / 4, NR = NX % 4;       // whole quads, chunks of the short quad
  constexpr int NS = NF + NR;                   // scale registers per row: a dword per whole quad, a byte per chunk of the short one
  typedef elem_t<DT> E;
  static_assert(PRO == PRO_PLAIN || PRO == PRO_RMSNORM, "fp4 forms: plain or RMSNorm prologue");
  static_assert(EPI == EPI_SILU_MUL || EPI == EPI_RESIDUAL || EPI == EPI_LOGITS, "fp4 forms: gate_up, down, lm_head");
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

  const unsigned char* const Qp = pa.Q + (size_t)kpart * (FP4_SLOT * NX);      // this k-part within a row
  unsigned int wa[NX], wb[NX], na[NX], nb[NX];           // a chunk's eight codes each
  unsigned int sa4[NS], sb4[NS], nsa4[NS], nsb4[NS];      // the scales: loaded with the unit's codes
  auto load_row = [&](const unsigned char* pr, unsigned int* tw, unsigned int* ts) {
#pragma unroll
    for (int h = 0; h < NF; h++) {
      const u32x4 v = load_nt(reinterpret_cast<const u32x4*>(pr + fp4_code_off(NX, lane, 4 * h)));
      tw[4 * h] = v[0]; tw[4 * h + 1] = v[1]; tw[4 * h + 2] = v[2]; tw[4 * h + 3] = v[3];
      ts[h] = __builtin_nontemporal_load(reinterpret_cast<const unsigned int*>(pr + fp4_scale_off(NX, lane, 4 * h)));
    }
#pragma unroll
    for (int i = 0; i < NR; i++) {
      tw[4 * NF + i] = __builtin_nontemporal_load(reinterpret_cast<const unsigned int*>(pr + fp4_code_off(NX, lane, 4 * NF + i)));
      ts[NF + i] = __builtin_nontemporal_load(pr + fp4_scale_off(NX, lane, 4 * NF + i));
    }
  };
  auto load_unit = [&](int ub, unsigned int* ta, unsigned int* tb, unsigned int* tsa, unsigned int* tsb) {
    const int u = min(ub + slot, a.units - 1);
    int ra, rb; bool v;
    unit_rows<EPI>(a, u, ra, rb, v);
    load_row(Qp + (size_t)ra * pa.row_bytes, ta, tsa);
    load_row(Qp + (size_t)rb * pa.row_bytes, tb, tsb);
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
  if (ub < a.units) load_unit(ub, wa, wb, sa4, sb4);
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
    if (has_next) load_unit(ub + stride, na, nb, nsa4, nsb4);

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

    // the unit's two rows: the even-j and the odd-j chain of each, elements 0..7 in order (gemv_kernel's dot8 per row); every weight is dq of its own block
    float acc_a0 = 0.f, acc_b0 = 0.f, acc_a1 = 0.f, acc_b1 = 0.f;
#pragma unroll
    for (int j = 0; j < NX; j++) {
      float s_a, s_b;
      if (j >= 4 * NF) { s_a = fp4_scale_operand<0>(sa4[NF + j - 4 * NF]); s_b = fp4_scale_operand<0>(sb4[NF + j - 4 * NF]); }      // the short quad: a byte each
      else switch (j & 3) {
        case 0: s_a = fp4_scale_operand<0>(sa4[j >> 2]); s_b = fp4_scale_operand<0>(sb4[j >> 2]); break;
        case 1: s_a = fp4_scale_operand<1>(sa4[j >> 2]); s_b = fp4_scale_operand<1>(sb4[j >> 2]); break;
        case 2: s_a = fp4_scale_operand<2>(sa4[j >> 2]); s_b = fp4_scale_operand<2>(sb4[j >> 2]); break;
        default: s_a = fp4_scale_operand<3>(sa4[j >> 2]); s_b = fp4_scale_operand<3>(sb4[j >> 2]); break;
      }
      if (j & 1) { acc_a1 = fp4_dot8(acc_a1, wa[j], s_a, xr[j]); acc_b1 = fp4_dot8(acc_b1, wb[j], s_b, xr[j]); }
      else       { acc_a0 = fp4_dot8(acc_a0, wa[j], s_a, xr[j]); acc_b0 = fp4_dot8(acc_b0, wb[j], s_b, xr[j]); }
    }
    float sa = wave_sum(acc_a0 + acc_a1);
    float sb = wave_sum(acc_b0 + acc_b1);

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
    for (int j = 0; j < NX; j++) { wa[j] = na[j]; wb[j] = nb[j]; }
#pragma unroll
    for (int h = 0; h < NS; h++) { sa4[h] = nsa4[h]; sb4[h] = nsb4[h]; }
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

// the exponent e of a block whose largest magnitude has the 15-bit pattern `amax` (rule 1 of include/tgx.h)
__device__ __forceinline__ int fp4_block_exp(unsigned int amax) {
  const int Ef = (int)(amax >> 7), M = (int)(amax & 0x7fu);
  if (amax == 0) return 0;
  if (Ef == 0) return FP4_E_MIN;                        // a block of bf16 subnormals only: far below the clamp
  const int x = Ef - 127;                               // amax = m * 2^x, m = 1.M in [1, 2)
  return max(M <= 0x40 ? x - 2 : x - 1, FP4_E_MIN);     // m <= 1.5  <=>  M <= 64
}
// the E2M1 code of the bf16 pattern `bits` under the block exponent e: the grid value nearest the exact quotient, ties to the even code, sign kept
__device__ __forceinline__ unsigned int fp4_code(unsigned int bits, int e) {
  const unsigned int s = (bits >> 12) & 8u, Ef = (bits >> 7) & 0xffu, M = bits & 0x7fu;
  const unsigned int sig = Ef ? (0x80u | M) : M;
  if (!sig) return s;
  const int t1 = (int)(Ef ? Ef : 1u) - 134 - e + 1;     // |w| / 2^e = sig * 2^t1 in units of 0.5, the subnormal code's step
  const int b = (31 - __clz((int)sig)) + t1;            // floor(log2) of that
  const int g = max(b - 1, 0);                          // the grid's step there is 2^g units: two significant bits, never finer than one unit
  const int sh = g - t1;                                // bits of sig below the grid
  unsigned int r;
  if (sh <= 0) r = sig << (-sh);
  else if (sh > 9) r = 0;
  else {
    const unsigned int q = sig >> sh, rem = sig & ((1u << sh) - 1u), half = 1u << (sh - 1);
    r = q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u);
  }
  return s | (((unsigned int)g << 1) + r);              // r in [2, 4] of a normal code, [0, 2] of a subnormal one: a carry moves into the exponent field by itself
}
// code * 2^e as a bf16 pattern (always exact, always a normal bf16 or a zero)
__device__ __forceinline__ unsigned int fp4_dq_bits(unsigned int code, int e) {
  const unsigned int s = (code & 8u) << 12, mag = code & 7u;
  if (!mag) return s;
  const unsigned int r = mag < 4 ? mag : (2u + (mag & 1u)) << ((mag >> 1) - 1);      // the magnitude in units of 0.5: 1, 2, 3, 4, 6, 8, 12
  const int mb = 31 - __clz((int)r);
  return s | ((unsigned int)(mb - 1 + e + 127) << 7) | ((r << (7 - mb)) & 0x7fu);
}

// one wave per row: stat[0] = the lowest row that holds a non-finite weight or a |w| >= 2^100 (untouched where there is none)
__global__ __launch_bounds__(64) void fp4_scan_rows_kernel(const bf16_t* W, int K, int* stat) {
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
  if (lane == 0 && (m >> 7) >= (unsigned int)FP4_EXP_BAD) atomicMin(stat, row);
}

struct Fp4QuantArgs {
  bf16_t* W;                // [N][K] inside rows of ldw elements, K % 8 == 0: overwritten with the dequantized values
  int K, ldw, ks, nx;
  unsigned char* Q;         // planes — every byte of them is written here, the padding included — or nullptr: the matrix has no stream
  long long row_bytes;
};

// One wave per row.  A lane takes one chunk per pass, so the four lanes of a group hold one block of 32 k (the row's last block may be shorter): they
// agree on its exponent by two shuffles.  Every chunk is quantized and written back dequantized; where the matrix has a stream the passes walk the k-parts'
// chunk slots, padding lanes included, and each slot gets its codes and each group's first lane stores the block's scale byte.
__global__ __launch_bounds__(64) void fp4_quant_rows_kernel(const Fp4QuantArgs a) {
  const int row = blockIdx.x, lane = threadIdx.x;
  u32x4* w = reinterpret_cast<u32x4*>(a.W + (size_t)row * a.ldw);
  const int nchunk = a.K >> 3, per = 64 * a.nx;
  const int passes = a.Q ? a.ks * a.nx : (nchunk + 63) / 64;
  for (int i = 0; i < passes; i++) {
    const int p = a.Q ? i / a.nx : 0, js = a.Q ? i - p * a.nx : i;      // k-part and chunk slot of the lane
    const int c = p * per + lane + 64 * js;
    const bool live = c < nchunk;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (live) v = w[c];
    unsigned int m = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) m = max(m, max(v[t] & 0x7fffu, (v[t] >> 16) & 0x7fffu));
    m = max(m, (unsigned int)__shfl_xor((int)m, 1, 64));
    m = max(m, (unsigned int)__shfl_xor((int)m, 2, 64));
    const int e = fp4_block_exp(m);
    u32x4 dq;
    unsigned int code = 0u;
#pragma unroll
    for (int t = 0; t < 8; t++) {
      const unsigned int bits = (v[t >> 1] >> (16 * (t & 1))) & 0xffffu;
      const unsigned int q = fp4_code(bits, e);
      code |= q << (4 * t);
      const unsigned int d = fp4_dq_bits(q, e) << (16 * (t & 1));
      if (t & 1) dq[t >> 1] |= d; else dq[t >> 1] = d;
    }
    if (live) w[c] = dq;
    if (a.Q) {
      unsigned char* part = a.Q + (size_t)row * a.row_bytes + (size_t)p * (FP4_SLOT * a.nx);
      *reinterpret_cast<unsigned int*>(part + fp4_code_off(a.nx, lane, js)) = live ? code : 0u;
      if ((lane & 3) == 0) part[fp4_scale_off(a.nx, lane, js)] = (unsigned char)(e + 127);      // (a block of padding has amax 0: byte 127)
    }
  }
}

}  // namespace tgx
