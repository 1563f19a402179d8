// gemv_packed.h — the batch-1 weight stream of gate_up, down and lm_head over bf16 weights stored as a LOSSLESS 12-bit form: 25 % fewer bytes per
// launch, every weight the kernel multiplies bit for bit the uploaded one (DESIGN.md §5 "Exponent-packed weights").
//
// Format "HL" of a bf16 matrix [N][K], K % 8 == 0 (option weights.packed, made once in tgx_finalize by pack_rows_kernel below; the bf16 original stays).
// A bf16 pattern is split into its LOW byte L = e0 << 7 | mantissa (e0 = the lowest bit of the exponent field) and its HIGH byte sign << 7 | exponent_field >> 1;
// the low byte is stored as it is, the high byte as a nibble:
//   window          E0h = max((Emax >> 1) - 7, 0), Emax = the largest exponent field below 255 in the matrix.  IN BAND are the weights whose exponent field
//                   lies in [2 E0h, 2 E0h + 15] without 0 and 255: 16 binades when Emax is odd, 15 when it is even.  Their nibble is n = sign << 3 | d,
//                   d = (exponent_field >> 1) - E0h in 0..7.  Every other weight (zeros, subnormals, anything below the window, inf / NaN) is an ESCAPE: it is
//                   written in band as n = 0, L = 0 (there is NO in-band flag) and listed in its row's record.
//   chunk           8 consecutive k of a row -> 12 bytes: two dwords L0, L1 of the low bytes in k order (w0..w3, w4..w7) and one dword of eight nibbles
//                     Nb = sum over t = 0..3 of n(w[t]) << 8t | n(w[4 + t]) << (8t + 4)
//   decode          four weights at once: t = Nb & 0x0f0f0f0f (or (Nb >> 4) & 0x0f0f0f0f for w4..w7), H4 = (((t << 4) + t) & 0x87878787) + E0h * 0x01010101
//                   (no carry crosses a byte: d + E0h <= 127); weight t as fp32 bits is H4.byte[t] << 24 | L.byte[t] << 16 — ONE byte permute with a constant
//                   selector, no bf16 intermediate.
//   escape record   16 bytes per (row, k-part), rec[row * ks + p]: up to PACKED_ESC entries `k << 16 | bits` (k the ROW's k, bits the weight's true 16 bits) of
//                   the escapes whose chunk k / 8 lies in k-part p's range [c_begin(p), c_end(p)) (below), in k order from entry 0, unused entries 0xffffffff.
//                   A wave of a K-split launch reads the record of its own k-part only: it never walks the escapes of the other waves' ranges.  At ks = 1
//                   this is one record per row.  A matrix with more than PACKED_ESC escapes in one (row, k-part) is NOT packed (per-matrix fallback to
//                   kernels/gemv.h, decided at finalize).
//   physical layout follows the thread -> (row, k) map of gemv_kernel launched with `ks` waves per row pair, NX = ceil(K / 8 / (64 ks)) chunks per lane:
//                   lane l of k-part p owns chunks c = p * per + l + 64 j (per = 64 NX), j = 0..NX-1.  Its chunks go in QUADS q = j / 4 of three 1 KiB planes
//                     plane 0: lane l's 16 bytes = L0, L1 of chunk 4q, L0, L1 of chunk 4q + 1       plane 1: the same of chunks 4q + 2, 4q + 3
//                     plane 2: lane l's 16 bytes = Nb of chunks 4q .. 4q + 3
//                   row r, k-part p, quad q, plane i starts at byte r * row_bytes + ((p * NQ + q) * 3 + i) * 1024, NQ = ceil(NX / 4), row_bytes = ks * NQ * 3072.
//                   Chunks past the row's end (j >= NX, c >= the k-part's end) are padding: all zero (a finite value; its activation is zero).
//                   At the 1B / 3B / 7B shapes NX is 4 or 8 and there is no padding: 1.5 bytes per weight.
//
// The kernel is gemv_kernel<DT_BF16, PRO, EPI, NX, 1, XACC> (kernels/gemv.h) with the weight loads and the dot product replaced: a lane decodes a chunk of
// each of its unit's two rows straight into fp32 and runs the two rows' FMA chains as ONE chain of 2-vectors (v_pk_fma_f32: both halves multiply the same
// activation).  FMA is exact per element, the element order 0..7, the even / odd-j accumulators, the wave reduction and the K-part sums are those of the
// plain kernel: the results are bit-identical.  Every lane issues 16-byte non-temporal loads over whole 1 KiB planes; the escape records of the wave's k-part
// of its two rows (one 16-byte load per row, the same address in every lane) leave with the unit's weight loads and are moved to scalar registers one unit
// ahead; the repair makes the escape's fp32 value bits << 16 (its two bytes inserted ahead of the permute) and runs only in a wave whose own record is
// non-empty — a wave-uniform branch with VALU work only, no load under it.
#pragma once
#include "gemv.h"

namespace tgx {

constexpr int PACKED_ESC = 4;            // escape entries per (row, K-part) (one 16-byte record)
constexpr int PACKED_K_MAX = 32768;      // k < 2^15: the empty entry 0xffffffff can never name a chunk of the row

struct PackedQuad { u32x4 l01, l23, nb; };      // one lane's 16 bytes of a quad's three planes

struct GemvPackedArgs {
  GemvArgs g;               // g.W is not read
  const unsigned char* P;   // packed planes
  const u32x4* rec;         // [N][ks] escape records
  long long row_bytes;
  unsigned int e0h4;        // E0h * 0x01010101
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// acc += w * x[0] (pk_fma_x0) or w * x[1] (pk_fma_x1) in both halves: v_pk_fma_f32 with the activation's half chosen by op_sel.  Written out because
// __builtin_elementwise_fma over a splat keeps every activation twice in registers (64 instead of 32 VGPRs at NX = 4, which spills); the instruction and its
// per-element result are the same.
__device__ __forceinline__ f32x2 pk_fma_x0(f32x2 w, f32x2 x, f32x2 acc) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(w), "v"(x));
  return acc;
}
__device__ __forceinline__ f32x2 pk_fma_x1(f32x2 w, f32x2 x, f32x2 acc) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(w), "v"(x));
  return acc;
}

// four nibbles, one per byte of t -> the four high bytes sign << 7 | exponent_field >> 1
__device__ __forceinline__ unsigned int packed_high4(unsigned int t, unsigned int e0h4) { return (((t << 4) + t) & 0x87878787u) + e0h4; }
// weight T of a half chunk as fp32: H.byte[T] << 24 | L.byte[T] << 16 (v_perm_b32: selector bytes 4..7 name H's bytes, 0..3 L's, 0x0c a zero byte)
template <int T> __device__ __forceinline__ float packed_weight(unsigned int H, unsigned int L) {
  return __uint_as_float(__builtin_amdgcn_perm(H, L, ((4u + T) << 24) | ((unsigned int)T << 16) | 0x0c0cu));
}
// a chunk's bytes ahead of the permutes: the high bytes H0 (w0..w3), H1 (w4..w7) expanded from the nibbles, and the low bytes as loaded
struct PackedBytes { unsigned int H0, H1, L0, L1; };
__device__ __forceinline__ PackedBytes packed_expand(unsigned int L0, unsigned int L1, unsigned int Nb, unsigned int e0h4) {
  return PackedBytes{packed_high4(Nb & 0x0f0f0f0fu, e0h4), packed_high4((Nb >> 4) & 0x0f0f0f0fu, e0h4), L0, L1};
}
__device__ __forceinline__ void packed_weights(const PackedBytes& b, float f[8]) {
  f[0] = packed_weight<0>(b.H0, b.L0); f[1] = packed_weight<1>(b.H0, b.L0); f[2] = packed_weight<2>(b.H0, b.L0); f[3] = packed_weight<3>(b.H0, b.L0);
  f[4] = packed_weight<0>(b.H1, b.L1); f[5] = packed_weight<1>(b.H1, b.L1); f[6] = packed_weight<2>(b.H1, b.L1); f[7] = packed_weight<3>(b.H1, b.L1);
}
// The repair: the row's record (in scalar registers) over the chunks c0 .. c0 + 63 that the wave's lanes hold now (c0 wave-uniform).  An escape's fp32 value
// is bits << 16, i.e. its two bytes in the places the permute reads: the entry's bytes are inserted into the expanded H and the L dword of the lane that
// holds its chunk (the expanded high byte is a whole byte, so every 16-bit pattern fits).  An entry of another chunk range — the empty entry names chunk
// 8191 — costs scalar work only.
__device__ __forceinline__ void packed_repair(PackedBytes& b, const u32x4 rec, int c0, int lane) {
#pragma unroll
  for (int e = 0; e < PACKED_ESC; e++) {
    const unsigned int en = rec[e], l = (en >> 19) - (unsigned int)c0;
    if (l < 64u) {
      const unsigned int sh = (en >> 13) & 0x18u;                                   // 8 * (t & 3), t = k & 7
      const unsigned int vh = ((en >> 8) & 0xffu) << sh, vl = (en & 0xffu) << sh;
      const unsigned int m = (unsigned int)lane == l ? 0xffu << sh : 0u;
      const unsigned int m0 = (en & 0x40000u) ? 0u : m, m1 = (en & 0x40000u) ? m : 0u;      // t < 4: the first half chunk
      b.H0 = (b.H0 & ~m0) | (vh & m0); b.L0 = (b.L0 & ~m0) | (vl & m0);
      b.H1 = (b.H1 & ~m1) | (vh & m1); b.L1 = (b.L1 & ~m1) | (vl & m1);
    }
  }
}

// R = 1, bf16.  The three forms: (PRO_RMSNORM, EPI_SILU_MUL), (PRO_PLAIN, EPI_RESIDUAL), (PRO_RMSNORM, EPI_LOGITS).  Everything outside load_unit and the
// decode + dot block is gemv_kernel's text for R = 1.
template <int PRO, int EPI, int NX, bool XACC = false>
__global__ __launch_bounds__(256, NX <= 4 ? 4 : 1) void gemv_packed_kernel(const GemvPackedArgs pa) {
  constexpr int DT = DT_BF16;
  constexpr int NQ = (NX + 3) / 4;
  typedef elem_t<DT> E;
  static_assert(PRO == PRO_PLAIN || PRO == PRO_RMSNORM, "packed forms: plain or RMSNorm prologue");
  static_assert(EPI == EPI_SILU_MUL || EPI == EPI_RESIDUAL || EPI == EPI_LOGITS, "packed forms: gate_up, down, lm_head");
  const GemvArgs& a = pa.g;
  const int n_wg = (int)gridDim.x;
  __shared__ float ps[4][2];
  __shared__ float sv[1][4];
  __shared__ int si[1][4];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int KS = a.ks, UPB = 4 / KS;
  const int slot = wv / KS, kpart = wv - slot * KS;
  const int nchunk = a.K >> 3;                                         // 16-byte weight slices per row
  const int per = ((nchunk + KS * 64 - 1) / (KS * 64)) * 64;           // slices per k-part (multiple of 64)
  const int c_begin = min(kpart * per, nchunk), c_end = min(c_begin + per, nchunk);
  const int stride = n_wg * UPB;
  const int c0_u = __builtin_amdgcn_readfirstlane(c_begin);            // the chunk of lane 0 at j = 0, in a scalar register (the repair's range test)

  int cidx[NX];
  bool cok[NX];
#pragma unroll
  for (int j = 0; j < NX; j++) {
    const int c = c_begin + lane + 64 * j;
    cok[j] = c < c_end;
    cidx[j] = cok[j] ? c : max(c_end - 1, 0);    // clamped: always a legal slice of the row
  }

  const size_t lane_off = (size_t)kpart * NQ * 3072 + (size_t)lane * 16;      // this lane's 16 bytes of its k-part's first plane
  PackedQuad wa[NQ], wb[NQ], na[NQ], nb[NQ];
  // the two rows' escape records: loaded ahead of the unit's planes (every lane the same 16 bytes), moved to scalar registers one unit ahead of their use
  u32x4 ea, eb, nea = {}, neb = {};
  auto load_unit = [&](int ub, PackedQuad* ta, PackedQuad* tb, u32x4& ra_rec, u32x4& rb_rec) {
    const int u = min(ub + slot, a.units - 1);
    int ra, rb; bool v;
    unit_rows<EPI>(a, u, ra, rb, v);
    ra_rec = pa.rec[(size_t)ra * KS + kpart]; rb_rec = pa.rec[(size_t)rb * KS + kpart];      // this wave's K-part of either row
    const unsigned char* pra = pa.P + (size_t)ra * pa.row_bytes + lane_off;
    const unsigned char* prb = pa.P + (size_t)rb * pa.row_bytes + lane_off;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const u32x4* qa = reinterpret_cast<const u32x4*>(pra + (size_t)q * 3072);
      const u32x4* qb = reinterpret_cast<const u32x4*>(prb + (size_t)q * 3072);
      ta[q].l01 = load_nt(qa); ta[q].l23 = load_nt(qa + 64); ta[q].nb = load_nt(qa + 128);
      tb[q].l01 = load_nt(qb); tb[q].l23 = load_nt(qb + 64); tb[q].nb = load_nt(qb + 128);
    }
  };
  auto rec_uniform = [](const u32x4 v) {
    return u32x4{(unsigned int)__builtin_amdgcn_readfirstlane((int)v[0]), (unsigned int)__builtin_amdgcn_readfirstlane((int)v[1]),
                 (unsigned int)__builtin_amdgcn_readfirstlane((int)v[2]), (unsigned int)__builtin_amdgcn_readfirstlane((int)v[3])};
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
  // (only the first: a second unit sent ahead of the prologue fits the registers, and made the gate_up launch 1.8 us LONGER — profiles/packed_weights_hl.txt)
  if (ub < a.units) load_unit(ub, wa, wb, nea, neb);
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
  ea = rec_uniform(nea); eb = rec_uniform(neb);

  for (; ub < a.units; ub += stride) {   // trip count uniform per workgroup
    const bool has_next = ub + stride < a.units;
    if (has_next) load_unit(ub + stride, na, nb, nea, neb);

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
    const bool rep_a = ea[0] != 0xffffffffu, rep_b = eb[0] != 0xffffffffu;      // (wave-uniform: records fill from entry 0; true only where this wave's own K-part holds an escape)
#pragma unroll
    for (int j = 0; j < NX; j++) {
      const int q = j >> 2, jj = j & 3;
      const u32x4 la4 = (jj & 2) ? wa[q].l23 : wa[q].l01, lb4 = (jj & 2) ? wb[q].l23 : wb[q].l01;
      PackedBytes ba = packed_expand(la4[(jj & 1) * 2], la4[(jj & 1) * 2 + 1], wa[q].nb[jj], pa.e0h4);
      PackedBytes bb = packed_expand(lb4[(jj & 1) * 2], lb4[(jj & 1) * 2 + 1], wb[q].nb[jj], pa.e0h4);
      if (rep_a) packed_repair(ba, ea, c0_u + 64 * j, lane);
      if (rep_b) packed_repair(bb, eb, c0_u + 64 * j, lane);
      float fa[8], fb[8];
      packed_weights(ba, fa); packed_weights(bb, fb);
      f32x2 acc = (j & 1) ? acc1 : acc0;
#pragma unroll
      for (int t = 0; t < 8; t += 2) {
        const f32x2 x2 = f32x2{xr[j][t], xr[j][t + 1]};
        acc = pk_fma_x0(f32x2{fa[t], fb[t]}, x2, acc);
        acc = pk_fma_x1(f32x2{fa[t + 1], fb[t + 1]}, x2, acc);
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
    for (int q = 0; q < NQ; q++) { wa[q] = na[q]; wb[q] = nb[q]; }
    ea = rec_uniform(nea); eb = rec_uniform(neb);      // (the records left before the next unit's planes: this waits for nothing behind them)
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

// ---- the packer (tgx_finalize) ---------------------------------------------------------------------------------------------------------------------
// stat[0] = Emax, stat[1] = rows with a K-part whose record overflowed, stat[2] = escapes of the matrix, stat[3] = most escapes in one ROW (all its K-parts)
__global__ __launch_bounds__(256) void packed_maxexp_kernel(const bf16_t* W, size_t n8, int* stat) {
  int m = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    const u32x4 v = reinterpret_cast<const u32x4*>(W)[i];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int e0 = (v[t] >> 7) & 0xff, e1 = (v[t] >> 23) & 0xff;
      if (e0 < 255) m = max(m, e0);
      if (e1 < 255) m = max(m, e1);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(stat, m);
}

// out of the window [2 E0h, 2 E0h + 15], or a zero / subnormal / inf / NaN at its edges
__device__ __forceinline__ bool packed_is_escape(unsigned int bits, int E0h) {
  const int e = (int)((bits >> 7) & 0xff), d = (e >> 1) - E0h;
  return d < 0 || d > 7 || e == 0 || e == 255;
}

struct PackRowsArgs {
  const bf16_t* W;          // [N][K]
  int N, K, ks, nx;
  unsigned char* P;
  u32x4* rec;
  long long row_bytes;
  int* stat;
};

// one wave per row: the records of the row's K-parts (ks <= 4), then its planes
__global__ __launch_bounds__(64) void pack_rows_kernel(const PackRowsArgs a) {
  __shared__ unsigned int ent[4][PACKED_ESC];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int E0h = max((a.stat[0] >> 1) - 7, 0);
  const bf16_t* w = a.W + (size_t)row * a.K;
  const int nchunk = a.K >> 3, nq = (a.nx + 3) / 4;
  const int per = ((nchunk + a.ks * 64 - 1) / (a.ks * 64)) * 64;
  if (lane < 4 * PACKED_ESC) ent[lane / PACKED_ESC][lane % PACKED_ESC] = 0xffffffffu;
  __syncthreads();
  int cnt = 0, part = 0, pcnt = 0, pmax = 0;      // escapes of the row; the K-part of the 64 k at hand and its escapes so far; the most in one K-part
  for (int k0 = 0; k0 < a.K; k0 += 64) {
    // the 8 chunks k0 / 8 .. k0 / 8 + 7 lie in one K-part (`per` is a multiple of 64 chunks), the one whose [c_begin, c_end) holds them; k ascends, so do the parts
    const int kp = (k0 >> 3) / per;
    if (kp != part) { part = kp; pcnt = 0; }
    const int k = k0 + lane;
    unsigned int bits = 0; bool esc = false;
    if (k < a.K) { bits = w[k]; esc = packed_is_escape(bits, E0h); }
    const unsigned long long bal = __ballot(esc);
    const int p = pcnt + __popcll(bal & ((1ull << lane) - 1ull));
    if (esc && p < PACKED_ESC) ent[part][p] = ((unsigned int)k << 16) | bits;
    const int n = __popcll(bal);
    cnt += n; pcnt += n; pmax = max(pmax, pcnt);
  }
  __syncthreads();
  if (lane < a.ks) a.rec[(size_t)row * a.ks + lane] = u32x4{ent[lane][0], ent[lane][1], ent[lane][2], ent[lane][3]};
  if (lane == 0) {
    if (pmax > PACKED_ESC) atomicAdd(a.stat + 1, 1);
    if (cnt) { atomicAdd(a.stat + 2, cnt); atomicMax(a.stat + 3, cnt); }
  }
  for (int p = 0; p < a.ks; p++) {
    const int c_begin = min(p * per, nchunk), c_end = min(c_begin + per, nchunk);
    for (int q = 0; q < nq; q++) {
      unsigned int L[8], Nb[4];
#pragma unroll
      for (int jj = 0; jj < 4; jj++) {
        const int j = 4 * q + jj, c = c_begin + lane + 64 * j;
        L[2 * jj] = 0; L[2 * jj + 1] = 0; Nb[jj] = 0;
        if (j < a.nx && c < c_end) {
          const u32x4 v = reinterpret_cast<const u32x4*>(w)[c];
          unsigned int lo[8], n[8];
#pragma unroll
          for (int t = 0; t < 8; t++) {
            const unsigned int bits = (v[t >> 1] >> (16 * (t & 1))) & 0xffffu;
            const bool esc = packed_is_escape(bits, E0h);
            lo[t] = esc ? 0u : (bits & 0xffu);
            n[t] = esc ? 0u : (((bits >> 12) & 8u) | (((bits >> 8) & 0x7fu) - (unsigned int)E0h));
          }
          L[2 * jj] = lo[0] | (lo[1] << 8) | (lo[2] << 16) | (lo[3] << 24);
          L[2 * jj + 1] = lo[4] | (lo[5] << 8) | (lo[6] << 16) | (lo[7] << 24);
          unsigned int nn = 0;
#pragma unroll
          for (int t = 0; t < 4; t++) nn |= (n[t] << (8 * t)) | (n[4 + t] << (8 * t + 4));
          Nb[jj] = nn;
        }
      }
      u32x4* dst = reinterpret_cast<u32x4*>(a.P + (size_t)row * a.row_bytes + ((size_t)p * nq + q) * 3072) + lane;
      dst[0] = u32x4{L[0], L[1], L[2], L[3]};
      dst[64] = u32x4{L[4], L[5], L[6], L[7]};
      dst[128] = u32x4{Nb[0], Nb[1], Nb[2], Nb[3]};
    }
  }
}

}  // namespace tgx
