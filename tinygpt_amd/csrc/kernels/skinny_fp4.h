// skinny_fp4.h — Y[M][N] = X[M][K] . dq(W)[N][K]^T for M <= 64 activation rows given as STORED two-term bf16 (hi / lo), the weight operand read as the MXFP4
// stream of option weights.fp4 (gemv_fp4.h: E2M1 codes, one E8M0 scale byte per block of 32 k of a row): the batched decode step, the verify / extend /
// advance passes and short prompts stream gate_up, down and lm_head at 4.25 bits per weight.  Opt-in: option weights.fp4_rows (include/tgx.h; default 0).
// The stream is read as it lies: no second copy of the codes and no second layout exists.
//
// How the layout meets the matrix cores.  A CHUNK (8 codes of 8 consecutive k, one dword) is what lane (weight row lane & 15, k group kg = lane >> 4) feeds
// to one v_mfma_f32_16x16x32_bf16.  RUN R of a row is its 512 k from 512 R: chunk slot j = R % NX of k-part p = R / NX, and its 16 blocks of 32 k, G = 0..15,
// are the chunks of gemv lanes 4G .. 4G + 3 — the MFMA lane's chunk of block G is gemv lane 4G + kg.  In a whole QUAD h (slots 4h .. 4h + 3) the 16 bytes at
// 1024 h + 16 (4G + kg) are therefore the lane's fragments of block G of FOUR runs, dword i for slot 4h + i, and the dword at 256 NX + 64 h + 4 G holds their
// four scales, byte i for slot 4h + i: 16 loads of 16 bytes bring a lane the codes of 2048 k of its row, four more the 64 scale bytes of the row's quad.  The
// SHORT quad (NX % 4 = REM slots) has REM dwords per gemv lane at stride 4 REM and REM scale bytes per block at 64 (NX / 4) + REM G + i.
//
// Work split (gfx950) — skinny_fp8.h's, one departure: the unit a product wave requests at a time is HALF a quad.
//   one workgroup = FIVE waves = 64 weight rows x one K range of launch_skinny's split rule; grid = (ceil(N / 64), K splits).
//   waves 0-3  own 16 weight rows each and stream codes and scales global -> registers, non-temporal.  A HALF QUAD (slots 4h + 2w, 4h + 2w + 1: two runs,
//              1024 k) of 16 rows is 16 loads of 8 bytes per lane (32 VGPRs, 8 KiB per wave), and the NEXT half quad is requested before the current one is
//              touched, 1024 k ahead of use as the FP8 kernel's plane is.  The quad's 64 scale bytes per row (4 loads of 16 bytes, 16 VGPRs) travel with its
//              first half and serve both.  Ordinary loads: the compiler counts them, and nothing else of these waves is in the vector-memory queue.
//   wave 4     moves the activation terms: 64 k of all 16 MB rows of both terms per stage, by LDS-DMA into a ring of 4 stages (skinny_dma.h's image and
//              swizzle), 3 stages ahead.  A wave of its own because vector-memory loads return in order: a wave that waited for an activation stage three
//              stages out would also wait for the codes it asked for 1024 k ahead.
//   One workgroup barrier per stage (wave 4: "stage k has landed"; waves 0-3: "stage k - 1 has been read").
// Activation stages run k ascending, so a quad is consumed run by run: dword i of all 16 blocks (G ascending, two per stage) before dword i + 1.  Why half
// quads and not the whole 16-byte loads: all 16 loads of a quad are live across its four runs, so two whole quads with their scales are 160 VGPRs — measured
// by the compiler at 250-256 with spills at four activation blocks, one workgroup per CU.  Two half quads are 64 + 32 of scales, the FP8 kernel's budget,
// and the registers of a consumed half are the ones the next request lands in.  The two halves of a 64-byte line are requested 1024 k apart by the same
// wave: the line crosses HBM once and L2 twice.  Two more consequences of the stream:
//   * a K range may begin or end inside a quad (down at K = 8192 in ranges of 1024 k is exactly half a quad): a half quad is loaded only if the range holds
//     one of its runs, and only the range's runs are consumed.  A range that begins at a quad's second half loads the quad's scales with it.
//   * the short quad's loads are dwords (at most two per block and half) into the same registers, and its scale bytes — packed REM per block — are spread to
//     the whole quad's form (dword G, byte i) once per short quad by fp4_short_scales, so the four consume bodies (one per slot of a quad) serve both kinds.
// Budget: LDS 4 x (2 x 16 MB rows x 128 B) = 16 / 32 / 64 KiB for MB = 1 / 2 / 4.  VGPRs: 96 for the two half quads and the two scale sets, 4 MB
// accumulators, 8 MB activation fragments, 4 of a decoded fragment (tools/check_spills.py; the counts are in profiles/weights_fp4_rows.txt).  No
// instantiation uses scratch.
//
// Decode: v_cvt_scalef32_pk_bf16_fp4 turns one byte of a chunk — two consecutive k — under the block's scale operand into the two bf16 halves of one dword of
// the MFMA fragment: four converts per chunk, no multiply, no permute.  The operand is made as gemv_fp4.h's fp4_scale_operand makes it: ONE shift that puts
// the scale byte into bits 30:23 (what the shift leaves elsewhere is not read).  Every dq = code * 2^e is exactly a bf16, so an exact convert gives the
// dequantized master's value bit for bit.  It is exact on the hardware: tools/probes/fp4_cvt_bf16_probe.hip finds 0 mismatches over all codes, byte selects
// and scale bytes 2..227, with clean and dirty operands (profiles/weights_fp4_rows.txt), and tests/test_hip_fp4_rows.py holds the kernel to the master bit for
// bit.  So the bf16 form shipped; the fp32 convert + v_perm_b32 fall-back was not needed.
// The scale reaches the weight inside the convert: never a partial sum, never the activations.
//
// Accumulation order is skinny.h's and skinny_dma.h's: per output element and K range k ascending in steps of 32, small term first; K ranges, slabs and
// epilogues are launch_skinny's; the gate_up row mapping is the FP8 kernel's (fp4_quant_rows_kernel lays out the merged matrix row by row of the master: gate
// rows, then up rows).  The product is bit-identical to those kernels over the dequantized master.
//
// Coverage (decided on the host, skinny_fp4_covers): K % 512 == 0 — no padding lane is ever met — and, for a split product, k_per % 64 == 0: whole stages.  A
// range that is no multiple of 512 k begins or ends inside a run and the kernel consumes that run's stages of the range only (launch_skinny's rule gives
// down at K = 10240 / 12288 over 256 output rows ranges of 768 k; whole runs only would leave them on the master).  Any NX up to 8; a single-range stream
// (Fp4Mat::parts == 1).  Everything else takes the master through the existing kernels and is counted
// (weights.fp4_row_fallbacks).  Out of scope: qkv / o_proj, 65-128 rows, fp16, three-term activations, the scaled MFMA's native fp4 operand forms.
#pragma once
#include <type_traits>
#include "skinny_dma.h"

namespace tgx {

struct SkinnyFp4Args {
  GemmArgs g;               // g.B is not read
  const unsigned char* Q;   // the stream: codes and block scales (gemv_fp4.h)
  long long row_bytes;
  int nx;                   // chunk slots (runs) per k-part
};

constexpr int SK4_D = 4;                                  // stages of the activation ring
constexpr int SK4_THREADS = 320;                          // four product waves + the activation wave
constexpr int SK4_SLOT = 272;                             // bytes of one chunk slot of a k-part (gemv_fp4.h's FP4_SLOT)
__host__ __device__ constexpr int sk4_stage_bytes(int mb) { return 2 * mb * 16 * SKD_KS * 2; }
__host__ __device__ constexpr size_t sk4_lds_bytes(int mb) { return (size_t)SK4_D * sk4_stage_bytes(mb); }

// byte I of the scale dword in the exponent field of the convert's scale operand (gemv_fp4.h's fp4_scale_operand)
// The shift is volatile: a quad's scale dwords do not change while its runs are consumed, and left to itself the compiler hoists all 64 shifted operands of a
// quad out of the run loop and keeps them in registers (measured: 202-223 VGPRs instead of the counts in the profile).
template <int I> __device__ __forceinline__ float sk4_scale_operand(unsigned int sd) {
  unsigned int r;
  if (I < 3) asm volatile("v_lshlrev_b32 %0, %1, %2" : "=v"(r) : "n"(23 - 8 * (I < 3 ? I : 0)), "v"(sd));
  else asm volatile("v_lshrrev_b32 %0, 1, %1" : "=v"(r) : "v"(sd));
  return __uint_as_float(r);
}

// the 8 codes of a chunk under the scale operand `so` -> the bf16 fragment of dq = code * 2^e
__device__ __forceinline__ bf16x8 fp4_chunk_bf16(unsigned int d, float so) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const bf16x2 v0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, so, 0), v1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, so, 1);
  const bf16x2 v2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, so, 2), v3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, so, 3);
  return bf16x8{v0[0], v0[1], v1[0], v1[1], v2[0], v2[1], v3[0], v3[1]};
}

// the short quad's scale bytes (REM per block, byte REM G + i of the 16 REM loaded) -> the whole quad's form: dword G, byte i
template <int REM>
__device__ __forceinline__ void fp4_short_scales(u32x4* s) {
  unsigned int o[16];
#pragma unroll
  for (int G = 0; G < 16; G++) {
    unsigned int v = 0;
#pragma unroll
    for (int i = 0; i < REM; i++) {
      const int b = G * REM + i;
      v |= ((s[b >> 4][(b >> 2) & 3] >> (8 * (b & 3))) & 0xffu) << (8 * i);
    }
    o[G] = v;
  }
#pragma unroll
  for (int G = 0; G < 16; G++) s[G >> 2][G & 3] = o[G];
}

template <int EPI, int MB>
__global__ __launch_bounds__(SK4_THREADS) void skinny_fp4_kernel(const SkinnyFp4Args pa) {
  constexpr int DT = DT_BF16, KS = SKD_KS, XROWS = 2 * MB * 16, XP = XROWS / 8, D = SK4_D, STAGE = sk4_stage_bytes(MB);
  static_assert((D - 2) * XP <= 63, "vmcnt is a 6-bit counter");
  extern __shared__ __attribute__((aligned(1024))) unsigned char sk4_lds[];
  const GemmArgs& a = pa.g;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k_begin = EPI == GEMM_PARTIAL ? (int)blockIdx.y * a.k_per : 0;
  const int k_end = EPI == GEMM_PARTIAL ? min(a.K, k_begin + a.k_per) : a.K;
  const int r_begin = k_begin >> 9, r_end = (k_end + 511) >> 9;      // the runs the range touches; K is whole runs, a split range whole stages (the launcher)
  const int nst = (k_end - k_begin) >> 6;                     // stages of 64 k: one barrier each in every wave

  if (wv == 4) {      // ---- the activation wave: skinny_dma.h's stage image, all pieces from this wave (skinny_fp8.h)
    const unsigned lds_base = (unsigned)(size_t)sk4_lds;
    const int prow = lane >> 3, pchunk = lane & 7;
    const bf16_t* src[XP];
#pragma unroll
    for (int j = 0; j < XP; j++) {
      const int row = j * 8 + prow;                           // row of the stage image: term t, activation row m
      const int t = row / (MB * 16), m = row - t * (MB * 16);
      const int chunk = pchunk ^ ((row >> 1) & 7);
      src[j] = (t == 0 ? a.A_hi : a.A_lo) + (size_t)min(m, a.M - 1) * a.K + chunk * 8;      // rows past M: clamped copies, masked at the store
    }
    // stages past the end reload the last real one (every wait then counts the same pieces)
    auto issue = [&](int s) {
      const int k0 = k_begin + min(s, nst - 1) * KS;
      const unsigned sb = lds_base + (unsigned)((s % D) * STAGE);
#pragma unroll
      for (int j = 0; j < XP; j++) dma_1k(src[j] + k0, sb + (unsigned)(j * 1024));
    };
    if (nst > 0) {
#pragma unroll
      for (int s = 0; s < D - 1; s++) issue(s);
      for (int k = 0; k < nst; k++) {
        wait_vmcnt_imm<(D - 2) * XP>();                       // stage k landed: only the D - 2 stages issued after it may still fly
        __builtin_amdgcn_s_barrier();                         // the product waves may read it; they are done with stage k - 1
        issue(k + D - 1);                                     // into the buffer stage k - 1 occupied
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // no DMA may land in this CU's LDS after the workgroup has gone
    }
    return;
  }

  // ---- the product waves
  const int n0 = blockIdx.x * 64 + wv * 16;
  const bool inter = EPI == GEMM_SILU || (EPI == GEMM_PARTIAL && a.interleave);
  const int frow = lane & 15, fsw = (frow >> 1) & 7, kg = lane >> 4;
  const int nb = min(n0 + frow, a.N - 1);                     // clamped: rows past N reload the last one, masked at the store
  const size_t brow = inter ? (size_t)((nb & 1) ? a.inter : 0) + (size_t)(nb >> 1) : (size_t)nb;
  const unsigned char* wrow = pa.Q + brow * (size_t)pa.row_bytes;
  const int NX = pa.nx, FULL = NX >> 2, REM = NX & 3;
  // the half quad of slot j (even) of k-part p: codes into dc[G] (dword i: slot j + i); with_scales: the quad's scale bytes into ds.  Every address lies inside
  // the row's k-part, 272 NX bytes from `part`
  auto load_half = [&](u32x2* dc, u32x4* ds, int p, int j, bool with_scales) {
    const unsigned char* part = wrow + (size_t)p * (size_t)(SK4_SLOT * NX);
    const int h = j >> 2, w = (j >> 1) & 1;
    const unsigned char* sp = part + 256 * NX + 64 * h;
    if (h < FULL) {
      const unsigned char* cp = part + h * 1024 + kg * 16 + w * 8;
#pragma unroll
      for (int G = 0; G < 16; G++) dc[G] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(cp + G * 64));
      if (with_scales) {
#pragma unroll
        for (int t = 0; t < 4; t++) ds[t] = load_nt(reinterpret_cast<const u32x4*>(sp + t * 16));
      }
    } else {            // the short quad: REM dwords per gemv lane, one or two of them in this half; 16 REM scale bytes
      const unsigned char* cp = part + FULL * 1024 + kg * 4 * REM + w * 8;
      const bool two = REM - 2 * w > 1;
#pragma unroll
      for (int G = 0; G < 16; G++) {
        const unsigned int* q = reinterpret_cast<const unsigned int*>(cp + G * 16 * REM);
        dc[G][0] = __builtin_nontemporal_load(q);
        if (two) dc[G][1] = __builtin_nontemporal_load(q + 1);
      }
      if (with_scales) {
        ds[0] = load_nt(reinterpret_cast<const u32x4*>(sp));
        if (REM > 1) ds[1] = load_nt(reinterpret_cast<const u32x4*>(sp + 16));
        if (REM > 2) ds[2] = load_nt(reinterpret_cast<const u32x4*>(sp + 32));
      }
    }
  };

  f32x4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; mb++) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x2 cur[16], nxt[16];
  u32x4 scur[4], snxt[4];
#pragma unroll
  for (int G = 0; G < 16; G++) { cur[G] = u32x2{0u, 0u}; nxt[G] = cur[G]; }      // (a short quad leaves the dwords it does not have as they are)
#pragma unroll
  for (int t = 0; t < 4; t++) { scur[t] = u32x4{0u, 0u, 0u, 0u}; snxt[t] = scur[t]; }
  int kst = 0;                                                // stages consumed
  // one run = 8 stages = 16 k-steps: slot I of the quad, dword I & 1 of the half quad in `cur`, scale byte I.  [s_lo, s_hi): the run's stages inside the K
  // range — all 8 but in the first and last run of a range that is no multiple of 512 k
  auto consume = [&](auto i_c, int s_lo, int s_hi) {
    constexpr int I = decltype(i_c)::value;
#pragma unroll
    for (int st = 0; st < 8; st++) {
      if (st < s_lo || st >= s_hi) continue;                  // (workgroup-uniform)
      __builtin_amdgcn_s_barrier();                         // stage kst has landed
      const unsigned char* sp = sk4_lds + (size_t)(kst % D) * STAGE;
      kst++;
#pragma unroll
      for (int ks = 0; ks < KS / 32; ks++) {
        const int G = 2 * st + ks;
        const int chunk = ((ks * 4 + kg) ^ fsw) * 16;
        const bf16x8 fb = fp4_chunk_bf16(cur[G][I & 1], sk4_scale_operand<I>(scur[G >> 2][G & 3]));
        bf16x8 fa[MB][2];
#pragma unroll
        for (int mb = 0; mb < MB; mb++)
#pragma unroll
          for (int t = 0; t < 2; t++) fa[mb][t] = *reinterpret_cast<const bf16x8*>(sp + ((t * MB + mb) * 16 + frow) * (KS * 2) + chunk);
#pragma unroll
        for (int mb = 0; mb < MB; mb++)
#pragma unroll
          for (int t = 1; t >= 0; t--) acc[mb] = mfma16x16<DT>(fa[mb][t], fb, acc[mb]);     // small term first
      }
    }
  };
  int run = r_begin;
  bool new_scales = true;                                     // scur holds a quad's scales as loaded (a short quad's are still to be spread)
  if (run < r_end) { const int p = run / NX; load_half(cur, scur, p, (run - p * NX) & ~1, true); }
  while (run < r_end) {
    const int p = run / NX, j = run - p * NX;
    const int u_end = min(p * NX + min((j | 1) + 1, NX), r_end);      // the half quad's runs inside this K range: [run, u_end)
    bool nxt_scales = false;
    if (u_end < r_end) {                                      // (u_end is the first slot of a half quad)
      const int p2 = u_end / NX, j2 = u_end - p2 * NX;
      nxt_scales = !(j2 & 2);                                 // a quad's first half brings its scales
      load_half(nxt, snxt, p2, j2, nxt_scales);
    }
    if (new_scales && (j >> 2) == FULL) { if (REM == 1) fp4_short_scales<1>(scur); else if (REM == 2) fp4_short_scales<2>(scur); else fp4_short_scales<3>(scur); }
    new_scales = false;
    for (int i = j & 3; run < u_end; i++, run++) {
      const int s_lo = max(k_begin - (run << 9), 0) >> 6, s_hi = min(k_end - (run << 9), 512) >> 6;
      if (i == 0) consume(std::integral_constant<int, 0>{}, s_lo, s_hi);
      else if (i == 1) consume(std::integral_constant<int, 1>{}, s_lo, s_hi);
      else if (i == 2) consume(std::integral_constant<int, 2>{}, s_lo, s_hi);
      else consume(std::integral_constant<int, 3>{}, s_lo, s_hi);
    }
#pragma unroll
    for (int G = 0; G < 16; G++) cur[G] = nxt[G];
    if (nxt_scales) {
#pragma unroll
      for (int t = 0; t < 4; t++) scur[t] = snxt[t];
      new_scales = true;
    }
  }

  // D: col n = lane&15, row m = 4*(lane>>4) + r   (skinny.h's epilogue)
  const int col = n0 + (lane & 15);
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = 16 * mb + 4 * (lane >> 4) + r;
      const float v = acc[mb][r];
      if (EPI == GEMM_SILU) {      // even lanes hold gate_i, odd lanes up_i (i = col / 2): the pair meets over the DPP crossbar
        const float other = dpp_mov<0xB1, 0xf>(v);
        if ((lane & 1) || col >= a.N || row >= a.M) continue;
        const size_t o = (size_t)row * a.inter + (size_t)(col >> 1);
        split16<DT>((v / (1.0f + expf(-v))) * other, a.out_hi[o], a.out_lo[o]);
        continue;
      }
      if (col >= a.N || row >= a.M) continue;
      if (EPI == GEMM_PARTIAL) { a.part[((size_t)blockIdx.y * a.M + row) * a.N + col] = v; continue; }
      float* dstp = a.C + (size_t)row * a.ldc + col;
      const float o = v + (a.bias ? elem_to_f32<DT>(a.bias[col]) : 0.f);
      *dstp = (EPI == GEMM_RESIDUAL) ? (*dstp + o) : o;
    }
}

}  // namespace tgx
