// skinny_fp8.h — Y[M][N] = X[M][K] . dq(W)[N][K]^T for M <= 64 activation rows given as STORED two-term bf16 (hi / lo), the weight operand read as the E4M3 code
// planes and row scales of option weights.fp8 (gemv_fp8.h): the batched decode step, the verify / extend passes and short prompts stream gate_up, down and lm_head
// at one byte per weight.  Opt-in: option weights.fp8_rows (include/tgx.h; default 0).  The planes are read as they lie: no second copy of the codes exists.
//
// How the layout meets the matrix cores: a CHUNK (8 codes of 8 consecutive k) is what lane (weight row lane & 15, k group lane >> 4) feeds to one
// v_mfma_f32_16x16x32_bf16.  RUN R of a row is its 64 chunks of k in [512 R, 512 R + 512); with NX runs per k-part and NH = ceil(NX / 2) planes, run R lies in
// plane (R / NX) NH + (R % NX) / 2, in the lower (even R % NX) or upper 8 bytes of every 16.  The 16 bytes at plane + 64 s + 16 g are the fragments of k-step s
// (k group g) of the plane's two runs.
//
// Work split (gfx950): one workgroup = FIVE waves = 64 weight rows x one K range of launch_skinny's split rule; grid = (ceil(N / 64), K splits).
//   waves 0-3  own 16 weight rows each and stream their codes global -> registers, non-temporal: one plane of 16 rows is 16 loads of 16 bytes per lane (64 VGPRs,
//              16 KiB per wave), and the NEXT plane is requested before the current one is touched — 16 KiB per wave, 64 KiB per workgroup in flight, 1024 k
//              ahead of use.  These are ordinary loads: the compiler counts them, and nothing else of these waves is in the vector-memory queue.
//   wave 4     moves the activation terms: 64 k of all 16 MB rows of both terms per stage, by LDS-DMA into a ring of 4 stages (skinny_dma.h's image and
//              swizzle), 3 stages ahead.  Why a wave of its own: vector-memory loads return in order, so a wave that waited for an activation stage three
//              stages out would also wait for the plane it asked for 1024 k ahead; with the two streams in two waves each is as deep as it likes.
//   One workgroup barrier per stage (wave 4: "stage k has landed"; waves 0-3: "stage k - 1 has been read").
// Both halves of a plane are consumed run by run — first the lower 8 bytes of all 16 loads (k-steps 0-15 of the even run), then the upper — so a plane's
// registers live for two runs; that is what the second register set is for.
// Budget: LDS 4 x (2 x 16 MB rows x 128 B) = 16 / 32 / 64 KiB for MB = 1 / 2 / 4.  VGPRs: 128 for the two planes, 4 MB accumulators, 8 MB activation fragments,
// 4 of a decoded fragment (tools/check_spills.py; the counts are in profiles/weights_fp8_rows.txt).  No instantiation uses scratch.
//
// Decode: v_cvt_pk_f32_fp8 gives the codes' own values, one multiply by the lane's row scale 2^e_r (a lane always serves the same weight row) gives dq — exact,
// a normal fp32 whose low 16 bits are zero — and v_perm_b32 packs the upper halves of two products into a dword of the bf16 fragment.  The scale is never
// applied to sums (gemv_fp8.h).  dq is the dequantized master's value bit for bit.
//
// Accumulation order is skinny.h's and skinny_dma.h's: per output element and K range k ascending in steps of 32, small term first; K ranges, slabs and
// epilogues are launch_skinny's.  The product is bit-identical to those kernels over the dequantized master.
//
// Coverage (decided on the host, launch_skinny): K % 512 == 0 and, for a split product, k_per % 512 == 0 — no run is cut and no padded chunk is ever met; any
// NX, odd ones included (an odd NX leaves the upper half of a k-part's last plane unused and the kernel steps over it), so the Mistral-7B down matrix
// (NX = 7, K = 14336 = 28 runs) is served when its split ranges are whole runs.  Everything else takes the master through the existing kernels and is counted
// (weights.fp8_row_fallbacks).  Out of scope: qkv / o_proj, 65-128 rows, fp16, three-term activations, the MFMA's native fp8 operand forms.
#pragma once
#include <type_traits>
#include "skinny_dma.h"

namespace tgx {

struct SkinnyFp8Args {
  GemmArgs g;               // g.B is not read
  const unsigned char* Q;   // code planes
  const float* scale;       // [N] 2^e_r
  long long row_bytes;
  int nx, nh;               // runs and planes per k-part
};

constexpr int SK8_D = 4;                                  // stages of the activation ring
constexpr int SK8_THREADS = 320;                          // four product waves + the activation wave
__host__ __device__ constexpr int sk8_stage_bytes(int mb) { return 2 * mb * 16 * SKD_KS * 2; }
__host__ __device__ constexpr size_t sk8_lds_bytes(int mb) { return (size_t)SK8_D * sk8_stage_bytes(mb); }

// the 8 codes of a chunk -> the bf16 fragment of dq = code * sc
__device__ __forceinline__ bf16x8 fp8_chunk_bf16(unsigned int d0, unsigned int d1, float sc) {
  auto pair = [&](auto v) { return __builtin_amdgcn_perm(__float_as_uint(v[1] * sc), __float_as_uint(v[0] * sc), 0x07060302u); };      // {hi16(v1 sc), hi16(v0 sc)}
  const u32x4 o = {pair(__builtin_amdgcn_cvt_pk_f32_fp8((int)d0, false)), pair(__builtin_amdgcn_cvt_pk_f32_fp8((int)d0, true)),
                   pair(__builtin_amdgcn_cvt_pk_f32_fp8((int)d1, false)), pair(__builtin_amdgcn_cvt_pk_f32_fp8((int)d1, true))};
  return __builtin_bit_cast(bf16x8, o);
}

template <int EPI, int MB>
__global__ __launch_bounds__(SK8_THREADS) void skinny_fp8_kernel(const SkinnyFp8Args pa) {
  constexpr int DT = DT_BF16, KS = SKD_KS, XROWS = 2 * MB * 16, XP = XROWS / 8, D = SK8_D, STAGE = sk8_stage_bytes(MB);
  static_assert((D - 2) * XP <= 63, "vmcnt is a 6-bit counter");
  extern __shared__ __attribute__((aligned(1024))) unsigned char sk8_lds[];
  const GemmArgs& a = pa.g;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k_begin = EPI == GEMM_PARTIAL ? (int)blockIdx.y * a.k_per : 0;
  const int k_end = EPI == GEMM_PARTIAL ? min(a.K, k_begin + a.k_per) : a.K;
  const int r_begin = k_begin >> 9, r_end = k_end >> 9;       // whole runs (checked by the launcher)
  const int nst = (r_end - r_begin) * 8;                      // stages of 64 k: one barrier each in every wave

  if (wv == 4) {      // ---- the activation wave: skinny_dma.h's stage image, all pieces from this wave
    const unsigned lds_base = (unsigned)(size_t)sk8_lds;
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
  const float sc = pa.scale[brow];
  const unsigned char* wrow = pa.Q + brow * (size_t)pa.row_bytes + (size_t)kg * 16;
  const int NX = pa.nx, NH = pa.nh;
  auto load_plane = [&](u32x4* dst, int run) {
    const int p = run / NX, j = run - p * NX;
    const unsigned char* pl = wrow + (size_t)(p * NH + (j >> 1)) * 1024;
#pragma unroll
    for (int s = 0; s < 16; s++) dst[s] = load_nt(reinterpret_cast<const u32x4*>(pl + s * 64));
  };

  f32x4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; mb++) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 cur[16], nxt[16];
  int kst = 0;                                                // stages consumed
  // one run = 8 stages = 16 k-steps out of half HALF of the plane in `cur`
  auto consume = [&](auto half_c) {
    constexpr int HALF = decltype(half_c)::value;
#pragma unroll
    for (int st = 0; st < 8; st++) {
      __builtin_amdgcn_s_barrier();                           // stage kst has landed
      const unsigned char* sp = sk8_lds + (size_t)(kst % D) * STAGE;
      kst++;
#pragma unroll
      for (int ks = 0; ks < KS / 32; ks++) {
        const int chunk = ((ks * 4 + kg) ^ fsw) * 16;
        const u32x4 w = cur[2 * st + ks];
        const bf16x8 fb = fp8_chunk_bf16(w[2 * HALF], w[2 * HALF + 1], sc);
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
  if (run < r_end) load_plane(cur, run);
  while (run < r_end) {
    const int j = run % NX;
    const bool two = !(j & 1) && j + 1 < NX && run + 1 < r_end;      // the plane's upper half is the next run of this range
    const int next = run + (two ? 2 : 1);
    if (next < r_end) load_plane(nxt, next);
    if (!(j & 1)) consume(std::integral_constant<int, 0>{});
    if ((j & 1) || two) consume(std::integral_constant<int, 1>{});
#pragma unroll
    for (int s = 0; s < 16; s++) cur[s] = nxt[s];
    run = next;
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
