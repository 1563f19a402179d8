// skinny_fp4.hip — the launches of kernels/skinny_fp4.h: the skinny products of gate_up, down and lm_head on the 4-bit code stream (option weights.fp4_rows).
// A translation unit of its own, built like skinny_fp8.hip (tinygpt_amd/build.py).  It allocates nothing.
#include "ctx.h"
#include "kernels/skinny_fp4.h"

// chunk slots (runs of 512 k) per k-part of the layout `q` was made for (kernels/gemv_fp4.h)
static int fp4_nx(const Fp4Mat& q, int K) { return ((K / 8) + q.ks * 64 - 1) / (q.ks * 64); }

// does the kernel cover this product?  k_per: the K range of one split (0: unsplit).  K in whole 512-k runs, split ranges in whole 64-k stages, a single-range
// stream laid out for this K, and a stream whose size is what the layout says.
bool skinny_fp4_covers(const tgx_ctx* c, const Fp4Mat& q, int M, int K, int k_per) {
  if (!q.Q || q.ks < 1 || q.parts != 1 || q.K != K || c->dt != tgx::DT_BF16 || M < 1 || M > 64) return false;
  if (K < 512 || K % 512 || (k_per && k_per % 64)) return false;
  const int nx = fp4_nx(q, K);
  return nx <= 8 && q.row_bytes == (long long)q.ks * tgx::SK4_SLOT * nx;
}

template <int EPI>
static void skinny_fp4_dispatch(tgx_ctx* c, dim3 grid, int mb, const tgx::SkinnyFp4Args& p) {
  const dim3 blk(tgx::SK4_THREADS);
  if (mb == 4) hipLaunchKernelGGL((tgx::skinny_fp4_kernel<EPI, 4>), grid, blk, tgx::sk4_lds_bytes(4), c->stream, p);
  else if (mb == 2) hipLaunchKernelGGL((tgx::skinny_fp4_kernel<EPI, 2>), grid, blk, tgx::sk4_lds_bytes(2), c->stream, p);
  else hipLaunchKernelGGL((tgx::skinny_fp4_kernel<EPI, 1>), grid, blk, tgx::sk4_lds_bytes(1), c->stream, p);
}

// g: launch_skinny's arguments (terms, epilogue operands, split geometry); epi: the epilogue after the split rule; mb: 1, 2 or 4 activation blocks
void launch_skinny_fp4(tgx_ctx* c, const tgx::GemmArgs& g, const Fp4Mat& q, int epi, int mb, int nsplit) {
  tgx::SkinnyFp4Args p{};
  p.g = g; p.g.B = nullptr; p.Q = q.Q; p.row_bytes = q.row_bytes; p.nx = fp4_nx(q, g.K);
  const dim3 grid((g.N + 63) / 64, nsplit);
  switch (epi) {
    case tgx::GEMM_PARTIAL: skinny_fp4_dispatch<tgx::GEMM_PARTIAL>(c, grid, mb, p); break;
    case tgx::GEMM_RESIDUAL: skinny_fp4_dispatch<tgx::GEMM_RESIDUAL>(c, grid, mb, p); break;
    case tgx::GEMM_SILU: skinny_fp4_dispatch<tgx::GEMM_SILU>(c, grid, mb, p); break;
    case tgx::GEMM_STORE: skinny_fp4_dispatch<tgx::GEMM_STORE>(c, grid, mb, p); break;
    default: c->launch_fault = "internal: skinny FP4 product with an epilogue it does not have"; return;
  }
  c->fp4_row_products++;
}

// the four-block ring is the 64 KiB default exactly: said explicitly, as for the other skinny kernels
int skinny_fp4_set_attrs(tgx_ctx* c) {
#define TGX_SK4_A(E_, MB_) HIP_OK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&tgx::skinny_fp4_kernel<E_, MB_>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tgx::sk4_lds_bytes(MB_)));
#define TGX_SK4_E(E_) TGX_SK4_A(E_, 1) TGX_SK4_A(E_, 2) TGX_SK4_A(E_, 4)
  TGX_SK4_E(tgx::GEMM_PARTIAL) TGX_SK4_E(tgx::GEMM_RESIDUAL) TGX_SK4_E(tgx::GEMM_SILU) TGX_SK4_E(tgx::GEMM_STORE)
#undef TGX_SK4_E
#undef TGX_SK4_A
  return TGX_OK;
}
