// skinny_fp4.hip — the launches of kernels/skinny_fp4.h: the skinny products of gate_up, down and lm_head on the 4-bit code stream (option weights.fp4_rows).
// A translation unit of its own, built like skinny_fp8.hip (tinygpt_amd/build.py).  It allocates nothing.
#include "stream_launch.h"
#include "kernels/skinny_fp4.h"

static constexpr auto sk4_kernel = [](auto E, auto MB) { return &tgx::skinny_fp4_kernel<decltype(E)::value, decltype(MB)::value>; };
#define TGX_SK4_EPIS tgx::GEMM_STORE, tgx::GEMM_SILU, tgx::GEMM_RESIDUAL, tgx::GEMM_PARTIAL      // (the list's order is the order the unit's kernels are emitted in)

// does the kernel cover this product?  k_per: the K range of one split (0: unsplit).  K in whole 512-k runs, split ranges in whole 64-k stages, a single-range
// stream laid out for this K, and a stream whose size is what the layout says.
bool skinny_fp4_covers(const tgx_ctx* c, const WeightStream& q, int M, int K, int k_per) {
  if (!q.planes || q.ks < 1 || q.parts != 1 || q.K != K || c->dt != tgx::DT_BF16 || M < 1 || M > 64) return false;
  if (K < 512 || K % 512 || (k_per && k_per % 64)) return false;
  const int nx = stream_nx(K, q.ks);
  return nx <= 8 && q.row_bytes == (long long)q.ks * tgx::SK4_SLOT * nx;
}

// g: launch_skinny's arguments (terms, epilogue operands, split geometry); epi: the epilogue after the split rule; mb: 1, 2 or 4 activation blocks
void launch_skinny_fp4(tgx_ctx* c, const tgx::GemmArgs& g, const WeightStream& q, int epi, int mb, int nsplit) {
  tgx::SkinnyFp4Args p{};
  p.g = g; p.g.B = nullptr; p.Q = q.planes; p.row_bytes = q.row_bytes; p.nx = stream_nx(g.K, q.ks);      // chunk slots per k-part of the layout `q` was made for
  launch_skinny_stream<TGX_SK4_EPIS>(c, p, dim3((g.N + 63) / 64, nsplit), tgx::SK4_THREADS, epi, mb, sk4_kernel, tgx::sk4_lds_bytes, c->quant_of(WS_FP4),
                                     "internal: skinny FP4 product with an epilogue it does not have");
}

int skinny_fp4_set_attrs(tgx_ctx* c) { return skinny_stream_set_attrs<TGX_SK4_EPIS>(c, sk4_kernel, tgx::sk4_lds_bytes); }
