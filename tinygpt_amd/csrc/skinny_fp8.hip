// skinny_fp8.hip — the launches of kernels/skinny_fp8.h: the skinny products of gate_up, down and lm_head on the 8-bit code stream (option weights.fp8_rows).
// A translation unit of its own: it is compiled without packed fp32 arithmetic (tinygpt_amd/build.py), the decode's multiplies stay scalar.
#include "stream_launch.h"
#include "kernels/skinny_fp8.h"

static constexpr auto sk8_kernel = [](auto E, auto MB) { return &tgx::skinny_fp8_kernel<decltype(E)::value, decltype(MB)::value>; };
#define TGX_SK8_EPIS tgx::GEMM_STORE, tgx::GEMM_SILU, tgx::GEMM_RESIDUAL, tgx::GEMM_PARTIAL      // (the list's order is the order the unit's kernels are emitted in)

// does the kernel cover this product?  k_per: the K range of one split (0: unsplit).  Whole 512-k runs only, and a stream whose size is what the layout says.
bool skinny_fp8_covers(const tgx_ctx* c, const WeightStream& q, int M, int K, int k_per) {
  if (!q.planes || !q.scale || q.ks < 1 || c->dt != tgx::DT_BF16 || M < 1 || M > 64) return false;
  if (K < 512 || K % 512 || (k_per && k_per % 512)) return false;
  const int nx = stream_nx(K, q.ks);
  return q.row_bytes == (long long)q.ks * ((nx + 1) / 2) * 1024;
}

// g: launch_skinny's arguments (terms, epilogue operands, split geometry); epi: the epilogue after the split rule; mb: 1, 2 or 4 activation blocks
void launch_skinny_fp8(tgx_ctx* c, const tgx::GemmArgs& g, const WeightStream& q, int epi, int mb, int nsplit) {
  tgx::SkinnyFp8Args p{};
  p.g = g; p.g.B = nullptr; p.Q = q.planes; p.scale = q.scale; p.row_bytes = q.row_bytes;
  p.nx = stream_nx(g.K, q.ks); p.nh = (p.nx + 1) / 2;      // runs and planes per k-part of the layout `q` was made for (kernels/gemv_fp8.h)
  launch_skinny_stream<TGX_SK8_EPIS>(c, p, dim3((g.N + 63) / 64, nsplit), tgx::SK8_THREADS, epi, mb, sk8_kernel, tgx::sk8_lds_bytes, c->quant_of(WS_FP8),
                                     "internal: skinny FP8 product with an epilogue it does not have");
}

int skinny_fp8_set_attrs(tgx_ctx* c) { return skinny_stream_set_attrs<TGX_SK8_EPIS>(c, sk8_kernel, tgx::sk8_lds_bytes); }
