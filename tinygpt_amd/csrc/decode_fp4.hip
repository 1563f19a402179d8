// decode_fp4.hip — the MXFP4 weight stream of the batch-1 step (kernels/gemv_fp4.h; option weights.fp4): its GEMV instantiations and its quantizer
// launches.  A unit of its own because it is built without packed fp32 arithmetic (build.py TU_FLAGS): the kernel's FMAs are scalar v_fma_f32.
// decode.hip decides when a launch takes this stream (launch_gemv) and which matrices tgx_finalize quantizes (quantize_weights).
#include "stream_launch.h"
#include "kernels/gemv_fp4.h"

template <int PRO, int EPI>
static void launch_gemv_fp4_form(tgx_ctx* c, const tgx::GemvFp4Args& p, int grid, int nx) {
  launch_gemv_stream<EPI != tgx::EPI_LOGITS>(c, p, grid, nx, [](auto NX, auto XA) { return &tgx::gemv_fp4_kernel<PRO, EPI, decltype(NX)::value, decltype(XA)::value>; });
}

void launch_gemv_fp4(tgx_ctx* c, int cls, const tgx::GemvArgs& a, const WeightStream& q, int grid, int nx) {
  tgx::GemvFp4Args p{};
  p.g = a; p.Q = q.planes; p.row_bytes = q.row_bytes;
  if (cls == TGX_KERNEL_GATEUP) launch_gemv_fp4_form<tgx::PRO_RMSNORM, tgx::EPI_SILU_MUL>(c, p, grid, nx);
  else if (cls == TGX_KERNEL_DOWN) launch_gemv_fp4_form<tgx::PRO_PLAIN, tgx::EPI_RESIDUAL>(c, p, grid, nx);
  else launch_gemv_fp4_form<tgx::PRO_RMSNORM, tgx::EPI_LOGITS>(c, p, grid, nx);
}

void fp4_scan_matrix(tgx_ctx* c, const ebyte* W, int N, int K, int* stat_dev) {
  hipLaunchKernelGGL(tgx::fp4_scan_rows_kernel, dim3(N), dim3(64), 0, c->stream, reinterpret_cast<const bf16_t*>(W), K, stat_dev);
}

long long fp4_row_bytes(int ks, int nx) { return (long long)ks * nx * tgx::FP4_SLOT; }

void fp4_quant_matrix(tgx_ctx* c, ebyte* W, int N, int K, int ldw, int ks, int nx, unsigned char* Q, long long row_bytes) {
  tgx::Fp4QuantArgs a{};
  a.W = reinterpret_cast<bf16_t*>(W); a.K = K; a.ldw = ldw; a.ks = ks; a.nx = nx; a.Q = Q; a.row_bytes = row_bytes;
  hipLaunchKernelGGL(tgx::fp4_quant_rows_kernel, dim3(N), dim3(64), 0, c->stream, a);
}
