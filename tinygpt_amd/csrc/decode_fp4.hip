// decode_fp4.hip — the MXFP4 weight stream of the batch-1 step (kernels/gemv_fp4.h; option weights.fp4): its GEMV instantiations and its quantizer
// launches.  A unit of its own because it is built without packed fp32 arithmetic (build.py TU_FLAGS): the kernel's FMAs are scalar v_fma_f32.
// decode.hip decides when a launch takes this stream (launch_gemv) and which matrices tgx_finalize quantizes (quantize_weights_fp4).
#include "ctx.h"
#include "kernels/gemv_fp4.h"

template <int PRO, int EPI, int NX>
static void launch_gemv_fp4_nx(tgx_ctx* c, const tgx::GemvFp4Args& p, int grid) {
  const dim3 g(grid), b(256);
  if constexpr (EPI != tgx::EPI_LOGITS) {      // the fixed-point residual stream behind the K-sliced o_proj (decode.hip launch_gemv_nx)
    if (p.g.x_acc || p.g.res_acc) { hipLaunchKernelGGL((tgx::gemv_fp4_kernel<PRO, EPI, NX, true>), g, b, p.g.x_acc ? (size_t)p.g.K * 4 : 0, c->stream, p); return; }
  }
  hipLaunchKernelGGL((tgx::gemv_fp4_kernel<PRO, EPI, NX, false>), g, b, 0, c->stream, p);
}

template <int PRO, int EPI>
static void launch_gemv_fp4_form(tgx_ctx* c, const tgx::GemvFp4Args& p, int grid, int nx) {
  switch (nx) {
    case 1: launch_gemv_fp4_nx<PRO, EPI, 1>(c, p, grid); break;
    case 2: launch_gemv_fp4_nx<PRO, EPI, 2>(c, p, grid); break;
    case 3: launch_gemv_fp4_nx<PRO, EPI, 3>(c, p, grid); break;
    case 4: launch_gemv_fp4_nx<PRO, EPI, 4>(c, p, grid); break;
    case 5: launch_gemv_fp4_nx<PRO, EPI, 5>(c, p, grid); break;
    case 6: launch_gemv_fp4_nx<PRO, EPI, 6>(c, p, grid); break;
    case 7: launch_gemv_fp4_nx<PRO, EPI, 7>(c, p, grid); break;
    default: launch_gemv_fp4_nx<PRO, EPI, 8>(c, p, grid); break;
  }
}

void launch_gemv_fp4(tgx_ctx* c, int cls, const tgx::GemvArgs& a, const Fp4Mat& q, int grid, int nx) {
  tgx::GemvFp4Args p{};
  p.g = a; p.Q = q.Q; p.row_bytes = q.row_bytes;
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
