// stream_launch.h — the host-side launch templates the weight-stream kernel families share (ctx.h WeightStream): each family stays instantiated in the unit
// that names it (decode.hip: packed, FP8; decode_fp4.hip; skinny_fp8.hip; skinny_fp4.hip), this header only writes the dispatch once.  A family is handed
// over as a generic lambda from compile-time constants to the kernel's address.  Host code only: nothing here adds to a unit's device code.
#pragma once
#include <type_traits>

#include "ctx.h"

template <int V> using stream_ic = std::integral_constant<int, V>;

// ---- batch-1 GEMV over a stream (kernels/gemv_packed.h, gemv_fp8.h, gemv_fp4.h): kern(NX, XACC) -> the kernel for NX chunk slots per lane, with (XACC) or
// without the fixed-point residual stream behind the K-sliced o_proj (decode.hip launch_gemv_nx).  XACC_FORMS: the epilogue has that form (all but the logits)
template <bool XACC_FORMS, typename Args, typename Kern>
void launch_gemv_stream(tgx_ctx* c, const Args& p, int grid, int nx, Kern kern) {
  const dim3 g(grid), b(256);
  auto go = [&](auto NX) {
    if constexpr (XACC_FORMS) {
      if (p.g.x_acc || p.g.res_acc) { hipLaunchKernelGGL(kern(NX, std::true_type{}), g, b, p.g.x_acc ? (size_t)p.g.K * 4 : 0, c->stream, p); return; }
    }
    hipLaunchKernelGGL(kern(NX, std::false_type{}), g, b, 0, c->stream, p);
  };
  switch (nx) {
    case 1: go(stream_ic<1>{}); break;
    case 2: go(stream_ic<2>{}); break;
    case 3: go(stream_ic<3>{}); break;
    case 4: go(stream_ic<4>{}); break;
    case 5: go(stream_ic<5>{}); break;
    case 6: go(stream_ic<6>{}); break;
    case 7: go(stream_ic<7>{}); break;
    default: go(stream_ic<8>{}); break;
  }
}

// ---- skinny products over a stream (kernels/skinny_fp8.h, skinny_fp4.h): kern(EPI, MB) -> the kernel of an epilogue and 1, 2 or 4 activation blocks;
// lds(MB): its dynamic shared memory.  EPIS: the epilogues the family is instantiated for
template <int... EPIS, typename F>
void skinny_stream_each(F&& f) { ((f(stream_ic<EPIS>{}, stream_ic<1>{}), f(stream_ic<EPIS>{}, stream_ic<2>{}), f(stream_ic<EPIS>{}, stream_ic<4>{})), ...); }

// issues the product and counts it in qf.row_products; an epilogue outside EPIS is the launch fault `fault`
template <int... EPIS, typename Args, typename Kern>
void launch_skinny_stream(tgx_ctx* c, const Args& p, dim3 grid, int threads, int epi, int mb, Kern kern, size_t (*lds)(int), QuantForm& qf, const char* fault) {
  const int blocks = mb == 4 ? 4 : (mb == 2 ? 2 : 1);
  bool issued = false;
  skinny_stream_each<EPIS...>([&](auto E, auto MB) {
    if (decltype(E)::value != epi || decltype(MB)::value != blocks) return;
    hipLaunchKernelGGL(kern(E, MB), grid, dim3(threads), lds(blocks), c->stream, p);
    issued = true;
  });
  if (issued) qf.row_products++;
  else c->launch_fault = fault;
}

// the four-block ring is the 64 KiB default exactly: said explicitly, as for the other skinny kernels
template <int... EPIS, typename Kern>
int skinny_stream_set_attrs(tgx_ctx* c, Kern kern, size_t (*lds)(int)) {
  hipError_t e = hipSuccess;
  skinny_stream_each<EPIS...>([&](auto E, auto MB) {
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern(E, MB)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds(decltype(MB)::value));
  });
  return e == hipSuccess ? TGX_OK : set_err(c, TGX_ERR_DEVICE, "hipFuncSetAttribute of a skinny stream kernel failed: %s", hipGetErrorString(e));
}
