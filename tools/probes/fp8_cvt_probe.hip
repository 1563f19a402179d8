// fp8_cvt_probe.hip — v_cvt_f32_fp8 and v_cvt_scalef32_pk_f32_fp8 over all 256 codes and ten power-of-two scales (2^-117 .. 2^92), against the value computed on the host.
// Build: hipcc --offload-arch=gfx950 -O2 tools/probes/fp8_cvt_probe.hip -o fp8_cvt_probe.  Result on an MI355X (profiles/weights_fp8.txt): both forms exact for all 254 finite codes,
// subnormal codes included; kernels/gemv_fp8.h uses the unscaled form and one exact multiply.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
typedef float f32x2 __attribute__((ext_vector_type(2)));
__global__ void probe(float* plain, float* scaled, const float* scales, int ns) {
  const int code = threadIdx.x;   // 256 threads
  const unsigned int w = (unsigned)code | ((unsigned)code << 8) | ((unsigned)code << 16) | ((unsigned)code << 24);
  plain[code] = __builtin_amdgcn_cvt_f32_fp8((int)w, 2);
  for (int s = 0; s < ns; s++) {
    f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, scales[s], false);
    f32x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, scales[s], true);
    scaled[(s * 256 + code) * 4 + 0] = lo[0]; scaled[(s * 256 + code) * 4 + 1] = lo[1];
    scaled[(s * 256 + code) * 4 + 2] = hi[0]; scaled[(s * 256 + code) * 4 + 3] = hi[1];
  }
}
static double code_value(int c) {
  int ef = (c >> 3) & 15, mm = c & 7;
  double mag = ef ? std::ldexp(1.0 + mm / 8.0, ef - 7) : mm * std::ldexp(1.0, -9);
  return (c & 0x80) ? -mag : mag;
}
int main() {
  const int exps[] = {-117, -100, -30, -12, -1, 0, 1, 17, 60, 92};
  const int ns = sizeof exps / sizeof exps[0];
  float hs[ns]; for (int i = 0; i < ns; i++) hs[i] = std::ldexp(1.0f, exps[i]);
  float *plain, *scaled, *scales;
  if (hipMalloc(&plain, 256 * 4) || hipMalloc(&scaled, ns * 256 * 16) || hipMalloc(&scales, ns * 4)) return 2;
  hipMemcpy(scales, hs, ns * 4, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(probe, dim3(1), dim3(256), 0, 0, plain, scaled, scales, ns);
  static float hp[256], hsc[10 * 256 * 4];
  if (hipMemcpy(hp, plain, sizeof hp, hipMemcpyDeviceToHost) || hipMemcpy(hsc, scaled, ns * 256 * 16, hipMemcpyDeviceToHost)) { printf("copy failed\n"); return 2; }
  int bad_plain = 0, bad_scaled = 0;
  for (int c = 0; c < 256; c++) {
    if ((c & 0x7f) == 0x7f) { printf("code %02x plain %g\n", c, hp[c]); continue; }
    float want = (float)code_value(c);
    if (std::memcmp(&want, &hp[c], 4)) { if (bad_plain++ < 12) printf("PLAIN code %02x got %a want %a\n", c, hp[c], want); }
    for (int s = 0; s < ns; s++) for (int k = 0; k < 4; k++) {
      float w2 = (float)std::ldexp(code_value(c), exps[s]), got = hsc[(s * 256 + c) * 4 + k];
      if (std::memcmp(&w2, &got, 4)) { if (bad_scaled++ < 24) printf("SCALED code %02x e %d k %d got %a want %a\n", c, exps[s], k, got, w2); }
    }
  }
  printf("plain mismatches %d of 254, scaled mismatches %d of %d\n", bad_plain, bad_scaled, 254 * ns * 4);
  return 0;
}
