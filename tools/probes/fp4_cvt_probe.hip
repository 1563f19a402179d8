// fp4_cvt_probe.hip — v_cvt_scalef32_pk_f32_fp4 over all 16 E2M1 codes, both nibbles, the four byte selects and every scale byte kernels/gemv_fp4.h can meet
// (2 .. 227: 2^-125 .. 2^100), against the value computed on the host.  Three scale operands per byte: the clean fp32 (byte << 23), the same with mantissa
// bits set, and the same with the sign bit set — does the instruction read the exponent field only?
// Build: hipcc --offload-arch=gfx950 -O2 tools/probes/fp4_cvt_probe.hip -o fp4_cvt_probe.  Result on an MI355X: profiles/weights_fp4.txt.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int S0 = 2, S1 = 227, NS = S1 - S0 + 1;
template <int SEL> __device__ void one(unsigned int w, float scale, float* out) {
  const f32x2 v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, SEL);
  out[2 * SEL] = v[0]; out[2 * SEL + 1] = v[1];
}
// thread = (low code, high code); block = scale byte; out[variant][scale][pair][8]: the eight values of a dword whose four bytes are all hi << 4 | lo
__global__ void probe(float* out) {
  const unsigned int pair = threadIdx.x, sb = S0 + blockIdx.x;
  const unsigned int w = pair * 0x01010101u;
  const unsigned int dirty[3] = {0u, 0x007fffffu, 0x80000000u};
  for (int v = 0; v < 3; v++) {
    const float scale = __uint_as_float((sb << 23) | dirty[v]);
    float* o = out + (((size_t)v * NS + blockIdx.x) * 256 + pair) * 8;
    one<0>(w, scale, o); one<1>(w, scale, o); one<2>(w, scale, o); one<3>(w, scale, o);
  }
}
static double code_value(int c) {
  static const double grid[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
  return (c & 8) ? -grid[c & 7] : grid[c & 7];
}
int main() {
  const size_t n = (size_t)3 * NS * 256 * 8;
  float* dev;
  if (hipMalloc(&dev, n * 4)) return 2;
  hipLaunchKernelGGL(probe, dim3(NS), dim3(256), 0, 0, dev);
  float* h = new float[n];
  if (hipMemcpy(h, dev, n * 4, hipMemcpyDeviceToHost)) { printf("copy failed\n"); return 2; }
  const char* names[3] = {"clean scale", "mantissa bits set", "sign bit set"};
  for (int v = 0; v < 3; v++) {
    int bad = 0;
    for (int s = 0; s < NS; s++) for (int pair = 0; pair < 256; pair++) for (int k = 0; k < 8; k++) {
      const float want = (float)std::ldexp(code_value((k & 1) ? pair >> 4 : pair & 15), S0 + s - 127), got = h[(((size_t)v * NS + s) * 256 + pair) * 8 + k];
      if (std::memcmp(&want, &got, 4)) { if (bad++ < 8) printf("  %s: scale byte %d byte %02x value %d got %a want %a\n", names[v], S0 + s, pair, k, got, want); }
    }
    printf("%s: %d mismatches of %d\n", names[v], bad, NS * 256 * 8);
  }
  return 0;
}
