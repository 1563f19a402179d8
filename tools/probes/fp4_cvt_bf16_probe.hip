// fp4_cvt_bf16_probe.hip — v_cvt_scalef32_pk_bf16_fp4 (the decode of kernels/skinny_fp4.h) over all 16 E2M1 codes, both nibbles, the four byte selects and
// every scale byte the quantizer can produce (2 .. 227: 2^-125 .. 2^100), against the bf16 pattern computed on the host.  Three scale operands per byte, as
// tools/probes/fp4_cvt_probe.hip: the clean fp32 (byte << 23), the same with mantissa bits set, and the same with the sign bit set.
// Build: hipcc --offload-arch=gfx950 -O2 tools/probes/fp4_cvt_bf16_probe.hip -o fp4_cvt_bf16_probe.  Result on an MI355X: profiles/weights_fp4_rows.txt.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
constexpr int S0 = 2, S1 = 227, NS = S1 - S0 + 1;
template <int SEL> __device__ void one(unsigned int w, float scale, unsigned int* out) {
  out[SEL] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, SEL));
}
// thread = (low code, high code); block = scale byte; out[variant][scale][pair][4]: the four result dwords of a dword whose four bytes are all hi << 4 | lo
__global__ void probe(unsigned int* out) {
  const unsigned int pair = threadIdx.x, sb = S0 + blockIdx.x;
  const unsigned int w = pair * 0x01010101u;
  const unsigned int dirty[3] = {0u, 0x007fffffu, 0x80000000u};
  for (int v = 0; v < 3; v++) {
    const float scale = __uint_as_float((sb << 23) | dirty[v]);
    unsigned int* o = out + (((size_t)v * NS + blockIdx.x) * 256 + pair) * 4;
    one<0>(w, scale, o); one<1>(w, scale, o); one<2>(w, scale, o); one<3>(w, scale, o);
  }
}
// the bf16 pattern of code * 2^(sb - 127): exact, its fp32 has a zero low half
static unsigned int want_bits(int code, int sb) {
  static const double grid[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
  const float f = (float)std::ldexp((code & 8) ? -grid[code & 7] : grid[code & 7], sb - 127);
  unsigned int u;
  std::memcpy(&u, &f, 4);
  return u >> 16;
}
int main() {
  const size_t n = (size_t)3 * NS * 256 * 4;
  unsigned int* dev;
  if (hipMalloc(&dev, n * 4)) return 2;
  hipLaunchKernelGGL(probe, dim3(NS), dim3(256), 0, 0, dev);
  unsigned int* h = new unsigned int[n];
  if (hipMemcpy(h, dev, n * 4, hipMemcpyDeviceToHost)) { printf("copy failed\n"); return 2; }
  const char* names[3] = {"clean scale", "mantissa bits set", "sign bit set"};
  int total = 0;
  for (int v = 0; v < 3; v++) {
    int bad = 0;
    for (int s = 0; s < NS; s++) for (int pair = 0; pair < 256; pair++) for (int k = 0; k < 4; k++) {
      const unsigned int want = want_bits(pair & 15, S0 + s) | (want_bits(pair >> 4, S0 + s) << 16), got = h[(((size_t)v * NS + s) * 256 + pair) * 4 + k];
      if (want != got) { if (bad++ < 8) printf("  %s: scale byte %d byte %02x select %d got %08x want %08x\n", names[v], S0 + s, pair, k, got, want); }
    }
    printf("%s: %d mismatches of %d\n", names[v], bad, NS * 256 * 4);
    total += bad;
  }
  return total ? 1 : 0;
}
