// beam_check.cpp — the CPU driver of tinygpt_amd/host/beam.h (built and run by tests/test_beam_host.py under the address and undefined-behaviour sanitizers; never
// loaded into Python).  It reads candidate streams from standard input, runs BeamScorer over them and prints what the scorer decided, numbers as bit patterns:
// the test compares the text with a restatement of the rules in Python, character for character.
//   input    <streams>, then per stream: K lengthPenalty(u32 bits) earlyStopping maxNewTokens nEnd end ids.. nSteps, then per step: n, then n x (beam token score(u32 bits) lp(u32 bits))
//   output   per step "S done running parent:token:score(u32 bits) ..", per kept hypothesis "H length sumLp(u32 bits) score(u64 bits) tokens ..", per stream "E"
#include "../tinygpt_amd/host/beam.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

static float f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t u32(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static uint64_t u64(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

int main() {
  int streams = 0;
  if (scanf("%d", &streams) != 1) return 2;
  for (int s = 0; s < streams; s++) {
    int K, early, nEnd, nSteps;
    uint32_t lpBits;
    long long maxNew;
    if (scanf("%d %" SCNu32 " %d %lld %d", &K, &lpBits, &early, &maxNew, &nEnd) != 5) return 2;
    std::vector<int32_t> ends((size_t)nEnd);
    for (int e = 0; e < nEnd; e++) if (scanf("%" SCNd32, &ends[(size_t)e]) != 1) return 2;
    if (scanf("%d", &nSteps) != 1) return 2;
    tgxh::BeamScorer sc(K, f32(lpBits), early != 0, maxNew, ends);
    for (int st = 0; st < nSteps; st++) {
      int n;
      if (scanf("%d", &n) != 1) return 2;
      std::vector<tgxh::BeamCand> c((size_t)n);
      for (int i = 0; i < n; i++) {
        uint32_t a, b;
        if (scanf("%" SCNd32 " %" SCNd32 " %" SCNu32 " %" SCNu32, &c[(size_t)i].beam, &c[(size_t)i].token, &a, &b) != 4) return 2;
        c[(size_t)i].score = f32(a); c[(size_t)i].lp = f32(b);
      }
      if (sc.done()) continue;      // (the stream goes on; the scorer has finished)
      const bool done = sc.step(c.data(), n);
      printf("S %d %d", done ? 1 : 0, sc.running());
      for (size_t j = 0; j < sc.parents().size(); j++) printf(" %d:%d:%" PRIu32, sc.parents()[j], sc.tokens()[j], u32(sc.scores()[j]));
      printf("\n");
    }
    for (const tgxh::BeamHyp& h : sc.finish()) {
      printf("H %d %" PRIu32 " %" PRIu64, h.length ? 1 : 0, u32(h.sumLp), u64(h.score));
      for (int32_t t : h.tokens) printf(" %d", t);
      printf("\n");
    }
    printf("E\n");
  }
  return 0;
}
