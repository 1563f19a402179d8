// gemv_grid_check.cpp — the CPU audit of tinygpt_amd/csrc/gemv_grid.h (built and run by tests/test_gemv_grid.py under the address and undefined-behaviour
// sanitizers).  For every units in 1..70000, units per workgroup in {1, 2, 4} and cap in {256, 512, 768, 1024} the plan is held to what the kernels' unit loop
// (ub = blockIdx * upb; ub < units; ub += grid * upb) needs: 1 <= grid <= cap, grid * upb * rounds >= units, no workgroup without a unit, rounds ==
// ceil(want / cap) with want = ceil(units / upb) — the fewest trips the cap allows.  Two rules meet these: the ragged one, min(want, cap), and the balanced
// one, ceil(want / rounds) (every workgroup the same trip count); both are restated here, they are the same grid whenever want <= cap, and the header's
// plan is the ragged one (profiles/packed_kpart_geometry.txt: the balanced grid measured no gain).
#include "../tinygpt_amd/csrc/gemv_grid.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#define REQUIRE(cond)                                                                                                                          \
  do {                                                                                                                                         \
    if (!(cond)) { fprintf(stderr, "gemv_grid_check: %s failed at line %d (units %d upb %d cap %d)\n", #cond, __LINE__, units, upb, cap); exit(1); } \
  } while (0)

int main() {
  long long plans = 0, multi_round = 0;
  for (int upb : {1, 2, 4})
    for (int cap : {256, 512, 768, 1024})
      for (int units = 1; units <= 70000; units++) {
        const tgx::GemvGrid g = tgx::gemv_grid_plan(units, upb, cap);
        const int want = (units + upb - 1) / upb;
        const int rounds = (want + cap - 1) / cap;
        const int ragged = want < cap ? want : cap, balanced = (want + rounds - 1) / rounds;
        REQUIRE(g.grid >= 1 && g.grid <= cap);
        REQUIRE((long long)g.grid * upb * g.rounds >= units);
        REQUIRE((long long)(g.grid - 1) * upb < units);          // the last workgroup's first unit exists: none is without a unit
        REQUIRE(g.rounds == rounds);
        // the unit loop's own trip counts: the first workgroup runs `rounds` trips, the last at least one
        int first = 0, last = 0;
        for (long long ub = 0; ub < units; ub += (long long)g.grid * upb) first++;
        for (long long ub = (long long)(g.grid - 1) * upb; ub < units; ub += (long long)g.grid * upb) last++;
        REQUIRE(first == g.rounds && last >= 1 && last <= first);
        // the two rules
        REQUIRE(balanced >= 1 && balanced <= ragged);
        REQUIRE((long long)balanced * upb * rounds >= units && (long long)(balanced - 1) * upb < units);
        if (want <= cap) REQUIRE(balanced == ragged);
        REQUIRE(g.grid == ragged);
        plans++;
        if (rounds > 1) multi_round++;
      }
  // the figures of the 1B decode step at 256 CUs: gate_up 8192 units (2048 workgroups' worth) and the lm_head's 64128
  {
    const int units = 8192, upb = 4, cap = 768;
    REQUIRE(tgx::gemv_grid_plan(units, upb, cap).grid == 768 && tgx::gemv_grid_plan(units, upb, cap).rounds == 3);
    REQUIRE(tgx::gemv_grid_plan(units, upb, 1024).grid == 1024 && tgx::gemv_grid_plan(units, upb, 1024).rounds == 2);
  }
  {
    const int units = 64128, upb = 4, cap = 1024;
    REQUIRE(tgx::gemv_grid_plan(units, upb, cap).grid == 1024 && tgx::gemv_grid_plan(units, upb, cap).rounds == 16);
  }
  {      // degenerate arguments are clamped, not divided by
    const int units = 0, upb = 0, cap = 0;
    REQUIRE(tgx::gemv_grid_plan(units, upb, cap).grid == 1 && tgx::gemv_grid_plan(units, upb, cap).rounds == 1);
  }
  printf("gemv_grid_check: ok (%lld plans, %lld of them with more than one round)\n", plans, multi_round);
  return 0;
}
