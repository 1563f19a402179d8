// gemv_grid.h — the grid of a batch-1..4 GEMV launch (kernels/gemv.h, kernels/gemv_packed.h) as a pure function: host only, no HIP, audited on the CPU
// by tests/gemv_grid_check.cpp.
//
// A launch has `units` row pairs; a 256-thread workgroup holds `upb` = 4 / ks of them at a time and walks the units
//   blockIdx * upb + slot,  + grid * upb,  + 2 grid * upb, ...
// so every workgroup runs ceil(units / (grid * upb)) rounds or one fewer.  `cap` is the most workgroups the launch may have (CUs x workgroups per CU).
#pragma once

namespace tgx {

struct GemvGrid {
  int grid;      // workgroups launched: 1 <= grid <= cap, none without a unit
  int rounds;    // trips of the longest workgroup's unit loop: grid * upb * rounds >= units
};

inline GemvGrid gemv_grid_plan(int units, int upb, int cap) {
  if (units < 1) units = 1;
  if (upb < 1) upb = 1;
  if (cap < 1) cap = 1;
  const int want = (units + upb - 1) / upb;                   // workgroups at one round each
  // Every workgroup the cap allows, the last round ragged: gate_up's 2048 workgroups' worth at a cap of 768 runs as rounds of 768, 768, 512.  A grid of equal
  // trip counts (ceil(want / rounds): 683 x 3) measured SLOWER — it gave back the whole gain of 3 workgroups per CU on gate_up and cost the lm_head 6 us
  // (1002 x 16 against 1024 x 15..16) — profiles/packed_kpart_geometry.txt section 4.
  const int grid = want < cap ? want : cap;
  return GemvGrid{grid, (want + grid - 1) / grid};            // (== ceil(want / cap): grid is want or cap)
}

}  // namespace tgx
