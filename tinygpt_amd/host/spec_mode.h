// spec_mode.h — which speculative path a generate call takes (GPTConfig::speculate / speculateSampled; engine.cpp).  Host-only, no dependencies:
// tests/spec_mode_check.cpp drives it on a CPU.
#pragma once
#include <cstddef>

namespace tgxh {

enum class SpecMode { Off, Greedy, Sampled };

// what the call and the backend offer
struct SpecInputs {
  int speculate = 0;                 // GPTConfig::speculate: the maximum draft length (0 = off)
  bool speculateSampled = false;     // GPTConfig::speculateSampled
  int batch = 1;
  bool greedy = true;                // the call's sampler is greedy (Sampler.cpp:15-21)
  bool processors = false;           // a penalty or a logit bias is on
  size_t stopIds = 0, maxStopIds = 0;   // the model's EOS ids against what a row's stop set holds
  bool rowStopCalls = false;         // the backend exports tgx_set_row_stop and tgx_decode_rows
  bool verifyRow = false;            // ... tgx_verify_row
  bool verifyRowSampled = false;     // ... tgx_verify_row_sampled, tgx_set_row_sampler and tgx_sample_row
  bool verifyRows = false;           // ... tgx_verify_rows (and tgx_forward_rows' per-row lifecycle): a batch of several sequences may speculate, all rows in one pass
};

// Greedy: as before this switch existed.  Sampled: only when asked for AND served — everything else keeps the loop it had, so a default configuration and a
// backend without the call (the CPU oracle) run exactly what they ran.  A batch of several sequences speculates only where the backend verifies rows jointly
// (verifyRows); without it every input gives what it gave before that call existed
inline SpecMode spec_mode(const SpecInputs& in) {
  if (in.speculate <= 0 || (in.batch != 1 && !(in.verifyRows && in.batch > 1)) || in.processors || !in.rowStopCalls || in.stopIds > in.maxStopIds) return SpecMode::Off;
  if (in.greedy) return in.verifyRow ? SpecMode::Greedy : SpecMode::Off;
  return in.speculateSampled && in.verifyRowSampled ? SpecMode::Sampled : SpecMode::Off;
}

}  // namespace tgxh
