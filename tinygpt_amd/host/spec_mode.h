// spec_mode.h — which speculative path a generate call takes (GPTConfig::speculate / speculateSampled / speculateProcessed; engine.cpp).  Host-only, no
// dependencies: tests/spec_mode_check.cpp and tests/spec_mode_processed_check.cpp drive it on a CPU.
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
  bool processors = false;           // a penalty, a logit bias or a regex is on
  bool verifyProcessed = false;      // GPTConfig::speculateProcessed AND a backend that takes option verify.processors: the verify calls accept processed rows
  size_t stopIds = 0, maxStopIds = 0;   // the model's EOS ids against what a row's stop set holds
  bool rowStopCalls = false;         // the backend exports tgx_set_row_stop and tgx_decode_rows
  bool verifyRow = false;            // ... tgx_verify_row
  bool verifyRowSampled = false;     // ... tgx_verify_row_sampled, tgx_set_row_sampler and tgx_sample_row
  bool verifyRows = false;           // ... tgx_verify_rows (and tgx_forward_rows' per-row lifecycle): a batch of several sequences may speculate, all rows in one pass
};

// Greedy: as before this switch existed.  Sampled: only when asked for AND served — everything else keeps the loop it had, so a default configuration and a
// backend without the call (the CPU oracle) run exactly what they ran.  A batch of several sequences speculates only where the backend verifies rows jointly
// (verifyRows); without it every input gives what it gave before that call existed.  Processors switch the drafts off unless the verify calls process every
// position as its step would (verifyProcessed); with it the greedy, sampled and rows rules hold as they stand
inline SpecMode spec_mode(const SpecInputs& in) {
  if (in.speculate <= 0 || (in.batch != 1 && !(in.verifyRows && in.batch > 1)) || (in.processors && !in.verifyProcessed) || !in.rowStopCalls || in.stopIds > in.maxStopIds) return SpecMode::Off;
  if (in.greedy) return in.verifyRow ? SpecMode::Greedy : SpecMode::Off;
  return in.speculateSampled && in.verifyRowSampled ? SpecMode::Sampled : SpecMode::Off;
}

}  // namespace tgxh
