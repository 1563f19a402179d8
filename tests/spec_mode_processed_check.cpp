// spec_mode_processed_check.cpp — SpecInputs::verifyProcessed (tinygpt_amd/host/spec_mode.h; GPTConfig::speculateProcessed) on a CPU, built with the address and
// undefined-behaviour sanitizers (tinygpt_amd/build.py build_spec_mode_processed_check).  Two statements, over every combination of the inputs:
//   1. verifyProcessed false: the function gives what it gave before the field existed — the old rule, restated here with `processors` switching the drafts off;
//   2. processors && verifyProcessed: the answer is that of the same inputs with neutral processors — the greedy, sampled and rows rules as they stand.
#include <cstdio>

#include "../tinygpt_amd/host/spec_mode.h"

using tgxh::SpecInputs;
using tgxh::SpecMode;

static const char* name(SpecMode m) { return m == SpecMode::Off ? "Off" : m == SpecMode::Greedy ? "Greedy" : "Sampled"; }

// the rule before verifyProcessed
static SpecMode old_rule(const SpecInputs& in) {
  const bool batch_ok = in.batch == 1 || (in.verifyRows && in.batch > 1);
  if (in.speculate <= 0 || !batch_ok || in.processors || !in.rowStopCalls || in.stopIds > in.maxStopIds) return SpecMode::Off;
  if (in.greedy) return in.verifyRow ? SpecMode::Greedy : SpecMode::Off;
  return in.speculateSampled && in.verifyRowSampled ? SpecMode::Sampled : SpecMode::Off;
}

int main() {
  int failures = 0, cases = 0;
  const int speculates[] = {-1, 0, 1, 7}, batches[] = {0, 1, 2, 5};
  const size_t stops[] = {0, 8, 9};
  for (int spec : speculates) for (int batch : batches) for (size_t stop : stops)
    for (int bits = 0; bits < 128; bits++) {
      SpecInputs in;
      in.speculate = spec; in.batch = batch; in.stopIds = stop; in.maxStopIds = 8;
      in.speculateSampled = bits & 1; in.greedy = bits & 2; in.processors = bits & 4; in.rowStopCalls = bits & 8; in.verifyRow = bits & 16; in.verifyRowSampled = bits & 32;
      in.verifyRows = bits & 64;
      cases++;
      // 1. the old fields alone
      const SpecMode got = tgxh::spec_mode(in), want = old_rule(in);
      if (in.verifyProcessed || got != want) { failures++; printf("FAIL (old inputs) speculate %d batch %d stops %zu bits %d: got %s want %s\n", spec, batch, stop, bits, name(got), name(want)); }
      // 2. with the verify calls taking processed rows
      SpecInputs on = in; on.verifyProcessed = true;
      SpecInputs neutral = in; neutral.processors = false;
      const SpecMode got_on = tgxh::spec_mode(on), want_on = old_rule(neutral);
      if (got_on != want_on) { failures++; printf("FAIL (verifyProcessed) speculate %d batch %d stops %zu bits %d: got %s want %s\n", spec, batch, stop, bits, name(got_on), name(want_on)); }
      // ... which changes nothing for a call without processors
      if (!in.processors && got_on != got) { failures++; printf("FAIL verifyProcessed changes a call with neutral processors (bits %d)\n", bits); }
    }
  // a processed greedy call drafts only with the field set
  SpecInputs g; g.speculate = 8; g.processors = true; g.rowStopCalls = true; g.verifyRow = true;
  if (tgxh::spec_mode(g) != SpecMode::Off) { failures++; printf("FAIL processors alone draft\n"); }
  g.verifyProcessed = true;
  if (tgxh::spec_mode(g) != SpecMode::Greedy) { failures++; printf("FAIL processors with verifyProcessed do not draft\n"); }
  if (failures) { printf("spec_mode_processed_check: %d of %d FAILED\n", failures, cases); return 1; }
  printf("spec_mode_processed_check: ok (%d cases)\n", cases);
  return 0;
}
