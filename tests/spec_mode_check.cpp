// spec_mode_check.cpp — which speculative path a generate call takes (tinygpt_amd/host/spec_mode.h) on a CPU, built with the address and undefined-behaviour
// sanitizers (tinygpt_amd/build.py build_spec_mode_check): every combination of the inputs against the rule spelled out.
#include <cstdio>

#include "../tinygpt_amd/host/spec_mode.h"

using tgxh::SpecInputs;
using tgxh::SpecMode;

static const char* name(SpecMode m) { return m == SpecMode::Off ? "Off" : m == SpecMode::Greedy ? "Greedy" : "Sampled"; }

int main() {
  int failures = 0, cases = 0;
  const int speculates[] = {-1, 0, 1, 7}, batches[] = {1, 2};
  const size_t stops[] = {0, 8, 9};
  for (int spec : speculates) for (int batch : batches) for (size_t stop : stops)
    for (int bits = 0; bits < 64; bits++) {
      SpecInputs in;
      in.speculate = spec; in.batch = batch; in.stopIds = stop; in.maxStopIds = 8;
      in.speculateSampled = bits & 1; in.greedy = bits & 2; in.processors = bits & 4; in.rowStopCalls = bits & 8; in.verifyRow = bits & 16; in.verifyRowSampled = bits & 32;
      // the rule: a draft length, one sequence, neutral processors, the row calls, a stop set that fits; then the sampler decides which call verifies
      SpecMode want = SpecMode::Off;
      const bool base = spec > 0 && batch == 1 && !in.processors && in.rowStopCalls && stop <= 8;
      if (base && in.greedy && in.verifyRow) want = SpecMode::Greedy;
      if (base && !in.greedy && in.speculateSampled && in.verifyRowSampled) want = SpecMode::Sampled;
      const SpecMode got = tgxh::spec_mode(in);
      cases++;
      if (got != want) { failures++; printf("FAIL speculate %d batch %d stops %zu bits %d: got %s want %s\n", spec, batch, stop, bits, name(got), name(want)); }
      // what every run before the switch relied on: without speculateSampled a sampling configuration never speculates, and a greedy one ignores the switch
      SpecInputs off = in; off.speculateSampled = false;
      if (!in.greedy && tgxh::spec_mode(off) != SpecMode::Off) { failures++; printf("FAIL sampled without the switch speculates (bits %d)\n", bits); }
      if (in.greedy && tgxh::spec_mode(off) != got) { failures++; printf("FAIL the switch changes a greedy call (bits %d)\n", bits); }
    }
  // the defaults: off
  if (tgxh::spec_mode(SpecInputs{}) != SpecMode::Off) { failures++; printf("FAIL defaults\n"); }
  if (failures) { printf("spec_mode_check: %d of %d FAILED\n", failures, cases); return 1; }
  printf("spec_mode_check: ok (%d cases)\n", cases);
  return 0;
}
