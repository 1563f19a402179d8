// spec_rows_check.cpp — SpecInputs::verifyRows (tinygpt_amd/host/spec_mode.h) on a CPU, built with the address and undefined-behaviour sanitizers
// (tinygpt_amd/build.py build_spec_rows_check): a backend that verifies the rows of a batch jointly (tgx_verify_rows) lets a batch of several sequences speculate
// exactly where one sequence does — and without it every input gives what it gave before the field existed.
#include <cstdio>

#include "../tinygpt_amd/host/spec_mode.h"

using tgxh::SpecInputs;
using tgxh::SpecMode;

static const char* name(SpecMode m) { return m == SpecMode::Off ? "Off" : m == SpecMode::Greedy ? "Greedy" : "Sampled"; }

// the rule as tests/spec_mode_check.cpp spells it out: the table of the function before verifyRows existed
static SpecMode before(const SpecInputs& in) {
  const bool base = in.speculate > 0 && in.batch == 1 && !in.processors && in.rowStopCalls && in.stopIds <= in.maxStopIds;
  if (base && in.greedy && in.verifyRow) return SpecMode::Greedy;
  if (base && !in.greedy && in.speculateSampled && in.verifyRowSampled) return SpecMode::Sampled;
  return SpecMode::Off;
}

int main() {
  int failures = 0, cases = 0;
  const int speculates[] = {-1, 0, 1, 7}, batches[] = {-1, 0, 1, 2, 3, 8};
  const size_t stops[] = {0, 8, 9};
  for (int spec : speculates) for (int batch : batches) for (size_t stop : stops)
    for (int bits = 0; bits < 64; bits++) {
      SpecInputs in;
      in.speculate = spec; in.batch = batch; in.stopIds = stop; in.maxStopIds = 8;
      in.speculateSampled = bits & 1; in.greedy = bits & 2; in.processors = bits & 4; in.rowStopCalls = bits & 8; in.verifyRow = bits & 16; in.verifyRowSampled = bits & 32;
      // verifyRows false (the default, and spelled out): today's table for every input
      cases++;
      if (tgxh::spec_mode(in) != before(in)) { failures++; printf("FAIL default verifyRows changes speculate %d batch %d stops %zu bits %d: got %s want %s\n", spec, batch, stop, bits, name(tgxh::spec_mode(in)), name(before(in))); }
      SpecInputs off = in; off.verifyRows = false;
      if (tgxh::spec_mode(off) != before(in)) { failures++; printf("FAIL verifyRows false changes speculate %d batch %d stops %zu bits %d\n", spec, batch, stop, bits); }
      // verifyRows true: a batch of several sequences gives what batch 1 gives with the same inputs; batch 1 itself, and no batch at all, what they gave
      SpecInputs on = in; on.verifyRows = true;
      SpecInputs one = in; one.batch = 1;
      const SpecMode want = batch > 1 ? before(one) : before(in);
      const SpecMode got = tgxh::spec_mode(on);
      cases++;
      if (got != want) { failures++; printf("FAIL verifyRows true speculate %d batch %d stops %zu bits %d: got %s want %s\n", spec, batch, stop, bits, name(got), name(want)); }
    }
  // batch 2 speculates with the call: both modes are reached
  SpecInputs g; g.speculate = 7; g.batch = 2; g.rowStopCalls = true; g.verifyRow = true; g.verifyRows = true;
  if (tgxh::spec_mode(g) != SpecMode::Greedy) { failures++; printf("FAIL batch 2 greedy\n"); }
  SpecInputs s = g; s.greedy = false; s.speculateSampled = true; s.verifyRowSampled = true;
  if (tgxh::spec_mode(s) != SpecMode::Sampled) { failures++; printf("FAIL batch 2 sampled\n"); }
  if (failures) { printf("spec_rows_check: %d of %d FAILED\n", failures, cases); return 1; }
  printf("spec_rows_check: ok (%d cases)\n", cases);
  return 0;
}
