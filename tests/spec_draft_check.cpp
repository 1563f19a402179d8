// spec_draft_check.cpp — the prompt-lookup drafter (tinygpt_amd/host/spec_draft.h) on a CPU, built with the address and undefined-behaviour sanitizers
// (tinygpt_amd/build.py build_spec_draft_check): the scripted cases of tests/test_spec_draft.py and a random run against a naive quadratic model.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tinygpt_amd/host/spec_draft.h"

typedef std::vector<int32_t> Ids;

static int failures = 0;
static void expect(const char* what, const Ids& seq, int max_draft, const Ids& want) {
  const Ids got = tgxh::ngram_draft(seq, max_draft);
  if (got == want) return;
  failures++;
  printf("FAIL %s: got [", what);
  for (int32_t t : got) printf(" %d", t);
  printf(" ] want [");
  for (int32_t t : want) printf(" %d", t);
  printf(" ]\n");
}

// the definition, spelled out: every suffix length from 3 down, every earlier start from the latest down
static Ids naive(const Ids& seq, int max_draft) {
  const int n = (int)seq.size();
  for (int k = 3; k >= 1; k--)
    for (int s = n - k - 1; s >= 0; s--) {
      bool same = true;
      for (int j = 0; j < k; j++) same = same && seq[(size_t)(s + j)] == seq[(size_t)(n - k + j)];
      if (!same) continue;
      Ids out;
      for (int i = s + k; i < n && (int)out.size() < max_draft; i++) out.push_back(seq[(size_t)i]);
      return out;
    }
  return Ids();
}

int main() {
  expect("empty sequence", {}, 7, {});
  expect("length 1", {5}, 7, {});
  expect("no match", {1, 2, 3, 4, 5}, 7, {});
  expect("the suffix itself is no earlier occurrence", {1, 2, 3}, 7, {});
  expect("longest suffix wins over a shorter, more recent one", {1, 2, 3, 9, 8, 7, 3, 6, 1, 2, 3}, 2, {9, 8});
  expect("most recent occurrence wins", {4, 5, 10, 4, 5, 20, 4, 5}, 1, {20});
  expect("clipped by max_draft", {1, 2, 3, 4, 5, 6, 7, 1, 2, 3}, 3, {4, 5, 6});
  expect("clipped by the end of the sequence", {1, 2, 3, 4, 1, 2, 3}, 15, {4, 1, 2, 3});
  expect("an overlapping earlier occurrence", {7, 7, 7, 7}, 5, {7});
  expect("max_draft 0", {1, 2, 1, 2}, 0, {});
  expect("length 2, repeated token", {3, 3}, 4, {3});
  unsigned long long x = 88172645463325252ull;
  for (int it = 0; it < 4000; it++) {
    Ids seq;
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    const int n = (int)(x % 40), alphabet = 2 + (int)((x >> 8) % 4), md = 1 + (int)((x >> 16) % 15);
    for (int i = 0; i < n; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; seq.push_back((int32_t)(x % (unsigned)alphabet)); }
    expect("random", seq, md, naive(seq, md));
  }
  if (failures) { printf("spec_draft_check: %d failures\n", failures); return 1; }
  printf("spec_draft_check: ok\n");
  return 0;
}
