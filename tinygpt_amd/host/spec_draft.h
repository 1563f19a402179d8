// spec_draft.h — the draft source of GPTConfig::speculate: prompt lookup.  No second model: the tokens that followed the most recent earlier occurrence of the
// sequence's own tail are proposed as its continuation (repeated spans — quoted text, code, lists — are where a guess is cheap and often right), and the device
// verifies them in one pass (include/tgx.h tgx_verify_row).  Host-only, the standard library alone: tests/spec_draft_check.cpp drives it on a CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tgxh {

// The longest suffix of seq (prompt + generated so far) of 3, then 2, then 1 tokens that also occurs EARLIER in seq (it may overlap the suffix, it is not the
// suffix itself); of its earlier occurrences the most recent; the tokens that followed it, at most max_draft and never past the end of seq.  Empty: no match.
// Linear in seq.size() per call (three scans, each comparing at most 3 tokens per position).
inline std::vector<int32_t> ngram_draft(const std::vector<int32_t>& seq, int max_draft) {
  std::vector<int32_t> out;
  const size_t n = seq.size();
  if (max_draft < 1) return out;
  for (size_t k = 3; k >= 1; k--) {
    if (n < k + 1) continue;
    const int32_t* suf = seq.data() + (n - k);
    for (size_t s = n - k; s-- > 0;) {      // start positions n - k - 1 .. 0: the most recent occurrence first
      bool same = true;
      for (size_t j = 0; j < k && same; j++) same = seq[s + j] == suf[j];
      if (!same) continue;
      for (size_t i = s + k; i < n && out.size() < (size_t)max_draft; i++) out.push_back(seq[i]);
      return out;
    }
  }
  return out;
}

}  // namespace tgxh
