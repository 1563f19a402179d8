// spec_draft.h — the draft source of GPTConfig::speculate: prompt lookup.  No second model: the tokens that followed the most recent earlier occurrence of the
// sequence's own tail are proposed as its continuation (repeated spans — quoted text, code, lists — are where a guess is cheap and often right), and the device
// verifies them in one pass (include/tgx.h tgx_verify_row).  Host-only, the standard library alone: tests/spec_draft_check.cpp drives it on a CPU.
#pragma once
#include <algorithm>
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

// ---- GPTConfig::speculateTree: a token TREE of guesses (include/tgx.h tgx_verify_tree).  A chain stops paying at its first wrong token; where the sequence's tail
// has occurred before with DIFFERENT continuations, the same budget of positions can hold several of them, and the device follows whichever the model produces.
struct DraftTree {
  std::vector<int32_t> tokens, parent;      // node i: its token, its parent node (-1: a child of the sequence's last token, else an index < i)
  int branches = 0;                         // the chains below the root (0: no match; 1: the tree is ngram_draft's chain)
};

// For the longest matching suffix (3, then 2, then 1 tokens: ngram_draft's) up to max_branches of its earlier occurrences, the most recent first, and only
// occurrences whose FIRST continuation token differs from every one taken before (siblings carry distinct tokens; an older occurrence with the same first token
// would only repeat or contradict a more recent guess below it).  The continuations are merged into a trie of at most max_nodes nodes — their first tokens
// differ, so the trie is one chain per occurrence below the root — emitted chain by chain: topological order.  The budget: every chain behind the first gets
// max_nodes / branches nodes, the first chain the rest; what a short continuation leaves unused is not handed on.  The first chain is exactly
// ngram_draft(seq, its share): a tree pass never accepts fewer tokens than the chain of that length would.
inline DraftTree ngram_tree(const std::vector<int32_t>& seq, int max_nodes, int max_branches) {
  DraftTree t;
  const size_t n = seq.size();
  if (max_nodes < 1 || max_branches < 1) return t;
  for (size_t k = 3; k >= 1; k--) {
    if (n < k + 1) continue;
    const int32_t* suf = seq.data() + (n - k);
    std::vector<size_t> starts;             // where each taken occurrence's continuation begins
    for (size_t s = n - k; s-- > 0 && starts.size() < (size_t)max_branches;) {
      bool same = true;
      for (size_t j = 0; j < k && same; j++) same = seq[s + j] == suf[j];
      if (!same) continue;
      bool fresh = true;
      for (size_t b : starts) fresh = fresh && seq[b] != seq[s + k];
      if (fresh) starts.push_back(s + k);
    }
    if (starts.empty()) continue;
    const int nb = (int)std::min<size_t>(starts.size(), (size_t)max_nodes);      // (every chain holds at least one node)
    const int share = max_nodes / nb, first = max_nodes - (nb - 1) * share;
    for (int b = 0; b < nb; b++) {
      const int room = b ? share : first;
      int prev = -1;
      for (size_t i = starts[(size_t)b]; i < n && (int)(i - starts[(size_t)b]) < room; i++) {
        t.tokens.push_back(seq[i]); t.parent.push_back(prev);
        prev = (int)t.tokens.size() - 1;
      }
    }
    t.branches = nb;
    return t;
  }
  return t;
}

}  // namespace tgxh
