// spec_tree_check.cpp — the tree drafter (tinygpt_amd/host/spec_draft.h ngram_tree) on a CPU, built with the address and undefined-behaviour sanitizers
// (tinygpt_amd/build.py build_spec_tree_check): scripted cases with hand-written expectations, and a random run against the properties the drafter promises.
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <set>
#include <vector>

#include "../tinygpt_amd/host/spec_draft.h"

typedef std::vector<int32_t> Ids;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the tree as its chains below the root, in emission order; checks the shape on the way
static std::vector<Ids> chains_of(const tgxh::DraftTree& t, int max_nodes) {
  std::vector<Ids> chains;
  const int n = (int)t.tokens.size();
  CHECK(t.parent.size() == t.tokens.size(), "tokens / parent sizes %zu / %zu", t.tokens.size(), t.parent.size());
  CHECK(n <= max_nodes || max_nodes < 1, "%d nodes for a budget of %d", n, max_nodes);
  std::set<int32_t> roots;
  for (int i = 0; i < n; i++) {
    const int p = t.parent[(size_t)i];
    CHECK(p >= -1 && p < i, "parent[%d] = %d: not topological", i, p);
    if (p == -1) {
      CHECK(roots.insert(t.tokens[(size_t)i]).second, "two children of the root carry token %d", t.tokens[(size_t)i]);
      chains.emplace_back();
    } else CHECK(p == i - 1, "node %d hangs below %d: the chains are emitted one after the other", i, p);
    if (!chains.empty()) chains.back().push_back(t.tokens[(size_t)i]);
  }
  CHECK((int)chains.size() == t.branches, "branches %d, chains %zu", t.branches, chains.size());
  return chains;
}

// every start position (the index of the first continuation token) behind an earlier occurrence of the last k tokens, the most recent first
static std::vector<int> occurrences(const Ids& seq, int k) {
  const int n = (int)seq.size();
  std::vector<int> out;
  for (int s = n - k - 1; s >= 0; s--) {
    bool same = true;
    for (int j = 0; j < k; j++) same = same && seq[(size_t)(s + j)] == seq[(size_t)(n - k + j)];
    if (same) out.push_back(s + k);
  }
  return out;
}

// The random audit checks what the drafter PROMISES, not how it computes it: the longest matching suffix; one chain per candidate, each the text behind the MOST
// RECENT occurrence with that first token; the chains ordered most recent first and none of the more recent candidates left out; distinct first tokens; at most
// max_branches chains and max_nodes nodes; every chain behind the first within max_nodes / chains and as long as its text and that share allow, the first chain
// with the rest of the budget and exactly ngram_draft cut to its length
static void audit(const Ids& seq, int max_nodes, int max_branches) {
  const tgxh::DraftTree t = tgxh::ngram_tree(seq, max_nodes, max_branches);
  const std::vector<Ids> got = chains_of(t, max_nodes);
  const int n = (int)seq.size();
  if (max_nodes < 1 || max_branches < 1) { CHECK(got.empty() && t.tokens.empty(), "a tree without a budget"); return; }
  int k = 0;
  std::vector<int> occ;
  for (int kk = 3; kk >= 1 && occ.empty(); kk--)
    if (n >= kk + 1) { occ = occurrences(seq, kk); k = kk; }
  const Ids chain = tgxh::ngram_draft(seq, max_nodes);
  CHECK(chain.empty() == occ.empty() && got.empty() == occ.empty(), "a tree exactly where some suffix has occurred before (k %d)", k);
  if (got.empty()) return;
  // the candidates: per distinct first continuation its most recent occurrence, most recent first
  std::vector<int> cand;
  std::set<int32_t> firsts;
  for (int st : occ)
    if (firsts.insert(seq[(size_t)st]).second) cand.push_back(st);
  const int want_nb = (int)std::min<size_t>({cand.size(), (size_t)max_branches, (size_t)max_nodes});
  CHECK((int)got.size() == want_nb, "%zu chains: %zu candidates, %d branches, %d nodes", got.size(), cand.size(), max_branches, max_nodes);
  int total = 0;
  for (size_t b = 0; b < got.size() && b < cand.size(); b++) {
    const Ids& c = got[b];
    const int st = cand[b];                                  // the b-th most recent candidate: none skipped, in this order
    CHECK(!c.empty() && c[0] == seq[(size_t)st], "chain %zu starts with %d, the %zu-th most recent candidate continues with %d", b, c.empty() ? -1 : c[0], b, seq[(size_t)st]);
    for (size_t i = 0; i < c.size(); i++) CHECK(st + (int)i < n && c[i] == seq[(size_t)st + i], "chain %zu token %zu is not the text behind its occurrence", b, i);
    total += (int)c.size();
  }
  CHECK(total <= max_nodes, "%d nodes for a budget of %d", total, max_nodes);
  const int nb = (int)got.size(), share = max_nodes / nb;
  for (size_t b = 1; b < got.size() && b < cand.size(); b++)
    CHECK((int)got[b].size() == std::min(share, n - cand[b]), "chain %zu holds %zu tokens: share %d, text %d", b, got[b].size(), share, n - cand[b]);
  CHECK((int)got[0].size() >= std::min(share, (int)chain.size()), "the first chain holds %zu tokens, less than a share (%d) of the chain (%zu)", got[0].size(), share, chain.size());
  CHECK((int)got[0].size() == std::min((int)chain.size(), max_nodes - (nb - 1) * share), "the first chain holds %zu tokens: the rest of the budget is %d, the chain %zu", got[0].size(), max_nodes - (nb - 1) * share, chain.size());
  CHECK(got[0] == tgxh::ngram_draft(seq, (int)got[0].size()), "the first chain is not ngram_draft cut to %zu tokens", got[0].size());
  if (max_branches == 1) CHECK(got.size() == 1 && got[0] == chain, "one branch is ngram_draft itself");
}

int main() {
  // scripted: "a b c X .. a b c Y .. a b c" proposes Y (the most recent) first, then X
  {
    const Ids seq = {1, 2, 3, 10, 11, 12, 1, 2, 3, 20, 21, 1, 2, 3};
    const tgxh::DraftTree t = tgxh::ngram_tree(seq, 6, 3);
    CHECK(t.branches == 2, "branches %d", t.branches);
    CHECK((t.tokens == Ids{20, 21, 1, 10, 11, 12}), "tokens");
    CHECK((t.parent == Ids{-1, 0, 1, -1, 3, 4}), "parents");
    const tgxh::DraftTree one = tgxh::ngram_tree(seq, 6, 1);
    CHECK(one.branches == 1 && one.tokens == tgxh::ngram_draft(seq, 6) && (one.parent == Ids{-1, 0, 1, 2, 3}), "one branch");      // (the continuation ends with the sequence: 5 tokens)
    const tgxh::DraftTree odd = tgxh::ngram_tree(seq, 7, 2);      // 7 nodes over two chains: 4 + 3
    CHECK((odd.tokens == Ids{20, 21, 1, 2, 10, 11, 12}) && (odd.parent == Ids{-1, 0, 1, 2, -1, 4, 5}), "7 nodes");
    CHECK(tgxh::ngram_tree(seq, 0, 3).tokens.empty() && tgxh::ngram_tree(seq, 5, 0).tokens.empty(), "no budget");
    CHECK(tgxh::ngram_tree(Ids{1, 2, 3, 4}, 8, 3).branches == 0, "no match");
    // an older occurrence with the same first continuation is not a second branch
    const Ids same = {5, 6, 7, 8, 5, 6, 7, 9, 5, 6};
    const tgxh::DraftTree s = tgxh::ngram_tree(same, 8, 3);
    CHECK(s.branches == 1 && (s.tokens == tgxh::ngram_draft(same, 8)), "same first continuation");
    // more branches than nodes
    const Ids many = {1, 2, 1, 3, 1, 4, 1, 5, 1};
    const tgxh::DraftTree m = tgxh::ngram_tree(many, 2, 4);
    CHECK(m.branches == 2 && (m.tokens == Ids{5, 4}) && (m.parent == Ids{-1, -1}), "two nodes, four candidates");
  }
  srand(7);
  for (int it = 0; it < 40000; it++) {
    const int n = rand() % 40, alphabet = 2 + rand() % 5;
    Ids seq((size_t)n);
    for (int i = 0; i < n; i++) seq[(size_t)i] = rand() % alphabet;
    audit(seq, rand() % 17, rand() % 6);
  }
  if (failures) { printf("spec_tree_check: %d FAILED\n", failures); return 1; }
  printf("spec_tree_check: ok\n");
  return 0;
}
