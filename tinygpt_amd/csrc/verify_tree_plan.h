// verify_tree_plan.h — the host side of tgx_verify_tree (include/tgx.h): the shape of a token tree as the pass needs it.  Host-only — the standard library alone, no
// HIP: tests/verify_tree_plan_check.cpp drives it on a CPU against a naive parent-pointer walk.
//
// The tree arrives as tokens[n] / parent[n] in TOPOLOGICAL order: parent[i] == -1 (a child of the row's current token, the root) or an index < i.  The pass runs
// M = n + 1 positions: position 0 is the root at depth 0, node i is position i + 1 at depth depth(parent) + 1.  Position p attends the row's history and, among the
// M new cache slots, exactly its ancestors and itself: anc[p] has bit q set iff position q is p or an ancestor of p (bit 0, the root, always).  Because a parent's
// index is below its child's, every set bit q of anc[p] has q <= p: the tree mask is a SUBSET of the causal mask.
//
// Refused (INVALID): n outside [1, MAX_NODES], parent[i] outside [-1, i), two children of one parent with the same token (the walk follows THE child that carries
// the produced token: there may be only one).
#pragma once
#include <cstdint>

namespace verify_tree_plan {

constexpr int MAX_NODES = 15;       // == TGX_MAX_TREE_NODES
constexpr int MAX_POS = 16;         // root + nodes == kernels/common.h VERIFY_MAX_POS
enum Status { OK = 0, BAD_COUNT = 1, BAD_PARENT = 2, DUP_SIBLING = 3 };

struct Plan {
  int M = 0;                        // positions of the pass
  int depth[MAX_POS] = {};          // per position
  int par[MAX_POS] = {};            // per position: its parent POSITION (position 0: -1)
  uint16_t anc[MAX_POS] = {};       // per position: the ancestor-or-self mask over positions
  int max_depth = 0;
  bool chain = false;               // parent[i] == i - 1 for every i: the tree is tgx_verify_row_sampled's draft
  int bad = -1;                     // the node a refusal names
};

// the shape alone (tokens == nullptr: no sibling check)
inline Status plan(const int64_t* tokens, const int32_t* parent, int n, Plan& p) {
  p = Plan{};
  if (n < 1 || n > MAX_NODES) return BAD_COUNT;
  p.M = n + 1;
  p.depth[0] = 0; p.par[0] = -1; p.anc[0] = 1;
  p.chain = true;
  for (int i = 0; i < n; i++) {
    const int pr = parent[i];
    if (pr < -1 || pr >= i) { p.bad = i; return BAD_PARENT; }
    const int q = i + 1, pq = pr + 1;      // positions
    p.par[q] = pq;
    p.depth[q] = p.depth[pq] + 1;
    p.anc[q] = (uint16_t)(p.anc[pq] | (1u << q));
    if (p.depth[q] > p.max_depth) p.max_depth = p.depth[q];
    if (pr != i - 1) p.chain = false;
  }
  if (tokens)
    for (int i = 0; i < n; i++)
      for (int j = 0; j < i; j++)
        if (parent[j] == parent[i] && tokens[j] == tokens[i]) { p.bad = i; return DUP_SIBLING; }
  return OK;
}

}  // namespace verify_tree_plan
