// verify_tree_plan_check.cpp — the CPU audit of tinygpt_amd/csrc/verify_tree_plan.h (the host side of tgx_verify_tree): every tree of up to 6 nodes and random trees
// of 15, against a naive walk along the parent pointers; the refusals.  Stand-alone: built with the address and undefined-behaviour sanitizers (tinygpt_amd/build.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../tinygpt_amd/csrc/verify_tree_plan.h"

namespace vt = verify_tree_plan;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } } while (0)

// the naive statement: from position p follow the parent pointers to the root
static void naive(const std::vector<int32_t>& parent, int p, int& depth, unsigned& mask) {
  depth = 0; mask = 0;
  int q = p;
  for (;;) {
    mask |= 1u << q;
    if (q == 0) break;
    q = parent[(size_t)(q - 1)] + 1;
    depth++;
  }
}

static long long g_trees = 0;
static void audit(const std::vector<int64_t>& tokens, const std::vector<int32_t>& parent) {
  const int n = (int)parent.size();
  vt::Plan p;
  // expected status by the naive rules
  bool dup = false;
  for (int i = 0; i < n && !dup; i++)
    for (int j = 0; j < i; j++)
      if (parent[(size_t)j] == parent[(size_t)i] && tokens[(size_t)j] == tokens[(size_t)i]) { dup = true; break; }
  const vt::Status st = vt::plan(tokens.data(), parent.data(), n, p);
  CHECK(st == (dup ? vt::DUP_SIBLING : vt::OK), "status %d, duplicate siblings %d (n %d)", (int)st, (int)dup, n);
  // the shape is computed before the sibling check: audit it either way
  CHECK(p.M == n + 1, "M %d for %d nodes", p.M, n);
  int md = 0;
  bool chain = true;
  for (int q = 0; q <= n; q++) {
    int d; unsigned m;
    naive(parent, q, d, m);
    CHECK(p.depth[q] == d, "depth[%d] %d, the walk gives %d", q, p.depth[q], d);
    CHECK(p.anc[q] == m, "anc[%d] %#x, the walk gives %#x", q, (unsigned)p.anc[q], m);
    CHECK((p.anc[q] & 1u) && (p.anc[q] >> q) == 1u, "anc[%d] %#x: bit 0 and bit %d set, none above", q, (unsigned)p.anc[q], q);
    CHECK(__builtin_popcount(p.anc[q]) == d + 1, "anc[%d] holds %d bits at depth %d", q, __builtin_popcount(p.anc[q]), d);
    CHECK(p.par[q] == (q ? parent[(size_t)(q - 1)] + 1 : -1), "par[%d] %d", q, p.par[q]);
    md = d > md ? d : md;
    if (q && parent[(size_t)(q - 1)] != q - 2) chain = false;
  }
  CHECK(p.max_depth == md, "max_depth %d, the walk gives %d", p.max_depth, md);
  CHECK(p.chain == chain, "chain %d, expected %d", (int)p.chain, (int)chain);
  CHECK(!chain || p.max_depth == n, "a chain of %d nodes has depth %d", n, p.max_depth);
  g_trees++;
}

static void enumerate(std::vector<int32_t>& parent, int n) {
  const int i = (int)parent.size();
  if (i == n) {
    std::vector<int64_t> distinct((size_t)n), same((size_t)n, 7), pairs((size_t)n);
    for (int k = 0; k < n; k++) { distinct[(size_t)k] = 100 + k; pairs[(size_t)k] = k / 2; }
    audit(distinct, parent);
    audit(same, parent);      // every pair of siblings is a duplicate
    audit(pairs, parent);
    return;
  }
  for (int pr = -1; pr < i; pr++) { parent.push_back(pr); enumerate(parent, n); parent.pop_back(); }
}

int main() {
  for (int n = 1; n <= 6; n++) { std::vector<int32_t> parent; enumerate(parent, n); }
  std::mt19937_64 rng(20240607);
  for (int t = 0; t < 20000; t++) {
    const int n = vt::MAX_NODES;
    std::vector<int32_t> parent((size_t)n);
    std::vector<int64_t> tokens((size_t)n);
    const int style = t % 4;      // uniform parents, bushy (near the root), deep (near the last node), few distinct tokens
    for (int i = 0; i < n; i++) {
      int pr = (int)(rng() % (unsigned)(i + 1)) - 1;
      if (style == 1) pr = (int)(rng() % (unsigned)((i + 1) < 3 ? (i + 1) : 3)) - 1;
      if (style == 2 && i) pr = i - 1 - (int)(rng() % (unsigned)(i < 2 ? i : 2));
      parent[(size_t)i] = pr;
      tokens[(size_t)i] = style == 3 ? (int64_t)(rng() % 3) : (int64_t)(rng() % 50000);
    }
    audit(tokens, parent);
  }
  // the shapes the issue names: star, chain, caterpillar, two interleaved branches, a binary tree of 14
  {
    std::vector<int32_t> star(15, -1), chain(15), cat, inter(15), bin(14);
    std::vector<int64_t> tok(15);
    for (int i = 0; i < 15; i++) { tok[(size_t)i] = i; chain[(size_t)i] = i - 1; inter[(size_t)i] = i < 2 ? -1 : i - 2; }
    for (int i = 0; i < 14; i++) bin[(size_t)i] = i < 2 ? -1 : (i - 2) / 2;
    audit(tok, star); audit(tok, chain); audit(tok, inter);
    audit(std::vector<int64_t>(tok.begin(), tok.begin() + 14), bin);
    vt::Plan p;
    CHECK(vt::plan(tok.data(), star.data(), 15, p) == vt::OK && p.max_depth == 1 && !p.chain, "star");
    CHECK(vt::plan(tok.data(), chain.data(), 15, p) == vt::OK && p.max_depth == 15 && p.chain, "chain");
    CHECK(vt::plan(tok.data(), inter.data(), 15, p) == vt::OK && p.max_depth == 8 && p.anc[15] == 0xAAAB, "interleaved: depth %d anc %#x", p.max_depth, (unsigned)p.anc[15]);
    CHECK(vt::plan(tok.data(), bin.data(), 14, p) == vt::OK && p.max_depth == 3, "binary tree: depth %d", p.max_depth);
    CHECK(vt::plan(tok.data(), chain.data(), 1, p) == vt::OK && p.chain && p.M == 2, "one node is a chain");
  }
  // refusals
  {
    vt::Plan p;
    const int64_t tok[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    int32_t par[16];
    for (int i = 0; i < 16; i++) par[i] = -1;
    CHECK(vt::plan(tok, par, 0, p) == vt::BAD_COUNT, "n 0");
    CHECK(vt::plan(tok, par, -3, p) == vt::BAD_COUNT, "n -3");
    CHECK(vt::plan(tok, par, 16, p) == vt::BAD_COUNT, "n 16");
    par[0] = 0;
    CHECK(vt::plan(tok, par, 3, p) == vt::BAD_PARENT && p.bad == 0, "parent[0] == 0");
    par[0] = -1; par[2] = 2;
    CHECK(vt::plan(tok, par, 3, p) == vt::BAD_PARENT && p.bad == 2, "parent[2] == 2");
    par[2] = 5;
    CHECK(vt::plan(tok, par, 3, p) == vt::BAD_PARENT && p.bad == 2, "parent[2] == 5");
    par[2] = -2;
    CHECK(vt::plan(tok, par, 3, p) == vt::BAD_PARENT && p.bad == 2, "parent[2] == -2");
    par[2] = 0;
    const int64_t dup[3] = {4, 4, 4};
    CHECK(vt::plan(dup, par, 3, p) == vt::DUP_SIBLING && p.bad == 1, "siblings 0 and 1 carry the same token");
    const int64_t ok[3] = {4, 5, 4};      // the same token under different parents is fine
    CHECK(vt::plan(ok, par, 3, p) == vt::OK, "the same token under different parents");
    CHECK(vt::plan(nullptr, par, 3, p) == vt::OK, "no tokens: the shape alone");
  }
  if (g_fail) { std::printf("verify_tree_plan_check: %d FAILED\n", g_fail); return 1; }
  std::printf("verify_tree_plan_check: ok (%lld trees)\n", g_trees);
  return 0;
}
