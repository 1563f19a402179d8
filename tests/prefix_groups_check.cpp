// prefix_groups_check.cpp — the CPU audit of tinygpt_amd/csrc/prefix_groups.h beside a real KvPool (built and run by tests/test_prefix_groups.py under the address and
// undefined-behaviour sanitizers; never loaded into Python): the pinned grouping rules of the header on hand-written pools, the cut at 32 / G rows, and the splits.
#include "../tinygpt_amd/csrc/prefix_groups.h"
#include <cstdio>
#include <cstdlib>
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "prefix_groups_check: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)
using prefix_groups::Group; using prefix_groups::Plan; typedef std::vector<int> Ints;
constexpr int BLK = 128, ROWS = 40, CUS = 256;

struct Sim {
  KvPool p;
  std::vector<prefix_groups::Row> st;
  KvPool::Changes ch;
  Sim() : st(ROWS) { p.init(ROWS, 64 * BLK, ROWS * 64 * BLK, BLK); }
  void grow(int row, long long n) { REQUIRE(p.grow(row, st[(size_t)row].past + n, ch) == KvPool::GROW_OK); st[(size_t)row].past += n; st[(size_t)row].live = true; }
  void fork(int src, int dst) {      // as tgx_fork_row: the full blocks by reference, a fresh block for the partial tail
    const long long past = st[(size_t)src].past;
    p.share(src, dst, (int)(past / BLK), past, ch);
    if (past % BLK) p.fork_tail(dst, ch);
    st[(size_t)dst] = st[(size_t)src];
  }
  // the plan; every group: live members in row order that share nb leading blocks, full for each; ranges [s bps, min((s + 1) bps, nb)): <= 16, none empty, the last ends at nb
  Plan plan(int G, int option = BLK, int kv_heads = 8) {
    const Plan pl = prefix_groups::make(p, st.data(), ROWS, G, option, kv_heads, CUS);
    for (const Group& g : pl.groups) {
      REQUIRE(g.n_rows >= 2 && g.n_rows <= 32 / G && g.nb * BLK >= option && g.nsplit >= 1 && g.nsplit <= 16 && (g.nsplit - 1) * g.bps < g.nb && g.nsplit * g.bps >= g.nb);
      for (int k = 0; k < g.n_rows; k++) {
        const int r = g.rows[k];
        REQUIRE(st[(size_t)r].live && (long long)g.nb * BLK <= st[(size_t)r].past && (k == 0 || r > g.rows[k - 1]));
        for (int b = 0; b < g.nb; b++) REQUIRE(p.block_at(r, b) == p.block_at(g.rows[0], b));
      }
    }
    return pl;
  }
};
static bool is(const Group& g, Ints rows, int nb) { return Ints(g.rows, g.rows + g.n_rows) == rows && g.nb == nb; }
static Plan nested(int more, bool d) {      // rows 0 (A) and 1 (B) share 2 + more blocks, row 2 (C; and 3, D) 2 of them
  Sim s;
  s.grow(0, 2 * BLK); s.fork(0, 2); if (d) s.fork(0, 3);
  s.grow(0, more * BLK); s.fork(0, 1);
  return s.plan(4);
}

int main() {
  {      // the option's threshold, G = 9, a bystander, finished / idle rows, a leftover single row
    Sim s;
    s.grow(0, 300); s.fork(0, 1); s.fork(0, 2); s.grow(3, 500);
    REQUIRE(s.plan(4).groups.size() == 1 && is(s.plan(4).groups[0], {0, 1, 2}, 2) && s.plan(4).skipped == 4);
    REQUIRE(s.plan(4, 256).groups.size() == 1 && s.plan(4, 257).groups.empty() && s.plan(4, 0).groups.empty() && s.plan(9).groups.empty() && s.plan(8).groups.size() == 1);
    s.st[1].live = false; REQUIRE(s.plan(4).groups.size() == 1 && is(s.plan(4).groups[0], {0, 2}, 2));
    s.st[2].live = false; REQUIRE(s.plan(4).groups.empty());
  }
  // nesting: A, B, C share 2 blocks.  A and B share 3: one group over 2 (skips 4 > 3).  A and B share 4: a tie, 4 == 4 -> (a), the three together.  A and B share 5:
  // {A, B} over 5, C ungrouped.  With D beside C the rows rule (b) leaves over form their own group: {A, B} over 5 + {C, D} over 2 skip 7 > 6
  REQUIRE(nested(1, false).groups.size() == 1 && is(nested(1, false).groups[0], {0, 1, 2}, 2));
  REQUIRE(nested(2, false).groups.size() == 1 && is(nested(2, false).groups[0], {0, 1, 2}, 2) && nested(2, false).skipped == 4);
  REQUIRE(nested(3, false).groups.size() == 1 && is(nested(3, false).groups[0], {0, 1}, 5) && nested(3, false).skipped == 5);
  REQUIRE(nested(3, true).groups.size() == 2 && is(nested(3, true).groups[0], {0, 1}, 5) && is(nested(3, true).groups[1], {2, 3}, 2));
  for (int G : {1, 2, 4, 7, 8}) {      // two prompts = two clusters, by their lowest row; a cluster of 32 / G + 3 rows cut in row order; 256 CUs / (2 kv heads x 3 groups) -> min(16, nb) ranges
    const int cap = 32 / G, n = cap + 3;
    Sim s;
    s.grow(0, 700);
    for (int r = 1; r < n; r++) s.fork(0, r);
    s.grow(n, 200); s.fork(n, n + 1);
    const Plan pl = s.plan(G, BLK, 2);
    REQUIRE(pl.groups.size() == 3 && pl.groups[0].n_rows == cap && pl.groups[0].rows[0] == 0 && pl.groups[0].rows[cap - 1] == cap - 1 && pl.groups[0].nb == 5 &&
            is(pl.groups[1], {cap, cap + 1, cap + 2}, 5) && pl.groups[0].nsplit == 5 && pl.groups[0].bps == 1 && is(pl.groups[2], {n, n + 1}, 1) && pl.groups[2].nsplit == 1);
  }
  {      // 32 / G + 1 rows: the leftover row is ungrouped.  Splits: 40 blocks, 8 kv heads -> 16 ranges of 3 lowered to 14; 32 kv heads x 4 groups -> 2 ranges each
    Sim s, t;
    for (int r = 0; r < 9; r++) { if (r) s.fork(0, r); else s.grow(0, 130); }
    REQUIRE(s.plan(4).groups.size() == 1 && s.plan(4).groups[0].n_rows == 8);
    t.grow(0, 40 * BLK + 5); t.fork(0, 1);
    REQUIRE(t.plan(4).groups[0].nb == 40 && t.plan(4).groups[0].bps == 3 && t.plan(4).groups[0].nsplit == 14);
    for (int r = 2; r < 8; r += 2) { t.grow(r, 9 * BLK); t.fork(r, r + 1); }
    const Plan pl = t.plan(4, BLK, 32);
    REQUIRE(pl.groups.size() == 4 && pl.groups[0].nsplit == 2 && pl.groups[0].bps == 20 && pl.groups[1].nsplit == 2 && pl.groups[1].bps == 5);
  }
  printf("prefix_groups_check: ok\n");
  return 0;
}
