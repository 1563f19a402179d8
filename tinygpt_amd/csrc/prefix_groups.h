// prefix_groups.h — the host side of the shared-prefix decode attention (option attn.shared_prefix; kernels/attn_prefix.h): which live rows of a batched step
// map the same leading blocks of the paged cache, so that those blocks are attended ONCE per group with the members' query heads side by side in the matrix
// instruction's 32 query columns.  Host-only — the standard library alone, no HIP: tests/prefix_groups_check.cpp drives it on a CPU, beside a KvPool.
//
// THE GROUPING (pinned: tests state it).  G = query heads per kv head; a group holds up to CAP = 32 / G rows (G > 8: no groups).
//   1. Finished and idle rows are never members.  The live rows that hold at least MIN = ceil(option / block) blocks are clustered by the physical id of their
//      block 0, the clusters taken by their lowest row.
//   2. A cluster S has the common run nb(S): the leading table entries that are the same physical block in every row of S (never beyond past / block of a row:
//      a shared block is full, kv_pool.h — stated here once more, so that pos >= nb * block holds for every member and its tail [nb * block, pos] is never empty).
//   3. plan(S): (a) S as it is — cut in row order into chunks of CAP rows, every chunk of two or more rows a group over ITS OWN common run, a leftover single
//      row ungrouped; or (b) S divided by the block at index nb(S): every sub-cluster of two or more rows planned by this same rule, and the rows that are left
//      (rows that end at nb(S), sub-clusters of one, the rows a sub-plan left over) chunked together as in (a).  The plan that skips more row x block reads — a
//      group of m rows over nb blocks skips (m - 1) * nb — is taken; on a tie (a), which keeps the lower row indices together.
//      A, B and C share 2 blocks, A and B share 3: (a) skips 4, (b) skips 3 -> one group of three over 2 blocks.  A and B share 5: (b) skips 5 -> {A, B} over 5.
//   4. A cluster whose common run is below MIN is divided by rule (b) alone, until the runs reach MIN or the rows run out.
//   5. Splits: every group's nb blocks are cut into nsplit = min(16, nb, max(1, CUs / (kv_heads * groups))) ranges of bps = ceil(nb / nsplit) whole blocks (nsplit then
//      lowered to the ranges that hold a block): kv_heads * sum(nsplit) workgroups are about one round of CUs, and the ranges cover [0, nb) exactly once.
// At most max_batch / 2 groups exist (every group has two rows).  The device table (table()): per row {nb, nsplit} (0, 0: ungrouped — the row's tail is its whole
// context), then per group GROUP_INTS ints {nb, nsplit, bps, n_rows, rows[32]}; unused groups are zeros (nsplit 0: their workgroups exit).
#pragma once
#include <algorithm>
#include <vector>

#include "kv_pool.h"

namespace prefix_groups {

constexpr int QCOLS = 32, GMAX = 8, MAX_SPLITS = 16, GROUP_INTS = 4 + QCOLS, ROW_INTS = 2;

struct Row { long long past = 0; bool live = false; };      // live: neither idle nor finished (ctx.h RowHost)
struct Group { int nb = 0, nsplit = 0, bps = 0, n_rows = 0; int rows[QCOLS] = {}; };
struct Plan {
  std::vector<Group> groups;
  long long skipped = 0;      // row x block reads the groups skip
};

namespace detail {
struct Ctx { const KvPool* pool; const Row* st; int cap, min_nb; };

inline int common_run(const Ctx& c, const std::vector<int>& S) {
  int lim = c.pool->row_blocks(S[0]);
  for (int r : S) lim = std::min(lim, std::min(c.pool->row_blocks(r), (int)(c.st[r].past / c.pool->block_tokens())));
  int nb = 0;
  for (; nb < lim; nb++) {
    const int b = c.pool->block_at(S[0], nb);
    bool same = true;
    for (int r : S) same = same && c.pool->block_at(r, nb) == b;
    if (!same) break;
  }
  return nb;
}
// S in row order into chunks of cap rows; groups behind `out`, single rows behind `left`
inline void chunk(const Ctx& c, const std::vector<int>& S, Plan& out, std::vector<int>& left) {
  for (size_t i = 0; i < S.size(); i += (size_t)c.cap) {
    const std::vector<int> part(S.begin() + (long)i, S.begin() + (long)std::min(S.size(), i + (size_t)c.cap));
    const int nb = part.size() >= 2 ? common_run(c, part) : 0;
    if (nb < c.min_nb) { left.insert(left.end(), part.begin(), part.end()); continue; }
    Group g;
    g.nb = nb; g.n_rows = (int)part.size();
    for (int k = 0; k < g.n_rows; k++) g.rows[k] = part[(size_t)k];
    out.groups.push_back(g);
    out.skipped += (long long)(g.n_rows - 1) * nb;
  }
}
inline void plan(const Ctx& c, const std::vector<int>& S, Plan& out, std::vector<int>& left) {
  if (S.size() < 2) { left.insert(left.end(), S.begin(), S.end()); return; }
  const int nb = common_run(c, S);
  Plan a; std::vector<int> la;
  if (nb >= c.min_nb) chunk(c, S, a, la); else la = S;
  // (b): divided by the block at index nb
  Plan b; std::vector<int> rest;
  std::vector<char> seen(S.size(), 0);
  bool divided = false;
  for (size_t i = 0; i < S.size(); i++) {
    if (seen[i]) continue;
    seen[i] = 1;
    const bool ends = c.pool->row_blocks(S[i]) <= nb || c.st[S[i]].past / c.pool->block_tokens() <= nb;
    std::vector<int> sub(1, S[i]);
    for (size_t k = i + 1; k < S.size() && !ends; k++)
      if (!seen[k] && c.pool->row_blocks(S[k]) > nb && c.pool->block_at(S[k], nb) == c.pool->block_at(S[i], nb)) { seen[k] = 1; sub.push_back(S[k]); }
    if (sub.size() >= 2 && sub.size() < S.size()) { divided = true; plan(c, sub, b, rest); }
    else rest.insert(rest.end(), sub.begin(), sub.end());
  }
  std::vector<int> lb;
  if (divided) {
    std::sort(rest.begin(), rest.end());
    if (nb >= c.min_nb) chunk(c, rest, b, lb); else lb = rest;
  }
  const bool take_b = divided && b.skipped > a.skipped;
  const Plan& p = take_b ? b : a;
  out.groups.insert(out.groups.end(), p.groups.begin(), p.groups.end());
  out.skipped += p.skipped;
  const std::vector<int>& l = take_b ? lb : la;
  left.insert(left.end(), l.begin(), l.end());
}
}   // namespace detail

// st: the state of rows [0, batch); option: attn.shared_prefix (tokens; 0 = off); G: query heads per kv head
inline Plan make(const KvPool& pool, const Row* st, int batch, int G, int option, int kv_heads, int num_cus) {
  Plan p;
  if (option <= 0 || G < 1 || G > GMAX || batch < 2) return p;
  detail::Ctx c{&pool, st, QCOLS / G, std::max(1, (option + pool.block_tokens() - 1) / pool.block_tokens())};
  std::vector<char> seen((size_t)batch, 0);
  for (int r = 0; r < batch; r++) {
    if (seen[(size_t)r] || !st[r].live || pool.row_blocks(r) < c.min_nb) continue;
    std::vector<int> S;
    for (int k = r; k < batch; k++)
      if (!seen[(size_t)k] && st[k].live && pool.row_blocks(k) >= c.min_nb && pool.block_at(k, 0) == pool.block_at(r, 0)) { seen[(size_t)k] = 1; S.push_back(k); }
    std::vector<int> left;
    detail::plan(c, S, p, left);
  }
  std::sort(p.groups.begin(), p.groups.end(), [](const Group& x, const Group& y) { return x.rows[0] < y.rows[0]; });
  const int target = std::max(1, num_cus / std::max(1, kv_heads * (int)p.groups.size()));
  for (Group& g : p.groups) {
    const int want = std::min(std::min(MAX_SPLITS, g.nb), target);
    g.bps = (g.nb + want - 1) / want;
    g.nsplit = (g.nb + g.bps - 1) / g.bps;
  }
  return p;
}

// the device table of a plan for a context of max_batch rows (header comment); always the same size
inline std::vector<int> table(const Plan& p, int max_batch) {
  std::vector<int> t((size_t)max_batch * ROW_INTS + (size_t)(max_batch / 2) * GROUP_INTS, 0);
  for (size_t gi = 0; gi < p.groups.size(); gi++) {
    const Group& g = p.groups[gi];
    int* e = t.data() + (size_t)max_batch * ROW_INTS + gi * GROUP_INTS;
    e[0] = g.nb; e[1] = g.nsplit; e[2] = g.bps; e[3] = g.n_rows;
    for (int k = 0; k < g.n_rows; k++) { e[4 + k] = g.rows[k]; t[(size_t)g.rows[k] * ROW_INTS] = g.nb; t[(size_t)g.rows[k] * ROW_INTS + 1] = g.nsplit; }
  }
  return t;
}

}   // namespace prefix_groups
