// kv_pool_check.cpp — the CPU audit of tinygpt_amd/csrc/kv_pool.h (built and run by tests/test_kv_pool.py under the address and undefined-behaviour sanitizers).
// Every operation goes through a harness that (1) applies the change list the pool returned to a shadow "device table" and requires the shadow to equal the
// pool's own mirror — the property the device push of abi.hip relies on — and (2) calls KvPool::check() with the rows' lengths.  Two parts: scripted cases on
// 128-token blocks (the figures of tests/test_hip_fork_row.py::test_block_accounting, and the states the entry points cannot reach), and a random run on 4-token
// blocks against a naive model (per row a plain list of block ids, counts recomputed from scratch) that decides whether an operation fits.
#include "../tinygpt_amd/csrc/kv_pool.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define REQUIRE(cond)                                                                              \
  do {                                                                                             \
    if (!(cond)) { fprintf(stderr, "kv_pool_check: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

struct Harness {
  KvPool p;
  std::vector<int> dev;                 // the shadow device table
  std::vector<long long> len;           // every row's length, as the library's row state would hold it
  KvPool::Changes ch;
  int rows = 0, blk = 0;

  Harness(int max_batch, int max_ctx, int budget_tokens, int block_tokens) : rows(max_batch), blk(block_tokens) {
    p.init(max_batch, max_ctx, budget_tokens, block_tokens);
    dev.assign((size_t)max_batch * p.tbl_stride(), 0);
    len.assign((size_t)max_batch, 0);
    audit();
  }
  int free_blocks() const { return (int)p.free_blocks(); }
  void audit() {      // push the pending changes, then: shadow == mirror, and the pool's own audit
    for (const auto& c : ch) { REQUIRE(c.first >= 0 && (size_t)c.first < dev.size()); dev[(size_t)c.first] = c.second; }
    ch.clear();
    for (int r = 0; r < rows; r++)
      for (int i = 0; i < p.tbl_stride(); i++) REQUIRE(dev[(size_t)r * p.tbl_stride() + i] == p.block_at(r, i));
    const char* wrong = p.check(len);
    if (wrong) { fprintf(stderr, "kv_pool_check: KvPool::check: %s\n", wrong); exit(1); }
  }
  // ---- the operations, composed as abi.hip composes them.  Each returns whether the pool accepted; a refusal must leave the pool bit-identical
  bool refused(const KvPool& before) { REQUIRE(p == before); REQUIRE(ch.empty()); audit(); return false; }
  KvPool::Grow grow(int row, long long tokens) {      // kv_ensure_blocks
    const KvPool before = p;
    const KvPool::Grow g = p.grow(row, tokens, ch);
    if (g != KvPool::GROW_OK) { refused(before); return g; }
    len[(size_t)row] = std::max(len[(size_t)row], tokens);
    audit();
    return g;
  }
  bool admit(int n, const int* r, const int* lens) {      // admit_rows: all or nothing, then release + grow
    const KvPool before = p;
    long long need = 0;
    for (int i = 0; i < n; i++) need += p.blocks_for(lens[i]);
    if (need > p.available_for(r, n)) return refused(before);
    for (int i = 0; i < n; i++) { p.release(r[i], ch); len[(size_t)r[i]] = 0; audit(); }
    for (int i = 0; i < n; i++) REQUIRE(grow(r[i], lens[i]) == KvPool::GROW_OK);
    return true;
  }
  bool fork(int src, int n, const int* dst) {      // tgx_fork_row: ONE change list for all destinations
    const KvPool before = p;
    const long long past = len[(size_t)src];
    const int n_full = (int)(past / blk), tail = (int)(past % blk);
    if ((tail ? n : 0) > p.available_for(dst, n)) return refused(before);
    for (int i = 0; i < n; i++) { p.release(dst[i], ch); len[(size_t)dst[i]] = 0; audit(); }
    for (int i = 0; i < n; i++) {
      p.share(src, dst[i], n_full, past, ch);
      if (tail) { const int b = p.fork_tail(dst[i], ch); REQUIRE(b >= 1 && p.sharers(b) == 1 && p.block_at(dst[i], n_full) == b); }
      len[(size_t)dst[i]] = past;
    }
    audit();
    return true;
  }
  bool extend(int row, int more) {      // tgx_extend_row
    const KvPool before = p;
    const long long tokens = len[(size_t)row] + more;
    if (p.blocks_for(tokens) - p.row_blocks(row) > p.available_for(nullptr, 0)) return refused(before);
    REQUIRE(grow(row, tokens) == KvPool::GROW_OK);
    return true;
  }
  bool truncate(int row, long long new_len, bool* copied = nullptr) {      // tgx_truncate_row
    const KvPool before = p;
    const int keep = p.blocks_for(new_len), tail = (int)(new_len % blk);
    if (copied) *copied = false;
    if (tail && p.shared(row, keep - 1)) {
      const int old = p.block_at(row, keep - 1), was = p.sharers(old);
      const std::pair<int, int> of = p.unshare_tail(row, keep - 1, ch);
      REQUIRE(of.first == old);
      if (!of.second) return refused(before);
      REQUIRE(p.block_at(row, keep - 1) == of.second && p.sharers(of.second) == 1 && p.sharers(old) == was - 1);
      if (copied) *copied = true;
    }
    p.trim(row, new_len, ch);
    len[(size_t)row] = new_len;
    audit();
    return true;
  }
  void release(int row) { p.release(row, ch); len[(size_t)row] = 0; audit(); }
};

static void scripted() {
  const int B = 128;
  {      // ---- test_block_accounting, budget 16 blocks
    Harness h(4, 512, 16 * B, B);
    REQUIRE(h.free_blocks() == 16 && h.p.n_blocks() == 17 && h.p.tbl_stride() == 4);
    REQUIRE(h.grow(0, 300) == KvPool::GROW_OK && h.free_blocks() == 13);
    REQUIRE(h.p.block_at(0, 0) == 1 && h.p.block_at(0, 1) == 2 && h.p.block_at(0, 2) == 3);      // the free list hands out 1, 2, 3, ...
    const int d[3] = {1, 2, 3};
    REQUIRE(h.fork(0, 3, d) && h.free_blocks() == 10);
    REQUIRE(h.p.block_at(1, 2) == 4 && h.p.block_at(2, 2) == 5 && h.p.block_at(3, 2) == 6 && h.p.sharers(1) == 4 && h.p.sharers(2) == 4);
    h.release(0); REQUIRE(h.free_blocks() == 11);
    h.release(2); REQUIRE(h.free_blocks() == 12);
    h.release(1); REQUIRE(h.free_blocks() == 13);
    h.release(3); REQUIRE(h.free_blocks() == 16);      // the last one gives back the two shared blocks as well
    REQUIRE(h.grow(0, 256) == KvPool::GROW_OK && h.free_blocks() == 14);
    REQUIRE(h.fork(0, 3, d) && h.free_blocks() == 14);      // no tail: a fork for nothing
    for (int r = 0; r < 4; r++) REQUIRE(h.grow(r, 257) == KvPool::GROW_OK);      // position 256 of every row into a block of its own
    REQUIRE(h.free_blocks() == 10);
    for (int r = 0; r < 4; r++) REQUIRE(!h.p.shared(r, 2) && h.p.shared(r, 0) && h.p.shared(r, 1));
  }
  {      // ---- budget 10 blocks
    Harness h(4, 512, 10 * B, B);
    for (int r = 0; r < 3; r++) REQUIRE(h.grow(r, 380) == KvPool::GROW_OK);
    REQUIRE(h.free_blocks() == 1 && h.grow(3, 380) == KvPool::GROW_EXHAUSTED && h.free_blocks() == 1);      // (Harness::grow compared the pool with its snapshot)
    const int r3 = 3, l3 = 380;
    REQUIRE(!h.admit(1, &r3, &l3));
    Harness g(4, 512, 10 * B, B);
    const int d[3] = {1, 2, 3};
    REQUIRE(g.grow(0, 380) == KvPool::GROW_OK && g.fork(0, 3, d) && g.free_blocks() == 4);
    for (int r = 0; r < 4; r++) REQUIRE(g.grow(r, 388) == KvPool::GROW_OK);      // 380 -> 388: a fourth block per row
    REQUIRE(g.free_blocks() == 0);
  }
  {      // ---- the state the entry points cannot reach: a target row that still holds blocks, some of them shared with a sibling
    Harness h(4, 1024, 8 * B, B);
    const int d1 = 1;
    REQUIRE(h.grow(0, 300) == KvPool::GROW_OK && h.fork(0, 1, &d1) && h.free_blocks() == 4);      // row 1: two shared blocks and a tail of its own
    REQUIRE(h.p.given_back(1) == 1 && h.p.given_back(0) == 1 && h.p.row_blocks(1) == 3);
    REQUIRE(h.p.available_for(&d1, 1) == 5);
    const int six = 6 * B, seven = 7 * B, five = 5 * B;
    REQUIRE(!h.admit(1, &d1, &seven));      // 7 blocks: only releasing the shared ones as well (4 + 3) would satisfy it
    REQUIRE(!h.admit(1, &d1, &six));
    REQUIRE(h.admit(1, &d1, &five) && h.free_blocks() == 0);      // fits exactly
    REQUIRE(h.p.sharers(1) == 1 && h.p.sharers(2) == 1 && h.p.row_blocks(0) == 3);      // row 0 kept its blocks, now its own
    // the same sum guards a fork whose destination holds blocks: rows 0 -> 2 (tail 44 of 300), 2 retired is what a fork into {2} gives back
    Harness f(4, 1024, 4 * B, B);
    const int d2 = 2, d3 = 3;
    REQUIRE(f.grow(0, 300) == KvPool::GROW_OK && f.fork(0, 1, &d2) && f.free_blocks() == 0);
    REQUIRE(!f.fork(0, 1, &d3));            // no free block and row 3 gives nothing back
    REQUIRE(f.fork(0, 1, &d2) && f.free_blocks() == 0);      // row 2 gives its own tail block back: exactly the one the new tail needs
  }
  {      // ---- truncation
    Harness h(4, 1024, 6 * B, B);
    const int d1 = 1;
    REQUIRE(h.grow(0, 600) == KvPool::GROW_OK && h.free_blocks() == 1);      // 5 blocks
    bool copied = true;
    REQUIRE(h.truncate(0, 384, &copied) && !copied && h.p.row_blocks(0) == 3 && h.free_blocks() == 3);      // to a block boundary: the trailing blocks dropped
    REQUIRE(h.truncate(0, 300, &copied) && !copied && h.free_blocks() == 3);                                // into an unshared block: no copy
    REQUIRE(h.fork(0, 1, &d1) && h.free_blocks() == 2);      // rows 0 and 1 share blocks 0, 1
    const int old = h.p.block_at(1, 1);
    REQUIRE(h.truncate(1, 200, &copied) && copied && h.free_blocks() == 2);      // into a shared block: a fresh one taken, row 1's tail block given back
    REQUIRE(h.p.block_at(0, 1) == old && h.p.block_at(1, 1) != old && h.p.sharers(old) == 1 && h.p.row_blocks(1) == 2);
    // with an empty free list
    Harness e(4, 1024, 4 * B, B);
    REQUIRE(e.grow(0, 300) == KvPool::GROW_OK && e.fork(0, 1, &d1) && e.free_blocks() == 0);
    REQUIRE(!e.truncate(1, 200) && e.p.row_blocks(1) == 3 && e.len[1] == 300);      // refused, nothing changed (Harness::refused compared the snapshot)
    REQUIRE(e.truncate(1, 256, &copied) && !copied && e.free_blocks() == 1);        // to the boundary needs no block
  }
  {      // ---- beyond the table
    Harness h(2, 512, 16 * B, B);
    REQUIRE(h.grow(0, 512) == KvPool::GROW_OK && h.grow(0, 513) == KvPool::GROW_BEYOND_TABLE && h.p.row_blocks(0) == 4 && h.free_blocks() == 12);
    REQUIRE(h.grow(1, 9999) == KvPool::GROW_BEYOND_TABLE && h.p.row_blocks(1) == 0);
  }
}

// ---- the random run
static uint64_t rng_state;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }      // [lo, hi]

enum Kind { ADMIT, GROW, FORK, EXTEND, TRUNCATE, TRUNCATE_COPY, RELEASE, N_KINDS };
static const char* kind_name[N_KINDS] = {"admit", "grow", "fork", "extend", "truncate", "truncate+copy", "release"};
static long accepted[N_KINDS], exhausted[N_KINDS], beyond[N_KINDS];

struct Model {      // naive: per row a plain list of block ids; counts and the free count recomputed from scratch on every question
  int rows, blk, stride, total;
  std::vector<std::vector<int>> blocks;
  std::vector<long long> len;
  int count(int b) const { int n = 0; for (const auto& r : blocks) n += (int)std::count(r.begin(), r.end(), b); return n; }
  int free_blocks() const {
    std::vector<int> all;
    for (const auto& r : blocks) all.insert(all.end(), r.begin(), r.end());
    std::sort(all.begin(), all.end());
    return total - (int)(std::unique(all.begin(), all.end()) - all.begin());
  }
  int given_back(int row) const { int n = 0; for (int b : blocks[(size_t)row]) n += count(b) == 1; return n; }
  int blocks_for(long long tokens) const { return (int)((tokens + blk - 1) / blk); }
};

// after an accepted operation: the rows' block counts, the free count and — entry by entry — the table must be the model's.  Blocks the model calls fresh
// (id -1) are read from the pool and must have been unused in the model
static void reconcile(Model& m, Harness& h) {
  for (int r = 0; r < m.rows; r++) {
    REQUIRE(h.p.row_blocks(r) == (int)m.blocks[(size_t)r].size());
    for (size_t i = 0; i < m.blocks[(size_t)r].size(); i++) {
      int& b = m.blocks[(size_t)r][i];
      if (b == -1) { const int got = h.p.block_at(r, (int)i); REQUIRE(got >= 1 && m.count(got) == 0); b = got; }
      REQUIRE(h.p.block_at(r, (int)i) == b);
    }
    REQUIRE(h.len[(size_t)r] == m.len[(size_t)r]);
  }
  REQUIRE(h.free_blocks() == m.free_blocks());
}

static void random_run(uint64_t seed, int n_ops) {
  const int ROWS = 6, CTX = 64, BLK = 4, BUDGET = 152;      // 38 blocks: ~40 % of ROWS * CTX tokens
  rng_state = seed;
  Harness h(ROWS, CTX, BUDGET, BLK);
  Model m{ROWS, BLK, CTX / BLK, BUDGET / BLK, std::vector<std::vector<int>>(ROWS), std::vector<long long>(ROWS, 0)};
  for (int op = 0; op < n_ops; op++) {
    const int dice = rnd_in(0, 99), row = rnd_in(0, ROWS - 1);
    std::vector<int> live, empty;
    for (int r = 0; r < ROWS; r++) (m.len[(size_t)r] ? live : empty).push_back(r);
    if (dice < 22) {      // ---- admit one or two prompts into any rows, whatever they hold
      int r[2] = {row, (row + rnd_in(1, ROWS - 1)) % ROWS}, lens[2] = {rnd_in(1, 40), rnd_in(1, 40)};
      const int n = rnd_in(1, 2);
      int need = 0, have = m.free_blocks();
      for (int i = 0; i < n; i++) { need += m.blocks_for(lens[i]); have += m.given_back(r[i]); }
      const bool fits = need <= have;
      (fits ? accepted : exhausted)[ADMIT]++;
      REQUIRE(h.admit(n, r, lens) == fits);
      if (fits) for (int i = 0; i < n; i++) { m.blocks[(size_t)r[i]].assign((size_t)m.blocks_for(lens[i]), -1); m.len[(size_t)r[i]] = lens[i]; }
      // (the blocks of r[0] must be reconciled as fresh before those of r[1]: both lists are -1 now and count() never sees a -1 as in use)
    } else if (dice < 50 || dice >= 90) {      // ---- decode-grow by 1..8, or extend by 1..24 within the context
      if (live.empty()) continue;
      const int r = live[(size_t)rnd_in(0, (int)live.size() - 1)];
      const bool ext = dice >= 90;
      if (ext && m.len[(size_t)r] == CTX) continue;
      const long long tokens = m.len[(size_t)r] + (ext ? rnd_in(1, std::min(24, CTX - (int)m.len[(size_t)r])) : rnd_in(1, 8));
      const int need = m.blocks_for(tokens) - (int)m.blocks[(size_t)r].size(), k = ext ? EXTEND : GROW;
      const KvPool::Grow want = need <= 0 ? KvPool::GROW_OK : m.blocks_for(tokens) > m.stride ? KvPool::GROW_BEYOND_TABLE : need > m.free_blocks() ? KvPool::GROW_EXHAUSTED : KvPool::GROW_OK;
      (want == KvPool::GROW_OK ? accepted : want == KvPool::GROW_EXHAUSTED ? exhausted : beyond)[k]++;
      if (ext) REQUIRE(h.extend(r, (int)(tokens - m.len[(size_t)r])) == (want == KvPool::GROW_OK));
      else REQUIRE(h.grow(r, tokens) == want);
      if (want == KvPool::GROW_OK) { m.blocks[(size_t)r].resize((size_t)m.blocks_for(tokens), -1); m.len[(size_t)r] = tokens; }
    } else if (dice < 62) {      // ---- fork a live row into 1..3 empty rows
      if (live.empty() || empty.empty()) continue;
      const int src = live[(size_t)rnd_in(0, (int)live.size() - 1)], n = std::min((int)empty.size(), rnd_in(1, 3));
      const long long past = m.len[(size_t)src];
      const int n_full = (int)(past / BLK), tail = (int)(past % BLK);
      const bool fits = (tail ? n : 0) <= m.free_blocks();
      (fits ? accepted : exhausted)[FORK]++;
      REQUIRE(h.fork(src, n, empty.data()) == fits);
      if (fits) for (int i = 0; i < n; i++) {
        std::vector<int>& d = m.blocks[(size_t)empty[(size_t)i]];
        d.assign(m.blocks[(size_t)src].begin(), m.blocks[(size_t)src].begin() + n_full);
        if (tail) d.push_back(-1);
        m.len[(size_t)empty[(size_t)i]] = past;
      }
    } else if (dice < 80) {      // ---- truncate; half of the time aimed inside a block the row shares, where it has one
      if (live.empty()) continue;
      const int r = live[(size_t)rnd_in(0, (int)live.size() - 1)];
      long long new_len = rnd_in(1, (int)m.len[(size_t)r]);
      std::vector<int> sh;
      for (size_t i = 0; i < m.blocks[(size_t)r].size(); i++) if (m.count(m.blocks[(size_t)r][i]) > 1) sh.push_back((int)i);
      if (!sh.empty() && rnd_in(0, 1)) new_len = (long long)sh[(size_t)rnd_in(0, (int)sh.size() - 1)] * BLK + rnd_in(1, BLK - 1);
      const int keep = m.blocks_for(new_len);
      const bool copy = new_len % BLK && m.count(m.blocks[(size_t)r][(size_t)keep - 1]) > 1, fits = !copy || m.free_blocks() > 0;
      (fits ? accepted : exhausted)[copy ? TRUNCATE_COPY : TRUNCATE]++;
      bool copied = false;
      REQUIRE(h.truncate(r, new_len, &copied) == fits && (!fits || copied == copy));
      if (fits) { m.blocks[(size_t)r].resize((size_t)keep); if (copy) m.blocks[(size_t)r].back() = -1; m.len[(size_t)r] = new_len; }
    } else {      // ---- release (a retired row releases nothing)
      accepted[RELEASE]++;
      h.release(row);
      m.blocks[(size_t)row].clear(); m.len[(size_t)row] = 0;
    }
    reconcile(m, h);
  }
}

int main() {
  scripted();
  const uint64_t seeds[8] = {1, 2, 3, 5, 8, 13, 21, 34};
  for (uint64_t s : seeds) random_run(s, 4000);
  bool enough = true;
  for (int k = 0; k < N_KINDS; k++) {
    printf("%-14s accepted %6ld   refused: exhausted %5ld, beyond the table %4ld\n", kind_name[k], accepted[k], exhausted[k], beyond[k]);
    enough = enough && accepted[k] >= 100 && (k == TRUNCATE || k == RELEASE || exhausted[k] >= 20);
  }
  if (!enough) { fprintf(stderr, "kv_pool_check: the random run was vacuous (every kind 100 times accepted, every budget-consuming kind 20 times exhausted)\n"); return 1; }
  printf("kv_pool_check: ok\n");
  return 0;
}
