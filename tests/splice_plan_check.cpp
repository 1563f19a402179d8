// splice_plan_check.cpp — the CPU audit of tinygpt_amd/csrc/splice_plan.h and of the KvPool calls tgx_splice_row makes (built and run by tests/test_splice_plan.py
// under the address and undefined-behaviour sanitizers; never loaded into Python).  The harness holds what the device would: a content word per (physical block,
// slot), written by admissions and appends, copied by forks, and moved by a splice exactly as abi.hip moves it — copy on write with the carried identity rows, a
// gather through the OLD table into a staging vector, a scatter through the NEW one.  The naive model is a vector of token tags per row: after every operation
// every row read through its table must equal its tags (so a sibling that shares blocks is seen to keep its content), KvPool::check must pass, and the free count
// must be the one counted from the tags' side.  A refusal must leave the pool equal (KvPool::operator==) to a copy taken before.
#include "../tinygpt_amd/csrc/splice_plan.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define REQUIRE(cond)                                                                                  \
  do {                                                                                                 \
    if (!(cond)) { fprintf(stderr, "splice_plan_check: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

typedef std::vector<std::pair<long long, long long>> Ranges;      // (start, length)

struct Sim {
  KvPool p;
  int rows, blk;
  std::vector<std::vector<long long>> data;      // [physical block][slot]: the tag stored there
  std::vector<std::vector<long long>> seq;       // the naive model: every row's tags
  std::vector<long long> len;
  long long next_tag = 1;
  Sim(int max_batch, int max_ctx, int budget, int block) : rows(max_batch), blk(block) {
    p.init(max_batch, max_ctx, budget, block);
    data.assign((size_t)p.n_blocks(), std::vector<long long>((size_t)block, 0));
    seq.assign((size_t)max_batch, {}); len.assign((size_t)max_batch, 0);
  }
  int free_blocks() const { return (int)p.free_blocks(); }
  long long& at(int row, long long pos) { return data[(size_t)p.block_at(row, (int)(pos / blk))][(size_t)(pos % blk)]; }
  void audit() {
    for (int r = 0; r < rows; r++) {
      REQUIRE(len[(size_t)r] == (long long)seq[(size_t)r].size());
      REQUIRE(p.row_blocks(r) >= p.blocks_for(len[(size_t)r]));
      for (long long t = 0; t < len[(size_t)r]; t++) REQUIRE(at(r, t) == seq[(size_t)r][(size_t)t]);
    }
    const char* wrong = p.check(len);
    if (wrong) { fprintf(stderr, "splice_plan_check: KvPool::check: %s\n", wrong); exit(1); }
  }
  void append(int row, long long n) {      // positions len .. len + n - 1: a writer of the cache writes no shared block
    for (long long i = 0; i < n; i++) {
      const long long t = len[(size_t)row]++;
      REQUIRE(!p.shared(row, (int)(t / blk)));
      at(row, t) = next_tag; seq[(size_t)row].push_back(next_tag++);
    }
  }
  bool admit(int row, long long n) {
    KvPool::Changes ch;
    if (p.blocks_for(n) > p.available_for(&row, 1)) return false;
    p.release(row, ch); seq[(size_t)row].clear(); len[(size_t)row] = 0;
    REQUIRE(p.grow(row, n, ch) == KvPool::GROW_OK);
    append(row, n); audit();
    return true;
  }
  bool extend(int row, long long n) {
    KvPool::Changes ch;
    if (p.grow(row, len[(size_t)row] + n, ch) != KvPool::GROW_OK) return false;
    append(row, n); audit();
    return true;
  }
  bool fork(int src, int dst) {      // dst is empty
    KvPool::Changes ch;
    const long long past = len[(size_t)src];
    const int n_full = (int)(past / blk), tail = (int)(past % blk);
    if ((tail ? 1 : 0) > p.available_for(&dst, 1)) return false;
    p.release(dst, ch);
    p.share(src, dst, n_full, past, ch);
    if (tail) { const int b = p.fork_tail(dst, ch); for (int i = 0; i < tail; i++) data[(size_t)b][(size_t)i] = data[(size_t)p.block_at(src, n_full)][(size_t)i]; }
    seq[(size_t)dst] = seq[(size_t)src]; len[(size_t)dst] = past; audit();
    return true;
  }
  void release(int row) { KvPool::Changes ch; p.release(row, ch); seq[(size_t)row].clear(); len[(size_t)row] = 0; audit(); }
  bool truncate(int row, long long new_len) {      // tgx_truncate_row, as tests/kv_pool_check.cpp composes it
    KvPool::Changes ch;
    const int keep = p.blocks_for(new_len), tail = (int)(new_len % blk);
    if (tail && p.shared(row, keep - 1)) {
      const std::pair<int, int> of = p.unshare_tail(row, keep - 1, ch);
      if (!of.second) return false;
      for (int i = 0; i < tail; i++) data[(size_t)of.second][(size_t)i] = data[(size_t)of.first][(size_t)i];
    }
    p.trim(row, new_len, ch);
    seq[(size_t)row].resize((size_t)new_len); len[(size_t)row] = new_len; audit();
    return true;
  }
  // tgx_splice_row.  0 done, 1 the ranges are invalid, 2 no block for a copy.  fresh_out: the fresh blocks taken
  int splice(int row, const Ranges& rg, int* fresh_out = nullptr, int n_keep_override = -1) {
    const KvPool before = p;
    std::vector<int64_t> st, ln;
    for (const auto& r : rg) { st.push_back(r.first); ln.push_back(r.second); }
    splice_plan::Plan plan;
    const char* why = splice_plan::make(len[(size_t)row], n_keep_override >= 0 ? n_keep_override : (int)rg.size(), st.data(), ln.data(), &plan);
    if (why) { REQUIRE(p == before); return 1; }
    // ---- the naive side: the new tags, f, and the merged segments cover them
    const std::vector<long long> old = seq[(size_t)row];
    std::vector<long long> now;
    for (const auto& r : rg) now.insert(now.end(), old.begin() + r.first, old.begin() + r.first + r.second);
    REQUIRE(plan.new_len == (long long)now.size());
    long long f = 0;
    while (f < plan.new_len && now[(size_t)f] == old[(size_t)f]) f++;
    REQUIRE(plan.f == f);
    long long covered = 0, last_delta = -1;
    for (int i = 0; i < plan.n_seg; i++) {
      const splice_plan::Seg& s = plan.seg[i];
      REQUIRE(s.dst == covered && s.len >= 1 && s.src - s.dst > last_delta);      // deltas strictly increasing: touching ranges were merged
      last_delta = s.src - s.dst; covered += s.len;
      REQUIRE((i < plan.first_moved) == (s.src == s.dst));
    }
    REQUIRE(covered == plan.new_len);
    for (long long d = 0; d < plan.new_len; d++) REQUIRE(old[(size_t)splice_plan::source_of(plan, d)] == now[(size_t)d]);
    REQUIRE(plan.truncation() == (plan.f == plan.new_len));
    // ---- blocks
    const splice_plan::Blocks b = splice_plan::blocks(p, row, plan);
    REQUIRE(b.first == (int)(f / blk) && b.end == p.blocks_for(plan.new_len));
    int shared_written = 0;
    for (int i = b.first; i < b.end; i++) shared_written += p.shared(row, i);
    REQUIRE((int)b.fresh.size() == shared_written);
    REQUIRE(b.carry == (shared_written && p.shared(row, b.first) ? (int)(f % blk) : 0));
    if (b.fresh.size() > p.free_blocks()) { REQUIRE(p == before); return 2; }
    const int free0 = free_blocks();
    int dropped_own = 0;
    for (int i = b.end; i < p.row_blocks(row); i++) dropped_own += !p.shared(row, i);
    // gather through the old table
    std::vector<long long> stage;
    for (int i = plan.first_moved; i < plan.n_seg; i++)
      for (long long k = 0; k < plan.seg[i].len; k++) stage.push_back(at(row, plan.seg[i].src + k));
    REQUIRE((long long)stage.size() == plan.moved() || plan.truncation());
    KvPool::Changes ch;
    for (size_t i = 0; i < b.fresh.size(); i++) {
      const std::pair<int, int> of = p.unshare(row, b.fresh[i], ch);
      REQUIRE(p.sharers(of.second) == 1 && p.block_at(row, b.fresh[i]) == of.second);
      if (i == 0) for (int k = 0; k < b.carry; k++) data[(size_t)of.second][(size_t)k] = data[(size_t)of.first][(size_t)k];
    }
    p.trim(row, plan.new_len, ch);
    // scatter through the new table: every block it writes is the row's alone
    size_t m = 0;
    for (int i = plan.first_moved; i < plan.n_seg; i++)
      for (long long k = 0; k < plan.seg[i].len; k++) {
        const long long d = plan.seg[i].dst + k;
        REQUIRE(!p.shared(row, (int)(d / blk)) && (int)(d / blk) >= b.first && (int)(d / blk) < b.end);
        at(row, d) = stage[m++];
      }
    seq[(size_t)row] = now; len[(size_t)row] = plan.new_len;
    REQUIRE(free_blocks() == free0 - (int)b.fresh.size() + dropped_own);
    if (fresh_out) *fresh_out = (int)b.fresh.size();
    audit();
    return 0;
  }
};

static void scripted() {
  const int B = 128;
  struct Shape { long long past; Ranges keep; };
  const Shape shapes[] = {
      {100, {{0, 10}, {30, 70}}},  {200, {{0, 5}, {6, 194}}},  {384, {{0, 128}, {256, 128}}}, {300, {{0, 4}, {50, 10}, {61, 129}, {250, 50}}},
      {140, {{7, 133}}},           {512, {{0, 4}, {260, 252}}}, {200, {{0, 77}}},              {200, {{0, 200}}},
  };
  for (const Shape& s : shapes)
    for (int forked = 0; forked < 2; forked++) {      // alone, and with a sibling that shares the row's full blocks
      Sim h(3, 512, 16 * B, B);
      REQUIRE(h.admit(0, s.past));
      if (forked) REQUIRE(h.fork(0, 1));
      long long kept = 0;
      for (const auto& r : s.keep) kept += r.second;
      REQUIRE(h.splice(0, s.keep) == 0 && h.len[0] == kept);
      REQUIRE(h.p.row_blocks(0) == h.p.blocks_for(kept));
      if (forked) REQUIRE(h.len[1] == s.past);
      REQUIRE(h.extend(0, 3));      // the next append lands in a block of the row's own (Sim::append requires it)
    }
  {      // touching ranges are one segment; the split form moves what the merged form moves
    splice_plan::Plan a, b;
    const int64_t s3[3] = {0, 10, 40}, l3[3] = {10, 10, 60}, s2[2] = {0, 40}, l2[2] = {20, 60};
    REQUIRE(!splice_plan::make(100, 3, s3, l3, &a) && !splice_plan::make(100, 2, s2, l2, &b));
    REQUIRE(a.n_seg == 2 && b.n_seg == 2 && a.f == 20 && a.new_len == 80 && a.first_moved == 1);
    for (int i = 0; i < 2; i++) REQUIRE(a.seg[i].src == b.seg[i].src && a.seg[i].dst == b.seg[i].dst && a.seg[i].len == b.seg[i].len);
    const int64_t s1[2] = {0, 50}, l1[2] = {50, 50};      // the whole row in two touching pieces: the no-op form
    REQUIRE(!splice_plan::make(100, 2, s1, l1, &a) && a.truncation() && a.new_len == 100 && a.moved() == 0);
  }
  {      // every refusal: the pool stays equal to its copy (Sim::splice compares)
    Sim h(2, 512, 8 * B, B);
    REQUIRE(h.admit(0, 200));
    REQUIRE(h.splice(0, {}) == 1);                                   // n_keep 0
    REQUIRE(h.splice(0, Ranges(17, {0, 1})) == 1);                   // n_keep 17
    REQUIRE(h.splice(0, {{0, 0}}) == 1);                             // empty
    REQUIRE(h.splice(0, {{10, 5}, {3, 2}}) == 1);                    // unsorted
    REQUIRE(h.splice(0, {{0, 10}, {9, 5}}) == 1);                    // overlapping
    REQUIRE(h.splice(0, {{0, 201}}) == 1 && h.splice(0, {{200, 1}}) == 1 && h.splice(0, {{-1, 5}}) == 1 && h.splice(0, {{199, 2}}) == 1);      // outside [0, past)
    REQUIRE(h.splice(0, {{0, (long long)1 << 62}}) == 1);
    splice_plan::Plan pl; const int64_t one = 1;
    REQUIRE(splice_plan::make(200, 1, nullptr, &one, &pl) && splice_plan::make(200, 1, &one, nullptr, &pl));
    REQUIRE(h.len[0] == 200);
    // the truncation and no-op forms leave the pool tgx_truncate_row leaves
    Sim t(2, 512, 8 * B, B), u(2, 512, 8 * B, B);
    REQUIRE(t.admit(0, 300) && u.admit(0, 300) && t.fork(0, 1) && u.fork(0, 1));
    int fresh = -1;
    REQUIRE(t.splice(1, {{0, 200}}, &fresh) == 0 && fresh == 1 && u.truncate(1, 200) && t.p == u.p);      // inside a shared block: one copy, rows [128, 200) carried
    REQUIRE(t.splice(0, {{0, 300}}, &fresh) == 0 && fresh == 0 && t.p == u.p);                            // the whole row: nothing
    REQUIRE(t.splice(0, {{0, 256}}, &fresh) == 0 && fresh == 0 && u.truncate(0, 256) && t.p == u.p);      // a block boundary: no copy
  }
  {      // fork, then splice with f inside a shared block: exactly one fresh block, and none left for it is a refusal that changes nothing
    Sim h(2, 512, 5 * B, B);
    REQUIRE(h.admit(0, 300) && h.fork(0, 1) && h.free_blocks() == 1);
    int fresh = -1;
    REQUIRE(h.splice(1, {{0, 150}, {160, 100}}, &fresh) == 0 && fresh == 1 && h.free_blocks() == 1);      // one taken, the tail block of 300 given back
    Sim e(2, 512, 4 * B, B);
    REQUIRE(e.admit(0, 300) && e.fork(0, 1) && e.free_blocks() == 0);
    REQUIRE(e.splice(1, {{0, 150}, {160, 100}}) == 2 && e.len[1] == 300);      // the tail block it would give back is not counted: the free list alone
    REQUIRE(e.splice(1, {{0, 256}, {260, 40}}) == 0 && e.free_blocks() == 0);   // f on the boundary: only the row's own tail block is written
    Sim g(2, 512, 6 * B, B);      // f = 0: both shared blocks are written, two fresh ones
    REQUIRE(g.admit(0, 300) && g.fork(0, 1) && g.free_blocks() == 2);
    REQUIRE(g.splice(1, {{7, 293}}, &fresh) == 0 && fresh == 2 && g.free_blocks() == 0);
  }
}

static uint64_t rng_state;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static long done, done_cow, refused_ranges, refused_blocks;

static void random_run(uint64_t seed, int n_ops) {
  const int ROWS = 5, CTX = 64, BLK = 4, BUDGET = 120;
  rng_state = seed;
  Sim h(ROWS, CTX, BUDGET, BLK);
  for (int op = 0; op < n_ops; op++) {
    const int dice = rnd_in(0, 99), row = rnd_in(0, ROWS - 1);
    std::vector<int> live, empty;
    for (int r = 0; r < ROWS; r++) (h.len[(size_t)r] ? live : empty).push_back(r);
    if (dice < 15) (void)h.admit(row, rnd_in(1, 48));
    else if (dice < 30) { if (!live.empty()) { const int r = live[(size_t)rnd_in(0, (int)live.size() - 1)]; if (h.len[(size_t)r] < CTX) (void)h.extend(r, rnd_in(1, std::min(12, CTX - (int)h.len[(size_t)r]))); } }
    else if (dice < 48) { if (!live.empty() && !empty.empty()) (void)h.fork(live[(size_t)rnd_in(0, (int)live.size() - 1)], empty[0]); }
    else if (dice < 55) h.release(row);
    else {
      if (live.empty()) continue;
      const int r = live[(size_t)rnd_in(0, (int)live.size() - 1)];
      const long long past = h.len[(size_t)r];
      Ranges rg;
      const bool broken = dice >= 95;
      long long at = rnd_in(0, 3) ? 0 : rnd_in(0, (int)past - 1);
      for (int i = 0, n = rnd_in(1, 5); i < n && at < past; i++) {
        const long long l = rnd_in(1, (int)std::min<long long>(past - at, 20));
        rg.emplace_back(at, l);
        at += l + (rnd_in(0, 3) ? rnd_in(1, 9) : 0);      // a gap, or a touching range
      }
      if (broken) { if (rnd_in(0, 1)) rg.back().second += past; else rg.emplace_back(rg[0]); }      // beyond the row, or unsorted / overlapping
      int fresh = 0;
      const int rc = h.splice(r, rg, &fresh);
      REQUIRE((rc == 1) == broken);
      if (rc == 0) { done++; done_cow += fresh > 0; } else if (rc == 1) refused_ranges++; else refused_blocks++;
      h.audit();
    }
  }
}

int main() {
  scripted();
  const uint64_t seeds[8] = {1, 2, 3, 5, 8, 13, 21, 34};
  for (uint64_t s : seeds) random_run(s, 4000);
  printf("splices done %ld (%ld with a copy on write), refused: ranges %ld, no free block %ld\n", done, done_cow, refused_ranges, refused_blocks);
  if (done < 1000 || done_cow < 100 || refused_ranges < 100 || refused_blocks < 20) { fprintf(stderr, "splice_plan_check: the random run was vacuous\n"); return 1; }
  printf("splice_plan_check: ok\n");
  return 0;
}
