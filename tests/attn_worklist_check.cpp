// attn_worklist_check.cpp — the CPU audit of tinygpt_amd/csrc/attn_worklist.h (built and run by tests/test_attn_worklist.py under the address and undefined-behaviour
// sanitizers).  Every list the builder returns goes through one verifier against a naive model that knows nothing of the builder's partition: per (sequence, query
// block, head) it marks the key tiles the block's causal range needs and requires every one covered exactly once and none beyond; ranges on tile boundaries (they
// are tile indices: checked to be ordered and inside [0, T]); at most 32 splits per block, numbered 0 .. ns - 1 in key order; both lists heaviest first; partial
// slots distinct and inside the size the builder reports; a merge item per (split block, head) whose slot walk (slot, slot + heads, ..) meets exactly the block's
// ranges in split order.  Two parts: scripted cases — the pass of tests/test_hip_advance_rows.py's first test at targets 0 / 1 / 3, at 0 item for item the list
// ragged_tables (prefill.hip) builds, restated here — and a random run.
#include "../tinygpt_amd/csrc/attn_worklist.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

using namespace attn_worklist;

#define REQUIRE(cond)                                                                                    \
  do {                                                                                                   \
    if (!(cond)) { fprintf(stderr, "attn_worklist_check: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

// the naive model: the last key position a query block may attend, hence its tiles
static int naive_tiles(const Seq& s, int qb) {
  int last_q = qb * 128 + 127;
  if (last_q > s.len - 1) last_q = s.len - 1;
  int tiles = 0;
  for (int key = 0; key <= s.past + last_q; key += 64) tiles++;
  return tiles;
}

static void verify(const std::vector<Seq>& seq, int heads, int target, const Lists& L) {
  const int n = (int)seq.size();
  typedef std::tuple<int, int, int> Key;      // (sequence, query block, head)
  std::map<Key, std::vector<int>> cover;      // per key tile: times covered
  std::map<Key, std::vector<const Item*>> ranges;
  for (int j = 0; j < n; j++)
    for (int qb = 0; qb * 128 < seq[(size_t)j].len; qb++)
      for (int h = 0; h < heads; h++) cover[Key(j, qb, h)].assign((size_t)naive_tiles(seq[(size_t)j], qb), 0);
  auto mark = [&](const Item& it) {
    REQUIRE(it.seq >= 0 && it.seq < n && it.h >= 0 && it.h < heads && it.qblk >= 0 && it.qblk * 128 < seq[(size_t)it.seq].len);
    std::vector<int>& c = cover[Key(it.seq, it.qblk, it.h)];
    REQUIRE(it.t0 >= 0 && it.t0 < it.t1 && it.t1 <= (int)c.size());
    for (int t = it.t0; t < it.t1; t++) c[(size_t)t]++;
  };
  // whole blocks
  int prev = 1 << 30;
  for (const Item& it : L.unsplit) {
    mark(it);
    REQUIRE(it.nsplit == 1 && it.split == 0 && it.t0 == 0);
    REQUIRE(target == 0 || it.t1 <= target);
    REQUIRE(it.t1 <= prev);      // heaviest first
    prev = it.t1;
  }
  // ranges
  prev = 1 << 30;
  std::vector<int> slot_used((size_t)L.n_slots, 0);
  for (const Item& it : L.split) {
    mark(it);
    REQUIRE(target >= 1);
    REQUIRE(it.nsplit >= 2 && it.nsplit <= MAX_SPLITS && it.split >= 0 && it.split < it.nsplit);
    REQUIRE(it.nsplit == MAX_SPLITS || it.t1 - it.t0 <= target);
    REQUIRE(it.t1 - it.t0 <= prev);
    prev = it.t1 - it.t0;
    REQUIRE(it.slot >= 0 && it.slot < L.n_slots);
    REQUIRE(slot_used[(size_t)it.slot]++ == 0);
    ranges[Key(it.seq, it.qblk, it.h)].push_back(&it);
  }
  for (int u : slot_used) REQUIRE(u == 1);      // the area is exactly the ranges' records
  // every needed tile exactly once, and a block is in one list only
  for (const auto& kv : cover)
    for (int cnt : kv.second) REQUIRE(cnt == 1);
  for (const Item& it : L.unsplit) REQUIRE(ranges.count(Key(it.seq, it.qblk, it.h)) == 0);
  // merge items: one per split (block, head); its slot walk meets the block's ranges in split = key order
  REQUIRE(L.merge.size() == ranges.size());
  for (const Item& m : L.merge) {
    const auto f = ranges.find(Key(m.seq, m.qblk, m.h));
    REQUIRE(f != ranges.end());
    const std::vector<const Item*>& rs = f->second;
    REQUIRE((int)rs.size() == m.nsplit);
    int t = 0;
    for (int s = 0; s < m.nsplit; s++) {
      const Item* found = nullptr;
      for (const Item* r : rs) if (r->slot == m.slot + s * heads) found = r;
      REQUIRE(found && found->split == s && found->nsplit == m.nsplit && found->t0 == t);
      t = found->t1;
    }
    REQUIRE(t == m.t1 && t == (int)cover[Key(m.seq, m.qblk, m.h)].size());
  }
  // the counts the device block is sized by
  const Counts c = count(seq.data(), n, heads, target);
  REQUIRE(c.unsplit == (int)L.unsplit.size() && c.split == (int)L.split.size() && c.merge == (int)L.merge.size() && c.slots == L.n_slots);
}

// ragged_tables' rule (prefill.hip), restated: blocks in (sequence, block) order, stable-sorted by key tiles descending, the heads of a block consecutive
static std::vector<std::tuple<int, int, int>> ragged_rule(const std::vector<Seq>& seq, int heads) {
  std::vector<std::pair<int, int>> blocks;
  for (int j = 0; j < (int)seq.size(); j++)
    for (int qb = 0; qb < (seq[(size_t)j].len + 127) / 128; qb++) blocks.emplace_back(j, qb);
  std::stable_sort(blocks.begin(), blocks.end(), [&](const std::pair<int, int>& x, const std::pair<int, int>& y) { return naive_tiles(seq[(size_t)x.first], x.second) > naive_tiles(seq[(size_t)y.first], y.second); });
  std::vector<std::tuple<int, int, int>> out;
  for (const auto& b : blocks)
    for (int h = 0; h < heads; h++) out.emplace_back(b.first, b.second, h);
  return out;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static int rnd(int lo, int hi) {      // inclusive
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return lo + (int)(rng_state % (uint64_t)(hi - lo + 1));
}

int main() {
  // ---- scripted: the joint pass of test 1 — STEP rows first (1 position at past 63, 8 at past 200), then a FEED of 200 at past 129, a FEED_MORE of 130 from 0
  const std::vector<Seq> pass1 = {{1, 63}, {8, 200}, {200, 129}, {130, 0}};
  for (int heads : {1, 4, 32}) {
    for (int target : {0, 1, 3}) verify(pass1, heads, target, build(pass1.data(), 4, heads, target));
    const Lists L0 = build(pass1.data(), 4, heads, 0);
    const auto want = ragged_rule(pass1, heads);
    REQUIRE(L0.split.empty() && L0.merge.empty() && L0.n_slots == 0 && L0.unsplit.size() == want.size());
    for (size_t k = 0; k < want.size(); k++)
      REQUIRE(std::make_tuple(L0.unsplit[k].seq, L0.unsplit[k].qblk, L0.unsplit[k].h) == want[k]);
  }
  {      // figures by hand, one head: tiles 1 | 4 | 5, 6 | 2, 3
    const Lists L1 = build(pass1.data(), 4, 1, 1);
    REQUIRE(L1.unsplit.size() == 1 && L1.unsplit[0].seq == 0);                    // the one-tile block stays whole
    REQUIRE(L1.split.size() == 4 + 5 + 6 + 2 + 3 && L1.merge.size() == 5 && L1.n_slots == 20);
    const Lists L3 = build(pass1.data(), 4, 1, 3);
    REQUIRE(L3.unsplit.size() == 3);                                              // tiles 3 (130-token block 1), 2, 1: in that order
    REQUIRE(L3.unsplit[0].seq == 3 && L3.unsplit[0].qblk == 1 && L3.unsplit[1].seq == 3 && L3.unsplit[1].qblk == 0 && L3.unsplit[2].seq == 0);
    REQUIRE(L3.split.size() == 2 + 2 + 2 && L3.n_slots == 6);                     // 4 -> 2 + 2, 5 -> 3 + 2, 6 -> 3 + 3
    REQUIRE(L3.split[0].t1 - L3.split[0].t0 == 3 && L3.split[5].t1 - L3.split[5].t0 == 2);
  }
  {      // the cap: a one-token row over 8191 positions at target 1 has 128 tiles -> 32 ranges of 4
    const std::vector<Seq> deep = {{1, 8191}};
    const Lists L = build(deep.data(), 1, 2, 1);
    verify(deep, 2, 1, L);
    REQUIRE(L.split.size() == 64 && L.split[0].nsplit == 32 && L.split[0].t1 - L.split[0].t0 == 4);
  }
  // ---- the automatic target: nothing to gain -> 0; else the largest target that reaches `want` items
  {
    const std::vector<Seq> steps = {{1, 4095}, {1, 4095}};      // 64 tiles each, 4 heads: 8 whole items
    REQUIRE(auto_target(steps.data(), 2, 4, 8) == 0);
    const int t = auto_target(steps.data(), 2, 4, 64);          // 8 ranges per block: 8 tiles per range
    REQUIRE(t == 9);                                            // ceil(64 / 9) = 8 ranges; 10 would give 7
    const Counts c = count(steps.data(), 2, 4, t);
    REQUIRE(c.unsplit + c.split >= 64);
    const std::vector<Seq> tiny = {{3, 0}};
    REQUIRE(auto_target(tiny.data(), 1, 1, 512) == 0);          // one tile: nothing to split
  }
  // ---- random
  long long items = 0;
  for (int round = 0; round < 400; round++) {
    const int n = rnd(1, 8), heads = rnd(1, 4), target = rnd(0, 9);
    std::vector<Seq> seq((size_t)n);
    for (Seq& s : seq) { s.len = rnd(1, 600); s.past = rnd(0, 900); }
    const Lists L = build(seq.data(), n, heads, target);
    verify(seq, heads, target, L);
    items += (long long)(L.unsplit.size() + L.split.size());
    const int want = rnd(1, 200), t = auto_target(seq.data(), n, heads, want);
    REQUIRE(t >= 0);
    verify(seq, heads, t, build(seq.data(), n, heads, t));
  }
  printf("attn_worklist_check: ok (%lld items in the random run)\n", items);
  return 0;
}
