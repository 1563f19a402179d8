// attn_worklist.h — the work list of the mixed attention (tgx_advance_rows; kernels/attn_mixed.h): the sequences of a ragged pass, each S_i new positions from its
// own past_i, cut into work items (sequence, query block, head, key-tile range).  Host-only — the standard library alone, no HIP: prefill.hip lays the lists out
// for the device, tests/attn_worklist_check.cpp drives the builder on a CPU.
//
// Blocking: the prompt attention's (kernels/prefill.h ATTN_QBLK / ATTN_KTILE — restated here, prefill.hip static_asserts the two agree): a query block is 128
// queries of one head, keys travel in tiles of 64.  Query block qb of a sequence needs the key tiles [0, T), T = (past + min(128 qb + 127, S - 1)) / 64 + 1 (causal:
// nothing behind its last query's position).
//   target 0      never split: one item per (block, head) over [0, T) — exactly ragged_tables' list (prefill.hip) in its order, blocks by T descending, ties in
//                 (sequence, block) order, the heads of a block consecutive
//   target N >= 1 a block with T > N is cut at tile boundaries into ns = min(32, ceil(T / N)) contiguous ranges, the first T % ns one tile longer (attn_extend.h's
//                 partition); a block with T <= N stays whole.  (At the cap of 32 a range holds more than N tiles: the merge walks at most 32 partials.)
// Three lists: `unsplit` (whole blocks: the work-list kernel's items), `split` (one item per (block, range, head), heaviest range first, ties in block / range /
// head order) and `merge` (one item per (split block, head)).  Partial slots: a split block of ns ranges owns ns x heads consecutive slots from its base;
// range s of head h writes slot base + s * heads + h, the merge item of head h reads base + h + s * heads for s = 0 .. ns - 1 in that order.
#pragma once
#include <algorithm>
#include <vector>

namespace attn_worklist {

constexpr int QBLK = 128, KTILE = 64, MAX_SPLITS = 32;

struct Seq { int len, past; };                                        // S_i >= 1 new positions behind past_i >= 0 held ones
struct Item { int seq, qblk, h, t0, t1, split, nsplit, slot; };       // key tiles [t0, t1); merge items: split 0, t0 = 0, t1 = T, slot = base + h

struct Lists {
  std::vector<Item> unsplit, split, merge;
  int n_slots = 0;                                                    // the partial area holds n_slots records
};

inline int block_tiles(const Seq& s, int qb) { return (s.past + std::min(qb * QBLK + QBLK - 1, s.len - 1)) / KTILE + 1; }
inline int block_splits(int tiles, int target) { return target < 1 || tiles <= target ? 1 : std::min(MAX_SPLITS, (tiles + target - 1) / target); }

// the counts alone (the device block's size, the automatic target's search)
struct Counts { int unsplit = 0, split = 0, merge = 0, slots = 0; };
inline Counts count(const Seq* seq, int n, int heads, int target) {
  Counts c;
  for (int j = 0; j < n; j++)
    for (int qb = 0; qb < (seq[j].len + QBLK - 1) / QBLK; qb++) {
      const int ns = block_splits(block_tiles(seq[j], qb), target);
      if (ns == 1) c.unsplit += heads;
      else { c.split += ns * heads; c.merge += heads; c.slots += ns * heads; }
    }
  return c;
}

inline Lists build(const Seq* seq, int n, int heads, int target) {
  Lists L;
  struct Block { int seq, qb, tiles, ns, base; };
  std::vector<Block> blocks;
  for (int j = 0; j < n; j++)
    for (int qb = 0; qb < (seq[j].len + QBLK - 1) / QBLK; qb++) {
      Block b{j, qb, block_tiles(seq[j], qb), 1, 0};
      b.ns = block_splits(b.tiles, target);
      if (b.ns > 1) { b.base = L.n_slots; L.n_slots += b.ns * heads; }
      blocks.push_back(b);
    }
  // whole blocks, heaviest first
  std::vector<const Block*> whole;
  for (const Block& b : blocks) if (b.ns == 1) whole.push_back(&b);
  std::stable_sort(whole.begin(), whole.end(), [](const Block* x, const Block* y) { return x->tiles > y->tiles; });
  for (const Block* b : whole)
    for (int h = 0; h < heads; h++) L.unsplit.push_back(Item{b->seq, b->qb, h, 0, b->tiles, 0, 1, -1});
  // ranges of the split blocks, heaviest first
  struct Range { const Block* b; int s, t0, t1; };
  std::vector<Range> ranges;
  for (const Block& b : blocks) {
    if (b.ns == 1) continue;
    const int base = b.tiles / b.ns, rem = b.tiles - base * b.ns;
    for (int s = 0; s < b.ns; s++) {
      const int t0 = s * base + std::min(s, rem);
      ranges.push_back(Range{&b, s, t0, t0 + base + (s < rem ? 1 : 0)});
    }
    for (int h = 0; h < heads; h++) L.merge.push_back(Item{b.seq, b.qb, h, 0, b.tiles, 0, b.ns, b.base + h});
  }
  std::stable_sort(ranges.begin(), ranges.end(), [](const Range& x, const Range& y) { return x.t1 - x.t0 > y.t1 - y.t0; });
  for (const Range& r : ranges)
    for (int h = 0; h < heads; h++) L.split.push_back(Item{r.b->seq, r.b->qb, h, r.t0, r.t1, r.s, r.b->ns, r.b->base + r.s * heads + h});
  return L;
}

// The automatic target: 0 when the whole blocks alone give `want` work items (two per CU, the rule profiles/verify_rows.txt measured for attn_extend_rg_kernel),
// else the LARGEST target — the fewest, longest ranges — whose lists hold `want` items, else 1.
inline int auto_target(const Seq* seq, int n, int heads, int want) {
  int most = 1;
  for (int j = 0; j < n; j++) most = std::max(most, block_tiles(seq[j], (seq[j].len - 1) / QBLK));
  if (count(seq, n, heads, 0).unsplit >= want) return 0;
  for (int t = most - 1; t >= 1; t--) {
    const Counts c = count(seq, n, heads, t);
    if (c.unsplit + c.split >= want) return t;
  }
  return most > 1 ? 1 : 0;
}

}  // namespace attn_worklist
