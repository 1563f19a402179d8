// splice_plan.h — the host side of tgx_splice_row (include/tgx.h): which positions of a row's cache move where when ranges are cut out of its middle, and which
// blocks of a paged cache that writes.  Host-only — the standard library alone, no HIP: tests/splice_plan_check.cpp drives it on a CPU.
//
// The kept ranges [starts[i], starts[i] + lens[i]) are sorted, non-empty, disjoint (they may touch) and lie inside [0, past).  Touching ranges are merged; merged range
// i moves DOWN by delta_i = src_i - dst_i >= 0, dst_i = the kept positions in front of it, and the deltas increase strictly from one merged range to the next.  f is
// the first position whose content changes — the end of the leading delta == 0 range (0 without one) — and for a pure truncation (one range from 0) f == new_len.
// The MOVED segments are the ones with delta > 0: new_len - f positions in all, the m-th of them counted in order.
//
// Paged cache (kv_pool.h): block indices [f / block, ceil(new_len / block)) are written — by the move, or, for a truncation, by the next append.  One of them that
// other rows map as well must be swapped for a fresh block first (copy on write); when f is inside the first written block and that block is swapped, its rows
// [0, f % block) are identity rows and have to be carried over.  Blocks below f / block are untouched and stay shared: they lie wholly below f <= new_len, so the
// pool's invariant "a shared block is full for every row that maps it" holds afterwards.
#pragma once
#include <cstdint>
#include <vector>

#include "kv_pool.h"

namespace splice_plan {

constexpr int MAX_RANGES = 16;      // == TGX_MAX_SPLICE_RANGES

struct Seg { long long src, dst, len; };
struct Plan {
  int n_seg = 0;                    // merged ranges, in order
  Seg seg[MAX_RANGES];
  long long f = 0, new_len = 0;     // first position whose content changes; positions kept
  int first_moved = 0;              // index of the first segment with src != dst (n_seg: none — a truncation or the whole row)
  long long moved() const { return new_len - f; }
  bool truncation() const { return n_seg == 1 && seg[0].src == 0; }      // one range [0, L): nothing moves
};

// nullptr and *out filled, or what is wrong with the ranges (nothing is written then)
inline const char* make(long long past, int n_keep, const int64_t* starts, const int64_t* lens, Plan* out) {
  if (!starts || !lens || !out) return "a null pointer";
  if (n_keep < 1 || n_keep > MAX_RANGES) return "n_keep outside [1, TGX_MAX_SPLICE_RANGES]";
  Plan p;
  long long end = 0, kept = 0;      // end of the previous range; positions kept so far
  for (int i = 0; i < n_keep; i++) {
    const long long s = starts[i], n = lens[i];
    if (n < 1) return "an empty range";
    if (s < 0 || s >= past || n > past - s) return "a range outside [0, past)";
    if (i && s < end) return "ranges unsorted or overlapping";
    if (i && s == end) p.seg[p.n_seg - 1].len += n;      // touching: one segment
    else p.seg[p.n_seg++] = {s, kept, n};
    end = s + n; kept += n;
  }
  p.new_len = kept;
  p.first_moved = p.seg[0].src == 0 ? 1 : 0;
  p.f = p.seg[0].src == 0 ? p.seg[0].len : 0;
  *out = p;
  return nullptr;
}

// source position of kept position d (d < new_len)
inline long long source_of(const Plan& p, long long d) {
  for (int i = 0; i < p.n_seg; i++)
    if (d < p.seg[i].dst + p.seg[i].len) return p.seg[i].src + (d - p.seg[i].dst);
  return -1;
}

struct Blocks {
  int first = 0, end = 0;           // block indices [first, end) of the row are written
  std::vector<int> fresh;           // those of them other rows map as well: each needs a fresh block before anything writes to it
  int carry = 0;                    // identity rows [0, carry) of block `first` to copy into its fresh block (0 unless `first` is in `fresh`)
};
inline Blocks blocks(const KvPool& pool, int row, const Plan& p) {
  Blocks b;
  const int bt = pool.block_tokens();
  b.first = (int)(p.f / bt); b.end = pool.blocks_for(p.new_len);
  for (int i = b.first; i < b.end; i++)
    if (pool.shared(row, i)) b.fresh.push_back(i);
  if (!b.fresh.empty() && b.fresh[0] == b.first) b.carry = (int)(p.f % bt);
  return b;
}

}   // namespace splice_plan
