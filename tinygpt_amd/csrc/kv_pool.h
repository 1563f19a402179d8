// kv_pool.h — the block pool of the paged KV cache (option kv.budget_tokens, include/tgx.h): which physical block of block_tokens positions backs which (row, block
// index), which rows map a block, which blocks are free.  Host-only — the standard library alone, no HIP: tests/kv_pool_check.cpp drives it on a CPU.  Block 0 is
// scratch: the table entries of a row beyond its blocks name it.  Every mutator updates the pool's table (the mirror of the device's) and appends the (flat table
// index, value) pairs it wrote to `ch`; the caller pushes that list to the device table, stream-ordered (abi.hip kv_tbl_push).
// THE INVARIANT: a block mapped by more than one row is FULL — every position in it is < past of every row that maps it — so no launch ever
// writes to it (every writer of the cache writes positions >= its row's past).  It is asserted where blocks are assigned: a block handed out for writing must be
// mapped by nobody (take), a block shared by reference must lie wholly below the source's past (share).  A violation would let one sequence write into another's
// cache: the process stops there (the library is built with NDEBUG, so the check is spelled out).  check() audits the whole pool (the CPU test alone calls it).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#define KV_ASSERT(cond, what)                                                                                   \
  do {                                                                                                          \
    if (!(cond)) { fprintf(stderr, "tgx: paged KV invariant violated (%s) at %s:%d\n", what, __FILE__, __LINE__); abort(); } \
  } while (0)
class KvPool {
 public:
  typedef std::vector<std::pair<int, int>> Changes;      // (flat table index, value)
  enum Grow { GROW_OK, GROW_BEYOND_TABLE, GROW_EXHAUSTED };
  void init(int max_batch, int max_ctx, int budget_tokens, int block_tokens) {
    block = block_tokens; nblocks = (budget_tokens + block - 1) / block + 1; stride = (max_ctx + block - 1) / block;      // (+ the scratch block 0)
    tbl.assign((size_t)max_batch * stride, 0); row_nblk.assign((size_t)max_batch, 0); ref.assign((size_t)nblocks, 0);
    free_list.clear();
    for (int b = nblocks - 1; b >= 1; b--) free_list.push_back(b);
  }
  int n_blocks() const { return nblocks; }        // physical blocks incl. the scratch block
  int tbl_stride() const { return stride; }       // table entries per row = ceil(max_ctx / block_tokens)
  int block_tokens() const { return block; }
  int blocks_for(long long tokens) const { return (int)((tokens + block - 1) / block); }
  size_t free_blocks() const { return free_list.size(); }
  int row_blocks(int row) const { return row_nblk[(size_t)row]; }
  int block_at(int row, int idx) const { return tbl[(size_t)row * stride + idx]; }
  int sharers(int blk) const { return ref[(size_t)blk]; }      // the rows whose tables map physical block blk (free at 0)
  bool shared(int row, int idx) const { return sharers(block_at(row, idx)) > 1; }
  // blocks that return to the free list when `row` releases its blocks: only those nobody else maps (a block a forked sibling still maps stays assigned)
  long long given_back(int row) const { long long n = 0; for (int i = 0; i < row_blocks(row); i++) n += !shared(row, i); return n; }
  // THE all-or-nothing sum: what a call that first releases rows[0..n) can take — the free list plus what those rows give back.  (A block shared ONLY among the
  // rows of one call is not counted: the sum errs towards refusing.)
  long long available_for(const int* rows, int n) const { long long have = (long long)free_list.size(); for (int i = 0; i < n; i++) have += given_back(rows[i]); return have; }
  // row `row` may hold `tokens` tokens after this; a refusal changes nothing
  Grow grow(int row, long long tokens, Changes& ch) {
    const int need = blocks_for(tokens); int& have = row_nblk[(size_t)row];
    if (need <= have) return GROW_OK;
    if (need > stride) return GROW_BEYOND_TABLE;
    if ((size_t)(need - have) > free_list.size()) return GROW_EXHAUSTED;
    for (; have < need; have++) set(row, have, take(), ch);
    return GROW_OK;
  }
  // the row keeps the blocks `tokens` tokens need; the others go back to the free list (a block a forked sibling still maps only loses this row's reference),
  // their table entries back to the scratch block
  void trim(int row, long long tokens, Changes& ch) {
    const int keep = blocks_for(tokens); int& have = row_nblk[(size_t)row];
    for (int i = keep; i < have; i++) { drop(block_at(row, i)); set(row, i, 0, ch); }
    if (keep < have) have = keep;
  }
  void release(int row, Changes& ch) { trim(row, 0, ch); }      // all of the row's blocks
  // tgx_fork_row: row `dst` (holding no block) maps the first n_full blocks of `src`, a row of src_past positions, by reference
  void share(int src, int dst, int n_full, long long src_past, Changes& ch) {
    KV_ASSERT((long long)n_full * block <= src_past && n_full <= row_blocks(src) && row_blocks(dst) == 0, "a block that is not full was about to be shared");
    for (int i = 0; i < n_full; i++) { ref[(size_t)block_at(src, i)]++; set(dst, i, block_at(src, i), ch); }
    row_nblk[(size_t)dst] = n_full;
  }
  // ... and one fresh block behind them for the copy of the source's partial tail (the caller counted: available_for)
  int fork_tail(int dst, Changes& ch) { const int b = take(); set(dst, row_nblk[(size_t)dst]++, b, ch); return b; }
  // copy on write for one block of a row (tgx_truncate_row: its new tail block; tgx_splice_row: every block it writes, splice_plan.h): block idx of `row`, which
  // other rows map as well, is swapped for a fresh one and loses this row's reference.  Returns (old, fresh) for the copy launch.  unshare: the caller counted the
  // fresh blocks against the free list; unshare_tail: fresh 0, and nothing changed, when no block is free
  std::pair<int, int> unshare(int row, int idx, Changes& ch) {
    const int old = block_at(row, idx), fresh = take();
    set(row, idx, fresh, ch); drop(old);
    return {old, fresh};
  }
  std::pair<int, int> unshare_tail(int row, int idx, Changes& ch) {
    if (free_list.empty()) return {block_at(row, idx), 0};
    return unshare(row, idx, ch);
  }
  bool operator==(const KvPool& o) const { return block == o.block && nblocks == o.nblocks && stride == o.stride && tbl == o.tbl && free_list == o.free_list && row_nblk == o.row_nblk && ref == o.ref; }
  // the full audit, given every row's length: nullptr, or what is wrong
  const char* check(const std::vector<long long>& row_len) const {
    std::vector<int> maps((size_t)nblocks, 0), listed((size_t)nblocks, 0);
    for (size_t row = 0; row < row_nblk.size(); row++)
      for (int i = 0; i < stride; i++) {
        const int b = block_at((int)row, i);
        if (b < 0 || b >= nblocks) return "a table entry names no block of the pool";
        if (i >= row_blocks((int)row)) { if (b != 0) return "a table entry beyond a row's blocks is not the scratch block"; continue; }
        if (b == 0) return "a row maps the scratch block";
        maps[(size_t)b]++;
      }
    for (int b : free_list) {
      if (b < 1 || b >= nblocks) return "the free list names the scratch block or no block of the pool";
      if (listed[(size_t)b]++) return "a block is on the free list twice";
    }
    for (int b = 0; b < nblocks; b++) {
      if (ref[(size_t)b] != maps[(size_t)b]) return "a block's count is not the number of table entries that name it";
      if (b >= 1 && (ref[(size_t)b] == 0) != (listed[(size_t)b] == 1)) return "the free list is not exactly the blocks with count 0";
    }
    for (size_t row = 0; row < row_nblk.size(); row++)
      for (int i = 0; i < row_blocks((int)row); i++)
        if (shared((int)row, i) && (long long)(i + 1) * block > row_len[row]) return "a block mapped by more than one row is not full for a row that maps it";
    return nullptr;
  }

 private:
  int block = 1, nblocks = 0, stride = 0;
  std::vector<int> tbl;           // [max_batch][stride]: the host mirror of the device table
  std::vector<int> free_list;     // free physical blocks, handed out from the back
  std::vector<int> row_nblk;      // blocks assigned to each row
  std::vector<int> ref;           // per physical block: the rows that map it.  A block leaves the free list at 0 -> 1 and returns to it at 1 -> 0
  void set(int row, int idx, int blk, Changes& ch) { tbl[(size_t)row * stride + idx] = blk; ch.emplace_back(row * stride + idx, blk); }
  int take() {
    KV_ASSERT(!free_list.empty(), "a block was taken from an empty free list");
    const int b = free_list.back(); free_list.pop_back();
    KV_ASSERT(ref[(size_t)b] == 0, "a block on the free list is still mapped by a row");
    ref[(size_t)b] = 1; return b;
  }
  void drop(int b) { if (--ref[(size_t)b] == 0) free_list.push_back(b); }
};
