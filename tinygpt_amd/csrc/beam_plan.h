// beam_plan.h — the host side of tgx_beam_advance (include/tgx.h): which rows of a beam group keep their sequence, which are retired, which row every new hypothesis
// lands in, what has to be copied, and how many fresh blocks of a paged cache that takes.  Host-only — the standard library alone, no HIP: tests/beam_plan_check.cpp
// drives it on a CPU, beside a KvPool.
//
// The group is rows[0 .. n_rows): each a SOURCE (a live, unfinished row of the batch that holds logits) or a SPARE (a retired or empty row < batch, or a row >= batch).
// New hypothesis j continues source rows[parent[j]].  THE PLACEMENT (pinned: callers and tests state it):
//   1. every source that has children keeps its lowest-j child IN PLACE — no copy, no block moves;
//   2. the sources without a child are retired (tgx_reset_row);
//   3. the other children, in ascending j, take the rows that are empty now — retired sources and spares — in ascending ARRAY index.
// n_next <= n_rows and every in-place child frees no row, so step 3 never runs out: empties = n_rows - (sources with children) >= n_next - (sources with children).
// A step therefore copies exactly n_next - (distinct parents) rows.  The new rows (>= batch) that receive a hypothesis must be exactly batch .. batch + m - 1, the
// rule of tgx_forward_rows: which spares receive one follows from the placement, so the caller lists its new rows in ascending order behind the rows of the batch.
//
// Paged cache (kv_pool.h): a copied child maps its parent's full blocks by reference and takes ONE fresh block for the partial tail (past % block != 0).  The fresh
// blocks are counted against the free list plus what the retired sources give back BEFORE anything changes (fresh_blocks / available); apply() then makes every pool
// change of the call and leaves ONE list of table entries, each index once (its last value), so one push carries it.
#pragma once
#include <cstdint>
#include <vector>

#include "kv_pool.h"

namespace beam_plan {

constexpr int MAX_BEAMS = 8;      // == TGX_MAX_BEAMS
enum Status { OK = 0, INVALID = 1, STATE = 4 };      // == TGX_OK / TGX_ERR_INVALID / TGX_ERR_STATE

struct RowState { long long past = 0; bool idle = false, fin = false, nologits = false; };      // the host's view of one row (ctx.h RowHost)

struct Group { int src = 0; long long past = 0; int n_dst = 0; int dst[MAX_BEAMS] = {}; };      // one parent with copied children: ONE copy launch
struct Plan {
  int n_rows = 0, n_next = 0;
  bool source[MAX_BEAMS] = {};          // rows[i] is a source (else a spare)
  int n_retire = 0, retire[MAX_BEAMS] = {};      // the sources without a child, in array order (row numbers)
  int out_rows[MAX_BEAMS] = {};         // where hypothesis j lives afterwards
  bool in_place[MAX_BEAMS] = {};        // hypothesis j stays in its parent's row
  int n_groups = 0;
  Group group[MAX_BEAMS];
  int n_copies = 0;                     // == n_next - (distinct parents)
  int new_batch = 0;                    // the batch afterwards
};

// OK and *out filled, or the status and *why (nothing is written to *out then).  st: the state of every row [0, max_batch)
inline Status make(int max_batch, int batch, int vocab, const RowState* st, int n_rows, const int32_t* rows, int n_next, const int32_t* parent, const int32_t* tokens,
                   Plan* out, const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  if (!st || !rows || !parent || !tokens || !out) { *why = "a null pointer"; return INVALID; }
  if (n_rows < 1 || n_rows > MAX_BEAMS) { *why = "n_rows outside [1, TGX_MAX_BEAMS]"; return INVALID; }
  if (n_next < 1 || n_next > n_rows) { *why = "n_next outside [1, n_rows]"; return INVALID; }
  Plan p;
  p.n_rows = n_rows; p.n_next = n_next;
  for (int i = 0; i < n_rows; i++) {
    if (rows[i] < 0 || rows[i] >= max_batch) { *why = "a row outside [0, max_batch)"; return INVALID; }
    for (int k = 0; k < i; k++)
      if (rows[k] == rows[i]) { *why = "a row named twice"; return INVALID; }
  }
  for (int j = 0; j < n_next; j++) {
    if (parent[j] < 0 || parent[j] >= n_rows) { *why = "a parent outside [0, n_rows)"; return INVALID; }
    if (tokens[j] < 0 || tokens[j] >= vocab) { *why = "a token outside [0, vocab)"; return INVALID; }
  }
  for (int i = 0; i < n_rows; i++) {
    const int r = rows[i];
    const bool empty = r >= batch || st[r].idle || st[r].past == 0;
    if (!empty && st[r].fin) { *why = "a row that finished on the device is neither a source nor a spare (tgx_reset_row it)"; return STATE; }
    if (!empty && st[r].nologits) { *why = "a row that holds no logits is neither a source nor a spare (tgx_extend_row it)"; return STATE; }
    p.source[i] = !empty;
  }
  for (int j = 0; j < n_next; j++)
    if (!p.source[parent[j]]) { *why = "a parent that is not a live row of the batch"; return STATE; }
  // 1. the lowest-j child of every source stays in place
  int first_child[MAX_BEAMS];
  for (int i = 0; i < n_rows; i++) first_child[i] = -1;
  for (int j = n_next - 1; j >= 0; j--) first_child[parent[j]] = j;
  // 2. the childless sources retire; the rows that are empty now, in array order
  int n_empty = 0, empty_idx[MAX_BEAMS];
  for (int i = 0; i < n_rows; i++) {
    if (p.source[i] && first_child[i] >= 0) continue;
    if (p.source[i]) p.retire[p.n_retire++] = rows[i];
    empty_idx[n_empty++] = i;
  }
  // 3. the other children take them
  int take = 0, group_of[MAX_BEAMS];
  for (int i = 0; i < n_rows; i++) group_of[i] = -1;
  for (int j = 0; j < n_next; j++) {
    const int pi = parent[j];
    if (first_child[pi] == j) { p.out_rows[j] = rows[pi]; p.in_place[j] = true; continue; }
    const int dst = rows[empty_idx[take++]];      // (take < n_empty: the header's count)
    p.out_rows[j] = dst;
    if (group_of[pi] < 0) { group_of[pi] = p.n_groups; p.group[p.n_groups].src = rows[pi]; p.group[p.n_groups].past = st[rows[pi]].past; p.n_groups++; }
    Group& g = p.group[group_of[pi]];
    g.dst[g.n_dst++] = dst;
    p.n_copies++;
  }
  // the new rows that receive a hypothesis: exactly batch .. batch + m - 1
  int m = 0;
  bool named[MAX_BEAMS] = {};
  for (int j = 0; j < n_next; j++) m += p.out_rows[j] >= batch;
  for (int j = 0; j < n_next; j++) {
    const int r = p.out_rows[j];
    if (r < batch) continue;
    if (r >= batch + m) { *why = "the new rows that receive a hypothesis must be batch .. batch + m - 1 (the batch grows in order)"; return INVALID; }
    named[r - batch] = true;
  }
  for (int k = 0; k < m; k++)
    if (!named[k]) { *why = "the new rows that receive a hypothesis must be batch .. batch + m - 1 (the batch grows in order)"; return INVALID; }
  p.new_batch = batch + m;
  *out = p;
  return OK;
}

// the fresh blocks the plan takes: one per copied child whose parent ends inside a block
inline long long fresh_blocks(const Plan& p, int block_tokens) {
  long long n = 0;
  for (int g = 0; g < p.n_groups; g++) n += p.group[g].past % block_tokens ? p.group[g].n_dst : 0;
  return n;
}
// ... and what it may take: the free list plus what the retired sources give back (KvPool::available_for: errs towards refusing)
inline long long available(const KvPool& pool, const Plan& p) { return pool.available_for(p.retire, p.n_retire); }

// every pool change of the plan (the caller counted: fresh_blocks <= available).  tail_blk[g][k]: the fresh tail block of group g's k-th destination (0: none),
// src_blk[g]: the parent's own tail block.  `ch` ends as one list with every table index once
struct Blocks { int tail_blk[MAX_BEAMS][MAX_BEAMS] = {}; int src_blk[MAX_BEAMS] = {}; };
inline Blocks apply(KvPool& pool, const Plan& p, KvPool::Changes& ch) {
  Blocks b;
  KvPool::Changes all;
  for (int i = 0; i < p.n_retire; i++) pool.release(p.retire[i], all);
  for (int g = 0; g < p.n_groups; g++) {
    const Group& gr = p.group[g];
    const int n_full = (int)(gr.past / pool.block_tokens());
    const bool tail = gr.past % pool.block_tokens() != 0;
    for (int k = 0; k < gr.n_dst; k++) {
      pool.share(gr.src, gr.dst[k], n_full, gr.past, all);
      if (tail) b.tail_blk[g][k] = pool.fork_tail(gr.dst[k], all);
    }
    if (tail) b.src_blk[g] = pool.block_at(gr.src, n_full);
  }
  // one entry per table index, its last value: the push writes the entries of a launch side by side
  for (size_t i = 0; i < all.size(); i++) {
    bool later = false;
    for (size_t k = i + 1; k < all.size() && !later; k++) later = all[k].first == all[i].first;
    if (!later) ch.push_back(all[i]);
  }
  return b;
}

}   // namespace beam_plan
