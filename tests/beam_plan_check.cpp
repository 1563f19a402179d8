// beam_plan_check.cpp — the CPU audit of tinygpt_amd/csrc/beam_plan.h and of the KvPool calls tgx_beam_advance makes (built and run by tests/test_beam_plan.py under
// the address and undefined-behaviour sanitizers; never loaded into Python).  The harness holds what the device would: a content word per (physical block, slot),
// written by admissions and steps, copied for a copied child's tail exactly as abi.hip copies it.  The naive model is a vector of token tags per row: after every
// operation every row read through its table must equal its tags, KvPool::check must pass, the placement must equal an independent restatement of the header's rule,
// the blocks taken must equal fresh_blocks, and the changes list must name every table index once.  A refusal must leave the pool equal (KvPool::operator==) to a
// copy taken before.
#include "../tinygpt_amd/csrc/beam_plan.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#define REQUIRE(cond)                                                                                  \
  do {                                                                                                 \
    if (!(cond)) { fprintf(stderr, "beam_plan_check: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

using beam_plan::Plan;
using beam_plan::RowState;
typedef std::vector<int32_t> Ints;

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned int rnd(unsigned int n) {      // splitmix64
  unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
  return (unsigned int)(z % n);
}

struct Sim {
  KvPool p;
  int max_batch, blk, batch = 0, vocab = 100;
  std::vector<std::vector<long long>> data;      // [physical block][slot]
  std::vector<std::vector<long long>> seq;       // the naive model: every row's tags
  std::vector<RowState> st;
  long long next_tag = 1;
  Sim(int mb, int max_ctx, int budget, int block) : max_batch(mb), blk(block) {
    p.init(mb, max_ctx, budget, block);
    data.assign((size_t)p.n_blocks(), std::vector<long long>((size_t)block, 0));
    seq.assign((size_t)mb, {}); st.assign((size_t)mb, RowState());
  }
  long long& at(int row, long long pos) { return data[(size_t)p.block_at(row, (int)(pos / blk))][(size_t)(pos % blk)]; }
  void audit() {
    std::vector<long long> len((size_t)max_batch, 0);
    for (int r = 0; r < max_batch; r++) {
      const bool live = r < batch && !st[(size_t)r].idle;
      len[(size_t)r] = live ? st[(size_t)r].past : 0;
      REQUIRE(len[(size_t)r] == (long long)seq[(size_t)r].size());
      if (!live) REQUIRE(p.row_blocks(r) == 0);
      REQUIRE(p.row_blocks(r) >= p.blocks_for(len[(size_t)r]));
      for (long long t = 0; t < len[(size_t)r]; t++) REQUIRE(at(r, t) == seq[(size_t)r][(size_t)t]);
    }
    const char* wrong = p.check(len);
    if (wrong) { fprintf(stderr, "beam_plan_check: KvPool::check: %s\n", wrong); exit(1); }
  }
  bool append(int row, long long n) {      // a writer of the cache writes no shared block
    KvPool::Changes ch;
    if (p.grow(row, st[(size_t)row].past + n, ch) != KvPool::GROW_OK) return false;
    for (long long i = 0; i < n; i++) {
      const long long t = st[(size_t)row].past++;
      REQUIRE(!p.shared(row, (int)(t / blk)));
      at(row, t) = next_tag; seq[(size_t)row].push_back(next_tag++);
    }
    return true;
  }
  bool admit(int row, long long n) {       // into an empty row (retired, or the next new one)
    REQUIRE(row <= batch && (row == batch || st[(size_t)row].idle || st[(size_t)row].past == 0));
    if (p.blocks_for(n) > (long long)p.free_blocks()) return false;
    st[(size_t)row] = RowState(); batch = std::max(batch, row + 1);
    REQUIRE(append(row, n)); audit();
    return true;
  }
  // tgx_beam_advance as abi.hip composes it: the status (0 OK, 1, 4, 8), and out_rows on success
  int advance(const Ints& rows, const Ints& parent, const Ints& tokens, Ints* out_rows, Plan* plan_out = nullptr) {
    const KvPool before = p;
    Plan plan;
    const char* why = nullptr;
    const int rc = beam_plan::make(max_batch, batch, vocab, st.data(), (int)rows.size(), rows.data(), (int)parent.size(), parent.data(), tokens.data(), &plan, &why);
    if (rc) { REQUIRE(why != nullptr); REQUIRE(p == before); return rc; }
    const long long need = beam_plan::fresh_blocks(plan, blk), have = beam_plan::available(p, plan);
    if (need > have) { REQUIRE(p == before); return 8; }
    long long back = 0;      // what really comes back: blocks only retired rows map
    {
      std::set<int> ret(plan.retire, plan.retire + plan.n_retire);
      std::set<int> seen;
      for (int r : ret)
        for (int i = 0; i < p.row_blocks(r); i++) {
          const int b = p.block_at(r, i);
          int others = 0;
          for (int q = 0; q < max_batch; q++)
            if (!ret.count(q))
              for (int k = 0; k < p.row_blocks(q); k++) others += p.block_at(q, k) == b;
          if (!others && seen.insert(b).second) back++;
        }
    }
    const long long free0 = (long long)p.free_blocks();
    for (int i = 0; i < plan.n_retire; i++) { st[(size_t)plan.retire[i]] = RowState(); st[(size_t)plan.retire[i]].idle = true; seq[(size_t)plan.retire[i]].clear(); }
    KvPool::Changes ch;
    const beam_plan::Blocks b = beam_plan::apply(p, plan, ch);
    REQUIRE((long long)p.free_blocks() == free0 + back - need);
    {      // every table index once, and the list leaves a mirror of the table where the pool's is
      std::set<int> idx;
      for (auto& e : ch) { REQUIRE(idx.insert(e.first).second); REQUIRE(p.block_at(e.first / p.tbl_stride(), e.first % p.tbl_stride()) == e.second); }
    }
    int copies = 0;
    for (int g = 0; g < plan.n_groups; g++) {
      const beam_plan::Group& gr = plan.group[g];
      REQUIRE(gr.past == st[(size_t)gr.src].past && gr.n_dst >= 1);
      const int tail = (int)(gr.past % blk);
      for (int k = 0; k < gr.n_dst; k++) {
        REQUIRE((b.tail_blk[g][k] != 0) == (tail != 0));
        for (int i = 0; i < tail; i++) data[(size_t)b.tail_blk[g][k]][(size_t)i] = data[(size_t)b.src_blk[g]][(size_t)i];
        seq[(size_t)gr.dst[k]] = seq[(size_t)gr.src];
        st[(size_t)gr.dst[k]] = RowState(); st[(size_t)gr.dst[k]].past = gr.past;
        copies++;
      }
    }
    REQUIRE(copies == plan.n_copies);
    batch = std::max(batch, plan.new_batch);
    out_rows->assign(plan.out_rows, plan.out_rows + plan.n_next);
    if (plan_out) *plan_out = plan;
    audit();
    return 0;
  }
};

// the header's placement, restated: in-place children first, then the rest into the empties
static Ints expected_rows(const Sim& s, const Ints& rows, const Ints& parent) {
  const int n = (int)rows.size(), m = (int)parent.size();
  Ints out((size_t)m, -1);
  std::vector<int> empties;
  for (int i = 0; i < n; i++) {
    const int r = rows[(size_t)i];
    const bool source = r < s.batch && !s.st[(size_t)r].idle && s.st[(size_t)r].past > 0;
    int j0 = -1;
    for (int j = m - 1; j >= 0; j--) if (parent[(size_t)j] == i) j0 = j;
    if (source && j0 >= 0) out[(size_t)j0] = r; else empties.push_back(r);
  }
  size_t e = 0;
  for (int j = 0; j < m; j++) if (out[(size_t)j] < 0) out[(size_t)j] = empties[e++];
  return out;
}

static void hand_written() {
  const int B = 16;
  {      // 1 -> 4 from a fresh prefill of 37 tokens (2 full blocks + a tail of 5): three copies, three tail blocks, new rows 1 .. 3
    Sim s(8, 256, 40 * B, B);
    REQUIRE(s.admit(0, 37));
    const long long f0 = (long long)s.p.free_blocks();
    Ints out; Plan pl;
    REQUIRE(s.advance({0, 1, 2, 3}, {0, 0, 0, 0}, {5, 6, 7, 8}, &out, &pl) == 0);
    REQUIRE((out == Ints{0, 1, 2, 3}) && pl.n_copies == 3 && pl.n_groups == 1 && pl.n_retire == 0 && s.batch == 4);
    REQUIRE((long long)s.p.free_blocks() == f0 - 3);
    for (int r = 1; r < 4; r++) { REQUIRE(s.p.block_at(r, 0) == s.p.block_at(0, 0) && s.p.block_at(r, 1) == s.p.block_at(0, 1) && s.p.block_at(r, 2) != s.p.block_at(0, 2)); }
    // the identity: nothing copied, nothing moved
    const KvPool before = s.p;
    REQUIRE(s.advance({0, 1, 2, 3}, {0, 1, 2, 3}, {1, 1, 1, 1}, &out, &pl) == 0);
    REQUIRE((out == Ints{0, 1, 2, 3}) && pl.n_copies == 0 && pl.n_retire == 0 && s.p == before);
    // a permutation with a repeated parent: parent = [2, 0, 2, 1]: rows 2, 0, 1 keep children 0, 1, 3; child 2 takes row 3 (retired: it has no child)
    for (int r = 0; r < 4; r++) REQUIRE(s.append(r, 1));
    REQUIRE(s.advance({0, 1, 2, 3}, {2, 0, 2, 1}, {1, 2, 3, 4}, &out, &pl) == 0);
    REQUIRE((out == Ints{2, 0, 3, 1}) && pl.n_copies == 1 && pl.n_retire == 1 && pl.retire[0] == 3 && pl.group[0].src == 2 && pl.group[0].dst[0] == 3);
    // all children of one parent (row 1): rows 0, 2, 3 retire and take children 1, 2, 3
    REQUIRE(s.advance({0, 1, 2, 3}, {1, 1, 1, 1}, {1, 2, 3, 4}, &out, &pl) == 0);
    REQUIRE((out == Ints{1, 0, 2, 3}) && pl.n_copies == 3 && pl.n_retire == 3);
    // a shrink: two hypotheses of four rows; rows 1 and 3 retire and stay empty
    REQUIRE(s.advance({0, 1, 2, 3}, {2, 0}, {9, 9}, &out, &pl) == 0);
    REQUIRE((out == Ints{2, 0}) && pl.n_copies == 0 && pl.n_retire == 2 && s.st[1].idle && s.st[3].idle && s.p.row_blocks(1) == 0 && s.p.row_blocks(3) == 0);
    // ... and grow again through the retired rows, array order deciding: rows listed 3 before 1
    REQUIRE(s.advance({0, 2, 3, 1}, {0, 0, 1}, {9, 9, 9}, &out, &pl) == 0);
    REQUIRE((out == Ints{0, 3, 2}) && pl.n_copies == 1);
  }
  {      // no tail: 32 tokens, copies take no block
    Sim s(4, 256, 10 * B, B);
    REQUIRE(s.admit(0, 32));
    const long long f0 = (long long)s.p.free_blocks();
    Ints out;
    REQUIRE(s.advance({0, 1, 2}, {0, 0, 0}, {1, 2, 3}, &out) == 0);
    REQUIRE((long long)s.p.free_blocks() == f0);
  }
  {      // every refusal
    Sim s(6, 256, 6 * B, B);
    REQUIRE(s.admit(0, 37) && s.admit(1, 20));      // 3 + 2 blocks: one free
    Ints out;
    s.st[1].fin = true;
    REQUIRE(s.advance({0, 1}, {0, 0}, {1, 1}, &out) == 4);        // a finished row named
    s.st[1].fin = false; s.st[1].nologits = true;
    REQUIRE(s.advance({0, 1}, {0, 0}, {1, 1}, &out) == 4);        // a row without logits named
    s.st[1].nologits = false;
    REQUIRE(s.advance({0, 2}, {1, 0}, {1, 1}, &out) == 4);        // a spare as parent
    REQUIRE(s.advance({0, 0}, {0, 0}, {1, 1}, &out) == 1);        // a row named twice
    REQUIRE(s.advance({0, 6}, {0, 0}, {1, 1}, &out) == 1);        // a row out of range
    REQUIRE(s.advance({0, -1}, {0, 0}, {1, 1}, &out) == 1);
    REQUIRE(s.advance({0, 2}, {0, 2}, {1, 1}, &out) == 1);        // a parent out of range
    REQUIRE(s.advance({0, 2}, {0, -1}, {1, 1}, &out) == 1);
    REQUIRE(s.advance({0, 2}, {0, 0}, {1, 100}, &out) == 1);      // a token out of range
    REQUIRE(s.advance({0, 2}, {0, 0}, {1, -1}, &out) == 1);
    REQUIRE(s.advance({0, 2}, {0, 0, 0}, {1, 1, 1}, &out) == 1);  // n_next > n_rows
    REQUIRE(s.advance({0, 2}, {}, {}, &out) == 1);                // n_next < 1
    REQUIRE(s.advance({}, {}, {}, &out) == 1);                    // n_rows < 1
    REQUIRE(s.advance({0, 1, 2, 3, 4, 5, 0, 1, 2}, {0}, {1}, &out) == 1);      // n_rows > TGX_MAX_BEAMS
    REQUIRE(s.advance({0, 3}, {0, 0}, {1, 1}, &out) == 1);        // a gap in the new rows (2 is next)
    REQUIRE(s.advance({0, 3, 2}, {0, 0}, {1, 1}, &out) == 1);     // ... by the placement: the first empty in array order is row 3
    {
      Plan pl; const char* why = nullptr;
      const int32_t r[2] = {0, 2}, pa[2] = {0, 0}, tk[2] = {1, 1};
      REQUIRE(beam_plan::make(6, s.batch, 100, s.st.data(), 2, nullptr, 2, pa, tk, &pl, &why) == 1);      // null pointers
      REQUIRE(beam_plan::make(6, s.batch, 100, s.st.data(), 2, r, 2, nullptr, tk, &pl, &why) == 1);
      REQUIRE(beam_plan::make(6, s.batch, 100, s.st.data(), 2, r, 2, pa, nullptr, &pl, &why) == 1);
      REQUIRE(beam_plan::make(6, s.batch, 100, s.st.data(), 2, r, 2, pa, tk, nullptr, &why) == 1);
    }
    REQUIRE(s.advance({0, 2, 3}, {0, 0, 0}, {1, 1, 1}, &out) == 8);        // two tail blocks, one free
    REQUIRE(s.advance({0, 1, 2}, {0, 0, 0}, {1, 1, 1}, &out) == 0);        // ... with row 1 childless its two blocks come back: fits
    REQUIRE((out == Ints{0, 1, 2}) && s.p.free_blocks() == 1);
  }
}

static void random_run(int rounds) {
  const int B = 8, MB = 10;
  for (int round = 0; round < rounds; round++) {
    Sim s(MB, 512, (12 + (int)rnd(30)) * B, B);
    REQUIRE(s.admit(0, 1 + rnd(40)));
    if (rnd(2)) s.admit(1, 1 + rnd(20));      // a bystander or a second source
    for (int op = 0; op < 60; op++) {
      std::vector<int> live, spare;
      for (int r = 0; r < MB; r++) (r < s.batch && !s.st[(size_t)r].idle && s.st[(size_t)r].past > 0 ? live : spare).push_back(r);
      if (live.empty()) break;
      if (rnd(3) == 0) {      // a step of every live row
        bool ok = true;
        for (int r : live) ok = ok && s.append(r, 1);
        s.audit();
        if (!ok) break;
        continue;
      }
      // a group: some live rows, then some spares (rows < batch first, then the new ones in order: the caller's side of the new-row rule), shuffled now and then
      Ints rows;
      for (int r : live) if (rows.size() < 8 && rnd(4)) rows.push_back(r);
      if (rows.empty()) rows.push_back(live[rnd((unsigned)live.size())]);
      const int n_src = (int)rows.size();
      for (int r : spare) if (rows.size() < 8 && rnd(3)) rows.push_back(r);
      const bool shuffled = rnd(4) == 0;
      if (shuffled) for (size_t i = rows.size(); i > 1; i--) std::swap(rows[i - 1], rows[rnd((unsigned)i)]);
      const int n_next = 1 + (int)rnd((unsigned)rows.size());
      Ints parent, tokens;
      for (int j = 0; j < n_next; j++) {
        int pi;
        do { pi = (int)rnd((unsigned)rows.size()); } while (std::find(live.begin(), live.end(), rows[(size_t)pi]) == live.end());
        parent.push_back(pi); tokens.push_back((int32_t)rnd(100));
      }
      (void)n_src;
      const Ints want = expected_rows(s, rows, parent);
      std::vector<std::vector<long long>> seq0 = s.seq;
      std::vector<RowState> st0 = s.st;
      Ints out; Plan pl;
      const int rc = s.advance(rows, parent, tokens, &out, &pl);
      if (rc) {      // a gap in the new rows (a shuffled or thinned spare list) or the budget: nothing changed
        REQUIRE(rc == 1 || rc == 8);
        if (rc == 1) {      // ... and the restated placement does leave a gap
          std::set<int> fresh;
          for (int r : want) if (r >= s.batch) fresh.insert(r);
          bool gap = false;
          for (int r : fresh) gap = gap || r >= s.batch + (int)fresh.size();
          REQUIRE(gap);
        }
        REQUIRE(s.seq == seq0);
        s.audit();
        continue;
      }
      REQUIRE(out == want);
      std::set<int> distinct(parent.begin(), parent.end());
      REQUIRE(pl.n_copies == n_next - (int)distinct.size());
      for (int j = 0; j < n_next; j++) REQUIRE(s.seq[(size_t)out[(size_t)j]] == seq0[(size_t)rows[(size_t)parent[(size_t)j]]]);      // every hypothesis holds its parent's sequence
      for (int r = 0; r < MB; r++)      // rows not named keep theirs
        if (std::find(rows.begin(), rows.end(), r) == rows.end()) REQUIRE(s.seq[(size_t)r] == seq0[(size_t)r]);
      for (size_t i = 0; i < rows.size(); i++)      // named rows that hold no hypothesis are empty
        if (std::find(out.begin(), out.end(), rows[i]) == out.end()) REQUIRE(s.seq[(size_t)rows[i]].empty() && s.p.row_blocks(rows[i]) == 0);
    }
  }
}

int main() {
  hand_written();
  random_run(400);
  printf("beam_plan_check: ok\n");
  return 0;
}
