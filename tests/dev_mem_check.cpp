// dev_mem_check.cpp — the CPU audit of tinygpt_amd/csrc/dev_mem.h (built and run by tests/test_dev_mem.py under the address and undefined-behaviour sanitizers).
// DevMem is bound to a counting malloc / free pair that logs every call and can be told to fail; after every operation the harness compares live() / live_bytes()
// and the allocator's outstanding count with a naive model (a map pointer -> bytes).  Two parts: a scripted case for each rule (grow's three, release(nullptr),
// release_all), and a random run of alloc / release / grow over a few slots with injected failures.  Every buffer handed out is written over its whole length and
// every buffer still live at the end is freed by release_all alone: a record that kept a dead pointer is a double free for AddressSanitizer, one that lost a live
// pointer a leak for LeakSanitizer at exit.
#include "../tinygpt_amd/csrc/dev_mem.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#define REQUIRE(cond)                                                                              \
  do {                                                                                             \
    if (!(cond)) { fprintf(stderr, "dev_mem_check: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

// ---- the bound allocator
static long outstanding;        // mallocs not yet freed
static bool fail_next;          // the next request fails (and clears the flag)
static std::string calls;       // 'A' a request served, 'X' a request refused, 'F' a free — in order
static void* counting_alloc(size_t bytes) {
  if (fail_next) { fail_next = false; calls += 'X'; return nullptr; }
  calls += 'A'; outstanding++;
  return malloc(bytes);
}
static void counting_free(void* p) { calls += 'F'; outstanding--; free(p); }

struct Harness {
  DevMem m{counting_alloc, counting_free};
  std::map<void*, size_t> model;
  void audit() {
    size_t bytes = 0;
    for (const auto& kv : model) bytes += kv.second;
    REQUIRE(m.live() == model.size() && m.live_bytes() == bytes && outstanding == (long)model.size());
  }
  // every operation: the rule's own postcondition, the model's update, the audit.  `fail`: the allocator refuses the request this operation makes, if it makes one
  void* alloc(size_t bytes, bool fail = false) {
    fail_next = fail;
    void* p = m.alloc(bytes);
    fail_next = false;
    REQUIRE((p == nullptr) == fail);
    if (p) { REQUIRE(!model.count(p)); memset(p, 0xA5, bytes); model[p] = bytes; }
    audit();
    return p;
  }
  void release(void* p) {
    m.release(p);
    if (p) REQUIRE(model.erase(p) == 1);
    audit();
  }
  bool grow(void** p, size_t* have, size_t need, bool fail = false) {
    void* const old = *p; const size_t had = *have, mark = calls.size();
    fail_next = fail;
    const bool ok = m.grow(p, have, need);
    fail_next = false;
    const std::string did = calls.substr(mark);
    if (need <= had) { REQUIRE(ok && *p == old && *have == had && did.empty()); audit(); return ok; }      // rule 1: nothing happens
    REQUIRE(did == (old ? (fail ? "FX" : "FA") : (fail ? "X" : "A")));      // rule 2: the old buffer goes BEFORE the new one is requested
    if (old) REQUIRE(model.erase(old) == 1);
    REQUIRE(ok == !fail);
    if (ok) { REQUIRE(*p && *have == need && !model.count(*p)); memset(*p, 0x5A, need); model[*p] = need; }
    else REQUIRE(*p == nullptr && *have == 0);      // rule 3: the failure leaves nothing, and (the audit) the record does not hold the dead pointer
    audit();
    return ok;
  }
  void release_all() { m.release_all(); model.clear(); audit(); REQUIRE(outstanding == 0); }
};

static void scripted() {
  Harness h;
  h.audit();
  h.release(nullptr);                                  // a no-op: no call of the allocator
  REQUIRE(calls.empty());
  void* a = h.alloc(100);
  void* b = h.alloc(1);
  REQUIRE(h.alloc(64, true) == nullptr && h.m.live() == 2 && h.m.live_bytes() == 101);      // a failed alloc records nothing
  void* p = nullptr; size_t have = 0;
  REQUIRE(h.grow(&p, &have, 0) && p == nullptr);       // need <= have at 0 / 0
  REQUIRE(h.grow(&p, &have, 256) && have == 256);      // from nothing: one request, no free
  void* const first = p;
  REQUIRE(h.grow(&p, &have, 256) && p == first);       // need == have
  REQUIRE(h.grow(&p, &have, 17) && p == first && have == 256);      // need < have: a buffer never shrinks
  REQUIRE(h.grow(&p, &have, 4096) && have == 4096 && h.m.live() == 3 && h.m.live_bytes() == 101 + 4096);      // replaced, not accumulated
  REQUIRE(!h.grow(&p, &have, 8192, true) && p == nullptr && have == 0 && h.m.live() == 2 && h.m.live_bytes() == 101);
  REQUIRE(h.grow(&p, &have, 8, false) && have == 8);   // ... and the next call starts over
  h.release(a);                                        // the oldest record, with newer ones behind it
  REQUIRE(h.m.live() == 2);
  h.release(p); p = nullptr; have = 0;
  (void)b;                                             // left for release_all
  h.alloc(33); h.alloc(7);
  h.release_all();
  h.release_all();                                     // idempotent
  void* again = h.alloc(5);                            // the owner goes on working
  h.release(again);
  REQUIRE(outstanding == 0);
}

// ---- the random run
static uint64_t rng_state;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }      // [lo, hi]

enum Kind { ALLOC, ALLOC_FAIL, RELEASE, RELEASE_NULL, GROW_NOOP, GROW, GROW_FAIL, RELEASE_ALL, N_KINDS };
static const char* kind_name[N_KINDS] = {"alloc", "alloc refused", "release", "release(nullptr)", "grow, need <= have", "grow", "grow refused", "release_all"};
static long done[N_KINDS];

static void random_run(uint64_t seed, int n_ops) {
  const int SLOTS = 24;
  rng_state = seed;
  Harness h;
  struct Slot { void* p = nullptr; size_t have = 0; } slot[SLOTS];
  for (int op = 0; op < n_ops; op++) {
    Slot& s = slot[rnd_in(0, SLOTS - 1)];
    const int dice = rnd_in(0, 99);
    const bool fail = rnd_in(0, 9) == 0;
    if (dice < 30) {      // ---- a fixed buffer into an empty slot (dev_alloc)
      if (s.p) continue;
      const size_t bytes = (size_t)rnd_in(1, 5000);
      s.p = h.alloc(bytes, fail);
      s.have = s.p ? bytes : 0;
      done[fail ? ALLOC_FAIL : ALLOC]++;
    } else if (dice < 55) {      // ---- dev_free: release and null
      done[s.p ? RELEASE : RELEASE_NULL]++;
      h.release(s.p);
      s = Slot{};
    } else if (dice < 99) {      // ---- a workspace that grows on demand; a third of the requests fit what it has
      const size_t need = rnd_in(0, 2) == 0 ? (size_t)rnd_in(0, (int)s.have) : s.have + (size_t)rnd_in(1, 3000);
      const bool noop = need <= s.have, ok = h.grow(&s.p, &s.have, need, fail);
      done[noop ? GROW_NOOP : ok ? GROW : GROW_FAIL]++;
    } else {      // ---- the context is destroyed and another one made
      done[RELEASE_ALL]++;
      h.release_all();
      for (Slot& t : slot) t = Slot{};
    }
  }
  h.release_all();
}

int main() {
  scripted();
  const uint64_t seeds[4] = {1, 2, 3, 5};
  for (uint64_t s : seeds) random_run(s, 3000);
  REQUIRE(outstanding == 0);
  bool enough = true;
  for (int k = 0; k < N_KINDS; k++) {
    printf("%-20s %6ld\n", kind_name[k], done[k]);
    enough = enough && done[k] >= (k == RELEASE_ALL ? 20 : 100);
  }
  if (!enough) { fprintf(stderr, "dev_mem_check: the random run was vacuous (every kind 100 times, release_all 20 times)\n"); return 1; }
  printf("dev_mem_check: ok\n");
  return 0;
}
