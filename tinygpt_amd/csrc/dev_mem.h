// dev_mem.h — the owner of a context's device allocations: every buffer is handed out by alloc / grow and recorded (pointer, bytes), so that destroying the context
// needs no list of names (release_all) and "grow a workspace" is written once.  Host-only — the standard library alone, no HIP: ctx.h binds it to hipMalloc /
// hipFree, tests/dev_mem_check.cpp drives it on a CPU with malloc / free.  No sub-allocation, no pooling: one alloc is one call of the bound allocator.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

class DevMem {
 public:
  typedef void* (*AllocFn)(size_t); typedef void (*FreeFn)(void*);      // AllocFn: nullptr = the allocation failed
  DevMem(AllocFn a, FreeFn f) : alloc_fn(a), free_fn(f) {}
  DevMem(const DevMem&) = delete; DevMem& operator=(const DevMem&) = delete;      // (a copy would free everything twice)
  void* alloc(size_t bytes) {      // nullptr on failure, and nothing recorded
    void* p = alloc_fn(bytes);
    if (p) recs.push_back({p, bytes});
    return p;
  }
  // frees and forgets; nullptr is a no-op.  A pointer that is not a live allocation of this owner would be a double free on the device: the process stops there
  // (the library is built with NDEBUG, so the check is spelled out)
  void release(void* p) {
    if (!p) return;
    size_t i = recs.size();
    while (i > 0 && recs[i - 1].p != p) i--;
    if (i == 0) { fprintf(stderr, "tgx: device memory invariant violated (release of a pointer that is not a live allocation) at %s:%d\n", __FILE__, __LINE__); abort(); }
    recs.erase(recs.begin() + (long)(i - 1));
    free_fn(p);
  }
  // the buffer *p of *have bytes holds `need` bytes after this: nothing happens at need <= *have; else the old buffer is released BEFORE the new one is requested
  // (the two never coexist) and its contents are gone.  false: the allocation failed, *p == nullptr and *have == 0
  bool grow(void** p, size_t* have, size_t need) {
    if (need <= *have) return true;
    release(*p);
    *p = alloc(need);
    *have = *p ? need : 0;
    return *p != nullptr;
  }
  void release_all() {      // newest first
    for (size_t i = recs.size(); i > 0; i--) free_fn(recs[i - 1].p);
    recs.clear();
  }
  size_t live() const { return recs.size(); }
  size_t live_bytes() const { size_t n = 0; for (const Rec& r : recs) n += r.bytes; return n; }

 private:
  struct Rec { void* p; size_t bytes; };
  AllocFn alloc_fn; FreeFn free_fn;
  std::vector<Rec> recs;      // live allocations in the order they were made (a context holds a few hundred; release searches from the newest)
};
