// row_snapshot_check.cpp — the CPU audit of tinygpt_amd/csrc/row_snapshot.h (built and run by tests/test_row_snapshot_format.py under the address and
// undefined-behaviour sanitizers).  Five parts: the size formula against a naive per-layer, per-head sum on the released geometries (one of them beyond 2^32 bytes);
// a header round trip (and drop_logits); every proper prefix of a valid small snapshot is refused; every single-field corruption the header of include/tgx.h lists is refused with the
// status it states; 10,000 random byte strings and 10,000 random mutations of a valid snapshot are never accepted unless every section is consistent.  Every buffer
// handed to validate() is a heap block of exactly `bytes` bytes: a read outside it is an AddressSanitizer report.
#include "../tinygpt_amd/csrc/row_snapshot.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace row_snapshot;

#define REQUIRE(cond)                                                                                   \
  do {                                                                                                  \
    if (!(cond)) { fprintf(stderr, "row_snapshot_check: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// validate() on a heap copy of exactly n bytes
static Verdict check(const std::vector<unsigned char>& b, size_t n, const Geometry& g, int64_t max_ctx, Layout* l = nullptr, int32_t* tok = nullptr) {
  unsigned char* p = static_cast<unsigned char*>(malloc(n ? n : 1));
  REQUIRE(p != nullptr);
  if (n) memcpy(p, b.data(), n);
  const char* why = nullptr;
  const Verdict v = validate(p, (int64_t)n, g, max_ctx, l, tok, &why);
  REQUIRE((v == OK) == (why == nullptr));
  free(p);
  return v;
}

// the section sizes summed the long way round
static void naive(const Geometry& g, int64_t past, bool logits, uint64_t* state, uint64_t* kv) {
  const uint64_t esz = g.compute_dtype == 0 ? 4 : 2;
  uint64_t n = 0;
  for (int l = 0; l < g.layers; l++)
    for (int which = 0; which < 2; which++)
      for (int h = 0; h < g.kv_heads; h++) n += (uint64_t)past * (uint64_t)g.head_dim * esz;
  *kv = n;
  uint64_t s = 4 + 4;
  if (logits) { for (int i = 0; i < g.hidden; i++) s += 4; for (int i = 0; i < g.vocab; i++) s += 4; }
  *state = s;
}

static std::vector<unsigned char> make(const Geometry& g, int64_t past, uint32_t flags, uint32_t tok) {
  const Layout l = layout(g, past, flags);
  std::vector<unsigned char> b((size_t)l.total);
  for (auto& x : b) x = (unsigned char)rnd();
  write_header(b.data(), g, l);
  put32(b.data() + l.state_off, (uint32_t)past); put32(b.data() + l.state_off + 4, tok);
  return b;
}

// is an accepted blob consistent?  every section where the geometry and its own past put it, the words behind the header what they must be
static void require_consistent(const std::vector<unsigned char>& b, size_t n, const Geometry& g, int64_t max_ctx, const Layout& l, int32_t tok) {
  uint64_t state, kv;
  REQUIRE(l.past >= 1 && l.past <= max_ctx);
  naive(g, l.past, (l.flags & FLAG_LOGITS) != 0, &state, &kv);
  REQUIRE(l.state_off == 128 && l.state_bytes == state && l.kv_off % 16 == 0 && l.kv_off >= 128 + state && l.kv_off < 128 + state + 16 && l.kv_bytes == kv);
  REQUIRE(l.total == n && l.kv_off + l.kv_bytes == n);
  REQUIRE(memcmp(b.data(), "TGXSNAP\0", 8) == 0 && get32(b.data() + 8) == 1 && get32(b.data() + 12) == 128 && get64(b.data() + 16) == n);
  REQUIRE(get64(b.data() + 72) == l.state_off && get64(b.data() + 80) == l.state_bytes && get64(b.data() + 88) == l.kv_off && get64(b.data() + 96) == l.kv_bytes);
  REQUIRE((int64_t)get64(b.data() + 64) == l.past && get32(b.data() + 60) == l.flags && l.flags <= 3 && l.flags != FLAG_TOKEN);
  REQUIRE((int64_t)get32(b.data() + 128) == l.past && (int32_t)get32(b.data() + 132) == tok);
  if (l.flags & FLAG_TOKEN) REQUIRE(tok >= 0 && tok < g.vocab);
  const int32_t w[9] = {g.family, g.hidden, g.layers, g.heads, g.kv_heads, g.head_dim, g.vocab, g.compute_dtype, g.qk_norm};
  for (int i = 0; i < 9; i++) REQUIRE((int32_t)get32(b.data() + 24 + 4 * i) == w[i]);
}

int main() {
  // ---- 1. the size formula on the released geometries: family, hidden, layers, heads, kv_heads, head_dim, vocab, dtype, qk_norm
  const Geometry released[] = {
      {2, 2048, 16, 32, 8, 64, 128256, 1, 0},      // Llama-3.2-1B bf16: 32 KiB per token
      {5, 4096, 32, 32, 8, 128, 32768, 2, 0},      // Mistral-7B-v0.3 fp16
      {4, 2048, 28, 16, 8, 128, 151936, 1, 1},     // Qwen3-1.7B bf16
      {3, 896, 24, 14, 2, 64, 151936, 1, 0},       // Qwen2.5-0.5B bf16
      {1, 768, 12, 12, 12, 64, 50257, 0, 0},       // GPT-2 fp32
      {2, 8192, 80, 64, 8, 128, 128256, 1, 0},     // the 70B geometry: 320 KiB per token
  };
  bool beyond32 = false;
  for (const Geometry& g : released)
    for (int64_t past : {1ll, 5ll, 128ll, 2048ll, 16384ll, 131072ll})
      for (uint32_t flags : {0u, 1u, 3u}) {
        uint64_t state, kv;
        naive(g, past, flags & 1, &state, &kv);
        const Layout l = layout(g, past, flags);
        REQUIRE(l.state_off == 128 && l.state_bytes == state && l.kv_bytes == kv && l.kv_off == ((128 + state + 15) / 16) * 16 && l.total == l.kv_off + kv);
        REQUIRE(layer_bytes(g, past) * (uint64_t)g.layers == kv);
        beyond32 = beyond32 || l.total > (1ull << 32);
      }
  REQUIRE(beyond32);
  REQUIRE(layout(released[0], 2048, 0).kv_bytes == 64ull << 20);      // 64 MiB at 2048 tokens of Llama-3.2-1B
  REQUIRE(layout(released[5], 16384, 0).kv_bytes == 5ull << 30);      // 5 GiB: past x layers x ... in 32 bits would wrap

  // ---- 2. a header round trip
  const Geometry g = {2, 8, 2, 2, 1, 4, 16, 1, 0}, other_hd = {2, 8, 2, 2, 1, 8, 16, 1, 0}, other_vocab = {2, 8, 2, 2, 1, 4, 8, 1, 0};
  const int64_t MAXC = 64;
  for (uint32_t flags : {0u, 1u, 3u})
    for (int64_t past : {1ll, 3ll, 64ll}) {
      const std::vector<unsigned char> b = make(g, past, flags, flags & 2 ? 15u : 0u);
      Layout l; int32_t tok = -1;
      REQUIRE(check(b, b.size(), g, MAXC, &l, &tok) == OK);
      require_consistent(b, b.size(), g, MAXC, l, tok);
      REQUIRE(l.past == past && l.flags == flags);
    }

  // ... and drop_logits: a snapshot with logits and a token becomes, in place, the prefix-only snapshot of the same positions with the same KV bytes
  for (int64_t past : {1ll, 3ll, 64ll}) {
    std::vector<unsigned char> b = make(g, past, 3, 9);
    const Layout was = layout(g, past, 3);
    const std::vector<unsigned char> kv(b.begin() + (long)was.kv_off, b.end());
    const Layout now = drop_logits(b.data(), g, was);
    Layout l; int32_t tok = -1;
    REQUIRE(now.flags == 0 && now.total < was.total && check(b, (size_t)now.total, g, MAXC, &l, &tok) == OK && tok == 0);
    require_consistent(b, (size_t)now.total, g, MAXC, l, tok);
    REQUIRE(l.kv_bytes == kv.size() && memcmp(b.data() + l.kv_off, kv.data(), kv.size()) == 0);
    REQUIRE(drop_logits(b.data(), g, now).total == now.total);      // nothing left to drop
  }

  // ---- 3. every proper prefix of a valid snapshot (and one byte more than it) is refused
  const std::vector<unsigned char> valid = make(g, 3, 3, 7);
  for (size_t n = 0; n < valid.size(); n++) REQUIRE(check(valid, n, g, MAXC) == INVALID);
  { std::vector<unsigned char> b = valid; b.push_back(0); REQUIRE(check(b, b.size(), g, MAXC) == INVALID); }

  // ---- 4. the single-field corruptions
  auto corrupt = [&](size_t off, int width, uint64_t value, Verdict want) {
    std::vector<unsigned char> b = valid;
    if (width == 4) put32(b.data() + off, (uint32_t)value); else if (width == 8) put64(b.data() + off, value); else b[off] = (unsigned char)value;
    REQUIRE(check(b, b.size(), g, MAXC) == want);
  };
  const Layout lv = layout(g, 3, 3);
  corrupt(0, 1, 'X', INVALID); corrupt(7, 1, 1, INVALID);            // magic
  corrupt(O_VERSION, 4, 2, INVALID); corrupt(O_VERSION, 4, 0, INVALID);
  corrupt(O_HEADER, 4, 64, INVALID);
  corrupt(O_TOTAL, 8, lv.total - 1, INVALID); corrupt(O_TOTAL, 8, lv.total + 1, INVALID);
  for (int i = 0; i < 9; i++) corrupt(O_GEOM + 4 * (size_t)i, 4, get32(valid.data() + O_GEOM + 4 * i) + 1, INVALID);      // every geometry word
  corrupt(O_FLAGS, 4, 2, INVALID);                                   // a token without logits
  corrupt(O_FLAGS, 4, 7, INVALID); corrupt(O_FLAGS, 4, 0, INVALID);  // an unknown bit; no logits in a blob sized for them
  corrupt(O_PAST, 8, 4, INVALID); corrupt(O_PAST, 8, 0, INVALID); corrupt(O_PAST, 8, ~0ull, INVALID);
  corrupt(O_PAST, 8, MAXC + 1, CONTEXT);                             // more positions than the context holds
  corrupt(O_STATE_OFF, 8, 144, INVALID); corrupt(O_STATE_BYTES, 8, lv.state_bytes + 4, INVALID);
  corrupt(O_KV_OFF, 8, lv.kv_off + 16, INVALID); corrupt(O_KV_BYTES, 8, lv.kv_bytes - 16, INVALID);
  corrupt(O_ZEROS, 1, 1, INVALID); corrupt(127, 1, 1, INVALID);
  corrupt(lv.state_off, 4, 2, INVALID);                              // the position word
  corrupt(lv.state_off + 4, 4, 16, INVALID);                         // the token word == vocab
  corrupt(lv.state_off + 4, 4, 0xFFFFFFFFu, INVALID);
  REQUIRE(check(valid, valid.size(), other_hd, MAXC) == INVALID);    // a context of the other head_dim, of another vocabulary
  REQUIRE(check(valid, valid.size(), other_vocab, MAXC) == INVALID);
  REQUIRE(check(valid, valid.size(), g, 2) == CONTEXT);              // a smaller context
  REQUIRE(check(valid, valid.size(), g, 3) == OK);
  REQUIRE(validate(nullptr, 1000, g, MAXC, nullptr, nullptr, nullptr) == INVALID);

  // ---- 5. random byte strings; random mutations of a valid snapshot.  Never a read outside the buffer (the sanitizer), never accepted unless consistent
  int accepted = 0;
  for (int it = 0; it < 10000; it++) {
    std::vector<unsigned char> b((size_t)(rnd() % 400));
    for (auto& x : b) x = (unsigned char)rnd();
    if (it % 2 && b.size() >= 24) { memcpy(b.data(), valid.data(), 24); put64(b.data() + O_TOTAL, b.size()); }      // past the first gates
    if (it % 4 == 3 && b.size() >= 60) memcpy(b.data() + O_GEOM, valid.data() + O_GEOM, 36);
    Layout l; int32_t tok = 0;
    if (check(b, b.size(), g, MAXC, &l, &tok) == OK) { accepted++; require_consistent(b, b.size(), g, MAXC, l, tok); }
  }
  for (int it = 0; it < 10000; it++) {
    std::vector<unsigned char> b = valid;
    const int n_mut = 1 + (int)(rnd() % 3);
    for (int k = 0; k < n_mut; k++) {
      const size_t at = (size_t)(rnd() % (lv.state_off + 8));      // the header and the two state words
      if (rnd() % 2) b[at] ^= (unsigned char)(1u << (rnd() % 8)); else b[at] = (unsigned char)rnd();
    }
    if (rnd() % 8 == 0) b.resize((size_t)(rnd() % (b.size() + 32)), 0);
    Layout l; int32_t tok = 0;
    if (check(b, b.size(), g, MAXC, &l, &tok) == OK) { accepted++; require_consistent(b, b.size(), g, MAXC, l, tok); }
  }
  printf("row_snapshot_check: ok (%d of 20000 random blobs were consistent snapshots)\n", accepted);
  return 0;
}
