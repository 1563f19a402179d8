// row_snapshot.h — the byte format of a row snapshot (include/tgx.h tgx_save_row / tgx_restore_row): the 128-byte header, the size formula and the validation of a
// blob against a context's geometry.  Host-only — the standard library alone, no HIP: abi.hip uses it for the three entry points, tests/row_snapshot_check.cpp drives
// it on a CPU.  Everything is little-endian and written byte by byte, and every size is 64-bit (past x layers x kv_heads x head_dim overflows 32 bits on the 70B
// geometries).  The layout (include/tgx.h documents it for callers):
//   header   [0, 128)   magic "TGXSNAP\0" | u32 version | u32 header bytes (128) | u64 total bytes | i32 family, hidden, layers, heads, kv_heads, head_dim, vocab,
//                       compute_dtype, qk_norm | u32 flags | i64 past | u64 state offset, state bytes, KV offset, KV bytes | zeros
//   state    at 128     u32 position word | u32 token word | iff flag bit 0: f32 hidden [hidden] | f32 logits [vocab]
//   KV       at the next multiple of 16: [layer][K, V][kv_head][past][head_dim] in the storage dtype
#pragma once
#include <cstdint>
#include <cstring>

namespace row_snapshot {

enum : uint32_t { VERSION = 1, HEADER_BYTES = 128, FLAG_LOGITS = 1, FLAG_TOKEN = 2 };
enum Verdict { OK = 0, INVALID = 1, CONTEXT = 8 };      // the tgx_status a blob earns (TGX_ERR_INVALID, TGX_ERR_CONTEXT)
static const unsigned char MAGIC[8] = {'T', 'G', 'X', 'S', 'N', 'A', 'P', 0};

// byte offsets of the header's fields
enum { O_MAGIC = 0, O_VERSION = 8, O_HEADER = 12, O_TOTAL = 16, O_GEOM = 24, O_FLAGS = 60, O_PAST = 64, O_STATE_OFF = 72, O_STATE_BYTES = 80, O_KV_OFF = 88, O_KV_BYTES = 96, O_ZEROS = 104 };

struct Geometry {      // what must match between the context that saved and the context that restores (the order of the header's nine words)
  int32_t family, hidden, layers, heads, kv_heads, head_dim, vocab, compute_dtype, qk_norm;
  bool operator==(const Geometry& o) const {
    return family == o.family && hidden == o.hidden && layers == o.layers && heads == o.heads && kv_heads == o.kv_heads && head_dim == o.head_dim && vocab == o.vocab &&
           compute_dtype == o.compute_dtype && qk_norm == o.qk_norm;
  }
};

struct Layout {        // the sections of a snapshot of `past` positions
  uint32_t flags = 0;
  int64_t past = 0;
  uint64_t state_off = 0, state_bytes = 0, kv_off = 0, kv_bytes = 0, total = 0;
};

inline uint64_t elem_bytes(int32_t compute_dtype) { return compute_dtype == 0 ? 4u : 2u; }      // tgx_dtype: TGX_F32 = 0, TGX_BF16 = 1, TGX_F16 = 2
// bytes of one layer of the KV section: both caches, every kv head, `past` positions
inline uint64_t layer_bytes(const Geometry& g, int64_t past) { return 2ull * (uint64_t)g.kv_heads * (uint64_t)past * (uint64_t)g.head_dim * elem_bytes(g.compute_dtype); }

inline Layout layout(const Geometry& g, int64_t past, uint32_t flags) {
  Layout l;
  l.flags = flags; l.past = past;
  l.state_off = HEADER_BYTES;
  l.state_bytes = 8 + ((flags & FLAG_LOGITS) ? 4ull * ((uint64_t)g.hidden + (uint64_t)g.vocab) : 0);
  l.kv_off = (l.state_off + l.state_bytes + 15) & ~15ull;
  l.kv_bytes = (uint64_t)g.layers * layer_bytes(g, past);
  l.total = l.kv_off + l.kv_bytes;
  return l;
}

inline void put32(unsigned char* p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (unsigned char)(v >> (8 * i)); }
inline void put64(unsigned char* p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (unsigned char)(v >> (8 * i)); }
inline uint32_t get32(const unsigned char* p) { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i); return v; }
inline uint64_t get64(const unsigned char* p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i); return v; }

// the 128 header bytes of a snapshot laid out as l
inline void write_header(unsigned char* h, const Geometry& g, const Layout& l) {
  memset(h, 0, HEADER_BYTES);
  memcpy(h + O_MAGIC, MAGIC, 8);
  put32(h + O_VERSION, VERSION); put32(h + O_HEADER, HEADER_BYTES); put64(h + O_TOTAL, l.total);
  const int32_t w[9] = {g.family, g.hidden, g.layers, g.heads, g.kv_heads, g.head_dim, g.vocab, g.compute_dtype, g.qk_norm};
  for (int i = 0; i < 9; i++) put32(h + O_GEOM + 4 * i, (uint32_t)w[i]);
  put32(h + O_FLAGS, l.flags); put64(h + O_PAST, (uint64_t)l.past);
  put64(h + O_STATE_OFF, l.state_off); put64(h + O_STATE_BYTES, l.state_bytes); put64(h + O_KV_OFF, l.kv_off); put64(h + O_KV_BYTES, l.kv_bytes);
}

// A valid snapshot laid out as l that holds logits becomes, in place, the "prefix only" snapshot of the same positions (flags 0: what a save of a row without logits
// writes): hidden row, logits and token leave, the KV section moves down behind the two state words.  Returns the new layout; its total is the new byte count
inline Layout drop_logits(unsigned char* buf, const Geometry& g, const Layout& l) {
  if (!(l.flags & FLAG_LOGITS)) return l;
  const Layout nl = layout(g, l.past, 0);
  memmove(buf + nl.kv_off, buf + l.kv_off, (size_t)l.kv_bytes);
  write_header(buf, g, nl);
  put32(buf + nl.state_off + 4, 0);                                                                  // no current token
  memset(buf + nl.state_off + nl.state_bytes, 0, (size_t)(nl.kv_off - nl.state_off - nl.state_bytes));   // the padding in front of the KV section
  return nl;
}

// Is buf[0, bytes) a snapshot that a context of geometry g and context size max_ctx can restore?  Reads nothing outside the buffer, and nothing behind the header
// but the two state words.  OK: *out is its layout and *out_tok its token word.  `why` (may be null) names the first thing that is wrong.
inline Verdict validate(const void* buf, int64_t bytes, const Geometry& g, int64_t max_ctx, Layout* out, int32_t* out_tok, const char** why) {
  const char* dummy; if (!why) why = &dummy;
  const unsigned char* h = static_cast<const unsigned char*>(buf);
  if (!h || bytes < (int64_t)HEADER_BYTES) { *why = "smaller than the header"; return INVALID; }
  if (memcmp(h + O_MAGIC, MAGIC, 8) != 0) { *why = "wrong magic"; return INVALID; }
  if (get32(h + O_VERSION) != VERSION) { *why = "unknown version"; return INVALID; }
  if (get32(h + O_HEADER) != HEADER_BYTES) { *why = "wrong header size"; return INVALID; }
  if (get64(h + O_TOTAL) != (uint64_t)bytes) { *why = "the byte count differs from the header's total"; return INVALID; }
  Geometry f;
  int32_t* w[9] = {&f.family, &f.hidden, &f.layers, &f.heads, &f.kv_heads, &f.head_dim, &f.vocab, &f.compute_dtype, &f.qk_norm};
  for (int i = 0; i < 9; i++) *w[i] = (int32_t)get32(h + O_GEOM + 4 * i);
  if (!(f == g)) { *why = "saved by another geometry (family, hidden, layers, heads, kv_heads, head_dim, vocab, dtype, qk_norm)"; return INVALID; }
  for (int i = O_ZEROS; i < (int)HEADER_BYTES; i++) if (h[i]) { *why = "reserved header bytes are not zero"; return INVALID; }
  const uint32_t flags = get32(h + O_FLAGS);
  if (flags & ~(uint32_t)(FLAG_LOGITS | FLAG_TOKEN)) { *why = "unknown flag bits"; return INVALID; }
  if ((flags & FLAG_TOKEN) && !(flags & FLAG_LOGITS)) { *why = "a current token without logits"; return INVALID; }
  const int64_t past = (int64_t)get64(h + O_PAST);
  if (past < 1) { *why = "past < 1"; return INVALID; }
  if (past > max_ctx) { *why = "more positions than the context size"; return CONTEXT; }      // (max_ctx bounds the products below)
  const Layout l = layout(g, past, flags);
  if (get64(h + O_STATE_OFF) != l.state_off || get64(h + O_STATE_BYTES) != l.state_bytes || get64(h + O_KV_OFF) != l.kv_off || get64(h + O_KV_BYTES) != l.kv_bytes ||
      l.total != (uint64_t)bytes) { *why = "section offsets or sizes do not follow from the geometry and past"; return INVALID; }
  const uint32_t pos = get32(h + l.state_off), tok = get32(h + l.state_off + 4);      // inside the buffer: bytes == total >= state_off + 8
  if ((int64_t)pos != past) { *why = "the position word differs from past"; return INVALID; }
  if ((flags & FLAG_TOKEN) && tok >= (uint32_t)g.vocab) { *why = "the token word is no id of the vocabulary"; return INVALID; }
  if (out) *out = l;
  if (out_tok) *out_tok = (int32_t)tok;
  return OK;
}

}   // namespace row_snapshot
