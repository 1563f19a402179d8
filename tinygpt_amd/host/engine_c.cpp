// engine_c.cpp — a C view of the host engine so that tests (ctypes) and other hosts can drive it.
#include <cstring>

#include "../csrc/automaton.h"
#include "constraint.h"
#include "engine.h"
#include "tokenizer.h"

#define TGXE_API extern "C" __attribute__((visibility("default")))

using tgxh::GPTEngine;

struct tgxe_engine {
  GPTEngine* e = nullptr;
  std::string err;
  tgxh::GPTOutput last;      // the log-probability lists of the last generate call (tgxe_last_logprobs)
};
static void keep_logprobs(tgxe_engine* h, tgxh::GPTOutput& r) {
  h->last = tgxh::GPTOutput();
  h->last.topLogprobs = r.topLogprobs;
  h->last.logprobs = std::move(r.logprobs); h->last.topIds = std::move(r.topIds); h->last.topLogprobValues = std::move(r.topLogprobValues);
  h->last.beamScores = r.beamScores;
}

TGXE_API tgxe_engine* tgxe_create2(const char* model_dir, const char* synthetic, const char* device, const char* backend_lib,
                                   const char* prefix, int device_ordinal, int dtype, int max_batch, const char* tokenizer_dir);
TGXE_API tgxe_engine* tgxe_create3(const char* model_dir, const char* synthetic, const char* device, const char* backend_lib,
                                   const char* prefix, int device_ordinal, int dtype, int max_batch, const char* tokenizer_dir, int weights_fp8);
TGXE_API tgxe_engine* tgxe_create(const char* model_dir, const char* synthetic, const char* device, const char* backend_lib,
                                  const char* prefix, int device_ordinal, int dtype, int max_batch) {
  return tgxe_create2(model_dir, synthetic, device, backend_lib, prefix, device_ordinal, dtype, max_batch, nullptr);
}
TGXE_API tgxe_engine* tgxe_create2(const char* model_dir, const char* synthetic, const char* device, const char* backend_lib,
                                   const char* prefix, int device_ordinal, int dtype, int max_batch, const char* tokenizer_dir) {
  return tgxe_create3(model_dir, synthetic, device, backend_lib, prefix, device_ordinal, dtype, max_batch, tokenizer_dir, 0);
}
// ... and GPTConfig::weightsFp8 (FP8 weights, include/tgx.h option "weights.fp8"): fixed at creation like the dtype — tgxe_prepare quantizes or fails
TGXE_API tgxe_engine* tgxe_create3(const char* model_dir, const char* synthetic, const char* device, const char* backend_lib,
                                   const char* prefix, int device_ordinal, int dtype, int max_batch, const char* tokenizer_dir, int weights_fp8) {
  tgxh::GPTConfig c;
  c.modelDir = model_dir ? model_dir : "";
  c.synthetic = synthetic ? synthetic : "";
  c.device = device ? device : "mi355x";
#ifdef TGXH_TEST_HOOKS
  c.backendLib = backend_lib ? backend_lib : "";
  if (prefix && *prefix) c.backendPrefix = prefix;
#else
  (void)prefix;
  if (backend_lib && *backend_lib) return nullptr;     // the shipped library binds libtgx_mi355x.so only
#endif
  c.deviceOrdinal = device_ordinal;
  c.dtype = dtype;
  c.weightsFp8 = weights_fp8 != 0;
  c.maxBatch = max_batch;
  if (tokenizer_dir) c.tokenizerDir = tokenizer_dir;
  auto* h = new tgxe_engine();
  h->e = new GPTEngine(c);
  return h;
}
TGXE_API void tgxe_destroy(tgxe_engine* h) { if (h) { delete h->e; delete h; } }
TGXE_API int tgxe_prepare(tgxe_engine* h) { return h && h->e->prepare() ? 0 : 1; }
TGXE_API const char* tgxe_last_error(tgxe_engine* h) { return h ? h->e->lastError().c_str() : "null engine"; }
TGXE_API int64_t tgxe_context_size(tgxe_engine* h) { return h ? h->e->contextSize() : -1; }
TGXE_API int tgxe_eos_ids(tgxe_engine* h, int32_t* out, int cap) {
  const auto& v = h->e->eosTokenIds();
  for (int i = 0; i < (int)v.size() && i < cap; i++) out[i] = v[(size_t)i];
  return (int)v.size();
}
// prefix reuse (GPTConfig::reusePrefix): generateAsync keeps row 0's KV cache between calls; tgxe_last_reused = the prompt tokens the last call served from it
TGXE_API void tgxe_set_reuse_prefix(tgxe_engine* h, int on) { if (h) h->e->setReusePrefix(on != 0); }
TGXE_API int64_t tgxe_last_reused(tgxe_engine* h) { return h ? h->e->lastReused() : -1; }
// session files (GPTEngine::saveSession / loadSession): row 0's conversation kept across processes; 0 = done, 1 = refused (tgxe_last_error says why)
TGXE_API int tgxe_save_session(tgxe_engine* h, const char* path) { return h && path && h->e->saveSession(path) ? 0 : 1; }
TGXE_API int tgxe_load_session(tgxe_engine* h, const char* path) { return h && path && h->e->loadSession(path) ? 0 : 1; }
// generation past the context (GPTConfig::contextShift / shiftKeep; off by default); tgxe_last_shifts = the shifts the last generate call made, over all its rows
TGXE_API void tgxe_set_context_shift(tgxe_engine* h, int on, int keep) { if (h) h->e->setContextShift(on != 0, keep); }
TGXE_API int64_t tgxe_last_shifts(tgxe_engine* h) { return h ? h->e->lastShifts() : 0; }
// greedy speculative decoding (GPTConfig::speculate): the maximum draft length (0 = off); tgxe_spec_stats writes {verify calls, draft tokens, accepted draft
// tokens, ordinary steps, produced-per-verify histogram [0 .. TGX_MAX_DRAFT + 1]} (up to cap values) and returns how many there are
TGXE_API void tgxe_set_speculate(tgxe_engine* h, int max_draft) { if (h) h->e->setSpeculate(max_draft); }
// ... under a sampling configuration as well (GPTConfig::speculateSampled; 0 = off, the default)
TGXE_API void tgxe_set_speculate_sampled(tgxe_engine* h, int on) { if (h) h->e->setSpeculateSampled(on != 0); }
// ... with penalties, a logit bias or a regex on (GPTConfig::speculateProcessed; 0 = off, the default)
TGXE_API void tgxe_set_speculate_processed(tgxe_engine* h, int on) { if (h) h->e->setSpeculateProcessed(on != 0); }
// ... with token trees (GPTConfig::speculateTree: branches, 0 = off, the default); tgxe_spec_tree_passes = how many of the verify passes ran a tree of two or more branches
TGXE_API void tgxe_set_speculate_tree(tgxe_engine* h, int branches) { if (h) h->e->setSpeculateTree(branches); }
TGXE_API int64_t tgxe_spec_tree_passes(tgxe_engine* h) { return h ? h->e->specStats().treePasses : 0; }
// the engine's device context (GPTEngine::ctx): for the diagnostic calls of include/tgx.h (tgx_read_pass_logits, tgx_read_kv) on what the engine just ran
TGXE_API void* tgxe_ctx(tgxe_engine* h) { return h ? (void*)h->e->ctx() : nullptr; }
TGXE_API int tgxe_spec_stats(tgxe_engine* h, int64_t* out, int cap) {
  const tgxh::SpecStats& s = h->e->specStats();
  const int n_hist = (int)(sizeof s.producedHist / sizeof s.producedHist[0]);
  const int64_t head[4] = {s.verifyCalls, s.draftTokens, s.acceptedDrafts, s.plainSteps};
  for (int i = 0; i < 4 + n_hist && i < cap; i++) out[i] = i < 4 ? head[i] : s.producedHist[i - 4];
  return 4 + n_hist;
}
// the drafter alone (spec_draft.h): the proposal for the sequence ids[0 .. n), at most max_draft tokens into out; returns their number
TGXE_API int tgxh_ngram_draft(const int32_t* ids, int n, int max_draft, int32_t* out) {
  const std::vector<int32_t> d = tgxh::ngram_draft(std::vector<int32_t>(ids, ids + (ids && n > 0 ? n : 0)), max_draft);
  for (size_t i = 0; i < d.size(); i++) out[i] = d[i];
  return (int)d.size();
}
// ... and the tree drafter (spec_draft.h ngram_tree): tokens / parents of at most max_nodes nodes into the two arrays; returns the node count, *out_branches the chains
TGXE_API int tgxh_ngram_tree(const int32_t* ids, int n, int max_nodes, int max_branches, int32_t* out_tokens, int32_t* out_parent, int32_t* out_branches) {
  const tgxh::DraftTree t = tgxh::ngram_tree(std::vector<int32_t>(ids, ids + (ids && n > 0 ? n : 0)), max_nodes, max_branches);
  for (size_t i = 0; i < t.tokens.size(); i++) { out_tokens[i] = t.tokens[i]; out_parent[i] = t.parent[i]; }
  if (out_branches) *out_branches = t.branches;
  return (int)t.tokens.size();
}
// per-token log-probabilities (GPTConfig::logprobs): top_n = -1 off, 0 .. TGX_MAX_LOGPROBS.  tgxe_last_logprobs copies what the last generate call recorded —
// out_lp [batch * new tokens], out_top_ids / out_top_lp [batch * new tokens * top_n] (either may be NULL), up to cap tokens — and returns the number of tokens
// recorded; *out_top_n = the top_n of that call
TGXE_API void tgxe_set_logprobs(tgxe_engine* h, int top_n) { if (h) h->e->setLogprobs(top_n); }
TGXE_API int64_t tgxe_last_logprobs(tgxe_engine* h, float* out_lp, int32_t* out_top_ids, float* out_top_lp, int64_t cap, int* out_top_n) {
  const tgxh::GPTOutput& r = h->last;
  const int64_t n = (int64_t)r.logprobs.size(), k = r.topLogprobs;
  if (out_top_n) *out_top_n = r.topLogprobs;
  for (int64_t i = 0; i < n && i < cap; i++) {
    if (out_lp) out_lp[i] = r.logprobs[(size_t)i];
    for (int64_t j = 0; j < k; j++) {
      if (out_top_ids) out_top_ids[i * k + j] = r.topIds[(size_t)(i * k + j)];
      if (out_top_lp) out_top_lp[i * k + j] = r.topLogprobValues[(size_t)(i * k + j)];
    }
  }
  return n;
}
// scoring a supplied sequence (GPTEngine::score; include/tgx.h tgx_score_row): out_lp [n - 1], out_top_ids / out_top_lp [n - 1][top_n] (either may be NULL).
// Returns 0, or 1 when the call failed (tgxe_last_error); the text form also reports the ids it scored (up to cap) and their number
TGXE_API int tgxe_score(tgxe_engine* h, const int32_t* ids, int n, int top_n, float* out_lp, int32_t* out_top_ids, float* out_top_lp) {
  const tgxh::ScoreOutput r = h->e->score(std::vector<int32_t>(ids, ids + (ids && n > 0 ? n : 0)), top_n);
  if (!r.ok) return 1;
  if (out_lp) memcpy(out_lp, r.logprobs.data(), r.logprobs.size() * 4);
  if (out_top_ids) memcpy(out_top_ids, r.topIds.data(), r.topIds.size() * 4);
  if (out_top_lp) memcpy(out_top_lp, r.topLogprobValues.data(), r.topLogprobValues.size() * 4);
  return 0;
}
TGXE_API int tgxe_score_text(tgxe_engine* h, const char* text, int top_n, int32_t* out_ids, int64_t cap, int64_t* out_n, float* out_lp, int32_t* out_top_ids, float* out_top_lp) {
  const tgxh::ScoreOutput r = h->e->score(std::string(text ? text : ""), top_n);
  if (!r.ok) return 1;
  if (out_n) *out_n = (int64_t)r.tokenIds.size();
  if ((int64_t)r.tokenIds.size() > cap) return 2;
  if (out_ids) memcpy(out_ids, r.tokenIds.data(), r.tokenIds.size() * 4);
  if (out_lp) memcpy(out_lp, r.logprobs.data(), r.logprobs.size() * 4);
  if (out_top_ids) memcpy(out_top_ids, r.topIds.data(), r.topIds.size() * 4);
  if (out_top_lp) memcpy(out_top_lp, r.topLogprobValues.data(), r.topLogprobValues.size() * 4);
  return 0;
}
// embeddings (GPTEngine::embed; include/tgx.h tgx_embed_rows): n texts, their ids back to back with lens[i] each; out [n][dims ? dims : hidden].  pool: TGX_POOL_*.
// Returns 0, or 1 when the call failed (tgxe_last_error); out_calls (may be NULL): the tgx_embed_rows calls the texts were batched into
TGXE_API int tgxe_embed(tgxe_engine* h, int n, const int32_t* ids, const int32_t* lens, int pool, int normalize, int dims, float* out, int64_t* out_calls) {
  if (!h || !ids || !lens || !out || n < 1) return 1;
  std::vector<std::vector<int32_t>> texts;
  for (int i = 0; i < n; i++) {
    const int len = lens[i] > 0 ? lens[i] : 0;
    texts.emplace_back(ids, ids + len);
    ids += len;
  }
  tgxh::EmbedConfig cfg;
  cfg.pool = pool; cfg.normalize = normalize != 0; cfg.dims = dims;
  const tgxh::EmbedOutput r = h->e->embed(texts, cfg);
  if (!r.ok) return 1;
  memcpy(out, r.vectors.data(), r.vectors.size() * 4);
  if (out_calls) *out_calls = r.calls;
  return 0;
}
// SamplerConfig's penalties and logit bias (neutral: 1, 0, 0 and n = 0); kept across tgxe_reconfigure until set again
TGXE_API void tgxe_set_processors(tgxe_engine* h, float repetition, float presence, float frequency, const int32_t* bias_ids, const float* bias, int n) {
  if (!h) return;
  std::map<int32_t, float> m;
  for (int i = 0; bias_ids && bias && i < n; i++) m[bias_ids[i]] = bias[i];
  h->e->setProcessors(repetition, presence, frequency, std::move(m));
}
// SamplerConfig::regex (constrained decoding; empty or NULL: off); kept across tgxe_reconfigure until set again
TGXE_API void tgxe_set_regex(tgxe_engine* h, const char* pattern) { if (h) h->e->setRegex(pattern ? pattern : ""); }
// beam search (GPTConfig::numBeams / lengthPenalty / earlyStopping / numReturn; num_beams 1 = off); kept across tgxe_reconfigure until set again.  A beam call of
// tgxe_generate_sync takes ONE prompt and writes num_return rows: out_ids needs num_return * (prompt + max_new) entries.  tgxe_last_beam_scores copies the rows'
// scores of the last tgxe_generate_sync call, best first (up to cap), and returns how many there are
TGXE_API void tgxe_set_beams(tgxe_engine* h, int num_beams, float length_penalty, int early_stopping, int num_return) {
  if (h) h->e->setBeams(num_beams, length_penalty, early_stopping != 0, num_return);
}
TGXE_API int tgxe_last_beam_scores(tgxe_engine* h, double* out, int cap) {
  if (!h) return 0;
  for (int i = 0; out && i < (int)h->last.beamScores.size() && i < cap; i++) out[i] = h->last.beamScores[(size_t)i];
  return (int)h->last.beamScores.size();
}
TGXE_API void tgxe_reconfigure(tgxe_engine* h, float temperature, int64_t top_k, float top_p, float min_p, int64_t max_new,
                               const int32_t* extra_stop, int n_extra) {
  tgxh::SamplerConfig s = h->e->samplerConfig();      // (the penalties / logit bias of tgxe_set_processors stay)
  s.temperature = temperature; s.topK = top_k; s.topP = top_p; s.minP = min_p;
  std::vector<int32_t> ex(extra_stop, extra_stop + (extra_stop ? n_extra : 0));
  h->e->reconfigure(s, max_new, ex);
}
// prompts: flat ids + per-row lengths.  out_ids capacity must be >= batch * (min(maxlen, ctx) + max_new).
TGXE_API int tgxe_generate_sync(tgxe_engine* h, const int32_t* flat, const int32_t* lens, int batch, int32_t pad,
                                int32_t* out_ids, int64_t cap, int64_t* out_n, int64_t* out_new, int* out_finish) {
  std::vector<std::vector<int32_t>> p((size_t)batch);
  size_t o = 0;
  for (int b = 0; b < batch; b++) { p[(size_t)b].assign(flat + o, flat + o + lens[b]); o += (size_t)lens[b]; }
  tgxh::GPTOutput r = h->e->generateSync(p, pad);
  keep_logprobs(h, r);
  if (r.batch == 0) return 1;
  if ((int64_t)r.tokenIds.size() > cap) return 2;
  memcpy(out_ids, r.tokenIds.data(), r.tokenIds.size() * 4);
  *out_n = (int64_t)r.tokenIds.size(); *out_new = r.newTokens; *out_finish = r.finishReason == tgxh::FinishReason::Stop ? 0 : 1;
  return 0;
}
typedef int (*tgxe_token_cb)(int32_t token, void* user);
TGXE_API int tgxe_generate_async(tgxe_engine* h, const int32_t* ids, int len, tgxe_token_cb cb, void* user,
                                 int32_t* out_ids, int64_t cap, int64_t* out_n, int64_t* out_new, int* out_finish) {
  std::vector<int32_t> p(ids, ids + len);
  tgxh::GPTOutput r = h->e->generateAsync(p, [&](int32_t t) { return cb ? cb(t, user) != 0 : true; });
  keep_logprobs(h, r);
  if (r.batch == 0) return 1;
  if ((int64_t)r.tokenIds.size() > cap) return 2;
  memcpy(out_ids, r.tokenIds.data(), r.tokenIds.size() * 4);
  *out_n = (int64_t)r.tokenIds.size(); *out_new = r.newTokens; *out_finish = r.finishReason == tgxh::FinishReason::Stop ? 0 : 1;
  return 0;
}
// text entry points.  texts: `batch` NUL-terminated UTF-8 strings.  out_text receives the decoded new tokens of every row joined
// by '\x1e' (record separator); out_ids as in tgxe_generate_sync.
TGXE_API int tgxe_generate_sync_text(tgxe_engine* h, const char* const* texts, int batch, int32_t* out_ids, int64_t cap, int64_t* out_n,
                                     int64_t* out_new, char* out_text, int64_t text_cap, int64_t* out_text_len) {
  std::vector<std::string> t;
  for (int b = 0; b < batch; b++) t.emplace_back(texts[b]);
  tgxh::GPTOutput r = h->e->generateSync(t);
  h->last.beamScores = r.beamScores;      // (tgxe_last_beam_scores; the log-probability lists of an earlier call stay as they were)
  if (r.batch == 0) return 1;
  if ((int64_t)r.tokenIds.size() > cap) return 2;
  memcpy(out_ids, r.tokenIds.data(), r.tokenIds.size() * 4);
  *out_n = (int64_t)r.tokenIds.size(); *out_new = r.newTokens;
  std::string joined;
  for (size_t b = 0; b < r.texts.size(); b++) { if (b) joined += '\x1e'; joined += r.texts[b]; }
  *out_text_len = (int64_t)joined.size();
  if ((int64_t)joined.size() > text_cap) return 2;
  memcpy(out_text, joined.data(), joined.size());
  return 0;
}
typedef int (*tgxe_text_cb)(const char* chunk, int64_t len, void* user);
TGXE_API int tgxe_generate_async_text(tgxe_engine* h, const char* text, tgxe_text_cb cb, void* user, int32_t* out_ids, int64_t cap,
                                      int64_t* out_n, int64_t* out_new, int* out_finish) {
  tgxh::GPTOutput r = h->e->generateAsync(std::string(text), [&](const std::string& c) { return cb ? cb(c.data(), (int64_t)c.size(), user) != 0 : true; });
  if (r.batch == 0) return 1;
  if ((int64_t)r.tokenIds.size() > cap) return 2;
  memcpy(out_ids, r.tokenIds.data(), r.tokenIds.size() * 4);
  *out_n = (int64_t)r.tokenIds.size(); *out_new = r.newTokens; *out_finish = r.finishReason == tgxh::FinishReason::Stop ? 0 : 1;
  return 0;
}
TGXE_API void tgxe_synth_tensor(uint64_t seed, const char* name, int64_t n, double std_dev, uint16_t* out) {
  tgxh::synth_tensor_bf16(seed, name, (size_t)n, std_dev, out);
}

// ---- tokenizer (tokenizer.h) -----------------------------------------------------------------------------------
struct tgxe_tokenizer {
  tgxh::Tokenizer t;
  std::string scratch;
};
TGXE_API tgxe_tokenizer* tgxe_tok_create(const char* tokenizer_json, const char* tokenizer_config_json, char* err, int err_cap) {
  auto* h = new tgxe_tokenizer();
  if (h->t.initWithConfig(tokenizer_json ? tokenizer_json : "", tokenizer_config_json ? tokenizer_config_json : "")) return h;
  if (err && err_cap > 0) { strncpy(err, h->t.lastError().c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
  delete h;
  return nullptr;
}
TGXE_API void tgxe_tok_destroy(tgxe_tokenizer* h) { delete h; }
// returns the number of ids (written up to cap)
TGXE_API int64_t tgxe_tok_encode(tgxe_tokenizer* h, const char* text, int64_t len, int allow_added, int32_t* out, int64_t cap) {
  const std::vector<int32_t> ids = h->t.encode(std::string(text, (size_t)len), allow_added != 0);
  for (int64_t i = 0; i < (int64_t)ids.size() && i < cap; i++) out[i] = ids[(size_t)i];
  return (int64_t)ids.size();
}
// mode 0: decode(ids); 1: decodeStream(ids); 2: decodeStreamFlush().  Returns the byte length; bytes are copied up to cap.
TGXE_API int64_t tgxe_tok_decode(tgxe_tokenizer* h, const int32_t* ids, int64_t n, int mode, char* out, int64_t cap) {
  const std::vector<int32_t> v(ids, ids + (ids ? n : 0));
  h->scratch = mode == 0 ? h->t.decode(v) : mode == 1 ? h->t.decodeStream(v) : h->t.decodeStreamFlush();
  const int64_t len = (int64_t)h->scratch.size();
  if (out && cap > 0) memcpy(out, h->scratch.data(), (size_t)(len < cap ? len : cap));
  return len;
}
// the bytes produced by the last tgxe_tok_decode call (the stream modes are stateful: read their result from here)
TGXE_API int64_t tgxe_tok_scratch(tgxe_tokenizer* h, char* out, int64_t cap) {
  const int64_t len = (int64_t)h->scratch.size();
  if (out && cap > 0) memcpy(out, h->scratch.data(), (size_t)(len < cap ? len : cap));
  return len;
}
TGXE_API int32_t tgxe_tok_special(tgxe_tokenizer* h, int which) { return which == 0 ? h->t.bosTokenId() : which == 1 ? h->t.eosTokenId() : h->t.padTokenId(); }
TGXE_API int32_t tgxe_tok_token_to_id(tgxe_tokenizer* h, const char* token) { return h->t.token2Id(token ? token : ""); }
// regex matchAll for the pre-tokenizer tests: writes (begin, end) byte offsets, returns the match count or -1 for an invalid pattern
TGXE_API int64_t tgxe_regex_match_all(const char* pattern, const char* text, int64_t len, int64_t* out, int64_t cap_pairs) {
  tgxh::Regex re(pattern);
  if (!re.valid()) return -1;
  std::vector<tgxh::Range> m;
  re.matchAll(std::string(text, (size_t)len), m);
  for (int64_t i = 0; i < (int64_t)m.size() && i < cap_pairs; i++) { out[2 * i] = (int64_t)m[(size_t)i].first; out[2 * i + 1] = (int64_t)m[(size_t)i].second; }
  return (int64_t)m.size();
}

// ---- the pattern compiler (constraint.h) for its tests
// the byte DFA of `pattern` over the string: 1 accepted, 0 not, -1 the pattern did not compile (err says why)
TGXE_API int tgxe_regex_dfa_match(const char* pattern, const char* text, int64_t len, char* err, int err_cap) {
  tgxh::ByteDfa d;
  std::string why;
  if (!tgxh::compileByteDfa(pattern ? pattern : "", d, why)) {
    if (err && err_cap > 0) { strncpy(err, why.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return -1;
  }
  return d.matches(std::string(text ? text : "", (size_t)(text ? len : 0))) ? 1 : 0;
}
// `pattern` compiled over the tokenizer in `tokenizer_dir` into a table `vocab` ids wide (0: the tokenizer's own size), the stop ids allowed in accepting states.
// Returns a handle (tgxe_constraint_info / _copy / _destroy) or NULL with err
struct tgxe_constraint { tgxh::TokenAutomaton a; };
TGXE_API tgxe_constraint* tgxe_constraint_compile(const char* tokenizer_dir, const char* pattern, const int32_t* stop_ids, int n_stop, int32_t vocab, int max_states, char* err, int err_cap) {
  auto refuse = [&](const std::string& why) -> tgxe_constraint* {
    if (err && err_cap > 0) { strncpy(err, why.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return nullptr;
  };
  tgxh::Tokenizer tok;
  const std::string dir = tokenizer_dir ? tokenizer_dir : "";
  if (!tok.initWithConfig(dir + "/tokenizer.json", dir + "/tokenizer_config.json")) return refuse("tokenizer: " + tok.lastError());
  tgxh::ConstraintLimits lim;
  if (max_states > 0) lim.maxStates = max_states;
  auto* h = new tgxe_constraint();
  std::string why;
  const std::vector<int32_t> stops(stop_ids, stop_ids + (stop_ids && n_stop > 0 ? n_stop : 0));
  if (tgxh::compileConstraint(pattern ? pattern : "", tok, vocab > 0 ? vocab : (int32_t)tok.vocabSize(), stops, h->a, why, lim)) return h;
  delete h;
  return refuse(why);
}
TGXE_API void tgxe_constraint_info(const tgxe_constraint* h, int32_t* n_states, int32_t* start, int32_t* vocab) { *n_states = h->a.nStates; *start = h->a.start; *vocab = h->a.vocab; }
TGXE_API void tgxe_constraint_copy(const tgxe_constraint* h, uint16_t* next /* [n_states][vocab] */, uint8_t* accept /* [n_states] */) {
  if (next) memcpy(next, h->a.next.data(), h->a.next.size() * sizeof(uint16_t));
  for (size_t i = 0; accept && i < h->a.accept.size(); i++) accept[i] = h->a.accept[i] ? 1 : 0;
}
TGXE_API void tgxe_constraint_destroy(tgxe_constraint* h) { delete h; }
// the table validation of tgx_automaton_create (csrc/automaton.h): 0 accepted, 1 refused (err says why)
TGXE_API int tgxe_automaton_validate(int32_t n_states, int32_t start, const uint16_t* next, int32_t vocab, char* err, int err_cap) {
  char why[160];
  const bool bad = automaton::validate(n_states, start, next, vocab, why, sizeof(why)) != nullptr;
  if (bad && err && err_cap > 0) { strncpy(err, why, (size_t)err_cap - 1); err[err_cap - 1] = 0; }
  return bad ? 1 : 0;
}

// Unicode normalisation for the normalizer tests: form 0 NFC, 1 NFD, 2 NFKC, 3 NFKD; returns the byte length, copies up to cap
TGXE_API int64_t tgxe_normalize(int form, const char* text, int64_t len, char* out, int64_t cap) {
  const std::string r = tgxh::normalize_unicode(std::string(text, (size_t)len), form == 0 || form == 2, form >= 2);
  if (out && cap > 0) memcpy(out, r.data(), (size_t)((int64_t)r.size() < cap ? (int64_t)r.size() : cap));
  return (int64_t)r.size();
}
