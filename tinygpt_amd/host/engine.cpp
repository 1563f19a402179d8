#include "engine.h"
#include "../csrc/row_snapshot.h"
#include "spec_mode.h"
#include "beam.h"

#include <chrono>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

namespace tgxh {

namespace {

std::string self_dir() {
  Dl_info info;
  if (dladdr(reinterpret_cast<void*>(&self_dir), &info) && info.dli_fname) {
    std::string p = info.dli_fname;
    size_t k = p.find_last_of('/');
    if (k != std::string::npos) return p.substr(0, k);
  }
  return ".";
}

tgx_sampler_cfg to_c(const SamplerConfig& s) { tgx_sampler_cfg c; c.temperature = s.temperature; c.top_k = s.topK; c.top_p = s.topP; c.min_p = s.minP; return c; }

}  // namespace

GPTEngine::GPTEngine(GPTConfig config) : config_(std::move(config)) {}

GPTEngine::~GPTEngine() {
  if (model_.ctx && be_.destroy) be_.destroy(model_.ctx);
  be_.close();
}

bool GPTEngine::fail(const std::string& what) {
  err_ = what;
  fprintf(stderr, "[tgx] %s\n", what.c_str());
  return false;
}

bool GPTEngine::prepare() {
  // device -> shim.  The reference maps everything that is not "cpu" to CUDA (examples/inference/main.cpp:76-80); here
  // "mi355x" binds the HIP library and any other value is refused — this engine has no CPU execution path of its own.
  std::string lib = self_dir() + "/libtgx_mi355x.so", prefix = "tgx_";
  bool hooked = false;
#ifdef TGXH_TEST_HOOKS
  if (!config_.backendLib.empty()) { hooked = true; lib = config_.backendLib; prefix = config_.backendPrefix; }
#endif
  if (config_.device != "mi355x" && !hooked)
    return fail("device '" + config_.device + "' is not provided by this engine (only --device mi355x); the reference's cpu path lives in TinyTorch");
  if (!be_.open(lib, prefix)) return fail("cannot bind device shim " + lib + ": " + be_.error);

  LoadOptions loadOpts;
  loadOpts.weightsFp8 = config_.weightsFp8;
  if (!config_.synthetic.empty()) {
    if (!known_config(config_.synthetic, config_.dtype, config_.maxBatch, model_.config)) return fail("unknown synthetic config: " + config_.synthetic);
    if (!load_synthetic(be_, model_.config, config_.deviceOrdinal, 1234, 0.02, &model_.ctx, err_, loadOpts)) return fail("Prepare failed: " + err_);
  } else {
    if (!load_model_dir(be_, config_.modelDir, config_.deviceOrdinal, config_.dtype, config_.maxBatch, model_, err_, loadOpts)) return fail("Prepare failed: " + err_);
  }
  // tokenizer: optional for the id entry points, required for the text ones (ModelLoader.cpp:60-69 always loads it)
  const std::string tdir = !config_.tokenizerDir.empty() ? config_.tokenizerDir : config_.modelDir;
  if (!tdir.empty()) {
    const std::string tj = tdir + "/tokenizer.json", tc = tdir + "/tokenizer_config.json";
    if (FILE* f = fopen(tj.c_str(), "rb")) {
      fclose(f);
      if (!tokenizer_.initWithConfig(tj, tc)) return fail("load tokenizer failed: " + tokenizer_.lastError());
      tokenizerOk_ = true;
    } else if (!config_.tokenizerDir.empty()) return fail("Cannot open file: " + tj);
  }
  // EOS ids: generation_config first, else the tokenizer's eos, else the model config's (:50-61)
  for (int64_t id : model_.generation.eos_token_ids) baseEosTokenIds_.push_back((int32_t)id);
  if (baseEosTokenIds_.empty() && tokenizerOk_ && tokenizer_.eosTokenId() >= 0) baseEosTokenIds_.push_back(tokenizer_.eosTokenId());
  if (baseEosTokenIds_.empty() && model_.config.eos_token_id >= 0) baseEosTokenIds_.push_back((int32_t)model_.config.eos_token_id);
  eosTokenIds_ = baseEosTokenIds_;
  prepared_ = true;
  return true;
}

void GPTEngine::reconfigure(const SamplerConfig& samplerConfig, int64_t maxNewTokens, const std::vector<int32_t>& extraStopTokenIds) {
  config_.samplerConfig = samplerConfig;
  config_.maxNewTokens = maxNewTokens;
  eosTokenIds_ = baseEosTokenIds_;
  for (int32_t id : extraStopTokenIds) if (!isEosToken(id)) eosTokenIds_.push_back(id);
  if (model_.ctx && !reuseActive()) be_.reset_cache(model_.ctx);           // context_.model->resetCache()  (:83); reusePrefix: the generate calls decide
  if (prepared_ && constraintOn()) constraintEnsure();                     // (a failure is reported by the generate call, which asks again)
}

// ---- SamplerConfig::regex: the pattern compiled over the tokenizer (constraint.h) and its table on the device (include/tgx.h tgx_automaton_create)
bool GPTEngine::constraintEnsure() {
  if (!(be_.automaton_create && be_.automaton_destroy && be_.set_row_automaton && be_.set_row_sampler && be_.sample_row && be_.set_row_stop && be_.decode_rows))
    return fail("regex: the device shim lacks tgx_automaton_create / tgx_set_row_automaton or the per-row calls they ride on");
  if (!tokenizerOk_) return fail("regex: no tokenizer loaded (tokenizerDir / modelDir must hold tokenizer.json)");
  if (eosTokenIds_.size() > (size_t)TGX_MAX_STOP_IDS) return fail("regex: the rows stop on the device, which holds at most " + std::to_string(TGX_MAX_STOP_IDS) + " stop ids");
  const std::string& pattern = config_.samplerConfig.regex;
  if (constraintId_ >= 0 && pattern == constraintPattern_ && eosTokenIds_ == constraintStops_) return true;
  TokenAutomaton a;
  std::string why;
  if (!compileConstraint(pattern, tokenizer_, desc().vocab, eosTokenIds_, a, why)) return fail("regex: " + why);
  if (constraintId_ >= 0) { be_.automaton_destroy(model_.ctx, constraintId_); constraintId_ = -1; }      // (every call switched its rows off when it ended)
  int32_t id = -1;
  if (be_.automaton_create(model_.ctx, a.nStates, a.start, a.next.data(), &id) != TGX_OK) return fail(std::string("regex: ") + be_.last_error(model_.ctx));
  constraintId_ = id; constraintPattern_ = pattern; constraintStops_ = eosTokenIds_;
  return true;
}

// reusePrefix: L = the common prefix of what row 0's cache holds and the new prompt, capped at prompt length - 1 (the last position's logits must be computed) and at
// the cache's length; row 0 is rolled back to L and extended with the rest
bool GPTEngine::prefillReusing(const std::vector<int64_t>& ids) {
  const int64_t S = (int64_t)ids.size();
  int64_t cap = std::min<int64_t>({(int64_t)cached_.size(), S - 1, be_.past_length(model_.ctx)});
  int64_t L = 0;
  while (L < cap && (int64_t)cached_[(size_t)L] == ids[(size_t)L]) L++;
  if (L < 1) return false;
  if (be_.truncate_row(model_.ctx, 0, L) != TGX_OK) return false;
  if (be_.extend_row(model_.ctx, 0, ids.data() + L, (int)(S - L)) != TGX_OK) return false;
  lastReused_ = L;
  return true;
}

// ---- GPTEngine::saveSession / loadSession (include/tgx.h tgx_save_row / tgx_restore_row): [magic 8][u32 version][u32 count][i32 ids x count][u64 snapshot bytes][snapshot]
static const unsigned char kSessionMagic[8] = {'T', 'G', 'X', 'S', 'E', 'S', 'S', 0};
enum : uint32_t { kSessionVersion = 1 };

static row_snapshot::Geometry session_geometry(const tgx_model_desc& d) {
  return {d.family, d.hidden, d.layers, d.heads, d.kv_heads, d.head_dim, d.vocab, d.compute_dtype, d.qk_norm};
}

bool GPTEngine::sessionCapable(const char* what) {
  if (!prepared_) return fail(std::string(what) + ": engine not prepared");
  if (!reuseActive()) return fail(std::string(what) + ": prefix reuse is not active (GPTConfig::reusePrefix and a backend with tgx_extend_row / tgx_truncate_row)");
  if (!be_.row_snapshot_bytes || !be_.save_row || !be_.restore_row) return fail(std::string(what) + ": the device shim lacks tgx_save_row / tgx_restore_row");
  return true;
}

bool GPTEngine::saveSession(const std::string& path) {
  if (!sessionCapable("saveSession")) return false;
  const int64_t held = be_.past_length(model_.ctx);
  if (cached_.empty() || held < 1 || held != (int64_t)cached_.size()) return fail("saveSession: row 0 holds no conversation (run generateAsync first)");
  const tgx_model_desc& d = desc();
  int64_t bytes = 0;
  if (be_.row_snapshot_bytes(model_.ctx, 0, &bytes) != TGX_OK) return fail(std::string("row_snapshot_bytes: ") + be_.last_error(model_.ctx));
  std::vector<unsigned char> file(16 + 4 * (size_t)held + 8 + (size_t)bytes);
  memcpy(file.data(), kSessionMagic, 8);
  row_snapshot::put32(file.data() + 8, kSessionVersion); row_snapshot::put32(file.data() + 12, (uint32_t)held);
  for (int64_t i = 0; i < held; i++) row_snapshot::put32(file.data() + 16 + 4 * (size_t)i, (uint32_t)cached_[(size_t)i]);
  unsigned char* const snap = file.data() + 16 + 4 * (size_t)held + 8;
  int64_t wrote = 0;
  if (be_.save_row(model_.ctx, 0, snap, bytes, &wrote) != TGX_OK) return fail(std::string("save_row: ") + be_.last_error(model_.ctx));
  // the next turn extends the row and computes its own logits: the file keeps the positions alone (the row on the device stays as it is)
  row_snapshot::Layout l;
  const char* why = "";
  if (row_snapshot::validate(snap, wrote, session_geometry(d), contextSize(), &l, nullptr, &why) != row_snapshot::OK || l.past != held)
    return fail(std::string("saveSession: the snapshot of row 0 is not what this engine expects: ") + why);
  wrote = (int64_t)row_snapshot::drop_logits(snap, session_geometry(d), l).total;
  row_snapshot::put64(snap - 8, (uint64_t)wrote);
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return fail("saveSession: cannot open " + path);
  const size_t n = (size_t)(snap - file.data()) + (size_t)wrote;
  const bool ok = fwrite(file.data(), 1, n, f) == n;
  if (fclose(f) != 0 || !ok) { remove(path.c_str()); return fail("saveSession: writing " + path + " failed"); }
  return true;
}

bool GPTEngine::loadSession(const std::string& path) {
  if (!sessionCapable("loadSession")) return false;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return fail("loadSession: cannot open " + path);
  std::vector<unsigned char> file;
  unsigned char chunk[1 << 16];
  for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + n);
  fclose(f);
  // ---- the whole file against this engine's model, before anything changes
  if (file.size() < 16 || memcmp(file.data(), kSessionMagic, 8) != 0) return fail("loadSession: " + path + " is not a session file");
  if (row_snapshot::get32(file.data() + 8) != kSessionVersion) return fail("loadSession: " + path + " has an unknown version");
  const uint64_t count = row_snapshot::get32(file.data() + 12), ids_end = 16 + 4 * count;
  if (count < 1 || file.size() < ids_end + 8) return fail("loadSession: " + path + " is truncated");
  const uint64_t bytes = row_snapshot::get64(file.data() + ids_end);
  if (bytes != file.size() - (ids_end + 8)) return fail("loadSession: " + path + " is truncated (the snapshot's size differs from what the file holds)");
  const tgx_model_desc& d = desc();
  std::vector<int32_t> ids((size_t)count);
  for (uint64_t i = 0; i < count; i++) {
    ids[(size_t)i] = (int32_t)row_snapshot::get32(file.data() + 16 + 4 * i);
    if (ids[(size_t)i] < 0 || ids[(size_t)i] >= d.vocab) return fail("loadSession: " + path + " holds a token id outside the vocabulary");
  }
  const unsigned char* const snap = file.data() + ids_end + 8;
  row_snapshot::Layout l;
  const char* why = "";
  if (row_snapshot::validate(snap, (int64_t)bytes, session_geometry(d), contextSize(), &l, nullptr, &why) != row_snapshot::OK)
    return fail("loadSession: " + path + " does not fit this model: " + why);
  if ((uint64_t)l.past != count) return fail("loadSession: " + path + " names " + std::to_string(count) + " token ids for a cache of " + std::to_string(l.past) + " positions");
  // ---- row 0 of a reset cache
  be_.reset_cache(model_.ctx);
  cached_.clear(); lastReused_ = 0;
  if (be_.restore_row(model_.ctx, 0, snap, (int64_t)bytes) != TGX_OK) return fail(std::string("restore_row: ") + be_.last_error(model_.ctx));
  cached_ = std::move(ids);
  return true;
}

// ---- GPTEngine::score (include/tgx.h tgx_score_row): one prefill pass over the sequence on row 0 of a reset cache
double ScoreOutput::perplexity() const {
  if (logprobs.empty()) return 0.0;
  double s = 0.0;
  for (float v : logprobs) s += (double)v;
  return std::exp(-s / (double)logprobs.size());
}

ScoreOutput GPTEngine::score(const std::vector<int32_t>& ids, int topN) {
  ScoreOutput out;
  if (!prepared_ || ids.empty()) { fail("score: engine not prepared or empty sequence"); return out; }
  if (!be_.score_row) { fail("score: the device shim lacks tgx_score_row"); return out; }
  if (topN < 0 || topN > TGX_MAX_LOGPROBS) { fail("score: at most " + std::to_string(TGX_MAX_LOGPROBS) + " alternatives per token"); return out; }
  const size_t keep = (size_t)std::min<int64_t>((int64_t)ids.size(), contextSize());      // beyond the context: the tail, like a prompt
  out.tokenIds.assign(ids.end() - (std::ptrdiff_t)keep, ids.end());
  out.dropped = (int64_t)(ids.size() - keep);
  const std::vector<int64_t> ids64(out.tokenIds.begin(), out.tokenIds.end());
  const size_t n = keep - 1, L = TGX_MAX_LOGPROBS;
  std::vector<float> lp(n), tlp(n * L);
  std::vector<int32_t> tid(n * L);
  be_.reset_cache(model_.ctx);
  cached_.clear(); lastReused_ = 0;
  const int rc = be_.score_row(model_.ctx, 0, ids64.data(), (int)keep, topN, lp.data(), tid.data(), tlp.data());
  if (rc != TGX_OK) fail(std::string("score_row: ") + be_.last_error(model_.ctx));
  be_.reset_cache(model_.ctx);      // as reconfigure leaves it: the next generate call prefills from an empty cache
  if (rc != TGX_OK) return out;
  out.topLogprobs = topN;
  out.logprobs = std::move(lp);
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < topN; k++) { out.topIds.push_back(tid[i * L + (size_t)k]); out.topLogprobValues.push_back(tlp[i * L + (size_t)k]); }
  out.ok = true;
  return out;
}

ScoreOutput GPTEngine::score(const std::string& text, int topN) {
  if (!tokenizerOk_) { fail("score: no tokenizer loaded (tokenizerDir / modelDir must hold tokenizer.json)"); return ScoreOutput{}; }
  return score(tokenizer_.encode(text, true), topN);
}

// ---- GPTEngine::embed (include/tgx.h tgx_embed_rows): the texts in calls of at most max_batch rows of an empty cache, every call releasing its rows
EmbedOutput GPTEngine::embed(const std::vector<std::vector<int32_t>>& ids, const EmbedConfig& cfg) {
  EmbedOutput out;
  // ---- every check before anything changes
  if (!prepared_ || ids.empty()) { fail("embed: engine not prepared or no text"); return out; }
  if (!be_.embed_rows) { fail("embed: the device shim lacks tgx_embed_rows"); return out; }
  const tgx_model_desc& d = desc();
  if (cfg.pool != TGX_POOL_LAST && cfg.pool != TGX_POOL_MEAN && cfg.pool != TGX_POOL_FIRST) { fail("embed: pool is none of last / mean / first"); return out; }
  if (cfg.dims < 0 || cfg.dims > d.hidden) { fail("embed: dims outside [0, " + std::to_string(d.hidden) + "]"); return out; }
  for (const auto& t : ids) if (t.empty()) { fail("embed: an empty text"); return out; }
  if (!cached_.empty()) { fail("embed: the engine holds a conversation in row 0 (prefix reuse) that the call's rows would collide with"); return out; }
  const int dims = cfg.dims ? cfg.dims : d.hidden, B = std::max(1, (int)d.max_batch);
  const tgx_embed_cfg ec{cfg.pool, cfg.normalize ? 1 : 0, cfg.dims, /*release=*/1};
  out.dims = dims;
  out.vectors.assign(ids.size() * (size_t)dims, 0.f);
  out.dropped.assign(ids.size(), 0);
  be_.reset_cache(model_.ctx);
  lastReused_ = 0;
  bool ok = true;
  for (size_t t0 = 0; t0 < ids.size() && ok; t0 += (size_t)B) {
    const int n = (int)std::min<size_t>((size_t)B, ids.size() - t0);
    std::vector<int32_t> rows((size_t)n), lens((size_t)n);
    std::vector<int64_t> flat;
    for (int i = 0; i < n; i++) {
      const std::vector<int32_t>& t = ids[t0 + (size_t)i];
      const size_t keep = (size_t)std::min<int64_t>((int64_t)t.size(), contextSize());      // beyond the context: the tail, like a prompt
      out.dropped[t0 + (size_t)i] = (int64_t)(t.size() - keep);
      rows[(size_t)i] = i; lens[(size_t)i] = (int32_t)keep;
      flat.insert(flat.end(), t.end() - (std::ptrdiff_t)keep, t.end());
    }
    const int rc = be_.embed_rows(model_.ctx, n, rows.data(), flat.data(), lens.data(), &ec, out.vectors.data() + t0 * (size_t)dims);
    if (rc != TGX_OK) { fail(std::string("embed_rows: ") + be_.last_error(model_.ctx)); ok = false; }
    else out.calls++;
  }
  be_.reset_cache(model_.ctx);      // as reconfigure leaves it: the next generate call prefills from an empty cache
  if (!ok) { out.vectors.clear(); out.dropped.clear(); out.calls = 0; return out; }
  out.ok = true;
  return out;
}

EmbedOutput GPTEngine::embed(const std::vector<std::string>& texts, const EmbedConfig& cfg) {
  if (!tokenizerOk_) { fail("embed: no tokenizer loaded (tokenizerDir / modelDir must hold tokenizer.json)"); return EmbedOutput{}; }
  std::vector<std::vector<int32_t>> ids;
  for (const std::string& t : texts) ids.push_back(tokenizer_.encode(t, true));
  return embed(ids, cfg);
}

// ---- GPTConfig::speculate: prompt-lookup drafts verified in one pass (spec_draft.h, include/tgx.h tgx_verify_row)
// (which of the two, or neither: spec_mode.h)
static tgxh::SpecMode spec_mode_of(const GPTConfig& cfg, const Backend& be, int batch, bool processors, size_t stopIds, bool verifyProcessed) {
  const SamplerConfig& s = cfg.samplerConfig;
  tgxh::SpecInputs in;
  in.speculate = cfg.speculate; in.speculateSampled = cfg.speculateSampled; in.batch = batch;
  in.greedy = !(s.temperature > 0.f || s.topK > 0 || s.topP < 1.f || s.minP > 0.f);      // Sampler.cpp:15-21
  in.processors = processors; in.verifyProcessed = verifyProcessed; in.stopIds = stopIds; in.maxStopIds = (size_t)TGX_MAX_STOP_IDS;
  in.rowStopCalls = be.set_row_stop && be.decode_rows;
  in.verifyRow = be.verify_row != nullptr;
  in.verifyRowSampled = be.verify_row_sampled && be.set_row_sampler && be.sample_row;
  in.verifyRows = be.verify_rows != nullptr;
  return tgxh::spec_mode(in);
}
// (GPTConfig::contextShift: the shifting loops take plain steps — a draft's positions are counted from the sequence, which a shifted row no longer holds in full)
bool GPTEngine::speculateActive(int batch) const { return !shiftActive() && spec_mode_of(config_, be_, batch, processorsOn(), eosTokenIds_.size(), verifyProcessedOn_) != tgxh::SpecMode::Off; }
bool GPTEngine::speculateSampledActive(int batch) const { return !shiftActive() && spec_mode_of(config_, be_, batch, processorsOn(), eosTokenIds_.size(), verifyProcessedOn_) == tgxh::SpecMode::Sampled; }
// GPTConfig::speculateProcessed: the device's verify calls take processed rows only under option verify.processors (include/tgx.h), which the engine holds at 1
// for the length of a generate call that drafts with processors on.  A backend without the option (or the option calls) keeps the plain steps
bool GPTEngine::verifyProcessedBegin() {
  verifyProcessedOn_ = false;
  if (!config_.speculateProcessed || config_.speculate <= 0 || !processorsOn() || !be_.set_option || !be_.get_option) return false;
  int was = 0;
  if (be_.get_option(model_.ctx, "verify.processors", &was) != TGX_OK || be_.set_option(model_.ctx, "verify.processors", 1) != TGX_OK) return false;
  verifyProcessedWas_ = was; verifyProcessedOn_ = true;
  return true;
}
void GPTEngine::verifyProcessedEnd() {
  if (verifyProcessedOn_) be_.set_option(model_.ctx, "verify.processors", verifyProcessedWas_);
  verifyProcessedOn_ = false;
}

bool GPTEngine::speculateMore(std::vector<int32_t>& seq, int64_t maxTotal, bool& finished) {
  const int64_t past = (int64_t)seq.size() - 1, room = maxTotal - (int64_t)seq.size();      // room: tokens the call may still produce
  // a pass over n draft tokens produces up to n + 1 tokens and fills positions past .. past + n
  const int64_t cap = !speculateActive(1) ? 0 : std::min<int64_t>({(int64_t)config_.speculate, (int64_t)TGX_MAX_DRAFT, room - 1, contextSize() - past - 1});      // (GPTConfig::logprobs alone feeds the consumer one step at a time)
  int32_t n = 0, fin = 0;
  int64_t ids[TGX_MAX_DRAFT + 1] = {0};
  // GPTConfig::speculateTree: the same positions as branches where the tail has continued in different ways before; a refusal as unsupported leaves the row as it
  // was (ALL OR NOTHING), and the chain below takes this iteration and the rest of the call
  bool treeDone = false;
  if (cap >= 2 && config_.speculateTree >= 2 && be_.verify_tree && !treeRefused_) {
    const tgxh::DraftTree tree = tgxh::ngram_tree(seq, (int)cap, config_.speculateTree);
    if (tree.branches >= 2) {
      int64_t t64[TGX_MAX_TREE_NODES];
      for (size_t i = 0; i < tree.tokens.size(); i++) t64[i] = tree.tokens[i];
      const int rc = be_.verify_tree(model_.ctx, 0, t64, tree.parent.data(), (int)tree.tokens.size(), ids, &n, &fin);
      if (rc == TGX_ERR_UNSUPPORTED) treeRefused_ = true;
      else if (rc != TGX_OK) return fail(std::string("verify_tree: ") + be_.last_error(model_.ctx));
      else {
        treeDone = true;
        spec_.verifyCalls++; spec_.treePasses++; spec_.draftTokens += (int64_t)tree.tokens.size(); spec_.acceptedDrafts += n - 1; spec_.producedHist[n]++;
      }
    }
  }
  const std::vector<int32_t> draft = cap >= 1 && !treeDone ? ngram_draft(seq, (int)cap) : std::vector<int32_t>();
  if (treeDone) {
  } else if (!draft.empty()) {
    int64_t d64[TGX_MAX_DRAFT];
    for (size_t i = 0; i < draft.size(); i++) d64[i] = draft[i];
    const auto verify = speculateSampledActive(1) ? be_.verify_row_sampled : be_.verify_row;      // (the row's sampler is the call's: rowsBegin)
    if (verify(model_.ctx, 0, d64, (int)draft.size(), ids, &n, &fin) != TGX_OK) return fail(std::string("verify: ") + be_.last_error(model_.ctx));
    spec_.verifyCalls++; spec_.draftTokens += (int64_t)draft.size(); spec_.acceptedDrafts += n - 1; spec_.producedHist[n]++;
  } else {
    if (be_.decode_rows(model_.ctx, 1, ids, &n, &fin) != TGX_OK) return fail(std::string("decode: ") + be_.last_error(model_.ctx));
    if (speculateActive(1)) spec_.plainSteps++;      // (GPTConfig::logprobs alone also steps through here: no statistic of the drafts)
  }
  for (int32_t i = 0; i < n; i++) seq.push_back((int32_t)ids[i]);
  finished = fin != 0;
  return n > 0 || finished ? true : fail("speculate: the row produced no token");
}

bool GPTEngine::speculateMoreRows(std::vector<std::vector<int32_t>>& seqs, int64_t maxTotal, std::vector<char>& finished, std::vector<int64_t>& produced) {
  const int B = (int)seqs.size();
  produced.assign((size_t)B, 0);
  std::vector<int32_t> rows, nDraft, outN, outFin;
  std::vector<int64_t> drafts, outIds;
  auto flush = [&]() -> bool {      // one tgx_verify_rows call over the rows gathered so far
    if (rows.empty()) return true;
    const size_t n = rows.size();
    outIds.assign(n * (TGX_MAX_DRAFT + 1), 0); outN.assign(n, 0); outFin.assign(n, 0);
    if (drafts.empty()) drafts.push_back(0);      // (a valid pointer for a call without any draft)
    if (be_.verify_rows(model_.ctx, (int)n, rows.data(), drafts.data(), nDraft.data(), outIds.data(), outN.data(), outFin.data()) != TGX_OK)
      return fail(std::string("verify_rows: ") + be_.last_error(model_.ctx));
    bool drafted = false;
    for (size_t i = 0; i < n; i++) {
      const int b = rows[i];
      if (outN[i] < 1 && !outFin[i]) return fail("speculate: a row produced no token");
      for (int32_t k = 0; k < outN[i]; k++) seqs[(size_t)b].push_back((int32_t)outIds[i * (TGX_MAX_DRAFT + 1) + (size_t)k]);
      produced[(size_t)b] = outN[i];
      finished[(size_t)b] = outFin[i] != 0;
      if (nDraft[i] > 0) { drafted = true; spec_.draftTokens += nDraft[i]; spec_.acceptedDrafts += outN[i] - 1; spec_.producedHist[outN[i]]++; }
      else spec_.plainSteps++;
    }
    if (drafted) spec_.verifyCalls++;
    rows.clear(); nDraft.clear(); drafts.clear();
    return true;
  };
  int64_t M = 0;
  for (int b = 0; b < B; b++) {
    std::vector<int32_t>& seq = seqs[(size_t)b];
    if (finished[(size_t)b] || (int64_t)seq.size() >= maxTotal) continue;
    const int64_t past = (int64_t)seq.size() - 1, room = maxTotal - (int64_t)seq.size();
    const int64_t cap = std::min<int64_t>({(int64_t)config_.speculate, (int64_t)TGX_MAX_DRAFT, room - 1, contextSize() - past - 1});
    const std::vector<int32_t> draft = cap >= 1 ? ngram_draft(seq, (int)cap) : std::vector<int32_t>();
    if (M + (int64_t)draft.size() + 1 > TGX_MAX_VERIFY_POSITIONS) { if (!flush()) return false; M = 0; }
    rows.push_back(b); nDraft.push_back((int32_t)draft.size());
    for (int32_t t : draft) drafts.push_back(t);
    M += (int64_t)draft.size() + 1;
  }
  return flush();
}

// ---- GPTConfig::logprobs: the per-row calls record on the device (include/tgx.h tgx_set_row_logprobs); the engine drains each row's ring after every call,
// and no call produces more than TGX_LOGPROB_RING tokens per row
bool GPTEngine::logprobsActive() const {
  return config_.logprobs >= 0 && config_.logprobs <= TGX_MAX_LOGPROBS && be_.set_row_logprobs && be_.read_row_logprobs && be_.set_row_sampler && be_.sample_row &&
         be_.set_row_stop && be_.decode_rows;
}

// a request the engine cannot serve is an error, never plain generation with empty lists
bool GPTEngine::logprobsRefused(bool async) {
  if (config_.logprobs < 0) return false;
  if (config_.logprobs > TGX_MAX_LOGPROBS) { fail("logprobs: at most " + std::to_string(TGX_MAX_LOGPROBS) + " alternatives per token"); return true; }
  if (!logprobsActive()) { fail("logprobs: the device shim lacks tgx_set_row_logprobs / tgx_read_row_logprobs or the per-row calls they ride on"); return true; }
  if (async && eosTokenIds_.size() > (size_t)TGX_MAX_STOP_IDS) { fail("logprobs: generateAsync stops the row on the device, which holds at most " + std::to_string(TGX_MAX_STOP_IDS) + " stop ids"); return true; }
  return false;
}

// ---- GPTConfig::contextShift (engine.h; include/tgx.h tgx_splice_row)
bool GPTEngine::shiftRow(int row, int32_t cur, const tgx_sampler_cfg& sc, int64_t* next, std::vector<int32_t>* held) {
  const int64_t past = be_.past_length_row(model_.ctx, row);
  if (past < 2) return fail("context shift: the row holds fewer than two positions");
  const int64_t n_keep = std::min<int64_t>(std::max(0, config_.shiftKeep), past - 1), n_discard = (past - n_keep) / 2;
  int64_t starts[2] = {0, n_keep + n_discard}, lens[2] = {n_keep, past - n_keep - n_discard}, new_len = 0;
  if (n_discard < 1)
    return fail("context shift: shiftKeep " + std::to_string(config_.shiftKeep) + " keeps all but one of the row's " + std::to_string(past) + " positions: nothing is left to discard");
  const int first = n_keep > 0 ? 0 : 1;
  if (be_.splice_row(model_.ctx, row, 2 - first, starts + first, lens + first, &new_len) != TGX_OK) return fail(std::string("splice_row: ") + be_.last_error(model_.ctx));
  const int64_t t = cur;
  if (be_.extend_row(model_.ctx, row, &t, 1) != TGX_OK) return fail(std::string("extend_row: ") + be_.last_error(model_.ctx));
  if (be_.sample_row(model_.ctx, row, &sc, config_.seed, next) != TGX_OK) return fail(std::string("sample_row: ") + be_.last_error(model_.ctx));
  if (held) {
    if ((int64_t)held->size() == past) { held->erase(held->begin() + n_keep, held->begin() + n_keep + n_discard); held->push_back(cur); }
    else held->clear();      // (unknown: the caller's record did not match the row)
  }
  lastShifts_++;
  return true;
}

// generateSync's decode under contextShift: every row through tgx_decode_rows with its length on the device (max_new = what it may still produce), never more steps
// per call than the fullest unfinished row has room for; a full row is shifted, which produces its next token.  got[b]: the tokens of row b after its first
bool GPTEngine::decodeRowsShifting(int B, const tgx_sampler_cfg& sc, int64_t n_more, bool constrained, std::vector<std::vector<int64_t>>& got, std::vector<RowLogprobs>* lp) {
  const int64_t ctxSize = contextSize();
  const int32_t* stops = constrained && !eosTokenIds_.empty() ? eosTokenIds_.data() : nullptr;
  const int n_stops = constrained ? (int)eosTokenIds_.size() : 0;
  std::vector<char> over((size_t)B, 0);
  for (int b = 0; b < B; b++) {
    if (constrained && !got[(size_t)b].empty() && isEosToken((int32_t)got[(size_t)b].back())) over[(size_t)b] = 1;
  }
  std::vector<int64_t> cur((size_t)B);
  for (int b = 0; b < B; b++) { cur[(size_t)b] = got[(size_t)b].back(); got[(size_t)b].clear(); }      // (in: the row's first token)
  auto restate = [&](int b) {
    const int64_t rem = n_more - (int64_t)got[(size_t)b].size();
    if (rem <= 0) {      // the row is done: retired, so that the other rows' steps leave it alone
      over[(size_t)b] = 1;
      return be_.reset_row(model_.ctx, b) == TGX_OK || fail(std::string("reset_row: ") + be_.last_error(model_.ctx));
    }
    return be_.set_row_stop(model_.ctx, b, (int32_t)rem, stops, n_stops) == TGX_OK || fail(std::string("set_row_stop: ") + be_.last_error(model_.ctx));
  };
  for (int b = 0; b < B; b++) {
    if (over[(size_t)b]) { if (be_.reset_row(model_.ctx, b) != TGX_OK) return fail(std::string("reset_row: ") + be_.last_error(model_.ctx)); }
    else if (!restate(b)) return false;
  }
  std::vector<int64_t> ids;
  std::vector<int32_t> made((size_t)B), fin((size_t)B);
  auto open = [&] { for (char o : over) if (!o) return true; return false; };
  while (open()) {
    int64_t room = TGX_LOGPROB_RING / 2;
    for (int b = 0; b < B; b++) {
      if (over[(size_t)b]) continue;
      if (be_.past_length_row(model_.ctx, b) >= ctxSize) {
        int64_t next = 0;
        if (!shiftRow(b, (int32_t)cur[(size_t)b], sc, &next, nullptr)) return false;
        got[(size_t)b].push_back(next); cur[(size_t)b] = next;
        if (lp && !logprobsDrain(b, 1, (*lp)[(size_t)b])) return false;
        if (constrained && isEosToken((int32_t)next)) { over[(size_t)b] = 1; if (be_.reset_row(model_.ctx, b) != TGX_OK) return fail(std::string("reset_row: ") + be_.last_error(model_.ctx)); continue; }
        if (!restate(b) || over[(size_t)b]) { if (!over[(size_t)b]) return false; continue; }
      }
      room = std::min<int64_t>({room, ctxSize - be_.past_length_row(model_.ctx, b), n_more - (int64_t)got[(size_t)b].size()});
    }
    if (!open()) break;
    const int m = (int)std::max<int64_t>(1, room);
    ids.assign((size_t)m * (size_t)B, -1);
    if (be_.decode_rows(model_.ctx, m, ids.data(), made.data(), fin.data()) != TGX_OK) return fail(std::string("decode: ") + be_.last_error(model_.ctx));
    for (int b = 0; b < B; b++) {
      if (over[(size_t)b]) continue;
      if (made[(size_t)b] < 1 && !fin[(size_t)b]) return fail("context shift: a row produced no token");
      for (int32_t i = 0; i < made[(size_t)b]; i++) got[(size_t)b].push_back(ids[(size_t)i * (size_t)B + (size_t)b]);
      if (made[(size_t)b] > 0) cur[(size_t)b] = got[(size_t)b].back();
      if (lp && !logprobsDrain(b, made[(size_t)b], (*lp)[(size_t)b])) return false;
      if (fin[(size_t)b]) over[(size_t)b] = 1;
    }
  }
  return true;
}

bool GPTEngine::rowsBegin(int batch, const tgx_sampler_cfg& sc, std::vector<int64_t>& first) {
  first.assign((size_t)batch, 0);
  const bool lp = logprobsActive();
  for (int b = 0; b < batch; b++) {
    if (be_.set_row_sampler(model_.ctx, b, &sc, config_.seed) != TGX_OK || (lp && be_.set_row_logprobs(model_.ctx, b, config_.logprobs) != TGX_OK) ||
        be_.sample_row(model_.ctx, b, &sc, config_.seed, &first[(size_t)b]) != TGX_OK)
      return fail(std::string(lp ? "logprobs: " : "sample_row: ") + be_.last_error(model_.ctx));
  }
  return true;
}

// ---- SamplerConfig's penalties and logit bias: per row on the device (include/tgx.h tgx_set_row_penalties); the engine supplies each row's history from the prompt
// it admitted and steps through the per-row calls, which count what the rows produce
bool GPTEngine::processorsRefused(bool async) {
  if (!processorsOn()) return false;
  if (constraintOn() && !constraintEnsure()) return true;
  if (!(be_.set_row_penalties && be_.set_row_logit_bias && be_.set_row_history && be_.set_row_sampler && be_.sample_row && be_.set_row_stop && be_.decode_rows)) {
    fail("penalties / logit bias: the device shim lacks tgx_set_row_penalties / tgx_set_row_logit_bias / tgx_set_row_history or the per-row calls they ride on");
    return true;
  }
  if (config_.samplerConfig.logitBias.size() > (size_t)TGX_MAX_LOGIT_BIAS) { fail("logit bias: at most " + std::to_string(TGX_MAX_LOGIT_BIAS) + " ids"); return true; }
  if (async && eosTokenIds_.size() > (size_t)TGX_MAX_STOP_IDS) { fail("penalties / logit bias: generateAsync stops the row on the device, which holds at most " + std::to_string(TGX_MAX_STOP_IDS) + " stop ids"); return true; }
  return false;
}

bool GPTEngine::processorsBegin(int row, const int64_t* prompt, int64_t n) {
  const SamplerConfig& s = config_.samplerConfig;
  const tgx_penalty_cfg pc{s.repetitionPenalty, s.presencePenalty, s.frequencyPenalty};
  std::vector<int32_t> ids; std::vector<float> val;
  for (const auto& kv : s.logitBias) { ids.push_back(kv.first); val.push_back(kv.second); }
  if (be_.set_row_penalties(model_.ctx, row, &pc) != TGX_OK || be_.set_row_logit_bias(model_.ctx, row, (int)ids.size(), ids.data(), val.data()) != TGX_OK ||
      be_.set_row_history(model_.ctx, row, prompt, (int)n, nullptr, 0) != TGX_OK)
    return fail(std::string("penalties / logit bias: ") + be_.last_error(model_.ctx));
  if (constraintOn() && be_.set_row_automaton(model_.ctx, row, constraintId_, -1) != TGX_OK) return fail(std::string("regex: ") + be_.last_error(model_.ctx));
  return true;
}

void GPTEngine::processorsEnd(int batch) {
  const tgx_penalty_cfg neutral{1.f, 0.f, 0.f};
  for (int b = 0; b < batch; b++) {
    be_.set_row_penalties(model_.ctx, b, &neutral);
    be_.set_row_logit_bias(model_.ctx, b, 0, nullptr, nullptr);
    be_.set_row_history(model_.ctx, b, nullptr, 0, nullptr, 0);
    if (be_.set_row_automaton) be_.set_row_automaton(model_.ctx, b, -1, -1);
  }
}

bool GPTEngine::logprobsDrain(int row, int64_t n, RowLogprobs& into) {
  if (n < 1) return true;
  std::vector<float> lp((size_t)n), tlp((size_t)n * TGX_MAX_LOGPROBS);
  std::vector<int32_t> tid((size_t)n * TGX_MAX_LOGPROBS);
  if (be_.read_row_logprobs(model_.ctx, row, (int)n, lp.data(), tid.data(), tlp.data(), nullptr) != TGX_OK) return fail(std::string("read_row_logprobs: ") + be_.last_error(model_.ctx));
  for (int64_t i = 0; i < n; i++) {
    into.lp.push_back(lp[(size_t)i]);
    for (int k = 0; k < config_.logprobs; k++) {
      into.topId.push_back(tid[(size_t)i * TGX_MAX_LOGPROBS + (size_t)k]);
      into.topLp.push_back(tlp[(size_t)i * TGX_MAX_LOGPROBS + (size_t)k]);
    }
  }
  return true;
}

// the rows' setting goes back to "off" however the call that switched it on ends: a failed drain or step must not leave a later call without logprobs
// paying the record launches
template <class F> struct AtExit { F f; ~AtExit() { f(); } };
template <class F> AtExit<F> at_exit(F f) { return AtExit<F>{std::move(f)}; }

// GPTConfig::speculateSampled made row 0's sampler the call's: back to the default, so that a later greedy call's per-row steps are greedy whatever ran before
void GPTEngine::rowSamplerEnd(int batch) {
  const tgx_sampler_cfg greedy{0.f, 0, 1.f, 0.f};
  for (int b = 0; b < batch; b++) be_.set_row_sampler(model_.ctx, b, &greedy, 0);
}

void GPTEngine::logprobsEnd(int batch) {
  for (int b = 0; b < batch; b++) be_.set_row_logprobs(model_.ctx, b, -1);
}

void GPTEngine::logprobsStore(GPTOutput& out, const std::vector<RowLogprobs>& rows, int64_t perRow) const {
  out.topLogprobs = config_.logprobs;
  for (const RowLogprobs& r : rows) {
    out.logprobs.insert(out.logprobs.end(), r.lp.begin(), r.lp.begin() + std::min<int64_t>(perRow, (int64_t)r.lp.size()));
    const int64_t k = std::min<int64_t>(perRow * config_.logprobs, (int64_t)r.topId.size());
    out.topIds.insert(out.topIds.end(), r.topId.begin(), r.topId.begin() + k);
    out.topLogprobValues.insert(out.topLogprobValues.end(), r.topLp.begin(), r.topLp.begin() + k);
  }
}

bool GPTEngine::isEosToken(int32_t id) const { return std::find(eosTokenIds_.begin(), eosTokenIds_.end(), id) != eosTokenIds_.end(); }

int64_t GPTEngine::contextSize() const { return model_.ctx ? be_.context_size(model_.ctx) : 0; }

std::vector<int64_t> GPTEngine::alignPrompts(const std::vector<std::vector<int32_t>>& prompts, int32_t padToken, int64_t& maxLen) const {
  maxLen = 0;
  for (const auto& p : prompts) maxLen = std::max<int64_t>(maxLen, (int64_t)p.size());
  maxLen = std::min<int64_t>(maxLen, contextSize());
  std::vector<int64_t> ids((size_t)(prompts.size() * maxLen));
  for (size_t b = 0; b < prompts.size(); b++) {
    const auto& t = prompts[b];
    int64_t* row = ids.data() + b * maxLen;
    if ((int64_t)t.size() > maxLen) {
      for (int64_t i = 0; i < maxLen; i++) row[i] = t[t.size() - (size_t)maxLen + (size_t)i];     // keep the tail (:127-129)
    } else {
      const int64_t pad = maxLen - (int64_t)t.size();
      for (int64_t i = 0; i < pad; i++) row[i] = padToken;                                         // left pad (:130-138)
      for (size_t i = 0; i < t.size(); i++) row[pad + (int64_t)i] = t[i];
    }
  }
  return ids;
}

GPTOutput GPTEngine::generateSync(const std::vector<std::vector<int32_t>>& prompts, int32_t padToken) {
  GPTOutput out;
  if (!prepared_ || prompts.empty()) { fail("generateSync: engine not prepared or empty batch"); return out; }
  if (config_.numBeams > 1) return beamsRefused(prompts.size()) ? out : generateBeams(prompts[0], padToken);
  if (logprobsRefused(false) || processorsRefused(false)) return out;
  verifyProcessedBegin();
  const auto verifyProcessedOff = at_exit([&] { verifyProcessedEnd(); });
  const int B = (int)prompts.size();
  int64_t S = 0;
  std::vector<int64_t> ids = alignPrompts(prompts, padToken, S);
  if (S == 0) { fail("generateSync: every prompt is empty (nothing to prefill)"); return out; }
  const tgx_sampler_cfg sc = to_c(config_.samplerConfig);
  const int64_t n_new = std::max<int64_t>(1, config_.maxNewTokens);
  lastReused_ = 0;
  if (reuseActive()) { be_.reset_cache(model_.ctx); cached_.clear(); }      // (reconfigure left the cache in place)

  // prefill (mask ignored, like the reference: "TODO padding mask", GPTEngine.cpp:95)
  const auto t0 = std::chrono::steady_clock::now();
  if (be_.forward(model_.ctx, ids.data(), B, (int)S) != TGX_OK) { fail(std::string("forward: ") + be_.last_error(model_.ctx)); return out; }
  std::vector<int64_t> first((size_t)B), rest((size_t)(B * (n_new - 1)));
  const bool lpOn = logprobsActive();
  std::vector<RowLogprobs> lpRows((size_t)(lpOn ? B : 0));
  const auto lpOff = at_exit([&] { if (lpOn) logprobsEnd(B); });
  const bool shift = shiftActive() && be_.reset_row;
  const bool procOn = processorsOn(), specSampled = speculateSampledActive(B), perRow = lpOn || procOn || specSampled || shift;
  lastShifts_ = 0;
  bool allStopped = false;      // SamplerConfig::regex: every row ended at a stop id
  const auto procOff = at_exit([&] { if (procOn) processorsEnd(B); });
  const auto samplerOff = at_exit([&] { if (specSampled) rowSamplerEnd(B); });
  if (procOn)      // every row's history: the prompt it admitted, without the left padding
    for (int b = 0; b < B; b++) {
      const int64_t n = std::min<int64_t>((int64_t)prompts[(size_t)b].size(), S);
      if (!processorsBegin(b, ids.data() + (size_t)(b * S + (S - n)), n)) return out;
    }
  if (perRow) {
    if (!rowsBegin(B, sc, first)) return out;
    for (int b = 0; lpOn && b < B; b++) if (!logprobsDrain(b, 1, lpRows[(size_t)b])) return out;
  } else
  if (be_.sample(model_.ctx, &sc, config_.seed, first.data()) != TGX_OK) { fail(std::string("sample: ") + be_.last_error(model_.ctx)); return out; }
  const auto t1 = std::chrono::steady_clock::now();
  // decode: maxNewTokens-1 iterations, no EOS check (:165-172)
  if (n_new > 1 && B > 1 && speculateActive(B)) {      // a batch: every unfinished row advances through tgx_verify_rows, with its own draft or none
    // (SamplerConfig::regex under speculateProcessed: the rows end on the device at an EOS id as in the per-row branch below, the pad token behind the stop)
    const bool constrained = constraintOn();
    std::vector<std::vector<int32_t>> seqs((size_t)B);
    std::vector<char> finished((size_t)B, 0);
    for (int b = 0; b < B; b++) {
      for (int64_t i = 0; i < S; i++) seqs[(size_t)b].push_back((int32_t)ids[(size_t)(b * S + i)]);
      seqs[(size_t)b].push_back((int32_t)first[(size_t)b]);
      if (be_.set_row_stop(model_.ctx, b, (int32_t)(n_new - 1), constrained && !eosTokenIds_.empty() ? eosTokenIds_.data() : nullptr, constrained ? (int)eosTokenIds_.size() : 0) != TGX_OK) { fail(std::string("set_row_stop: ") + be_.last_error(model_.ctx)); return out; }
      if (constrained && isEosToken((int32_t)first[(size_t)b])) finished[(size_t)b] = 1;
    }
    std::vector<int64_t> produced;
    auto open = [&] { for (int b = 0; b < B; b++) if (!finished[(size_t)b] && (int64_t)seqs[(size_t)b].size() < S + n_new) return true; return false; };
    while (open()) {
      if (!speculateMoreRows(seqs, S + n_new, finished, produced)) return out;
      for (int b = 0; lpOn && b < B; b++) if (!logprobsDrain(b, produced[(size_t)b], lpRows[(size_t)b])) return out;
    }
    allStopped = constrained;
    for (int b = 0; b < B; b++) {
      const std::vector<int32_t>& seq = seqs[(size_t)b];
      if (!constrained && (int64_t)seq.size() != S + n_new) { fail("speculate: a row finished before maxNewTokens"); return out; }
      for (int64_t i = 0; i + 1 < n_new; i++) rest[(size_t)(i * B + b)] = S + 1 + i < (int64_t)seq.size() ? seq[(size_t)(S + 1 + i)] : padTokenId();
      allStopped = allStopped && isEosToken(seq.back());
    }
  } else if (n_new > 1 && speculateActive(B)) {      // ... of which a verified draft covers several at once: no stop ids (no EOS check here), the length on the device
    std::vector<int32_t> seq;
    for (int64_t i = 0; i < S; i++) seq.push_back((int32_t)ids[(size_t)i]);
    seq.push_back((int32_t)first[0]);
    const bool constrained = constraintOn();      // (SamplerConfig::regex under speculateProcessed: as in the batch branch above)
    if (be_.set_row_stop(model_.ctx, 0, (int32_t)(n_new - 1), constrained && !eosTokenIds_.empty() ? eosTokenIds_.data() : nullptr, constrained ? (int)eosTokenIds_.size() : 0) != TGX_OK) { fail(std::string("set_row_stop: ") + be_.last_error(model_.ctx)); return out; }
    bool finished = constrained && isEosToken((int32_t)first[0]);
    treeRefused_ = false;      // (GPTConfig::speculateTree: a refusal holds for one call)
    while ((int64_t)seq.size() < S + n_new && !finished) {
      const size_t before = seq.size();
      if (!speculateMore(seq, S + n_new, finished)) return out;
      if (lpOn && !logprobsDrain(0, (int64_t)(seq.size() - before), lpRows[0])) return out;
    }
    if (!constrained && (int64_t)seq.size() != S + n_new) { fail("speculate: the row finished before maxNewTokens"); return out; }
    for (int64_t i = 0; i + 1 < n_new; i++) rest[(size_t)i] = S + 1 + i < (int64_t)seq.size() ? seq[(size_t)(S + 1 + i)] : padTokenId();
    allStopped = constrained && isEosToken(seq.back());
  } else if (shift && n_new > 1) {      // GPTConfig::contextShift: the rows may pass the context (decodeRowsShifting)
    const bool constrained = constraintOn();
    std::vector<std::vector<int64_t>> got((size_t)B);
    for (int b = 0; b < B; b++) got[(size_t)b].push_back(first[(size_t)b]);
    if (!decodeRowsShifting(B, sc, n_new - 1, constrained, got, lpOn ? &lpRows : nullptr)) return out;
    const int32_t pad = padTokenId();
    allStopped = constrained;
    for (int b = 0; b < B; b++) {
      bool stopped = constrained && isEosToken((int32_t)first[(size_t)b]);
      if (!constrained && (int64_t)got[(size_t)b].size() != n_new - 1) { fail("context shift: a row finished before maxNewTokens"); return out; }
      for (int64_t i = 0; i + 1 < n_new; i++) {
        int64_t& t = rest[(size_t)(i * B + b)];
        if (stopped || i >= (int64_t)got[(size_t)b].size()) { t = pad; continue; }
        t = got[(size_t)b][(size_t)i];
        if (constrained && isEosToken((int32_t)t)) stopped = true;
      }
      allStopped = allStopped && stopped;
    }
  } else if (perRow) {      // every row with the call's settings through tgx_decode_rows (its ids are tgx_decode's), a ring's worth of steps at most per call
    // under a regex the rows end on the device at an EOS / stop id, which the automaton allows only where a match may end; otherwise no EOS check, as below
    const bool constrained = constraintOn();
    for (int b = 0; b < B; b++)
      if (be_.set_row_stop(model_.ctx, b, 0, constrained && !eosTokenIds_.empty() ? eosTokenIds_.data() : nullptr, constrained ? (int)eosTokenIds_.size() : 0) != TGX_OK) { fail(std::string("set_row_stop: ") + be_.last_error(model_.ctx)); return out; }
    std::vector<int32_t> fin((size_t)B, 0), made((size_t)B, 0);
    if (constrained) for (int b = 0; b < B; b++) fin[(size_t)b] = isEosToken((int32_t)first[(size_t)b]) ? 1 : 0;      // (a pattern that matches the empty string: tgx_sample_row does not test the stop set)
    auto running = [&] { for (int32_t f : fin) if (!f) return true; return false; };
    int64_t done = 0;
    while (done < n_new - 1 && running()) {
      const int m = (int)std::min<int64_t>(n_new - 1 - done, TGX_LOGPROB_RING / 2);
      if (be_.decode_rows(model_.ctx, m, rest.data() + (size_t)(done * B), constrained ? made.data() : nullptr, constrained ? fin.data() : nullptr) != TGX_OK) { fail(std::string("decode: ") + be_.last_error(model_.ctx)); return out; }
      for (int b = 0; lpOn && b < B; b++) if (!logprobsDrain(b, constrained ? made[(size_t)b] : m, lpRows[(size_t)b])) return out;
      done += m;
    }
    if (constrained) {      // behind a row's stop: the pad token
      const int32_t pad = padTokenId();
      for (int b = 0; b < B; b++) {
        bool stopped = isEosToken((int32_t)first[(size_t)b]);
        for (int64_t i = 0; i + 1 < n_new; i++) {
          int64_t& t = rest[(size_t)(i * B + b)];
          if (stopped || i >= done || t < 0) t = pad;
          else if (isEosToken((int32_t)t)) stopped = true;
        }
      }
      allStopped = !running();
    }
  } else
  if (n_new > 1 && be_.decode(model_.ctx, &sc, config_.seed, (int)(n_new - 1), rest.data()) != TGX_OK) {
    fail(std::string("decode: ") + be_.last_error(model_.ctx));
    return out;
  }
  if (lpOn) logprobsStore(out, lpRows, n_new);
  out.firstTokenMs = std::chrono::duration<double, std::milli>(t1 - t0).count();
  out.decodeMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  out.batch = B;
  out.newTokens = n_new;
  out.tokenIds.resize((size_t)(B * (S + n_new)));
  for (int b = 0; b < B; b++) {
    int32_t* row = out.tokenIds.data() + (size_t)b * (size_t)(S + n_new);
    for (int64_t i = 0; i < S; i++) row[i] = (int32_t)ids[(size_t)(b * S + i)];
    row[S] = (int32_t)first[(size_t)b];
    for (int64_t i = 0; i + 1 < n_new; i++) row[S + 1 + i] = (int32_t)rest[(size_t)(i * B + b)];
  }
  out.finishReason = allStopped ? FinishReason::Stop : FinishReason::Length;
  return out;
}

// ---- GPTConfig::numBeams > 1 (beam.h holds the rules; include/tgx.h tgx_beam_select / tgx_beam_advance the device side)
static_assert(sizeof(BeamCand) == sizeof(tgx_beam_cand), "beam.h BeamCand == tgx_beam_cand");
bool GPTEngine::beamsRefused(size_t prompts) {
  const int K = config_.numBeams;
  const SamplerConfig& s = config_.samplerConfig;
  if (K > TGX_MAX_BEAMS) { fail("beam search: numBeams " + std::to_string(K) + " exceeds TGX_MAX_BEAMS " + std::to_string(TGX_MAX_BEAMS)); return true; }
  if (config_.numReturn < 1 || config_.numReturn > K) { fail("beam search: numReturn " + std::to_string(config_.numReturn) + " outside [1, numBeams]"); return true; }
  if (s.temperature > 0.f || s.topK > 0 || s.topP < 1.f || s.minP > 0.f) { fail("beam search: needs a greedy sampler configuration (temperature 0, no top-k / top-p / min-p)"); return true; }
  if (prompts != 1) { fail("beam search: one prompt per generateSync call, got " + std::to_string(prompts)); return true; }
  if (config_.speculate > 0 || config_.logprobs >= 0 || config_.contextShift) { fail("beam search does not combine with speculate, logprobs or contextShift"); return true; }
  if (config_.maxBatch < K) { fail("beam search: maxBatch " + std::to_string(config_.maxBatch) + " < numBeams " + std::to_string(K)); return true; }
  if (eosTokenIds_.size() > (size_t)TGX_MAX_STOP_IDS) { fail("beam search: at most " + std::to_string(TGX_MAX_STOP_IDS) + " EOS / stop ids"); return true; }
  if (!(be_.beam_select && be_.beam_advance && be_.forward_row && be_.decode_rows)) { fail("beam search: the device shim lacks tgx_beam_select / tgx_beam_advance or the per-row calls they ride on"); return true; }
  return processorsRefused(false);
}

GPTOutput GPTEngine::generateBeams(const std::vector<int32_t>& prompt, int32_t padToken) {
  GPTOutput out;
  const int K = config_.numBeams;
  int64_t S = 0;
  const std::vector<int64_t> ids = alignPrompts({prompt}, padToken, S);
  if (S == 0) { fail("generateSync: every prompt is empty (nothing to prefill)"); return out; }
  const int64_t n_new = std::max<int64_t>(1, config_.maxNewTokens);
  lastReused_ = 0; lastShifts_ = 0;
  cached_.clear();
  const auto t0 = std::chrono::steady_clock::now();
  auto dev = [&](int rc, const char* what) { if (rc != TGX_OK) fail(std::string("beam search: ") + what + ": " + be_.last_error(model_.ctx)); return rc == TGX_OK; };
  if (!dev(be_.reset_cache(model_.ctx), "reset_cache") || !dev(be_.forward_row(model_.ctx, 0, ids.data(), (int)S), "forward_row")) return out;
  const bool procOn = processorsOn();
  const auto procOff = at_exit([&] { if (procOn) processorsEnd(K); be_.reset_cache(model_.ctx); });
  if (procOn && !processorsBegin(0, ids.data(), S)) return out;
  // a copied child carries its parent's history words and automaton state; penalties and bias are settings, and a retired row's are back at their defaults
  auto settings = [&](int row) {
    if (!procOn) return true;
    const SamplerConfig& s = config_.samplerConfig;
    const tgx_penalty_cfg pc{s.repetitionPenalty, s.presencePenalty, s.frequencyPenalty};
    std::vector<int32_t> bi; std::vector<float> bv;
    for (const auto& kv : s.logitBias) { bi.push_back(kv.first); bv.push_back(kv.second); }
    return dev(be_.set_row_penalties(model_.ctx, row, &pc), "set_row_penalties") && dev(be_.set_row_logit_bias(model_.ctx, row, (int)bi.size(), bi.data(), bv.data()), "set_row_logit_bias");
  };
  BeamScorer scorer(K, config_.lengthPenalty, config_.earlyStopping, n_new, eosTokenIds_);
  std::vector<int32_t> rows(1, 0), group((size_t)K), placed((size_t)K);
  for (int b = 0; b < K; b++) group[(size_t)b] = b;
  std::vector<tgx_beam_cand> cands(TGX_MAX_BEAM_CAND);
  auto t1 = t0;
  for (int64_t step = 0;; step++) {
    int32_t n = 0;
    if (!dev(be_.beam_select(model_.ctx, (int)rows.size(), rows.data(), scorer.scores().data(), K, eosTokenIds_.empty() ? nullptr : eosTokenIds_.data(), (int)eosTokenIds_.size(), cands.data(), &n), "beam_select")) return out;
    if (step == 0) t1 = std::chrono::steady_clock::now();
    if (scorer.step(reinterpret_cast<const BeamCand*>(cands.data()), n)) break;
    const int m = (int)scorer.parents().size();
    const std::vector<int32_t>& from = step ? rows : group;      // the first step seats the group: row 0 and numBeams - 1 spares
    if (!dev(be_.beam_advance(model_.ctx, (int)from.size(), from.data(), m, scorer.parents().data(), scorer.tokens().data(), placed.data()), "beam_advance")) return out;
    rows.assign(placed.begin(), placed.begin() + m);
    for (int32_t r : rows) if (!settings(r)) return out;
    if (!dev(be_.decode_rows(model_.ctx, 1, nullptr, nullptr, nullptr), "decode_rows")) return out;
  }
  const std::vector<BeamHyp> hyps = scorer.finish();
  const int R = (int)std::min<size_t>((size_t)config_.numReturn, hyps.size());
  if (R < 1) { fail("beam search: no hypothesis (every candidate was masked)"); return out; }
  out.firstTokenMs = std::chrono::duration<double, std::milli>(t1 - t0).count();
  out.decodeMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  out.batch = R; out.newTokens = n_new;
  out.tokenIds.assign((size_t)(R * (S + n_new)), padToken);
  for (int b = 0; b < R; b++) {
    int32_t* row = out.tokenIds.data() + (size_t)b * (size_t)(S + n_new);
    for (int64_t i = 0; i < S; i++) row[i] = (int32_t)ids[(size_t)i];
    for (size_t i = 0; i < hyps[(size_t)b].tokens.size() && (int64_t)i < n_new; i++) row[S + (int64_t)i] = hyps[(size_t)b].tokens[i];
    out.beamScores.push_back(hyps[(size_t)b].score);
  }
  out.finishReason = hyps[0].length ? FinishReason::Length : FinishReason::Stop;
  return out;
}

GPTOutput GPTEngine::generateAsync(const std::vector<int32_t>& prompt, const GenerateCallback& callback) {
  GPTOutput out;
  if (!prepared_) { fail("generateAsync: engine not prepared"); return out; }
  if (config_.numBeams > 1) { fail("beam search: generateAsync streams one sequence; use generateSync (numBeams " + std::to_string(config_.numBeams) + ")"); return out; }
  if (logprobsRefused(true) || processorsRefused(true)) return out;
  verifyProcessedBegin();
  const auto verifyProcessedOff = at_exit([&] { verifyProcessedEnd(); });
  int64_t S = 0;
  std::vector<int64_t> ids = alignPrompts({prompt}, 0, S);
  if (S == 0) { fail("generateAsync: the prompt is empty (nothing to prefill)"); return out; }
  const tgx_sampler_cfg sc = to_c(config_.samplerConfig);
  const auto t0 = std::chrono::steady_clock::now();
  lastReused_ = 0;
  const bool reuse = reuseActive();
  if (!reuse || !prefillReusing(ids)) {
    if (reuse) be_.reset_cache(model_.ctx);      // (reconfigure left the cache in place; a failed truncate / extend pair ends here as well)
    if (be_.forward(model_.ctx, ids.data(), 1, (int)S) != TGX_OK) { cached_.clear(); fail(std::string("forward: ") + be_.last_error(model_.ctx)); return out; }
  }
  cached_.clear();      // (set again below, once the call knows what the cache holds)
  int64_t cur = 0;
  const bool lpOn = logprobsActive();
  std::vector<RowLogprobs> lpRows((size_t)(lpOn ? 1 : 0));
  const auto lpOff = at_exit([&] { if (lpOn) logprobsEnd(1); });
  const bool shift = shiftActive();
  const bool procOn = processorsOn(), specSampled = speculateSampledActive(1), perRow = lpOn || procOn || specSampled || shift;
  lastShifts_ = 0;
  const auto procOff = at_exit([&] { if (procOn) processorsEnd(1); });
  const auto samplerOff = at_exit([&] { if (specSampled) rowSamplerEnd(); });
  if (procOn && !processorsBegin(0, ids.data(), S)) return out;
  if (perRow) {
    std::vector<int64_t> first;
    if (!rowsBegin(1, sc, first) || (lpOn && !logprobsDrain(0, 1, lpRows[0]))) return out;
    cur = first[0];
  } else
  if (be_.sample(model_.ctx, &sc, config_.seed, &cur) != TGX_OK) { fail(std::string("sample: ") + be_.last_error(model_.ctx)); return out; }
  const auto t1 = std::chrono::steady_clock::now();
  std::vector<int32_t> tokens;
  for (int64_t i = 0; i < S; i++) tokens.push_back((int32_t)ids[(size_t)i]);
  tokens.push_back((int32_t)cur);

  bool hitEos = false, aborted = false, broke = false;
  if ((speculateActive(1) || perRow) && config_.maxNewTokens > 1) {      // (logprobs without speculate: the same consumer, fed one tgx_decode_rows step at a time)
    // The same consumer as the loop below — token i is checked for EOS and reported in iteration i, the maxNewTokens-th is appended unreported — fed from `seq`,
    // which grows by a verified draft or one step whenever the consumer runs dry.  EOS and the length stop the row on the device (tgx_set_row_stop), so a
    // draft is never accepted past either.
    std::vector<int32_t> seq = tokens;
    const int64_t maxNew = config_.maxNewTokens;
    bool finished = false;
    treeRefused_ = false;      // (GPTConfig::speculateTree: a refusal holds for one call)
    if (be_.set_row_stop(model_.ctx, 0, (int32_t)(maxNew - 1), eosTokenIds_.empty() ? nullptr : eosTokenIds_.data(), (int)eosTokenIds_.size()) != TGX_OK) {
      fail(std::string("set_row_stop: ") + be_.last_error(model_.ctx)); broke = true;
    }
    // GPTConfig::contextShift: the ids the cache holds, once the row has been shifted — `held` as of the last shift, then seq from `mark` on
    std::vector<int32_t> held;
    bool shifted = false;
    size_t mark = 0;
    auto heldNow = [&](int64_t past) {
      if (!shifted) return past <= (int64_t)seq.size() ? std::vector<int32_t>(seq.begin(), seq.begin() + past) : std::vector<int32_t>();
      std::vector<int32_t> h = held;
      const int64_t more = past - (int64_t)h.size();
      if (h.empty() || more < 0 || mark + (size_t)more > seq.size()) return std::vector<int32_t>();
      h.insert(h.end(), seq.begin() + (int64_t)mark, seq.begin() + (int64_t)mark + more);
      return h;
    };
    auto have = [&](int64_t k) {      // token k (1-based) of the generation is in seq
      while (!broke && (int64_t)seq.size() - S < k && !finished) {
        const size_t before = seq.size();
        if (shift && be_.past_length_row(model_.ctx, 0) >= contextSize()) {      // the next step would exceed the context: shift, which produces the next token
          int64_t next = 0;
          std::vector<int32_t> h = heldNow(be_.past_length_row(model_.ctx, 0));
          broke = !shiftRow(0, seq.back(), sc, &next, &h);
          if (!broke) {
            held = std::move(h); shifted = true; mark = seq.size();
            seq.push_back((int32_t)next);
            const int64_t rem = S + maxNew - (int64_t)seq.size();      // tgx_extend_row started the produced-token count afresh: the stop with what remains
            if (rem <= 0) finished = true;
            else if (be_.set_row_stop(model_.ctx, 0, (int32_t)rem, eosTokenIds_.empty() ? nullptr : eosTokenIds_.data(), (int)eosTokenIds_.size()) != TGX_OK) {
              fail(std::string("set_row_stop: ") + be_.last_error(model_.ctx)); broke = true;
            }
          }
        } else
        broke = !speculateMore(seq, S + maxNew, finished);
        if (!broke && lpOn) broke = !logprobsDrain(0, (int64_t)(seq.size() - before), lpRows[0]);
      }
      return !broke && (int64_t)seq.size() - S >= k;
    };
    int64_t count = 1;
    bool reported = false;
    for (int64_t i = 1; i < maxNew && !broke; i++) {
      if (!have(i)) { broke = true; break; }
      const int32_t tokenId = seq[(size_t)(S + i - 1)];
      count = i;
      if (isEosToken(tokenId)) { hitEos = true; break; }
      if (callback && !callback(tokenId)) { aborted = true; break; }
      reported = true;
    }
    if (!hitEos && !aborted && !broke && reported && have(maxNew)) count = maxNew;
    tokens.assign(seq.begin(), seq.begin() + (size_t)(S + count));
    out.firstTokenMs = std::chrono::duration<double, std::milli>(t1 - t0).count();
    out.decodeMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    if (reuse) {      // the cache holds every input of a pass or step that produced a token: all of seq but its last token
      const int64_t n_held = broke ? 0 : be_.past_length(model_.ctx);
      if (n_held >= 1 && (shifted || n_held <= (int64_t)seq.size())) cached_ = heldNow(n_held);
      else cached_.clear();
    }
    out.batch = 1;
    out.newTokens = (int64_t)tokens.size() - S;
    out.tokenIds = std::move(tokens);
    out.finishReason = (hitEos || aborted) ? FinishReason::Stop : FinishReason::Length;
    if (lpOn) logprobsStore(out, lpRows, out.newTokens);
    return out;
  }
  if (lpOn) logprobsStore(out, lpRows, 1);      // (one token asked for: the loop below takes no step, the first token's record is all there is)
  const bool pipelined = be_.step_async && be_.fetch_token;
  // ticket 0 names the token the last tgx_sample produced (T1); ticket k the token of the k-th step issued since
  int64_t ticket_cur = 0, pending = cur;
  bool have_pending_ticket = false;
  for (int64_t i = 1; i < config_.maxNewTokens; i++) {
    // submitToken(cur); futureToken = genNextToken(cur); tokenId = fetchTokenId()   (GPTEngine.cpp:197-200):
    // the next step is enqueued BEFORE the current id is read back, so the 4-byte read overlaps its compute.
    int32_t tokenId;
    int64_t ticket_next = 0, future = 0;
    if (pipelined) {
      if (be_.step_async(model_.ctx, &sc, config_.seed, &ticket_next) != TGX_OK) { fail(std::string("step: ") + be_.last_error(model_.ctx)); broke = true; break; }
      if (be_.fetch_token(model_.ctx, ticket_cur, &tokenId) != TGX_OK) { fail(std::string("fetch: ") + be_.last_error(model_.ctx)); broke = true; break; }
    } else {
      tokenId = (int32_t)pending;
      if (be_.decode(model_.ctx, &sc, config_.seed, 1, &future) != TGX_OK) { fail(std::string("decode: ") + be_.last_error(model_.ctx)); broke = true; break; }
    }
    if (i > 1) tokens.push_back(tokenId);      // the reference appended it at the end of the previous iteration (:215-216)
    if (isEosToken(tokenId)) { hitEos = true; break; }
    if (callback && !callback(tokenId)) { aborted = true; break; }
    ticket_cur = ticket_next;
    pending = future;
    have_pending_ticket = true;
  }
  if (!hitEos && !aborted && !broke && have_pending_ticket) {
    // loop ended by length: the last futureToken is part of the token list but was never reported
    int32_t last = (int32_t)pending;
    if (pipelined && be_.fetch_token(model_.ctx, ticket_cur, &last) != TGX_OK) fail(std::string("fetch: ") + be_.last_error(model_.ctx));
    tokens.push_back(last);
  }
  out.firstTokenMs = std::chrono::duration<double, std::milli>(t1 - t0).count();
  out.decodeMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  if (reuse) {      // every step appended its input token: the cache holds the first past_length ids of prompt + generated tokens
    const int64_t held = broke ? 0 : be_.past_length(model_.ctx);
    if (held >= 1 && held <= (int64_t)tokens.size()) cached_.assign(tokens.begin(), tokens.begin() + held);
    else cached_.clear();
  }
  out.batch = 1;
  out.newTokens = (int64_t)tokens.size() - S;
  out.tokenIds = std::move(tokens);
  out.finishReason = (hitEos || aborted) ? FinishReason::Stop : FinishReason::Length;
  return out;
}

// ---- text entry points ---------------------------------------------------------------------------------------------
int32_t GPTEngine::padTokenId() const {
  if (tokenizerOk_ && tokenizer_.padTokenId() >= 0) return tokenizer_.padTokenId();
  if (tokenizerOk_ && tokenizer_.eosTokenId() >= 0) return tokenizer_.eosTokenId();
  return 0;                                              // default pad token id (GPTEngine.cpp:112)
}

GPTOutput GPTEngine::generateSync(const std::vector<std::string>& texts) {
  if (!tokenizerOk_) { fail("generateSync(texts): no tokenizer loaded"); return GPTOutput(); }
  const std::vector<std::vector<int32_t>> prompts = tokenizer_.encodeBatch(texts);
  GPTOutput out = generateSync(prompts, padTokenId());
  if (out.batch > 0 && (constraintOn() || config_.numBeams > 1)) {      // a row's text ends where the row stopped: the stop id and the pad tokens behind it are not part of the match
    const size_t row = out.tokenIds.size() / (size_t)out.batch, S = row - (size_t)out.newTokens;
    for (int64_t b = 0; b < out.batch; b++) {
      std::vector<int32_t> ids;
      for (size_t i = S; i < row && !isEosToken(out.tokenIds[(size_t)b * row + i]); i++) ids.push_back(out.tokenIds[(size_t)b * row + i]);
      out.texts.push_back(tokenizer_.decode(ids));
    }
  } else
  if (out.batch > 0) out.texts = tokenizer_.decodeBatch(out.tokenIds, (uint32_t)out.batch, (uint32_t)(out.tokenIds.size() / (size_t)out.batch - (size_t)out.newTokens));
  return out;
}

GPTOutput GPTEngine::generateAsync(const std::string& text, const TextCallback& callback) {
  if (!tokenizerOk_) { fail("generateAsync(text): no tokenizer loaded"); return GPTOutput(); }
  tokenizer_.decodeStreamFlush();                        // a fresh stream
  bool aborted = false;
  const std::vector<int32_t> prompt = tokenizer_.encode(text);
  GPTOutput out = generateAsync(prompt, [&](int32_t id) {
    const std::string chunk = tokenizer_.decodeStream({id});
    if (!chunk.empty() && callback && !callback(chunk)) { aborted = true; return false; }
    return true;
  });
  if (!aborted) {                                        // flush bytes of an unfinished character (:219-227)
    const std::string rest = tokenizer_.decodeStreamFlush();
    if (!rest.empty() && callback) callback(rest);
  }
  if (out.batch > 0) out.texts = tokenizer_.decodeBatch(out.tokenIds, 1, (uint32_t)(out.tokenIds.size() - (size_t)out.newTokens));
  return out;
}

// ---------------------------------------------------------------------------------------------------------------
// synthetic checkpoints (bit-identical to tinygpt_amd/synth.py)
// ---------------------------------------------------------------------------------------------------------------
namespace {

inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline uint64_t fnv1a64(const std::string& s) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (unsigned char b : s) h = (h ^ b) * 0x100000001B3ull;
  return h;
}
inline uint16_t f32_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
bool ends_with(const std::string& s, const char* suf) { size_t n = strlen(suf); return s.size() >= n && !s.compare(s.size() - n, n, suf); }

}  // namespace

void synth_tensor_bf16(uint64_t seed, const std::string& name, size_t n, double std_dev, uint16_t* out) {
  const uint64_t base = fnv1a64(name) ^ (seed * 0xD1342543DE82EF95ull);
  // leaf module name decides the distribution: norm weights are 1 + U(-0.1, 0.1)
  std::string leaf, last;
  {
    size_t k = name.find_last_of('.');
    last = k == std::string::npos ? name : name.substr(k + 1);
    std::string rest = k == std::string::npos ? "" : name.substr(0, k);
    size_t k2 = rest.find_last_of('.');
    leaf = k2 == std::string::npos ? rest : rest.substr(k2 + 1);
  }
  const bool is_norm = last == "weight" && (ends_with(leaf, "norm") || ends_with(leaf, "layernorm") || leaf == "ln_1" || leaf == "ln_2" || leaf == "ln_f");
  const float lo = is_norm ? 1.0f : 0.0f;
  const float a = is_norm ? 0.1f : (float)(std_dev * 1.7320508);
  const float two_a = 2.0f * a;
  const unsigned nthreads = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
  auto work = [&](size_t s, size_t e) {
    for (size_t i = s; i < e; i++) {
      const uint64_t z = splitmix64(base + (uint64_t)i * 0x9E3779B97F4A7C15ull);
      const float u24 = (float)(z >> 40);
      const float f = (u24 * 5.9604644775390625e-08f - 0.5f) * two_a + lo;
      out[i] = f32_to_bf16(f);
    }
  };
  if (n < (1u << 20) || nthreads == 1) { work(0, n); return; }
  std::vector<std::thread> th;
  const size_t per = (n + nthreads - 1) / nthreads;
  for (unsigned t = 0; t < nthreads; t++) { size_t s = t * per, e = std::min(n, s + per); if (s < e) th.emplace_back(work, s, e); }
  for (auto& t : th) t.join();
}

bool known_config(const std::string& key, int compute_dtype, int max_batch, ModelConfig& out) {
  struct K { const char* name; int fam, H, L, nh, nkv, I, V, tied, bias, ctx; float eps, theta; int scaled; };
  static const K table[] = {
      {"llama-3.2-1b", TGX_FAMILY_LLAMA, 2048, 16, 32, 8, 8192, 128256, 1, 0, 131072, 1e-5f, 500000.f, 1},
      {"llama-3.2-3b", TGX_FAMILY_LLAMA, 3072, 28, 24, 8, 8192, 128256, 1, 0, 131072, 1e-5f, 500000.f, 1},
      {"qwen2.5-0.5b", TGX_FAMILY_QWEN2, 896, 24, 14, 2, 4864, 151936, 1, 1, 32768, 1e-6f, 1000000.f, 0},
      {"mistral-7b-v0.3", TGX_FAMILY_MISTRAL, 4096, 32, 32, 8, 14336, 32768, 0, 0, 32768, 1e-5f, 1000000.f, 0},
      {"qwen2.5-3b", TGX_FAMILY_QWEN2, 2048, 36, 16, 2, 11008, 151936, 1, 1, 32768, 1e-6f, 1000000.f, 0},
      {"llama-3.1-70b", TGX_FAMILY_LLAMA, 8192, 80, 64, 8, 28672, 128256, 0, 0, 131072, 1e-5f, 500000.f, 2},
  };
  if (key == "gpt2") {   // GPT-2 124M (BASELINE.json configs[0]): head = wte, n_ctx = n_positions = 1024
    out = ModelConfig();
    tgx_model_desc& d = out.desc;
    d.family = TGX_FAMILY_GPT2; d.hidden = 768; d.layers = 12; d.heads = d.kv_heads = 12; d.head_dim = 64; d.inter = 3072; d.vocab = 50257;
    d.max_ctx = 1024; d.n_positions = 1024; d.qkv_bias = 1; d.tied = 1; d.compute_dtype = compute_dtype; d.norm_eps = 1e-5f;
    d.max_batch = max_batch < 1 ? 1 : max_batch;
    out.model_type = "gpt2";
    return true;
  }
  if (key == "qwen3-1.7b") {
    out = ModelConfig();
    tgx_model_desc& d = out.desc;
    d.family = TGX_FAMILY_QWEN3; d.hidden = 2048; d.layers = 28; d.heads = 16; d.kv_heads = 8; d.head_dim = 128; d.inter = 6144; d.vocab = 151936;
    d.max_ctx = 40960; d.tied = 1; d.qk_norm = 1; d.compute_dtype = compute_dtype; d.norm_eps = 1e-6f; d.rope_theta = 1000000.f;
    d.max_batch = max_batch < 1 ? 1 : max_batch;
    out.model_type = "qwen3";
    return true;
  }
  if (key == "qwen3-0.6b") {   // explicit head_dim (q_dim 2048 != hidden 1024), per-head q/k RMSNorm (ModelQwen3.h:23-40)
    out = ModelConfig();
    tgx_model_desc& d = out.desc;
    d.family = TGX_FAMILY_QWEN3; d.hidden = 1024; d.layers = 28; d.heads = 16; d.kv_heads = 8; d.head_dim = 128; d.inter = 3072; d.vocab = 151936;
    d.max_ctx = 40960; d.tied = 1; d.qk_norm = 1; d.compute_dtype = compute_dtype; d.norm_eps = 1e-6f; d.rope_theta = 1000000.f;
    d.max_batch = max_batch < 1 ? 1 : max_batch;
    out.model_type = "qwen3";
    return true;
  }
  for (const K& k : table) {
    if (key != k.name) continue;
    out = ModelConfig();
    tgx_model_desc& d = out.desc;
    d.family = k.fam; d.hidden = k.H; d.layers = k.L; d.heads = k.nh; d.kv_heads = k.nkv; d.head_dim = k.H / k.nh;
    d.inter = k.I; d.vocab = k.V; d.max_ctx = k.ctx; d.qkv_bias = k.bias; d.tied = k.tied; d.compute_dtype = compute_dtype;
    d.norm_eps = k.eps; d.rope_theta = k.theta; d.max_batch = max_batch < 1 ? 1 : max_batch;
    if (k.scaled) { d.rope_factor = k.scaled == 2 ? 8.f : 32.f; d.rope_high_freq = 4.f; d.rope_low_freq = 1.f; d.rope_orig_ctx = 8192; d.max_ctx = 8192; }
    out.model_type = k.fam == TGX_FAMILY_LLAMA ? "llama" : k.fam == TGX_FAMILY_QWEN2 ? "qwen2" : "mistral";
    return true;
  }
  return false;
}

bool load_synthetic(const Backend& be, const ModelConfig& cfg, int device_ordinal, uint64_t seed, double std_dev, tgx_ctx** ctx, std::string& err,
                    const LoadOptions& opts) {
  const tgx_model_desc& d = cfg.desc;
  if (be.create(&d, device_ordinal, ctx) != TGX_OK) { err = std::string("create failed: ") + be.last_error(*ctx); if (*ctx) be.destroy(*ctx); *ctx = nullptr; return false; }
  if (!apply_load_options(be, *ctx, opts, err)) { be.destroy(*ctx); *ctx = nullptr; return false; }
  const int64_t H = d.hidden, I = d.inter, V = d.vocab, qd = (int64_t)d.heads * d.head_dim, kvd = (int64_t)d.kv_heads * d.head_dim;
  std::vector<uint16_t> buf;
  auto put = [&](const std::string& name, int64_t r, int64_t c) -> bool {
    const size_t n = (size_t)(c < 0 ? r : r * c);
    buf.resize(n);
    synth_tensor_bf16(seed, name, n, std_dev, buf.data());
    int64_t shape[2] = {r, c};
    if (be.upload(*ctx, name.c_str(), buf.data(), shape, c < 0 ? 1 : 2, TGX_BF16) != TGX_OK) { err = be.last_error(*ctx); return false; }
    return true;
  };
  if (d.family == TGX_FAMILY_GPT2) {   // hub layout, Conv1D weights [in][out] (ModelGPT2.h:26,226); same names and shapes as desc.py
    bool ok = put("wte.weight", V, H) && put("wpe.weight", d.n_positions, H);
    for (int l = 0; ok && l < d.layers; l++) {
      const std::string p = "h." + std::to_string(l) + ".";
      ok = put(p + "ln_1.weight", H, -1) && put(p + "ln_1.bias", H, -1) && put(p + "attn.c_attn.weight", H, 3 * H) && put(p + "attn.c_attn.bias", 3 * H, -1) &&
           put(p + "attn.c_proj.weight", H, H) && put(p + "attn.c_proj.bias", H, -1) && put(p + "ln_2.weight", H, -1) && put(p + "ln_2.bias", H, -1) &&
           put(p + "mlp.c_fc.weight", H, I) && put(p + "mlp.c_fc.bias", I, -1) && put(p + "mlp.c_proj.weight", I, H) && put(p + "mlp.c_proj.bias", H, -1);
    }
    ok = ok && put("ln_f.weight", H, -1) && put("ln_f.bias", H, -1);
    if (ok && be.finalize(*ctx) != TGX_OK) { err = be.last_error(*ctx); ok = false; }
    if (!ok) { be.destroy(*ctx); *ctx = nullptr; }
    return ok;
  }
  bool ok = put("model.embed_tokens.weight", V, H);
  for (int l = 0; ok && l < d.layers; l++) {
    const std::string p = "model.layers." + std::to_string(l) + ".";
    ok = put(p + "input_layernorm.weight", H, -1) && put(p + "self_attn.q_proj.weight", qd, H) && put(p + "self_attn.k_proj.weight", kvd, H) &&
         put(p + "self_attn.v_proj.weight", kvd, H);
    if (ok && d.qkv_bias) ok = put(p + "self_attn.q_proj.bias", qd, -1) && put(p + "self_attn.k_proj.bias", kvd, -1) && put(p + "self_attn.v_proj.bias", kvd, -1);
    if (ok && d.qk_norm) ok = put(p + "self_attn.q_norm.weight", d.head_dim, -1) && put(p + "self_attn.k_norm.weight", d.head_dim, -1);
    ok = ok && put(p + "self_attn.o_proj.weight", H, qd) && put(p + "post_attention_layernorm.weight", H, -1) &&
         put(p + "mlp.gate_proj.weight", I, H) && put(p + "mlp.up_proj.weight", I, H) && put(p + "mlp.down_proj.weight", H, I);
  }
  ok = ok && put("model.norm.weight", H, -1);
  if (ok && !d.tied) ok = put("lm_head.weight", V, H);
  if (ok && be.finalize(*ctx) != TGX_OK) { err = be.last_error(*ctx); ok = false; }
  if (!ok) { be.destroy(*ctx); *ctx = nullptr; }
  return ok;
}

}  // namespace tgxh
