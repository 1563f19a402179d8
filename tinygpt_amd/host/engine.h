// engine.h — the host engine above the C ABI: the counterpart of GPTEngine (src/engine/GPTEngine.h:42-73,
// GPTEngine.cpp:37-232).  Text entry points (tokenizer.h) and token-id entry points share one path: encode,
// left-padding without a mask, tail truncation to contextSize, prefill + maxNewTokens-1 decode steps, no EOS stop in
// generateSync, one-step-lookahead streaming with EOS/abort and UTF-8-safe chunks in generateAsync, reconfigure()
// resetting the KV cache — the reference's behaviour line by line.
#pragma once
#include <cstdint>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "backend.h"
#include "constraint.h"
#include "loader.h"
#include "spec_draft.h"
#include "tokenizer.h"

namespace tgxh {

struct SamplerConfig {   // src/engine/Sampler.h:13-22
  float temperature = 0.f;
  int64_t topK = 0;
  float topP = 1.f;
  float minP = 0.f;
  // Not in the reference (the completions protocol's presence_penalty / frequency_penalty / logit_bias and HF's repetition_penalty; include/tgx.h
  // tgx_set_row_penalties).  The neutral defaults leave the generate loops exactly as they were.  Any non-neutral value: the engine steps through tgx_sample_row /
  // tgx_decode_rows (the shape the `logprobs` path has), sets every row's history from the prompt it admitted (pad tokens are not counted) and switches the rows
  // back to neutral when the call ends; `speculate` falls back to plain steps.  A backend without the calls FAILS the generate call with a message (lastError).
  // generation_config.json's repetition_penalty is NOT applied by default: the reference ignores it.
  float repetitionPenalty = 1.f;
  float presencePenalty = 0.f;
  float frequencyPenalty = 0.f;
  std::map<int32_t, float> logitBias;      // id -> value added to the id's logit; -INFINITY bans the id
  // Constrained decoding (constraint.h states the supported subset; include/tgx.h tgx_automaton_create): empty = off.  Otherwise every row's output must match the
  // pattern as a whole.  The engine compiles it over its tokenizer into a token automaton (on reconfigure / prepare, and the same pattern twice compiles once), with
  // its EOS ids and extra stop ids allowed exactly where a match may end; it sets every row's automaton at its admission, steps through the per-row path the
  // penalties take, stops every row on the device at such an id and switches the rows off when the call ends.  `speculate` falls back to plain steps.  A row that
  // stops has produced a full match (finish reason Stop; generateSync: when every row stopped; positions of a row behind its stop hold the pad token); a row that
  // maxNewTokens ends first has produced a PREFIX of a match, finish reason Length.  A backend without the calls, no tokenizer, a tokenizer that is not ByteLevel,
  // more stop ids than TGX_MAX_STOP_IDS or a failed compile FAILS the generate call with a message (lastError).
  std::string regex;
  bool processorsNeutral() const { return repetitionPenalty == 1.f && presencePenalty == 0.f && frequencyPenalty == 0.f && logitBias.empty() && regex.empty(); }
};

enum class FinishReason { Stop, Length };

struct GPTConfig {       // src/engine/GPTEngine.h:25-32 (+ where to find the device shim)
  std::string modelDir;              // HF directory; empty with `synthetic` set
  std::string synthetic;             // "llama-3.2-1b" ...: deterministic synthetic checkpoint of that public config
  std::string device = "mi355x";     // the reference's CLI knows "cpu" and "cuda" (main.cpp:76-80)
  int dtype = TGX_BF16;
  SamplerConfig samplerConfig;
  int64_t maxNewTokens = 16;
  int deviceOrdinal = 0;
  int maxBatch = 4;
  uint64_t seed = 0;
  std::string tokenizerDir;          // tokenizer.json + tokenizer_config.json; default: modelDir (lets --synthetic runs take text)
  // Not in the reference (its engine resets the cache per request and prefills the whole conversation again): generateAsync keeps row 0's KV cache between calls
  // and prefills only what follows the longest prefix the new prompt shares with it (tgx_truncate_row + tgx_extend_row).  Needs a backend with both symbols;
  // generateSync and any failure of the two calls take the reset path.
  bool reusePrefix = false;
  // Not in the reference (its generation ends at contextSize()): generation past the context.  Off by default: every run as it was.  With it set and a backend that
  // exports tgx_splice_row (and the per-row calls), the generate loops step through tgx_sample_row / tgx_decode_rows, never more steps per call than the row that
  // holds the most positions has room for, and a row whose next step would exceed contextSize() is SHIFTED (include/tgx.h tgx_splice_row): with
  // n_keep = min(shiftKeep, past - 1) and n_discard = (past - n_keep) / 2 it keeps [0, n_keep) + [n_keep + n_discard, past), its current token is fed again
  // (tgx_extend_row of one token), the next token is sampled from that (tgx_sample_row) and the row's stop is restated with what remains of maxNewTokens
  // (tgx_extend_row starts the produced-token count afresh).  reusePrefix's record of what row 0 holds is spliced the same way.  A sampled row's draw key hashes
  // the position, and positions repeat after a shift: a sampled run draws position p's variate again the second time it reaches p.
  // A shiftKeep that keeps all but one of a full row's positions leaves nothing to discard: the generate call then ends there with a message that names it.
  // While it is on no drafts are proposed (speculate), and a prompt is still cut to contextSize() before its prefill, keeping the tail.  generateSync's rows are
  // aligned to one length, so they fill up — and shift — at the same step unless a regex ends one early.
  bool contextShift = false;
  int shiftKeep = 0;
  // Not in the reference: greedy speculative decoding with prompt lookup (spec_draft.h).  0 = off: the loops below exactly as they were.  N > 0: up to N draft
  // tokens (clamped to TGX_MAX_DRAFT) are proposed per iteration and verified in one pass (tgx_verify_row); without a match one ordinary step runs.  Active only
  // for a greedy sampler configuration, ONE sequence, at most TGX_MAX_STOP_IDS EOS ids and a backend that has the calls — otherwise the existing loop runs.  The
  // produced ids are those of the existing loop up to the summation order between kernel paths (include/tgx.h tgx_verify_row).  A backend that exports
  // tgx_verify_rows lifts "one sequence" in generateSync: every row of the batch drafts on its own sequence and all rows advance through one joint call.
  int speculate = 0;
  // ... and under a SAMPLING configuration (default false: every existing run is unchanged).  With it set, speculate > 0, one sequence, a non-greedy sampler,
  // neutral processors and a backend that exports tgx_verify_row_sampled, the generate loops take the per-row path: the row's sampler is the call's
  // (tgx_set_row_sampler), the first token comes from tgx_sample_row, prompt-lookup drafts go through tgx_verify_row_sampled and steps without a draft through
  // tgx_decode_rows.  A sampled token is a pure function of its logits and the draw key (seed, token index, row), so the ids are those of the plain loop up to
  // the summation order between kernel paths.  A backend without the call keeps the old loop.
  bool speculateSampled = false;
  // ... and with logit processors on (default false: every existing run is unchanged — `speculate` falls back to plain steps while a penalty, a logit bias or a
  // regex is on).  With it set and a backend that takes option "verify.processors" (include/tgx.h), the engine sets that option for the length of the generate
  // call and keeps drafting: the verify calls process every position of a pass as the row's step would have, so the ids are those of speculate = 0.  Under a
  // sampling configuration speculateSampled is needed as well; speculateTree falls back to chains (the device refuses a processed row on a tree that is no chain).
  bool speculateProcessed = false;
  // ... with a token TREE of guesses (default 0 = off: every existing run is unchanged; 1 is the same as 0 — one branch is a chain).  B >= 2 (needs speculate > 0;
  // ONE sequence): where the sequence's tail has
  // occurred before with different continuations, up to B of them share the pass's `speculate` positions as branches below the current token (spec_draft.h
  // ngram_tree) and the device follows whichever the row produces (include/tgx.h tgx_verify_tree); the first branch is the chain `speculate` alone would draft,
  // cut to its share.  One candidate is a chain and goes the chain's way.  Where the device refuses a tree with TGX_ERR_UNSUPPORTED (fp32 storage, GPT-2, log-
  // probability records, ..) the engine falls back to chain drafts for the rest of the call.  The ids are those of speculate = 0, as for the chain.
  int speculateTree = 0;
  // Not in the reference's engine (its server speaks the completions protocol's `logprobs`): -1 = off, the loops below exactly as they were.  N in
  // [0, TGX_MAX_LOGPROBS]: every produced token comes with its log-probability under the model's distribution and the N most likely alternatives
  // (include/tgx.h tgx_set_row_logprobs).  The engine then steps through tgx_sample_row / tgx_decode_rows (tgx_verify_row under `speculate`) and drains the rows'
  // record rings before they can wrap; the ids are those of the existing loops (tgx_decode_rows' draw identity).  generateSync drains once per tgx_decode_rows call
  // of up to 128 steps (or per verify pass).  generateAsync reports token by token, so it takes ONE tgx_decode_rows step and ONE ring read per token (each
  // synchronises the stream; a verified draft under `speculate` covers several tokens per read): the one-step lookahead of the plain loop is given up.
  // A request that cannot be served FAILS the generate call with a message (lastError): N > TGX_MAX_LOGPROBS, a backend without the calls, and in generateAsync
  // more EOS / stop ids than TGX_MAX_STOP_IDS (the row stops on the device).
  int logprobs = -1;
  // Not in the reference: beam search (include/tgx.h tgx_beam_select / tgx_beam_advance; beam.h holds the rules).  numBeams 1 = off: every loop as it was.  With
  // numBeams > 1, generateSync of ONE prompt prefills it into row 0, selects with n = 1, advances 1 -> numBeams, and then per step runs tgx_decode_rows(1) + select +
  // advance on numBeams rows; it returns numReturn rows, best first (a row's tokens behind its end are the pad token), and GPTOutput::beamScores.  A finished
  // hypothesis scores sum_lp / L^lengthPenalty; earlyStopping ends the search once numBeams hypotheses are finished.  SamplerConfig::regex and the penalties compose
  // (the select reads the processed vector).  The generate call FAILS with a message (lastError): a non-greedy sampler, several prompts, generateAsync, speculate /
  // logprobs / contextShift together with beams, maxBatch < numBeams, numBeams > TGX_MAX_BEAMS, numReturn outside [1, numBeams], more EOS ids than
  // TGX_MAX_STOP_IDS, a backend without the two calls.
  int numBeams = 1;
  float lengthPenalty = 1.f;
  bool earlyStopping = false;
  int numReturn = 1;
  // Not in the reference: FP8 weights (include/tgx.h option "weights.fp8"; default false: every run as it was).  Opt-in and LOSSY: the loader sets the option
  // between tgx_create and tgx_finalize, which quantizes the gate_up, down and lm_head matrices to E4M3 codes with a power-of-two scale per row — every path then
  // computes the quantized model, and the batch-1 step streams half the bytes of those matrices.  It costs one more byte per quantized weight of device memory.
  // prepare() FAILS with a message that names the option when the backend has no tgx_set_option or refuses the key, and when tgx_finalize refuses the model
  // (a storage dtype other than bf16, GPT-2, a non-finite weight): it never continues unquantized.
  bool weightsFp8 = false;
#ifdef TGXH_TEST_HOOKS
  // Only in the test build (tests/_build/libtgx_host_test.so, tgx_cli_test: -DTGXH_TEST_HOOKS): bind another library that exports the tgx ABI
  // (the CPU oracle) to check host logic without a GPU.  The shipped library and CLI do not contain these fields or the code that reads them:
  // they can only dlopen libtgx_mi355x.so from their own directory.  LAST in the struct: every field above keeps its offset in both builds.
  std::string backendLib;
  std::string backendPrefix = "tgx_";
#endif
};

struct GPTOutput {       // src/engine/GPTEngine.h:34-40
  int64_t batch = 0;
  int64_t newTokens = 0;
  std::vector<int32_t> tokenIds;     // [batch][padded prompt + new], row-major — prompt tokens included, like the reference
  std::vector<std::string> texts;    // the new tokens of every row, decoded (text entry points only)
  FinishReason finishReason = FinishReason::Stop;
  // not in the reference's struct: the generate call split at the first token (SURVEY.md §8 row H asks the harness for decode-only tok/s)
  double firstTokenMs = 0.0;         // encode-to-first-token: prefill + first sample
  double decodeMs = 0.0;             // the remaining newTokens-1 steps
  // GPTConfig::logprobs >= 0: the log-probability of every new token [batch][newTokens] and its topLogprobs alternatives [batch][newTokens][topLogprobs] as
  // (id, logprob), most likely first; empty otherwise
  std::vector<double> beamScores;    // GPTConfig::numBeams > 1: the score of every returned row (sum_lp / L^lengthPenalty), best first; empty otherwise
  int topLogprobs = 0;
  std::vector<float> logprobs;
  std::vector<int32_t> topIds;
  std::vector<float> topLogprobValues;
};

// what GPTConfig::speculate did since prepare(): verify passes, the draft tokens they carried and how many of those were accepted, ordinary steps taken for want
// of a draft, and the histogram of tokens produced per verify pass (1 = the draft's first token was wrong .. TGX_MAX_DRAFT + 1)
struct SpecStats {
  int64_t verifyCalls = 0, draftTokens = 0, acceptedDrafts = 0, plainSteps = 0;
  int64_t producedHist[TGX_MAX_DRAFT + 2] = {};
  int64_t treePasses = 0;      // of verifyCalls: passes over a tree of two or more branches (GPTConfig::speculateTree)
};

// GPTEngine::score: the log-probability of tokenIds[i + 1] under the model's distribution after tokenIds[0 .. i], for i in [0, n - 1) — n - 1 values, one per
// supplied token but the first — and, with topN >= 1, each position's topN most likely tokens as (id, logprob), most likely first (include/tgx.h tgx_score_row)
struct ScoreOutput {
  bool ok = false;
  std::vector<int32_t> tokenIds;     // what was scored (a text after the tokenizer; a sequence beyond contextSize keeps its tail, like a prompt)
  int64_t dropped = 0;               // tokens of the supplied sequence ahead of that tail: logprobs[i] belongs to the supplied token dropped + i + 1
  int topLogprobs = 0;
  std::vector<float> logprobs;       // [n - 1]
  std::vector<int32_t> topIds;       // [n - 1][topLogprobs]
  std::vector<float> topLogprobValues;
  double perplexity() const;         // exp(-mean logprob); 0 with nothing scored
};

// GPTEngine::embed: how the final hidden states of a text become one vector (include/tgx.h tgx_embed_rows) and what comes back
struct EmbedConfig {
  int pool = TGX_POOL_LAST;          // TGX_POOL_LAST / TGX_POOL_MEAN / TGX_POOL_FIRST
  bool normalize = true;             // divide by the L2 norm
  int dims = 0;                      // 0: the hidden size; else keep the first dims components (before normalisation)
};
struct EmbedOutput {
  bool ok = false;
  int dims = 0;                      // components per vector
  int64_t calls = 0;                 // tgx_embed_rows calls the texts were batched into
  std::vector<float> vectors;        // [texts][dims]
  std::vector<int64_t> dropped;      // per text: tokens ahead of the tail that was embedded (a text beyond contextSize keeps its tail, like a prompt)
};

using GenerateCallback = std::function<bool(int32_t tokenId)>;   // return false to abort (GPTEngine.cpp:208-213)
using TextCallback = std::function<bool(const std::string& chunk)>;   // the reference's GenerateCallback: complete UTF-8 only

class GPTEngine {
 public:
  explicit GPTEngine(GPTConfig config);
  ~GPTEngine();
  GPTEngine(const GPTEngine&) = delete;
  GPTEngine& operator=(const GPTEngine&) = delete;

  bool prepare();                                                            // GPTEngine.cpp:41-65
  void reconfigure(const SamplerConfig& samplerConfig, int64_t maxNewTokens,
                   const std::vector<int32_t>& extraStopTokenIds = {});      // GPTEngine.cpp:67-84
  GPTOutput generateSync(const std::vector<std::vector<int32_t>>& prompts, int32_t padToken);   // :154-174
  GPTOutput generateAsync(const std::vector<int32_t>& prompt, const GenerateCallback& callback);   // :180-232
  // text entry points (need a tokenizer: tokenizerDir / modelDir must hold tokenizer.json + tokenizer_config.json)
  GPTOutput generateSync(const std::vector<std::string>& texts);                                   // :154-174 incl. encodeTexts :101-144
  GPTOutput generateAsync(const std::string& text, const TextCallback& callback);                  // :180-232 incl. decodeStream
  // Not in the reference: score a supplied sequence in ONE prefill pass on row 0 of a reset cache, which it leaves empty again; generates nothing.  ok == false (lastError set): a backend
  // without tgx_score_row, topN outside [0, TGX_MAX_LOGPROBS], an empty sequence, no tokenizer for the text form, or a failed call
  ScoreOutput score(const std::vector<int32_t>& ids, int topN = 0);
  ScoreOutput score(const std::string& text, int topN = 0);
  // Not in the reference: one vector per text — the pooled final-norm hidden state (include/tgx.h tgx_embed_rows), no lm_head.  The texts go through calls of at most
  // max_batch rows of an empty cache, each releasing its rows, and the cache is left empty; generates nothing.  ok == false (lastError set), NOTHING changed: a backend
  // without tgx_embed_rows, no text or an empty one, a bad pool or dims, no tokenizer for the text form, or an engine that holds a conversation in row 0 (prefix reuse:
  // the rows of the call would collide with it — setReusePrefix(false) or a generate call without reuse first).  A failed device call leaves the cache empty
  EmbedOutput embed(const std::vector<std::vector<int32_t>>& ids, const EmbedConfig& cfg = {});
  EmbedOutput embed(const std::vector<std::string>& texts, const EmbedConfig& cfg = {});
  // Not in the reference: the conversation row 0's cache holds (GPTConfig::reusePrefix), kept across processes.  saveSession writes a small header (magic "TGXSESS\0",
  // u32 version 1, u32 count, the count cached token ids as i32, u64 snapshot bytes) followed by row 0's snapshot (include/tgx.h tgx_save_row) WITHOUT its hidden row,
  // logits and token (csrc/row_snapshot.h drop_logits, on the host): the next turn extends the row and computes its own, and 4 * (hidden + vocab) bytes stay out of the
  // file.  (A deviation from rolling the row back by one position before the save: that would leave the reloaded engine one reusable position short of the engine
  // that never stopped, and it would change the live row; the price is a second producer of the snapshot format, checked by tests/row_snapshot_check.cpp.)
  // loadSession validates the whole file against this engine's model before anything changes, then restores row 0 of a reset cache and takes over the ids: the
  // next generateAsync prefills only what follows the shared prefix (lastReused()).  Both need prefix reuse active and a backend with the snapshot calls; false
  // with lastError set otherwise.  A missing, truncated or mismatching file is rejected by that validation and leaves the engine as it was; should tgx_restore_row
  // itself fail behind it (a device allocation), the engine is left with an EMPTY cache and serves the next call from scratch.
  // saveSession needs the conversation generateAsync left in row 0: a call that ran the per-row path to its end (GPTConfig::speculate, logprobs, or a non-neutral
  // penalty / logit bias — the row then finishes on the device by its stop conditions and its cache is not kept for reuse) leaves nothing to save, and saveSession
  // returns false with a message.  Little-endian, like the snapshot.
  bool saveSession(const std::string& path);
  bool loadSession(const std::string& path);
  bool hasTokenizer() const { return tokenizerOk_; }
  Tokenizer& tokenizer() { return tokenizer_; }
  int32_t padTokenId() const;                                                                       // pad -> eos -> 0 (:108-114)

  bool isEosToken(int32_t id) const;
  const std::vector<int32_t>& eosTokenIds() const { return eosTokenIds_; }
  int64_t contextSize() const;
  const tgx_model_desc& desc() const { return model_.config.desc; }
  const std::string& lastError() const { return err_; }
  tgx_ctx* ctx() { return model_.ctx; }
  const Backend& backend() const { return be_; }
  void setReusePrefix(bool on) {
    if (!on && reuseActive() && model_.ctx) be_.reset_cache(model_.ctx);      // (as reconfigure would have left it)
    config_.reusePrefix = on;
    cached_.clear();
  }
  void setContextShift(bool on, int keep) { config_.contextShift = on; config_.shiftKeep = keep < 0 ? 0 : keep; }
  int64_t lastShifts() const { return lastShifts_; }      // context shifts the last generate call made, over all its rows
  int64_t lastReused() const { return lastReused_; }      // prompt tokens the last generate call served from the cache
  void setSpeculate(int maxDraft) { config_.speculate = maxDraft; }
  void setSpeculateSampled(bool on) { config_.speculateSampled = on; }
  void setSpeculateProcessed(bool on) { config_.speculateProcessed = on; }
  void setSpeculateTree(int branches) { config_.speculateTree = branches; }
  void setLogprobs(int topN) { config_.logprobs = topN; }
  const SamplerConfig& samplerConfig() const { return config_.samplerConfig; }
  void setProcessors(float repetition, float presence, float frequency, std::map<int32_t, float> bias) {      // kept by the C view across tgxe_reconfigure
    config_.samplerConfig.repetitionPenalty = repetition; config_.samplerConfig.presencePenalty = presence; config_.samplerConfig.frequencyPenalty = frequency;
    config_.samplerConfig.logitBias = std::move(bias);
  }
  void setBeams(int numBeams, float lengthPenalty, bool earlyStopping, int numReturn) {      // kept by the C view across tgxe_reconfigure
    config_.numBeams = numBeams; config_.lengthPenalty = lengthPenalty; config_.earlyStopping = earlyStopping; config_.numReturn = numReturn;
  }
  void setRegex(std::string pattern) { config_.samplerConfig.regex = std::move(pattern); }      // kept by the C view across tgxe_reconfigure, like setProcessors
  const SpecStats& specStats() const { return spec_; }

 private:
  // == encodeTexts minus the tokenizer (GPTEngine.cpp:101-144): truncate to contextSize keeping the tail, left-pad
  std::vector<int64_t> alignPrompts(const std::vector<std::vector<int32_t>>& prompts, int32_t padToken, int64_t& maxLen) const;
  bool fail(const std::string& what);
  bool reuseActive() const { return config_.reusePrefix && be_.extend_row && be_.truncate_row; }
  bool sessionCapable(const char* what);                       // prefix reuse active and the backend has the snapshot calls; else err_ set
  bool prefillReusing(const std::vector<int64_t>& ids);      // the prompt after its cached prefix; false: nothing reusable (the caller resets and prefills)
  bool shiftActive() const {
    return config_.contextShift && be_.splice_row && be_.extend_row && be_.sample_row && be_.set_row_sampler && be_.set_row_stop && be_.decode_rows && be_.past_length_row;
  }
  // the shift of `row`, whose current token is cur and whose cache is full: splice, feed cur again, sample the next token into *next.  held (may be null): the ids
  // the row's cache holds, kept in step.  false: a call failed (err_ set)
  bool shiftRow(int row, int32_t cur, const tgx_sampler_cfg& sc, int64_t* next, std::vector<int32_t>* held);
  bool speculateActive(int batch) const;                      // GPTConfig::speculate applies to this call
  bool speculateSampledActive(int batch) const;               // ... through tgx_verify_row_sampled (GPTConfig::speculateSampled; spec_mode.h)
  // row 0 holds seq minus its last token, which is its current token; the row's stop conditions are set.  Drafts from seq, verifies (or takes one ordinary
  // step), appends what the row produced — never more than maxTotal tokens in seq.  finished: the row finished on the device.  false: a call failed (err_ set)
  bool speculateMore(std::vector<int32_t>& seq, int64_t maxTotal, bool& finished);
  // the same for a batch (the backend exports tgx_verify_rows): seqs[b] as seq above for row b, every unfinished row advanced by ONE tgx_verify_rows call per chunk
  // of TGX_MAX_VERIFY_POSITIONS positions — its prompt-lookup draft, or no draft at all (the row then takes one token).  produced[b]: tokens appended to row b
  bool speculateMoreRows(std::vector<std::vector<int32_t>>& seqs, int64_t maxTotal, std::vector<char>& finished, std::vector<int64_t>& produced);
  // GPTConfig::logprobs
  struct RowLogprobs { std::vector<float> lp, topLp; std::vector<int32_t> topId; };
  bool logprobsActive() const;
  bool logprobsRefused(bool async);                                                            // logprobs asked for and not servable: err_ set, the generate call fails
  bool logprobsDrain(int row, int64_t n, RowLogprobs& into);                                  // appends the row's last n records
  void logprobsEnd(int batch);
  void rowSamplerEnd(int batch = 1);                          // GPTConfig::speculateSampled: the rows' sampler back to the default when the call ends
  void logprobsStore(GPTOutput& out, const std::vector<RowLogprobs>& rows, int64_t perRow) const;
  // GPTConfig::contextShift, generateSync: got[b] holds row b's first token on entry and its tokens after the first on return
  bool decodeRowsShifting(int batch, const tgx_sampler_cfg& sc, int64_t n_more, bool constrained, std::vector<std::vector<int64_t>>& got, std::vector<RowLogprobs>* lp);
  // SamplerConfig's penalties / logit bias
  bool processorsOn() const { return !config_.samplerConfig.processorsNeutral(); }
  bool processorsRefused(bool async);                                                          // asked for and not servable: err_ set, the generate call fails
  bool processorsBegin(int row, const int64_t* prompt, int64_t n);                            // the row's settings, and its history from the prompt it admitted
  void processorsEnd(int batch);                                                               // neutral again, histories cleared
  bool constraintOn() const { return !config_.samplerConfig.regex.empty(); }
  bool constraintEnsure();                                                                     // SamplerConfig::regex compiled and its table on the device (kept while pattern and stop ids stay); false: err_ set
  bool rowsBegin(int batch, const tgx_sampler_cfg& sc, std::vector<int64_t>& first);          // the rows' sampler (and logprobs) settings, then every row's first token through tgx_sample_row

  // GPTConfig::numBeams > 1
  bool beamsRefused(size_t prompts);                                                           // not servable: err_ set, the generate call fails
  GPTOutput generateBeams(const std::vector<int32_t>& prompt, int32_t padToken);

  GPTConfig config_;
  Backend be_;
  LoadedModel model_;
  std::vector<int32_t> baseEosTokenIds_, eosTokenIds_;
  std::string err_;
  bool prepared_ = false;
  Tokenizer tokenizer_;
  bool tokenizerOk_ = false;
  std::vector<int32_t> cached_;      // reusePrefix: the token ids row 0's cache holds, position by position (empty: unknown / nothing)
  int64_t lastReused_ = 0, lastShifts_ = 0;
  SpecStats spec_;
  bool verifyProcessedBegin();                                // GPTConfig::speculateProcessed: option verify.processors on for this call (false: the backend refused it)
  void verifyProcessedEnd();                                  // ... and back to what it was
  bool verifyProcessedOn_ = false;                            // between the two: the verify calls take processed rows (spec_mode.h SpecInputs::verifyProcessed)
  int verifyProcessedWas_ = 0;
  bool treeRefused_ = false;                                  // GPTConfig::speculateTree: the device refused a tree as unsupported — chain drafts for the rest of the call
  std::string constraintPattern_;            // the pattern and stop ids of the table the device holds (constraintId_ >= 0)
  std::vector<int32_t> constraintStops_;
  int32_t constraintId_ = -1;
};

// Deterministic synthetic checkpoint — bit-identical to tinygpt_amd/synth.py (same integer hash).
void synth_tensor_bf16(uint64_t seed, const std::string& name, size_t n, double std_dev, uint16_t* out);
bool known_config(const std::string& key, int compute_dtype, int max_batch, ModelConfig& out);
bool load_synthetic(const Backend& be, const ModelConfig& cfg, int device_ordinal, uint64_t seed, double std_dev, tgx_ctx** ctx, std::string& err,
                    const LoadOptions& opts = LoadOptions());

}  // namespace tgxh
