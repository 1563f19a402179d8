// tgx_cli — the inference harness of the reference (examples/inference/main.cpp): the same four text prompts when a
// tokenizer is available (--model dir or --tokenizer dir), token-id prompts otherwise;
// same flags and defaults (--model --device --dtype --max-tokens --temperature --top-p), the same timing window
// (generate only; load excluded, main.cpp:97-102) and the same "speed" convention (ALL ids incl. prompt / wall time,
// main.cpp:112-114) — plus the new-token rate, the time to first token and the decode-only rate.  `--device mi355x` is the only device this binary executes on.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "engine.h"

// INPUT_STRS (main.cpp:12-17), and their gpt2 ids for runs without a tokenizer (usable with any vocabulary >= 50257)
static const std::vector<std::string> kInputStrs = {"Hello, my name is", "The president of the United States is", "The capital of France is", "The future of AI is"};
static const std::vector<std::vector<int32_t>> kDefaultPrompts = {
    {15496, 11, 616, 1438, 318}, {464, 1893, 286, 262, 1578, 1829, 318}, {464, 3139, 286, 4881, 318}, {464, 2003, 286, 9552, 318}};

static void usage(const char* prog) {
  fprintf(stderr,
          "Usage: %s [options]\n"
          "  --model <path>            HuggingFace model directory (config.json, generation_config.json, model.safetensors[.index.json])\n"
          "  --synthetic <name>        instead of --model: llama-3.2-1b | llama-3.2-3b | qwen2.5-0.5b | mistral-7b-v0.3 (deterministic weights)\n"
          "  --device <mi355x>         device type (default: mi355x)\n"
          "  --dtype <bf16>            data type (default: bf16)\n"
          "  --weights-fp8             FP8 weights (opt-in, lossy): gate_up, down and lm_head are quantized to E4M3 codes with a power-of-two scale per row when\n"
          "                            the model is loaded (bf16 only); the run fails if the device library cannot do it (default: off)\n"
          "  --max-tokens <n>          max new tokens (default: 32)\n"
          "  --temperature <f>         sampling temperature (default: 0.8)\n"
          "  --top-p <f>               top-p sampling (default: 0.9)\n"
          "  --top-k <n> --min-p <f>   (default: off)\n"
          "  --tokenizer <dir>         tokenizer.json + tokenizer_config.json (default: the --model directory)\n"
          "  --prompt <text>           a text prompt (repeatable; default with a tokenizer: the reference's 4 prompts)\n"
          "  --stream                  batch-1 generateAsync: print UTF-8-safe chunks as they are produced\n"
          "  --prompt-ids <a,b,c;d,e>  prompts as token ids, ';' between batch rows (default without a tokenizer: the 4 prompts as gpt2 ids)\n"
          "  --pad-id <n>              left-pad id (default: eos_token_id of the model, else 0)\n"
          "  --seed <n>                sampler seed (default: 0)\n"
          "  --logprobs <n>            print every new token's log-probability and its n most likely alternatives (0 .. 20; default: off)\n"
          "  --score                   generate nothing: print the log-probability of every prompt token but the first (position id lp, %%.9g; with --logprobs n the n most\n"
          "                            likely alternatives as id:lp) and the prompt's perplexity, one prefill pass per prompt; of a prompt\n"
          "                            longer than the context the last contextSize tokens are scored (positions count from the prompt's start)\n"
          "  --embed                   generate nothing: print one JSON array per prompt, its embedding (the pooled final hidden state, no lm_head; %%.9g); the prompts\n"
          "                            share ragged passes of up to four rows (or as many as there are prompts); of a prompt longer than the context the last\n"
          "                            contextSize tokens are embedded\n"
          "  --pool <last|mean|first>  with --embed: the position(s) pooled (default: last)\n"
          "  --embed-dims <n>          with --embed: keep the first n components before normalisation (default: 0 = the hidden size)\n"
          "  --no-normalize            with --embed: do not divide by the L2 norm\n"
          "  --repetition-penalty <r> --presence-penalty <p> --frequency-penalty <f>\n"
          "                            penalties over each row's prompt and produced tokens, applied to the logits on the device (default: 1 0 0 = off)\n"
          "  --logit-bias <id:val,...> added to those ids' logits; -inf bans an id (at most 320 ids; default: none)\n"
          "  --regex <pattern>         constrained decoding: the output must match the pattern as a whole (needs a ByteLevel tokenizer; host/constraint.h\n"
          "                            lists the supported subset; a run that --max-tokens ends first prints a prefix of a match)\n"
          "  --stop-ids <id,...>       stop token ids beside the model's EOS ids (--stream ends there; --regex allows them where a match may end)\n"
          "  --session-load <file>     with --stream and one text prompt: start from the conversation cache a --session-save run left (only what follows the shared\n"
          "                            prefix is prefilled; the file must come from the same model and dtype)\n"
          "  --session-save <file>     with --stream and one text prompt: keep the conversation's KV cache (prompt + generated tokens) in a file when the run ends\n"
          "                            (neither flag combines with --speculate, --logprobs, the penalties or --logit-bias: those runs end with the row finished on the\n"
          "                            device, which keeps no cache to save)\n"
          "  --num-beams <n>           beam search over n hypotheses of ONE prompt (2 .. 8; needs --temperature 0 --top-p 1; not with --stream, --speculate, --logprobs)\n"
          "  --length-penalty <f>      ... a finished hypothesis scores sum of log-probabilities / length^f (default 1)\n"
          "  --early-stopping          ... stop once n hypotheses are finished\n"
          "  --num-return <n>          ... print the n best hypotheses, best first, each with its score (default 1)\n"
          "  --speculate <n>           greedy speculative decoding: up to n prompt-lookup draft tokens verified per pass (--temperature 0 --top-p 1; several prompts: every row's\n"
          "                            draft in one joint pass; default: 0 = off)\n"
          "  --speculate-sampled       with --speculate: verify drafts under a sampling configuration as well, with the row's own sampler (the ids of the plain loop)\n"
          "  --speculate-processed     with --speculate: keep drafting while --regex, a penalty or --logit-bias is on — every position of a verify pass is processed as its\n"
          "                            step would have been (the ids of the run without --speculate; with a sampling configuration --speculate-sampled as well)\n"
          "  --speculate-tree <b>      with --speculate, one prompt: where the text's tail has continued in different ways before, up to b of them share the pass's\n"
          "                            positions as branches of a token tree, and the device follows the one the model produces (b >= 2; default: 0 = off, 1 is the same: one branch is a chain)\n"
          "  --context-shift           generate past the context: a full row keeps its first --keep positions, drops half of the rest and slides the tail down, its keys\n"
          "                            re-rotated (no drafts are proposed while it is on; default: off, the run ends at the context)\n"
          "  --keep <n>                with --context-shift: positions kept at the front of a shifted row (default: 0)\n",
          prog);
}

// --speculate: what the drafts did (nothing is printed without the flag)
static void print_spec(const tgxh::GPTConfig& cfg, const tgxh::GPTEngine& engine) {
  if (cfg.speculate <= 0) return;
  const tgxh::SpecStats& s = engine.specStats();
  printf("speculate: %lld verify passes, %lld of %lld draft tokens accepted, %lld ordinary steps\n", (long long)s.verifyCalls, (long long)s.acceptedDrafts, (long long)s.draftTokens,
         (long long)s.plainSteps);
  if (cfg.speculateTree >= 2) printf("speculate-tree: %lld of the verify passes ran a tree of two or more branches\n", (long long)s.treePasses);
}

// --num-beams: one line per returned hypothesis, best first (nothing is printed without the flag)
static void print_beams(const tgxh::GPTOutput& out) {
  for (size_t b = 0; b < out.beamScores.size(); b++) printf("beam %zu score %.6f\n", b, out.beamScores[b]);
}

// --logprobs: one line per new token — row, index, id, its log-probability and the alternatives as id:logprob, most likely first
static void print_logprobs(const tgxh::GPTOutput& out) {
  if (out.logprobs.empty()) return;
  const int64_t per = (int64_t)out.logprobs.size() / out.batch, row = (int64_t)out.tokenIds.size() / out.batch, k = out.topLogprobs;
  for (int64_t b = 0; b < out.batch; b++)
    for (int64_t i = 0; i < per; i++) {
      const size_t at = (size_t)(b * per + i);
      printf("logprob row %lld token %lld id %d: %.6f |", (long long)b, (long long)i, out.tokenIds[(size_t)(b * row + row - out.newTokens + i)], out.logprobs[at]);
      for (int64_t j = 0; j < k; j++) printf(" %d:%.6f", out.topIds[at * (size_t)k + (size_t)j], out.topLogprobValues[at * (size_t)k + (size_t)j]);
      printf("\n");
    }
}

// --score: per prompt one line per scored token — its position in the prompt, its id, its log-probability, then the alternatives — and `ppl exp(-mean lp)`
static bool print_score(const tgxh::ScoreOutput& r) {
  if (!r.ok) return false;
  const size_t k = (size_t)r.topLogprobs;
  for (size_t i = 0; i < r.logprobs.size(); i++) {
    printf("%lld %d %.9g", (long long)(r.dropped + (int64_t)i + 1), r.tokenIds[i + 1], (double)r.logprobs[i]);      // the position in the prompt as supplied
    for (size_t j = 0; j < k; j++) printf(" %d:%.9g", r.topIds[i * k + j], (double)r.topLogprobValues[i * k + j]);
    printf("\n");
  }
  printf("ppl %.9g\n", r.perplexity());
  return true;
}

int main(int argc, char** argv) {
  tgxh::GPTConfig cfg;
  cfg.maxNewTokens = 32;
  cfg.samplerConfig.temperature = 0.8f;
  cfg.samplerConfig.topP = 0.9f;
  std::string dtype = "bf16", prompt_ids, session_load, session_save;
  std::vector<int32_t> stop_ids;
  long pad_id = -1;
  std::vector<std::string> text_prompts;
  bool stream = false, score = false, embed = false;
  tgxh::EmbedConfig embed_cfg;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
    if (a == "--help" || a == "-h") { usage(argv[0]); return 0; }
    else if (a == "--model") cfg.modelDir = next();
    else if (a == "--synthetic") cfg.synthetic = next();
    else if (a == "--device") cfg.device = next();
    else if (a == "--dtype") dtype = next();
    else if (a == "--weights-fp8") cfg.weightsFp8 = true;
    else if (a == "--max-tokens") cfg.maxNewTokens = atoi(next());
    else if (a == "--temperature") cfg.samplerConfig.temperature = strtof(next(), nullptr);
    else if (a == "--top-p") cfg.samplerConfig.topP = strtof(next(), nullptr);
    else if (a == "--top-k") cfg.samplerConfig.topK = atoll(next());
    else if (a == "--min-p") cfg.samplerConfig.minP = strtof(next(), nullptr);
    else if (a == "--prompt-ids") prompt_ids = next();
    else if (a == "--prompt") text_prompts.push_back(next());
    else if (a == "--tokenizer") cfg.tokenizerDir = next();
    else if (a == "--stream") stream = true;
    else if (a == "--score") score = true;
    else if (a == "--embed") embed = true;
    else if (a == "--pool") {
      const std::string v = next();
      if (v == "last") embed_cfg.pool = TGX_POOL_LAST;
      else if (v == "mean") embed_cfg.pool = TGX_POOL_MEAN;
      else if (v == "first") embed_cfg.pool = TGX_POOL_FIRST;
      else { fprintf(stderr, "--pool: expected last, mean or first, got '%s'\n", v.c_str()); return 1; }
    }
    else if (a == "--embed-dims") {
      const std::string v = next();
      char* end = nullptr;
      const long n = strtol(v.c_str(), &end, 10);
      if (v.empty() || *end != '\0' || n < 0 || n > 0x7fffffffL) { fprintf(stderr, "--embed-dims: expected a component count, got '%s'\n", v.c_str()); return 1; }
      embed_cfg.dims = (int)n;
    }
    else if (a == "--no-normalize") embed_cfg.normalize = false;
    else if (a == "--pad-id") pad_id = atol(next());
    else if (a == "--seed") cfg.seed = strtoull(next(), nullptr, 10);
    else if (a == "--num-beams") cfg.numBeams = atoi(next());
    else if (a == "--length-penalty") cfg.lengthPenalty = strtof(next(), nullptr);
    else if (a == "--early-stopping") cfg.earlyStopping = true;
    else if (a == "--num-return") cfg.numReturn = atoi(next());
    else if (a == "--speculate") cfg.speculate = atoi(next());
    else if (a == "--speculate-sampled") cfg.speculateSampled = true;
    else if (a == "--speculate-processed") cfg.speculateProcessed = true;
    else if (a == "--speculate-tree") cfg.speculateTree = atoi(next());
    else if (a == "--context-shift") cfg.contextShift = true;
    else if (a == "--keep") cfg.shiftKeep = std::max(0, atoi(next()));
    else if (a == "--session-load") session_load = next();
    else if (a == "--session-save") session_save = next();
    else if (a == "--logprobs") cfg.logprobs = atoi(next());
    else if (a == "--repetition-penalty") cfg.samplerConfig.repetitionPenalty = strtof(next(), nullptr);
    else if (a == "--presence-penalty") cfg.samplerConfig.presencePenalty = strtof(next(), nullptr);
    else if (a == "--frequency-penalty") cfg.samplerConfig.frequencyPenalty = strtof(next(), nullptr);
    else if (a == "--regex") cfg.samplerConfig.regex = next();
    else if (a == "--stop-ids") {
      std::stringstream list(next());
      std::string item;
      while (std::getline(list, item, ',')) if (!item.empty()) stop_ids.push_back((int32_t)atol(item.c_str()));
    }
    else if (a == "--logit-bias") {
      std::stringstream ss(next());
      std::string item;
      while (std::getline(ss, item, ',')) {
        const size_t colon = item.find(':');
        if (colon == std::string::npos || colon == 0 || colon + 1 >= item.size()) { fprintf(stderr, "--logit-bias: expected id:val[,id:val...], got '%s'\n", item.c_str()); return 1; }
        const std::string id_s = item.substr(0, colon), val_s = item.substr(colon + 1);
        char *id_end = nullptr, *val_end = nullptr;
        const long id = strtol(id_s.c_str(), &id_end, 10);
        const float val = strtof(val_s.c_str(), &val_end);      // (strtof reads "-inf")
        if (*id_end != '\0' || *val_end != '\0' || id < 0 || id > 0x7fffffffL) { fprintf(stderr, "--logit-bias: '%s' is not id:val (a token id and a number)\n", item.c_str()); return 1; }
        cfg.samplerConfig.logitBias[(int32_t)id] = val;
      }
    }
#ifdef TGXH_TEST_HOOKS
    // tgx_cli_test only (tests/_build, -DTGXH_TEST_HOOKS): bind the host engine to a library of the test's choice that exports the tgx ABI
    // (the CPU oracle), to check host logic on a machine without a GPU.  The shipped tgx_cli has neither flag.
    else if (a == "--backend-lib") cfg.backendLib = next();
    else if (a == "--backend-prefix") cfg.backendPrefix = next();
#endif
    else { fprintf(stderr, "Unknown argument: %s\n", a.c_str()); usage(argv[0]); return 1; }
  }
  if (cfg.modelDir.empty() && cfg.synthetic.empty()) { fprintf(stderr, "Error: --model (or --synthetic) is required\n"); usage(argv[0]); return 1; }
  cfg.dtype = dtype == "fp32" ? TGX_F32 : dtype == "fp16" ? TGX_F16 : TGX_BF16;

  std::vector<std::vector<int32_t>> prompts = kDefaultPrompts;
  if (!prompt_ids.empty()) {
    prompts.clear();
    std::stringstream rows(prompt_ids);
    std::string row;
    while (std::getline(rows, row, ';')) {
      std::vector<int32_t> ids;
      std::stringstream toks(row);
      std::string t;
      while (std::getline(toks, t, ',')) if (!t.empty()) ids.push_back((int32_t)atol(t.c_str()));
      if (!ids.empty()) prompts.push_back(ids);
    }
  }
  cfg.maxBatch = (int)std::max(std::max(prompts.size(), text_prompts.size()), kInputStrs.size());

  const int score_top = std::max(0, cfg.logprobs);
  if (score) cfg.logprobs = -1;      // (--logprobs n names the alternatives of --score: nothing is generated, nothing recorded)
  if (embed && (score || stream)) { fprintf(stderr, "Error: --embed does not combine with --score or --stream (nothing is generated)\n"); return 1; }
  if (embed) cfg.logprobs = -1;
  const bool session = !session_load.empty() || !session_save.empty();
  if (session && (!stream || score || embed || !prompt_ids.empty() || text_prompts.size() != 1)) {
    fprintf(stderr, "Error: --session-load / --session-save need --stream and exactly one --prompt (the single-prompt streaming path keeps row 0's cache)\n");
    return 1;
  }
  if (session && (cfg.speculate > 0 || cfg.logprobs >= 0 || !cfg.samplerConfig.processorsNeutral())) {
    fprintf(stderr, "Error: --session-load / --session-save do not combine with --speculate, --logprobs, the penalties or --logit-bias (the row finishes on the device and keeps no cache)\n");
    return 1;
  }
  if (session) cfg.reusePrefix = true;
  tgxh::GPTEngine engine(cfg);
  if (!engine.prepare()) { fprintf(stderr, "Prepare engine failed\n"); return 1; }
  if (!stop_ids.empty()) engine.reconfigure(cfg.samplerConfig, cfg.maxNewTokens, stop_ids);
  if (session && !engine.hasTokenizer()) { fprintf(stderr, "Error: --session-load / --session-save need a tokenizer (--model or --tokenizer)\n"); return 1; }
  if (!session_load.empty() && !engine.loadSession(session_load)) fprintf(stderr, "session not loaded, starting from an empty cache: %s\n", engine.lastError().c_str());

  if (embed) {      // one JSON array per prompt, in prompt order
    const bool texts = engine.hasTokenizer() && prompt_ids.empty();
    if (texts && text_prompts.empty()) text_prompts = kInputStrs;
    if (!texts) for (auto& p : prompts) for (auto& t : p) if (t >= engine.desc().vocab) t = t % engine.desc().vocab;
    const tgxh::EmbedOutput r = texts ? engine.embed(text_prompts, embed_cfg) : engine.embed(prompts, embed_cfg);
    if (!r.ok) { fprintf(stderr, "embed failed: %s\n", engine.lastError().c_str()); return 1; }
    const size_t n = r.vectors.size() / (size_t)r.dims;
    for (size_t b = 0; b < n; b++) {
      printf("[");
      for (int k = 0; k < r.dims; k++) printf(k ? ", %.9g" : "%.9g", (double)r.vectors[b * (size_t)r.dims + (size_t)k]);
      printf("]\n");
    }
    return 0;
  }
  if (score) {
    const bool texts = engine.hasTokenizer() && prompt_ids.empty();
    if (texts && text_prompts.empty()) text_prompts = kInputStrs;
    const size_t n = texts ? text_prompts.size() : prompts.size();
    for (size_t b = 0; b < n; b++) {
      if (!texts) for (auto& t : prompts[b]) if (t >= engine.desc().vocab) t = t % engine.desc().vocab;
      if (!print_score(texts ? engine.score(text_prompts[b], score_top) : engine.score(prompts[b], score_top))) { fprintf(stderr, "score failed: %s\n", engine.lastError().c_str()); return 1; }
    }
    return 0;
  }
  if (engine.hasTokenizer() && prompt_ids.empty()) {       // the reference's flow: texts in, texts out (main.cpp:97-114)
    if (text_prompts.empty()) text_prompts = kInputStrs;
    const auto t0 = std::chrono::steady_clock::now();
    tgxh::GPTOutput out;
    if (stream) {
      printf("%s", text_prompts[0].c_str());
      out = engine.generateAsync(text_prompts[0], [](const std::string& chunk) { fputs(chunk.c_str(), stdout); fflush(stdout); return true; });
      printf("\n");
      if (session && out.batch) fprintf(stderr, "session: %lld prompt tokens served from the cache\n", (long long)engine.lastReused());
      if (!session_save.empty() && out.batch && !engine.saveSession(session_save)) { fprintf(stderr, "session not saved: %s\n", engine.lastError().c_str()); return 1; }
    } else out = engine.generateSync(text_prompts);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (out.batch == 0) { fprintf(stderr, "generate failed: %s\n", engine.lastError().c_str()); return 1; }
    if (!stream) {
      printf("Generated Outputs:\n------------------------------------------------------------\n");
      for (int64_t b = 0; b < out.batch; b++)
        printf("Prompt:    '%s'\nOutput:    '%s'\n------------------------------------------------------------\n", text_prompts[out.beamScores.empty() ? (size_t)b : 0].c_str(), out.texts[(size_t)b].c_str());
    }
    printf("Time cost: %lld ms, speed: %.2f token/s\n", (long long)ms, out.tokenIds.size() * 1000.0 / ms);
    printf("new tokens: %lld, new-token rate: %.2f token/s\n", (long long)(out.batch * out.newTokens), out.batch * out.newTokens * 1000.0 / ms);
    if (out.newTokens > 1) printf("time to first token: %.1f ms, decode-only rate: %.2f token/s\n", out.firstTokenMs, out.batch * (out.newTokens - 1) * 1000.0 / out.decodeMs);
    print_logprobs(out);
    print_beams(out);
    print_spec(cfg, engine);
    return 0;
  }
  int32_t pad = pad_id >= 0 ? (int32_t)pad_id : (!engine.eosTokenIds().empty() ? engine.eosTokenIds()[0] : 0);
  for (auto& p : prompts) for (auto& t : p) if (t >= engine.desc().vocab) t = t % engine.desc().vocab;

  const auto t0 = std::chrono::steady_clock::now();
  tgxh::GPTOutput out = engine.generateSync(prompts, pad);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (out.batch == 0) { fprintf(stderr, "generate failed: %s\n", engine.lastError().c_str()); return 1; }

  printf("Generated Outputs:\n------------------------------------------------------------\n");
  const int64_t row = (int64_t)out.tokenIds.size() / out.batch;
  for (int64_t b = 0; b < out.batch; b++) {
    printf("Prompt ids: ");
    for (int64_t i = 0; i < row - out.newTokens; i++) printf("%d ", out.tokenIds[(size_t)(b * row + i)]);
    printf("\nOutput ids: ");
    for (int64_t i = row - out.newTokens; i < row; i++) printf("%d ", out.tokenIds[(size_t)(b * row + i)]);
    printf("\n------------------------------------------------------------\n");
  }
  printf("Time cost: %lld ms, speed: %.2f token/s\n", (long long)ms, out.tokenIds.size() * 1000.0 / ms);
  printf("new tokens: %lld, new-token rate: %.2f token/s\n", (long long)(out.batch * out.newTokens), out.batch * out.newTokens * 1000.0 / ms);
  if (out.newTokens > 1) printf("time to first token: %.1f ms, decode-only rate: %.2f token/s\n", out.firstTokenMs, out.batch * (out.newTokens - 1) * 1000.0 / out.decodeMs);
  print_logprobs(out);
  print_beams(out);
  print_spec(cfg, engine);
  return 0;
}
