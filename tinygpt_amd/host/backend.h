// backend.h — the device shim as a table of C function pointers resolved with dlopen/dlsym.
// `--device mi355x` binds tinygpt_amd/lib/libtgx_mi355x.so (symbols tgx_*, include/tgx.h).  The table is the C++
// counterpart of the reference's virtual GPTModel + Sampler + AsyncTokenPipeline (src/model/GPTModel.h:80-106,
// src/engine/Sampler.h:30, src/engine/GPTEngine.cpp:17-35); the host engine sees nothing else of the device.
// Any library exporting the same entry points under another prefix can be bound (the tests bind the CPU oracle).
#pragma once
#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/tgx.h"

namespace tgxh {

struct Backend {
  void* handle = nullptr;
  std::string error;

  int (*device_count)(int*) = nullptr;
  int (*create)(const tgx_model_desc*, int, tgx_ctx**) = nullptr;
  int (*upload)(tgx_ctx*, const char*, const void*, const int64_t*, int, int) = nullptr;
  int (*finalize)(tgx_ctx*) = nullptr;
  void (*destroy)(tgx_ctx*) = nullptr;
  int (*forward)(tgx_ctx*, const int64_t*, int, int) = nullptr;
  int (*read_logits)(tgx_ctx*, float*, int) = nullptr;
  int (*sample)(tgx_ctx*, const tgx_sampler_cfg*, uint64_t, int64_t*) = nullptr;
  int (*decode)(tgx_ctx*, const tgx_sampler_cfg*, uint64_t, int, int64_t*) = nullptr;
  int (*step_async)(tgx_ctx*, const tgx_sampler_cfg*, uint64_t, int64_t*) = nullptr;   // optional
  int (*fetch_token)(tgx_ctx*, int64_t, int32_t*) = nullptr;                            // optional
  int (*reset_cache)(tgx_ctx*) = nullptr;
  int64_t (*past_length)(const tgx_ctx*) = nullptr;
  int64_t (*context_size)(const tgx_ctx*) = nullptr;
  const char* (*last_error)(const tgx_ctx*) = nullptr;
  // per-row sequence lifecycle (include/tgx.h ABI 3; optional: a backend without them serves whole-batch generation only)
  int (*reset_row)(tgx_ctx*, int) = nullptr;
  int (*forward_row)(tgx_ctx*, int, const int64_t*, int) = nullptr;
  int (*sample_row)(tgx_ctx*, int, const tgx_sampler_cfg*, uint64_t, int64_t*) = nullptr;
  int64_t (*past_length_row)(const tgx_ctx*, int) = nullptr;
  // prefix reuse (optional: GPTConfig::reusePrefix needs both)
  int (*extend_row)(tgx_ctx*, int, const int64_t*, int) = nullptr;
  int (*truncate_row)(tgx_ctx*, int, int64_t) = nullptr;
  // context shift (optional: GPTConfig::contextShift needs it with extend_row, sample_row, set_row_sampler, set_row_stop, decode_rows and past_length_row)
  int (*splice_row)(tgx_ctx*, int, int, const int64_t*, const int64_t*, int64_t*) = nullptr;
  // greedy speculative decoding (optional: GPTConfig::speculate needs all three — the draft is verified by verify_row, steps without a draft go through
  // decode_rows so that every produced token is counted against the row's stop conditions on the device)
  int (*verify_row)(tgx_ctx*, int, const int64_t*, int, int64_t*, int32_t*, int32_t*) = nullptr;
  int (*set_row_stop)(tgx_ctx*, int, int32_t, const int32_t*, int) = nullptr;
  int (*decode_rows)(tgx_ctx*, int, int64_t*, int32_t*, int32_t*) = nullptr;
  // ... under sampling (optional: GPTConfig::speculateSampled needs verify_row_sampled, set_row_sampler and sample_row besides; read_pass_logits is the tests' view of a pass)
  int (*verify_row_sampled)(tgx_ctx*, int, const int64_t*, int, int64_t*, int32_t*, int32_t*) = nullptr;
  int (*read_pass_logits)(tgx_ctx*, float*, int, int32_t*) = nullptr;
  // ... of a token tree (optional: GPTConfig::speculateTree needs it; without it the drafts stay chains)
  int (*verify_tree)(tgx_ctx*, int, const int64_t*, const int32_t*, int, int64_t*, int32_t*, int32_t*) = nullptr;
  // ... of a batch of several sequences (optional: all rows' drafts in one joint pass; without it a batch keeps the plain loop)
  int (*verify_rows)(tgx_ctx*, int, const int32_t*, const int64_t*, const int32_t*, int64_t*, int32_t*, int32_t*) = nullptr;
  // chunked prefill (optional; bound for a batch engine to come — nothing in this host engine calls it yet): prompt chunks and live rows' steps in one ragged pass
  int (*advance_rows)(tgx_ctx*, int, const int32_t*, const int32_t*, const int64_t*, const int32_t*, int64_t*, int32_t*, int32_t*) = nullptr;
  // per-token log-probabilities (optional: GPTConfig::logprobs needs these three, sample_row and decode_rows — the engine then steps through the per-row calls)
  int (*set_row_sampler)(tgx_ctx*, int, const tgx_sampler_cfg*, uint64_t) = nullptr;
  int (*set_row_logprobs)(tgx_ctx*, int, int) = nullptr;
  int (*read_row_logprobs)(tgx_ctx*, int, int, float*, int32_t*, float*, int32_t*) = nullptr;
  // per-row logit processors (optional: a non-neutral SamplerConfig penalty or logit bias needs these three, and the per-row calls the logprobs path steps through)
  int (*set_row_penalties)(tgx_ctx*, int, const tgx_penalty_cfg*) = nullptr;
  int (*set_row_logit_bias)(tgx_ctx*, int, int, const int32_t*, const float*) = nullptr;
  int (*set_row_history)(tgx_ctx*, int, const int64_t*, int, const int64_t*, int) = nullptr;
  // token automata (optional: SamplerConfig::regex needs create, destroy and set_row_automaton, and the per-row calls the processors step through)
  int (*automaton_create)(tgx_ctx*, int32_t, int32_t, const uint16_t*, int32_t*) = nullptr;
  int (*automaton_destroy)(tgx_ctx*, int32_t) = nullptr;
  int (*set_row_automaton)(tgx_ctx*, int, int32_t, int32_t) = nullptr;
  int (*read_row_automaton)(tgx_ctx*, int, int32_t*, int32_t*) = nullptr;
  // run-time options (optional: GPTConfig::speculateProcessed sets "verify.processors" for the length of a generate call and needs both)
  int (*set_option)(tgx_ctx*, const char*, int) = nullptr;
  int (*get_option)(const tgx_ctx*, const char*, int*) = nullptr;
  // scoring a supplied sequence (optional: GPTEngine::score needs it)
  int (*score_row)(tgx_ctx*, int, const int64_t*, int, int, float*, int32_t*, float*) = nullptr;
  // embeddings (optional: GPTEngine::embed needs it)
  int (*embed_rows)(tgx_ctx*, int, const int32_t*, const int64_t*, const int32_t*, const tgx_embed_cfg*, float*) = nullptr;
  // beam search (optional: GPTConfig::numBeams > 1 needs both, forward_row, decode_rows and reset_row)
  int (*beam_select)(tgx_ctx*, int, const int32_t*, const float*, int, const int32_t*, int, tgx_beam_cand*, int32_t*) = nullptr;
  int (*beam_advance)(tgx_ctx*, int, const int32_t*, int, const int32_t*, const int32_t*, int32_t*) = nullptr;
  // row snapshots (optional: GPTEngine::saveSession / loadSession need all three, and prefix reuse)
  int (*row_snapshot_bytes)(const tgx_ctx*, int, int64_t*) = nullptr;
  int (*save_row)(tgx_ctx*, int, void*, int64_t, int64_t*) = nullptr;
  int (*restore_row)(tgx_ctx*, int, const void*, int64_t) = nullptr;

  bool open(const std::string& path, const std::string& prefix) {
    // RTLD_NODELETE: the shim's runtime owns threads (HIP's signal/event workers; libgomp's team under the CPU oracle) that
    // outlive the last context, so dlclose() must drop the handle without unmapping their code.
    handle = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL | RTLD_NODELETE);
    if (!handle) { error = std::string("dlopen failed: ") + dlerror(); return false; }
    bool ok = true;
    auto sym = [&](const char* name, bool required) -> void* {
      void* p = dlsym(handle, (prefix + name).c_str());
      if (!p && required) { error += "missing symbol " + prefix + name + "; "; ok = false; }
      return p;
    };
#define TGXH_BIND(field, required) field = reinterpret_cast<decltype(field)>(sym(#field, required))
    TGXH_BIND(device_count, false);
    TGXH_BIND(create, true); TGXH_BIND(upload, true); TGXH_BIND(finalize, true); TGXH_BIND(destroy, true);
    TGXH_BIND(forward, true); TGXH_BIND(read_logits, true); TGXH_BIND(sample, true); TGXH_BIND(decode, true);
    TGXH_BIND(step_async, false); TGXH_BIND(fetch_token, false);
    TGXH_BIND(reset_cache, true); TGXH_BIND(past_length, true); TGXH_BIND(context_size, true); TGXH_BIND(last_error, true);
    TGXH_BIND(reset_row, false); TGXH_BIND(forward_row, false); TGXH_BIND(sample_row, false); TGXH_BIND(past_length_row, false);
    TGXH_BIND(extend_row, false); TGXH_BIND(truncate_row, false); TGXH_BIND(splice_row, false);
    TGXH_BIND(verify_row, false); TGXH_BIND(set_row_stop, false); TGXH_BIND(decode_rows, false);
    TGXH_BIND(verify_row_sampled, false); TGXH_BIND(read_pass_logits, false); TGXH_BIND(verify_rows, false); TGXH_BIND(verify_tree, false);
    TGXH_BIND(advance_rows, false);
    TGXH_BIND(set_row_sampler, false); TGXH_BIND(set_row_logprobs, false); TGXH_BIND(read_row_logprobs, false);
    TGXH_BIND(set_row_penalties, false); TGXH_BIND(set_row_logit_bias, false); TGXH_BIND(set_row_history, false);
    TGXH_BIND(automaton_create, false); TGXH_BIND(automaton_destroy, false); TGXH_BIND(set_row_automaton, false); TGXH_BIND(read_row_automaton, false);
    TGXH_BIND(set_option, false); TGXH_BIND(get_option, false);
    TGXH_BIND(score_row, false); TGXH_BIND(embed_rows, false);
    TGXH_BIND(beam_select, false); TGXH_BIND(beam_advance, false);
    TGXH_BIND(row_snapshot_bytes, false); TGXH_BIND(save_row, false); TGXH_BIND(restore_row, false);
#undef TGXH_BIND
    return ok;
  }
  void close() { if (handle) dlclose(handle); handle = nullptr; }
};

}  // namespace tgxh
