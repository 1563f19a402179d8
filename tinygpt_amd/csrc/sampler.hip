// sampler.hip — Sampler::sample on the logits of a step (Sampler.cpp:23-79) + token publish / pastLength / next embedding.
// Greedy: one finalize launch per row (decode.hip).  Otherwise the staged sampler of kernels/sampler.h: ceil(V/1024) workgroups per row
// (rows on blockIdx.y) for the first digit of each active filter and for the compaction of its threshold bin, one workgroup per row for the
// filter's tail — which also draws the token when the chain ends there.
#include "ctx.h"
#include "kernels/sampler.h"
#include "kernels/logprobs.h"
#include "kernels/logit_proc.h"
#include "kernels/beam.h"
#include <cstddef>
#include <type_traits>

static int proc_tiles(const tgx_ctx* c) { return (c->d.vocab + tgx::PROC_TILE - 1) / tgx::PROC_TILE; }
// processed: the rows' logits and maxima come from the processed slab and its partials (kernels/logit_proc.h; launch_logit_proc ran ahead)
static tgx::SampArgs samp_args(tgx_ctx* c, int row0, const tgx_sampler_cfg& cfg, bool processed = false) {
  const int V = c->d.vocab;
  RowState& r = c->rows[(size_t)row0];
  tgx::SampArgs a{};
  a.logits = r.logits; a.logits_stride = V;
  a.part_val = r.part_val; a.part_stride = c->lm_grid; a.n_part = c->lm_grid;
  if (processed) {
    const int T = proc_tiles(c);
    a.logits = c->proc_logits + (size_t)row0 * V;
    a.part_val = c->proc_part_val + (size_t)row0 * T; a.part_stride = T; a.n_part = T;
  }
  a.sc = c->samp_scratch + row0;
  a.probs_out = r.probs; a.probs_stride = V;
  a.V = V; a.idx_bits = 1;
  while ((1 << a.idx_bits) < V) a.idx_bits++;
  a.temperature = cfg.temperature; a.top_k = cfg.top_k; a.top_p = cfg.top_p; a.min_p = cfg.min_p;
  a.list_comp = c->samp_list_comp + (size_t)row0 * V; a.list_v = c->samp_list_v + (size_t)row0 * V;
  // the normaliser of the final kept set: left by the last filter's tail, or — with min-p, or without any filter — the ordered sum of stage 1's tile sums
  a.z_from_tail = ((cfg.top_k > 0 || cfg.top_p < 1.f) && !(cfg.min_p > 0.f)) ? 1 : 0;
  return a;
}

// the finalize arguments of row `row` reading the processed partials instead of the lm_head's
static void finalize_from_processed(tgx_ctx* c, tgx::FinalizeArgs& f, int row) {
  const int T = proc_tiles(c);
  f.part_val = c->proc_part_val + (size_t)row * T; f.part_idx = c->proc_part_idx + (size_t)row * T; f.n_part = T;
}

// the uniform chain of `cfg` over R rows (blockIdx.y) of `a`: the stages every row of the launch takes, ending in the draw.  pa0: the draw's arguments (its `s` is
// the chain's state at the draw).  positions: the draw-only mode of the tail and the pick (SampPickArgs.draws), else they publish for storage dtype c->dt
static void launch_chain(tgx_ctx* c, tgx::SampArgs a, const tgx_sampler_cfg& cfg, int R, tgx::SampPickArgs pa0, bool positions) {
  const bool setK = cfg.top_k > 0, setP = cfg.top_p < 1.f, setM = cfg.min_p > 0.f;
  const int nwg = (a.V + tgx::SAMP_TILE - 1) / tgx::SAMP_TILE;
  const dim3 grid(nwg, R), blk(tgx::SAMP_WG);
  pa0.nwg = nwg;
  auto pick_args = [&](const tgx::SampArgs& now) { tgx::SampPickArgs pa = pa0; pa.s = now; return pa; };
  // a filter = first digit over the vocabulary, compaction of the threshold's bin, the tail (four digits, threshold) in one workgroup; the tail of the
  // chain's LAST filter also draws when no min-p follows
  a.mx_ready = 0;                 // the first launch that needs max(logits / T) reduces the lm_head partials and leaves it in sc->mx for the others
  auto tail = [&](auto mode, bool draws) {
    constexpr int MODE = decltype(mode)::value;
    const tgx::SampPickArgs pa = pick_args(a);
    if (!draws) { hipLaunchKernelGGL((tgx::samp_tail_kernel<MODE, false, 0>), dim3(1, R), blk, 0, c->stream, pa); return; }
    if (positions) { hipLaunchKernelGGL((tgx::samp_tail_kernel<MODE, true, 0, false, true>), dim3(1, R), blk, 0, c->stream, pa); return; }
    TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL((tgx::samp_tail_kernel<MODE, true, DT>), dim3(1, R), blk, 0, c->stream, pa))
  };
  if (setK) {
    hipLaunchKernelGGL(tgx::samp_level0_kernel<0>, grid, blk, 0, c->stream, a);       // (counts: no maximum needed)
    hipLaunchKernelGGL(tgx::samp_compact_kernel<0>, grid, blk, 0, c->stream, a);
    a.mx_ready = 1;
    tail(std::integral_constant<int, 0>{}, !setP && !setM);
  }
  if (setP) {
    hipLaunchKernelGGL(tgx::samp_level0_kernel<1>, grid, blk, 0, c->stream, a);
    a.mx_ready = 1;
    hipLaunchKernelGGL(tgx::samp_compact_kernel<1>, grid, blk, 0, c->stream, a);
    tail(std::integral_constant<int, 1>{}, !setM);
  }
  if (a.z_from_tail) return;      // the last tail drew
  // with min-p (its cut depends on the normaliser of the set it looks at) or without any filter: partial-sum stages over the vocabulary, then the pick
  if (setM) { hipLaunchKernelGGL(tgx::samp_sum_kernel<0>, grid, blk, 0, c->stream, a); a.mx_ready = 1; }
  hipLaunchKernelGGL(tgx::samp_sum_kernel<1>, grid, blk, 0, c->stream, a);
  a.mx_ready = 1;
  {
    const tgx::SampPickArgs pa = pick_args(a);
    if (positions) { hipLaunchKernelGGL((tgx::samp_pick_kernel<0, false, true>), dim3(1, R), blk, 0, c->stream, pa); return; }
    TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL(tgx::samp_pick_kernel<DT>, dim3(1, R), blk, 0, c->stream, pa))
  }
}

void launch_sample(tgx_ctx* c, int row0, int R, const tgx_sampler_cfg& cfg, bool advance_pos, bool log_step, bool processed) {
  if (is_greedy(&cfg)) {
    if (!processed) { launch_finalize_greedy(c, row0, R, advance_pos, log_step); return; }
    for (int b = row0; b < row0 + R; b++) {
      tgx::FinalizeArgs f = make_finalize_args(c, b, advance_pos, log_step);
      finalize_from_processed(c, f, b);
      TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL(tgx::finalize_greedy_kernel<DT>, dim3(1), dim3(256), 0, c->stream, f))
    }
    return;
  }
  // the draw's arguments — the last launch of the chain, one workgroup per row (blockIdx.y; the row that completes the batch's count moves the step counter)
  tgx::SampPickArgs pa{};
  pa.seed = c->seed_dev;
  pa.fin = make_finalize_args(c, row0, advance_pos, log_step);      // (the pick publishes the token it drew: the argmax partials are not read)
  pa.x_stride = c->d.hidden;
  launch_chain(c, samp_args(c, row0, cfg, processed), cfg, R, pa, /*positions=*/false);
}

// tgx_verify_row_sampled: the M positions of row `row`'s verify pass ride on blockIdx.y of the uniform chain of the row's cfg, over the pass's logits and argmax
// partials (vf_*) with a scratch and lists of their own (vs_*).  The end of the chain draws every position with the row's seed and the key of the token that
// position produces (kernels/common.h draw_key) into vs_draws and publishes nothing: the accept launch decides what the row takes
int vs_alloc(tgx_ctx* c) {
  if (c->vs_draws) return TGX_OK;            // the last of the four: set only when all of them exist
  const size_t R = tgx_ctx::VERIFY_ROWS, V = (size_t)c->d.vocab;
  int rc;
  if ((rc = dev_alloc(c, &c->vs_scratch, R)) || (rc = dev_alloc(c, &c->vs_list_comp, R * V)) || (rc = dev_alloc(c, &c->vs_list_v, R * V)) || (rc = dev_alloc(c, &c->vs_draws, R))) {
    dev_free(c, &c->vs_scratch); dev_free(c, &c->vs_list_comp); dev_free(c, &c->vs_list_v); dev_free(c, &c->vs_draws);      // all or nothing, as proc_alloc
    return rc;
  }
  return vs_rezero(c);      // (the chain's launches leave it zero again)
}
int vs_rezero(tgx_ctx* c) {
  if (c->vs_scratch) HIP_OK(c, hipMemsetAsync(c->vs_scratch, 0, sizeof(tgx::SampScratch) * (size_t)tgx_ctx::VERIFY_ROWS, c->stream));
  return TGX_OK;
}

void launch_sample_positions(tgx_ctx* c, int row, int M, const tgx_sampler_cfg& cfg, int joint_first, const int* depth, bool processed) {
  const bool joint = joint_first >= 0;      // tgx_verify_rows: the row's slice of the joint pass's workspace; the scratch and lists are the one-row call's (chains are stream-ordered)
  if (!c->vs_draws || !(joint ? c->vj_draws : c->vf_rec) || M > (int)tgx_ctx::VERIFY_ROWS) { c->launch_fault = "sampled verification requested before its buffers exist"; return; }
  const int V = c->d.vocab;
  tgx::SampArgs a{};
  a.logits = joint ? c->vj_logits + (size_t)joint_first * V : c->vf_logits; a.logits_stride = V;
  a.part_val = joint ? c->vj_part_val + (size_t)joint_first * c->lm_grid : c->vf_part_val; a.part_stride = c->lm_grid; a.n_part = c->lm_grid;
  if (processed) {      // option verify.processors: the row's positions in the processed slab (launch_logit_proc_positions ran ahead) and its per-tile maxima
    if (!(joint ? c->vpj_states : c->vp_states)) { c->launch_fault = "processed verification requested before its buffers exist"; return; }
    const int T = proc_tiles(c);
    a.logits = joint ? c->vpj_logits + (size_t)joint_first * V : c->vp_logits;
    a.part_val = joint ? c->vpj_part_val + (size_t)joint_first * T : c->vp_part_val; a.part_stride = T; a.n_part = T;
  }
  a.sc = c->vs_scratch;
  a.V = V; a.idx_bits = 1;
  while ((1 << a.idx_bits) < V) a.idx_bits++;
  a.temperature = cfg.temperature; a.top_k = cfg.top_k; a.top_p = cfg.top_p; a.min_p = cfg.min_p;
  a.list_comp = c->vs_list_comp; a.list_v = c->vs_list_v;
  a.z_from_tail = ((cfg.top_k > 0 || cfg.top_p < 1.f) && !(cfg.min_p > 0.f)) ? 1 : 0;
  tgx::SampPickArgs pa{};
  pa.fin.pos = c->rows[(size_t)row].pos; pa.fin.req = c->row_req + row; pa.fin.row = row;      // the key's words: read, never written
  pa.draws = joint ? c->vj_draws + joint_first : c->vs_draws;
  pa.depth = depth;      // (tgx_verify_tree: the device depth table of the pass's positions)
  launch_chain(c, a, cfg, M, pa, /*positions=*/true);
}

// tgx_decode_rows: every row samples with its own settings (tgx_set_row_sampler; kernels/sampler.h samp_row_apply).  `un` = the union of the rows' chains
// (row_union_of): greedy rows publish from the argmax partials in one finalize launch, the sampled rows through the union of their filter stages — each
// workgroup leaves at once when its row has no such stage, and every row publishes exactly once (the step counter moves on the batch's count).  The cfg
// values are read on the device: a new request's settings need no recapture.
static void launch_sample_rows_sampled(tgx_ctx* c, int row0, int R, int un);
void launch_sample_rows(tgx_ctx* c, int row0, int R, int un) {
  tgx::RowReq* req = c->row_req + row0;
  // some row of the batch has a logit processor on: every row's logits pass through the processed slab (unprocessed rows are copied), and every consumer below but
  // the log-probabilities — the MODEL's distribution — reads that slab and its partials
  if (un & ROWU_AUTO) {       // some row has an automaton on: the rows' state words consume the current tokens ahead of the launch that masks with them
    tgx::AutoAdvanceArgs aa{req, c->rows[(size_t)row0].tok, R, c->d.vocab};
    hipLaunchKernelGGL(tgx::automaton_advance_kernel, dim3(1), dim3(tgx::WAVE), 0, c->stream, aa);
  }
  if (un & ROWU_PROC) launch_logit_proc(c, row0, R, /*step=*/true);
  if (un & ROWU_GREEDY) {
    tgx::FinalizeRowsArgs fa{};
    fa.f = make_finalize_args(c, row0, /*advance_pos=*/true, /*log_step=*/true);
    fa.f.req = req;
    fa.part_stride = c->lm_grid; fa.x_stride = c->d.hidden;
    if (un & ROWU_PROC) { finalize_from_processed(c, fa.f, row0); fa.part_stride = proc_tiles(c); }
    TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL((tgx::finalize_rows_kernel<DT, true>), dim3(R), dim3(256), 0, c->stream, fa))
  }
  if (un & (ROWU_K | ROWU_P | ROWU_M | ROWU_SUM)) launch_sample_rows_sampled(c, row0, R, un);
  if (un & ROWU_LP) launch_logprobs(c, row0, R, /*force=*/false);      // behind the publish: the rows that record read their just-published token words
}

static void launch_sample_rows_sampled(tgx_ctx* c, int row0, int R, int un) {
  tgx::RowReq* req = c->row_req + row0;
  const tgx_sampler_cfg none{0.f, 0, 1.f, 0.f};
  tgx::SampArgs a = samp_args(c, row0, none, (un & ROWU_PROC) != 0);     // cfg fields, mx_ready and z_from_tail: per row on the device
  a.req = req;
  const int nwg = (a.V + tgx::SAMP_TILE - 1) / tgx::SAMP_TILE;
  const dim3 grid(nwg, R), blk(tgx::SAMP_WG);
  tgx::SampPickArgs pa{};
  pa.s = a; pa.nwg = nwg; pa.seed = c->seed_dev;
  pa.fin = make_finalize_args(c, row0, /*advance_pos=*/true, /*log_step=*/true);
  pa.fin.req = req;
  pa.x_stride = c->d.hidden;
  if (un & ROWU_K) {
    hipLaunchKernelGGL((tgx::samp_level0_kernel<0, true>), grid, blk, 0, c->stream, a);
    hipLaunchKernelGGL((tgx::samp_compact_kernel<0, true>), grid, blk, 0, c->stream, a);
    TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL((tgx::samp_tail_kernel<0, true, DT, true>), dim3(1, R), blk, 0, c->stream, pa))
  }
  if (un & ROWU_P) {
    hipLaunchKernelGGL((tgx::samp_level0_kernel<1, true>), grid, blk, 0, c->stream, a);
    hipLaunchKernelGGL((tgx::samp_compact_kernel<1, true>), grid, blk, 0, c->stream, a);
    TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL((tgx::samp_tail_kernel<1, true, DT, true>), dim3(1, R), blk, 0, c->stream, pa))
  }
  if (un & ROWU_M) hipLaunchKernelGGL((tgx::samp_sum_kernel<0, true>), grid, blk, 0, c->stream, a);
  if (un & ROWU_SUM) {
    hipLaunchKernelGGL((tgx::samp_sum_kernel<1, true>), grid, blk, 0, c->stream, a);
    TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL((tgx::samp_pick_kernel<DT, true>), dim3(1, R), blk, 0, c->stream, pa))
  }
}

// the union of the chains of rows [0, batch) under their own settings (host mirror of the request states)
int row_union_of(const tgx_ctx* c) {
  int un = 0;
  for (int b = 0; b < c->batch; b++) {
    const tgx::RowReq& q = c->row_req_host[(size_t)b];
    const bool K = q.top_k > 0, P = q.top_p < 1.f, M = q.min_p > 0.f, sampled = K || P || M || q.temperature > 0.f;
    if (row_records(c, b)) un |= ROWU_LP;
    if (row_processed(c, b)) un |= ROWU_PROC | ((q.proc & tgx::PROC_AUTOMATON) ? ROWU_AUTO : 0);
    if (!sampled) { un |= ROWU_GREEDY; continue; }
    if (K) un |= ROWU_K;
    if (P) un |= ROWU_P;
    if (M) un |= ROWU_M;
    if (!((K || P) && !M)) un |= ROWU_SUM;
  }
  return un;
}

// tgx_read_probs: the final probability vector of row `row`'s last sampled step, evaluated from what that step left on the device (its logits, the
// filters' thresholds, the normalisers) — the step itself never needs the vector
void launch_probs(tgx_ctx* c, int row, const tgx_sampler_cfg& cfg, bool processed) {
  tgx::SampArgs a = samp_args(c, row, cfg, processed);
  a.mx_ready = 0;
  const int nwg = (a.V + tgx::SAMP_TILE - 1) / tgx::SAMP_TILE;
  hipLaunchKernelGGL(tgx::samp_sum_kernel<2>, dim3(nwg, 1), dim3(tgx::SAMP_WG), 0, c->stream, a);
}

// ---- per-row logit processors (kernels/logit_proc.h)
static_assert(tgx::PROC_MAX_BIAS == TGX_MAX_LOGIT_BIAS && tgx::PROC_TILE == tgx::SAMP_TILE, "kernels/logit_proc.h");
// does the row process its logits in the steps: its settings, unless it is retired (like the log-probability setting, they are kept on the host and travel with the admission)
bool row_processed(const tgx_ctx* c, int row) { return c->row_req_host[(size_t)row].proc != 0 && !c->row_host[(size_t)row].idle; }

int proc_alloc(tgx_ctx* c) {
  if (c->proc_part_idx) return TGX_OK;       // the last of the six: set only when all of them exist
  const size_t B = (size_t)c->d.max_batch, V = (size_t)c->d.vocab, T = (size_t)proc_tiles(c);
  int rc;
  if ((rc = dev_alloc(c, &c->proc_hist, B * V)) || (rc = dev_alloc(c, &c->proc_bias_ids, B * tgx::PROC_MAX_BIAS)) || (rc = dev_alloc(c, &c->proc_bias_val, B * tgx::PROC_MAX_BIAS)) ||
      (rc = dev_alloc(c, &c->proc_logits, B * V)) || (rc = dev_alloc(c, &c->proc_part_val, B * T)) || (rc = dev_alloc(c, &c->proc_part_idx, B * T))) {
    // all or nothing: a later attempt starts over instead of allocating over live pointers (dev_free of a null pointer is a no-op)
    dev_free(c, &c->proc_hist); dev_free(c, &c->proc_bias_ids); dev_free(c, &c->proc_bias_val); dev_free(c, &c->proc_logits); dev_free(c, &c->proc_part_val); dev_free(c, &c->proc_part_idx);
    return rc;
  }
  HIP_OK(c, hipMemsetAsync(c->proc_hist, 0, B * V * sizeof(unsigned int), c->stream));
  return TGX_OK;
}

// ---- the processors over a verify pass's positions (kernels/logit_proc.h logit_proc_pos_kernel; option verify.processors)
static_assert(tgx::PROC_MAX_POS == TGX_MAX_VERIFY_POSITIONS && (int)tgx_ctx::VERIFY_ROWS <= tgx::PROC_MAX_POS, "kernels/logit_proc.h");
int ensure_verify_proc_ws(tgx_ctx* c, bool joint) {
  float*& lg = joint ? c->vpj_logits : c->vp_logits; float*& pv = joint ? c->vpj_part_val : c->vp_part_val;
  int*& pi = joint ? c->vpj_part_idx : c->vp_part_idx; int*& st = joint ? c->vpj_states : c->vp_states;
  if (st) return TGX_OK;                     // the last of the four: set only when all of them exist
  const size_t R = joint ? (size_t)tgx_ctx::VERIFY_POSITIONS : (size_t)tgx_ctx::VERIFY_ROWS, V = (size_t)c->d.vocab, T = (size_t)proc_tiles(c);
  int rc;
  if ((rc = dev_alloc(c, &lg, R * V)) || (rc = dev_alloc(c, &pv, R * T)) || (rc = dev_alloc(c, &pi, R * T)) || (rc = dev_alloc(c, &st, R))) {
    dev_free(c, &lg); dev_free(c, &pv); dev_free(c, &pi); dev_free(c, &st);      // all or nothing, as proc_alloc
    return rc;
  }
  return TGX_OK;
}
void launch_logit_proc_positions(tgx_ctx* c, int n, const int* rows, const int* first, const int* lens, const long long* const* ids, const char* processed, bool joint) {
  if (!c->proc_part_idx || !(joint ? c->vpj_states : c->vp_states) || !(joint ? c->vj_logits : c->vf_logits)) { c->launch_fault = "processed verification requested before its buffers exist"; return; }
  const int slots = joint ? (int)tgx_ctx::VERIFY_POSITIONS : (int)tgx_ctx::VERIFY_ROWS;
  tgx::AutoWalkArgs w{};
  tgx::LogitProcPosArgs a{};
  int np = 0;
  bool any_auto = false;
  for (int j = 0; j < n; j++) {
    if (!processed[j]) continue;
    if (first[j] < 0 || lens[j] < 1 || lens[j] > (int)tgx_ctx::VERIFY_ROWS || first[j] + lens[j] > slots || np + lens[j] > tgx::PROC_MAX_POS) { c->launch_fault = "processed verification: a row's positions do not fit the workspace"; return; }
    any_auto = any_auto || (c->row_req_host[(size_t)rows[j]].proc & tgx::PROC_AUTOMATON);
    w.r[w.n++] = tgx::AutoWalkRow{c->row_req + rows[j], ids[j], first[j], lens[j]};
    for (int i = 0; i < lens[j]; i++) a.pos[np++] = tgx::ProcPos{rows[j], i, first[j] + i, 0, ids[j]};
  }
  if (!np) return;
  w.states = joint ? c->vpj_states : c->vp_states; w.V = c->d.vocab;
  if (any_auto) hipLaunchKernelGGL(tgx::automaton_walk_kernel, dim3(1), dim3(tgx::PROC_MAX_POS), 0, c->stream, w);
  a.logits = joint ? c->vj_logits : c->vf_logits;
  a.req = c->row_req; a.hist = c->proc_hist; a.bias_ids = c->proc_bias_ids; a.bias_val = c->proc_bias_val; a.states = w.states;
  a.out = joint ? c->vpj_logits : c->vp_logits; a.part_val = joint ? c->vpj_part_val : c->vp_part_val; a.part_idx = joint ? c->vpj_part_idx : c->vp_part_idx;
  a.V = c->d.vocab; a.n_tile = proc_tiles(c);
  hipLaunchKernelGGL(tgx::logit_proc_pos_kernel, dim3((unsigned)a.n_tile, (unsigned)np), dim3(tgx::PROC_WG), 0, c->stream, a);
}

void launch_logit_proc(tgx_ctx* c, int row0, int R, bool step) {
  if (!c->proc_part_idx) { c->launch_fault = "logit processors requested before their buffers exist"; return; }
  const size_t V = (size_t)c->d.vocab, T = (size_t)proc_tiles(c);
  tgx::LogitProcArgs a{};
  a.logits = c->rows[(size_t)row0].logits; a.logits_stride = (long long)V;
  a.req = c->row_req + row0; a.tok = c->rows[(size_t)row0].tok;
  a.hist = c->proc_hist + row0 * V;
  a.bias_ids = c->proc_bias_ids + (size_t)row0 * tgx::PROC_MAX_BIAS; a.bias_val = c->proc_bias_val + (size_t)row0 * tgx::PROC_MAX_BIAS;
  a.out = c->proc_logits + row0 * V; a.part_val = c->proc_part_val + row0 * T; a.part_idx = c->proc_part_idx + row0 * T;
  a.V = (int)V; a.n_tile = (int)T; a.step = step ? 1 : 0;
  hipLaunchKernelGGL(tgx::logit_proc_kernel, dim3((unsigned)T, (unsigned)R), dim3(tgx::PROC_WG), 0, c->stream, a);
}

// ---- per-token log-probabilities (kernels/logprobs.h)
static_assert(tgx::LP_MAX == TGX_MAX_LOGPROBS && tgx::LP_RING == TGX_LOGPROB_RING, "kernels/logprobs.h");
static int lp_tiles(const tgx_ctx* c) { return (c->d.vocab + tgx::SAMP_TILE - 1) / tgx::SAMP_TILE; }

int logprobs_alloc(tgx_ctx* c) {
  if (c->lp_rows) return TGX_OK;
  const size_t B = (size_t)c->d.max_batch, rows = std::max<size_t>(B, tgx_ctx::VERIFY_ROWS), T = (size_t)lp_tiles(c);
  int rc;
  if ((rc = dev_alloc(c, &c->lp_ring, B * tgx::LP_RING)) || (rc = dev_alloc(c, &c->lp_tile_max, rows * T)) || (rc = dev_alloc(c, &c->lp_tile_sum, rows * T)) ||
      (rc = dev_alloc(c, &c->lp_tile_keys, rows * T * tgx::LP_MAX)) || (rc = dev_alloc(c, &c->lp_rows, B))) return rc;
  HIP_OK(c, hipMemsetAsync(c->lp_rows, 0, B * sizeof(tgx::LpRow), c->stream));
  return TGX_OK;
}

static tgx::LpArgs lp_args(tgx_ctx* c) {
  tgx::LpArgs a{};
  a.V = c->d.vocab; a.nwg = lp_tiles(c); a.logits_stride = c->d.vocab;
  return a;
}
static void lp_launch(tgx_ctx* c, const tgx::LpArgs& a, int R) {
  hipLaunchKernelGGL(tgx::lp_tile_kernel, dim3(a.nwg, R), dim3(tgx::SAMP_WG), 0, c->stream, a);
  hipLaunchKernelGGL(tgx::lp_record_kernel, dim3(1, R), dim3(tgx::SAMP_WG), 0, c->stream, a);
}

void launch_logprobs(tgx_ctx* c, int row0, int R, bool force) {
  if (!c->lp_rows) { c->launch_fault = "log-probabilities requested before their buffers exist"; return; }
  tgx::LpArgs a = lp_args(c);
  const size_t T = (size_t)a.nwg;
  a.logits = c->rows[(size_t)row0].logits;
  a.req = c->row_req + row0; a.st = c->lp_rows + row0; a.tok = c->rows[(size_t)row0].tok;
  a.force = force ? 1 : 0;
  a.tile_max = c->lp_tile_max + row0 * T; a.tile_sum = c->lp_tile_sum + row0 * T; a.tile_keys = c->lp_tile_keys + row0 * T * tgx::LP_MAX;
  a.ring = c->lp_ring + (size_t)row0 * tgx::LP_RING;
  lp_launch(c, a, R);
}

void launch_logprobs_verify(tgx_ctx* c, int row, int M, int joint_first, int joint_i) {
  if (!c->lp_rows) { c->launch_fault = "log-probabilities requested before their buffers exist"; return; }
  const bool joint = joint_first >= 0;
  tgx::LpArgs a = lp_args(c);
  a.logits = joint ? c->vj_logits + (size_t)joint_first * c->d.vocab : c->vf_logits;
  a.req = c->row_req + row; a.st = c->lp_rows + row;
  a.rec = joint ? reinterpret_cast<const tgx::VerifyRecord*>(c->vj_rec) + joint_i : reinterpret_cast<const tgx::VerifyRecord*>(c->vf_rec);
  a.tile_max = c->lp_tile_max; a.tile_sum = c->lp_tile_sum; a.tile_keys = c->lp_tile_keys;
  a.ring = c->lp_ring + (size_t)row * tgx::LP_RING;
  lp_launch(c, a, M);
}

int sampler_alloc(tgx_ctx* c) {
  const tgx_model_desc& d = c->d;
  int rc;
  if ((rc = dev_alloc(c, &c->samp_scratch, (size_t)d.max_batch))) return rc;
  HIP_OK(c, hipMemset(c->samp_scratch, 0, sizeof(tgx::SampScratch) * (size_t)d.max_batch));
  // the compacted list of a filter's threshold bin: a few thousand entries on real logits, the whole vocabulary when every logit is equal
  if ((rc = dev_alloc(c, &c->samp_list_comp, (size_t)d.max_batch * d.vocab)) || (rc = dev_alloc(c, &c->samp_list_v, (size_t)d.max_batch * d.vocab))) return rc;
  if ((d.vocab + tgx::SAMP_TILE - 1) / tgx::SAMP_TILE > tgx::SAMP_MAX_WG) return set_err(c, TGX_ERR_UNSUPPORTED, "vocabulary %d exceeds the sampler's %d entries", d.vocab, tgx::SAMP_MAX_WG * tgx::SAMP_TILE);
  return TGX_OK;
}

// ---- beam search (kernels/beam.h; include/tgx.h tgx_beam_select / tgx_beam_advance)
static_assert(tgx::BEAM_MAX_ROWS == TGX_MAX_BEAMS && tgx::BEAM_MAX_CAND == TGX_MAX_BEAM_CAND && tgx::BEAM_ROW_CAND == TGX_MAX_BEAMS + TGX_MAX_STOP_IDS, "kernels/beam.h");
static_assert(sizeof(tgx::BeamCand) == sizeof(tgx_beam_cand) && offsetof(tgx::BeamCand, score) == offsetof(tgx_beam_cand, score), "kernels/beam.h BeamCand");

int beam_select_run(tgx_ctx* c, int n, const int32_t* rows, const float* scores, int k, const int32_t* end_ids, int n_end, tgx_beam_cand* out, int32_t* out_n) {
  const size_t V = (size_t)c->d.vocab, T = (size_t)lp_tiles(c), R = (size_t)tgx::BEAM_MAX_ROWS;
  // the workspace, widest elements first: tile sums | tile keys | row lse | row keys | record | tile maxima
  const size_t o_sum = 0, o_keys = o_sum + R * T * 8, o_lse = o_keys + R * T * tgx::LP_MAX * 8, o_rkeys = o_lse + R * 8, o_rec = o_rkeys + R * tgx::BEAM_ROW_CAND * 8,
               o_max = o_rec + sizeof(tgx::BeamRecord), total = o_max + R * T * 4;
  if (!c->beam_ws) { if (int rc = dev_alloc(c, &c->beam_ws, total)) return rc; }      // sized by the first call: the vocabulary is the context's
  tgx::BeamSelArgs a{};
  for (int i = 0; i < n; i++) {
    const int row = rows[i];
    const bool processed = row_processed(c, row);      // what tgx_sample_row would draw from: the row's processors without the counting step, no state moves
    if (processed) launch_logit_proc(c, row, 1, /*step=*/false);
    a.lg[i] = processed ? c->proc_logits + (size_t)row * V : c->rows[(size_t)row].logits;
    a.score[i] = scores[i];
  }
  for (int e = 0; e < n_end; e++) a.end_id[e] = end_ids[e];
  a.n = n; a.k = k; a.n_end = n_end; a.top_n = k + n_end;
  a.V = (int)V; a.nwg = (int)T;
  a.tile_sum = reinterpret_cast<double*>(c->beam_ws + o_sum); a.tile_keys = reinterpret_cast<unsigned long long*>(c->beam_ws + o_keys);
  a.row_lse = reinterpret_cast<double*>(c->beam_ws + o_lse); a.row_keys = reinterpret_cast<unsigned long long*>(c->beam_ws + o_rkeys);
  a.rec = reinterpret_cast<tgx::BeamRecord*>(c->beam_ws + o_rec); a.tile_max = reinterpret_cast<float*>(c->beam_ws + o_max);
  hipLaunchKernelGGL(tgx::beam_tile_kernel, dim3((unsigned)T, (unsigned)n), dim3(tgx::SAMP_WG), 0, c->stream, a);
  hipLaunchKernelGGL(tgx::beam_row_kernel, dim3((unsigned)n), dim3(tgx::SAMP_WG), 0, c->stream, a);
  hipLaunchKernelGGL(tgx::beam_rank_kernel, dim3(1), dim3(tgx::BEAM_MAX_ROWS * tgx::BEAM_ROW_CAND), 0, c->stream, a);
  HIP_OK(c, hipGetLastError());
  LAUNCH_OK(c);
  tgx::BeamRecord rec;
  HIP_OK(c, hipMemcpyAsync(&rec, a.rec, sizeof(rec), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  const int m = std::max(0, std::min(rec.n, (int)tgx::BEAM_MAX_CAND));
  for (int i = 0; i < m; i++) { out[i].beam = rec.cand[i].beam; out[i].token = rec.cand[i].token; out[i].score = rec.cand[i].score; out[i].lp = rec.cand[i].lp; }
  *out_n = m;
  return TGX_OK;
}

void launch_beam_publish(tgx_ctx* c, int n, const int* rows, const int32_t* tokens) {
  tgx::BeamPublishArgs a{};
  for (int j = 0; j < n; j++) {
    RowState& r = c->rows[(size_t)rows[j]];
    a.tok[j] = r.tok; a.pos[j] = r.pos; a.x[j] = r.x; a.token[j] = tokens[j];
  }
  a.embed = c->embed; a.wpe = c->gpt2 ? c->wpe : nullptr; a.H = c->d.hidden; a.n_pos = c->d.n_positions > 0 ? c->d.n_positions : 1;
  TGX_DT_SWITCH(c->dt, hipLaunchKernelGGL(tgx::beam_publish_kernel<DT>, dim3((unsigned)n), dim3(256), 0, c->stream, a))
}

#ifdef TGX_SAMP_TIMELINE
// experiment builds only (tools/sampler_timeline.py): row 0's stamps, [64][10] ticks of the 100 MHz wall clock + the number of steps stamped
extern "C" __attribute__((visibility("default"))) int tgx_debug_samp_timeline(tgx_ctx* c, unsigned long long* out, unsigned int* n) {
  if (hipStreamSynchronize(c->stream) != hipSuccess) return 1;
  tgx::SampScratch h;
  if (hipMemcpy(&h, c->samp_scratch, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  memcpy(out, h.tl, sizeof(h.tl)); *n = h.tl_n;
  return 0;
}
#endif
