// beam.h — the hypothesis bookkeeping of beam search above tgx_beam_select / tgx_beam_advance (include/tgx.h).  Host-only — the standard library alone:
// tests/beam_check.cpp drives it on a CPU against a restatement of the rules in Python (tests/test_beam_host.py).
//
// THE RULES (pinned):
//   * a step hands the scorer the candidate list of tgx_beam_select, best first.  A candidate whose token is an end id is a hypothesis that ENDS here — it counts
//     only at list index < numBeams; every other candidate, in list order, is the next running beam, until numBeams of them are taken.
//   * a finished hypothesis scores sum_lp / L^lengthPenalty, L = its produced tokens including the end id, in double.  The best numBeams finished hypotheses are
//     kept: a new one replaces the worst kept one only if it scores strictly higher.
//   * the search is DONE when numBeams hypotheses are finished and either earlyStopping is set or the best running beam can no longer beat the worst kept one:
//     its sum_lp / D^lengthPenalty, D = maxNewTokens for lengthPenalty > 0 and the current length otherwise, is not above the worst kept score.  It is also done
//     when no running beam is left.
//   * at maxNewTokens — the done test above comes first — the running beams are added as they stand (finish reason Length), by the same "strictly higher" rule,
//     in beam order.
//   * the result is the kept hypotheses, best first; equal scores keep the order in which they were added.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace tgxh {

struct BeamCand { int32_t beam, token; float score, lp; };      // == tgx_beam_cand

struct BeamHyp {
  std::vector<int32_t> tokens;      // the produced tokens (the end id included when it ended on one)
  float sumLp = 0.f;
  double score = 0.0;
  bool length = false;              // finish reason Length (it was still running at maxNewTokens); else Stop
  long long order = 0;              // when it was added
};

class BeamScorer {
 public:
  BeamScorer(int numBeams, float lengthPenalty, bool earlyStopping, int64_t maxNewTokens, std::vector<int32_t> endIds)
      : K_(numBeams), lp_(lengthPenalty), early_(earlyStopping), maxNew_(maxNewTokens), ends_(std::move(endIds)) {
    run_.assign(1, {}); scores_.assign(1, 0.f);      // one empty hypothesis: the prompt
  }
  int running() const { return (int)run_.size(); }
  const std::vector<float>& scores() const { return scores_; }          // the running beams' sum_lp, in beam order: tgx_beam_select's `scores`
  const std::vector<int32_t>& parents() const { return parents_; }      // after step(): beam j continues beam parents()[j] of before ...
  const std::vector<int32_t>& tokens() const { return tokens_; }        // ... with this token: tgx_beam_advance's `parent` and `tokens`
  int64_t length() const { return len_; }
  bool isEnd(int32_t t) const { for (int32_t e : ends_) if (e == t) return true; return false; }

  // one step's candidate list; true: the search is done (finish() has the result)
  bool step(const BeamCand* c, int n) {
    std::vector<std::vector<int32_t>> next;
    std::vector<float> nextScore;
    parents_.clear(); tokens_.clear();
    len_++;
    for (int i = 0; i < n && (int)next.size() < K_; i++) {
      if (c[i].beam < 0 || c[i].beam >= (int)run_.size()) continue;
      std::vector<int32_t> seq = run_[(size_t)c[i].beam];
      seq.push_back(c[i].token);
      if (isEnd(c[i].token)) {
        if (i < K_) add(std::move(seq), c[i].score, false);
        continue;
      }
      next.push_back(std::move(seq)); nextScore.push_back(c[i].score);
      parents_.push_back(c[i].beam); tokens_.push_back(c[i].token);
    }
    run_ = std::move(next); scores_ = std::move(nextScore);
    if (run_.empty()) return done_ = true;
    if ((int)kept_.size() >= K_) {
      if (early_) return done_ = true;
      const double d = lp_ > 0.f ? (double)maxNew_ : (double)len_;
      const double bound = (double)scores_[0] / std::pow(d, (double)lp_);      // scores_[0]: the list is best first
      if (!(bound > worst().score)) return done_ = true;
    }
    if (len_ >= maxNew_) {
      for (size_t b = 0; b < run_.size(); b++) add(run_[b], scores_[b], true);
      return done_ = true;
    }
    return false;
  }
  bool done() const { return done_; }
  // the kept hypotheses, best first
  std::vector<BeamHyp> finish() const {
    std::vector<BeamHyp> out = kept_;
    for (size_t i = 1; i < out.size(); i++)      // insertion sort: score descending, then the order of adding
      for (size_t k = i; k > 0 && (out[k].score > out[k - 1].score || (out[k].score == out[k - 1].score && out[k].order < out[k - 1].order)); k--) std::swap(out[k], out[k - 1]);
    return out;
  }

 private:
  const BeamHyp& worst() const {
    size_t w = 0;
    for (size_t i = 1; i < kept_.size(); i++)
      if (kept_[i].score < kept_[w].score || (kept_[i].score == kept_[w].score && kept_[i].order > kept_[w].order)) w = i;
    return kept_[w];
  }
  void add(std::vector<int32_t> seq, float sumLp, bool length) {
    BeamHyp h;
    h.sumLp = sumLp; h.length = length; h.order = added_++;
    h.score = (double)sumLp / std::pow((double)seq.size(), (double)lp_);
    h.tokens = std::move(seq);
    if ((int)kept_.size() < K_) { kept_.push_back(std::move(h)); return; }
    const BeamHyp& w = worst();
    if (h.score > w.score) kept_[(size_t)(&w - kept_.data())] = std::move(h);
  }
  int K_;
  float lp_;
  bool early_;
  int64_t maxNew_;
  std::vector<int32_t> ends_;
  std::vector<std::vector<int32_t>> run_;
  std::vector<float> scores_;
  std::vector<int32_t> parents_, tokens_;
  std::vector<BeamHyp> kept_;
  int64_t len_ = 0;
  long long added_ = 0;
  bool done_ = false;
};

}   // namespace tgxh
