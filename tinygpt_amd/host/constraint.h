// constraint.h — constrained decoding on the host: a regular expression compiled into a token automaton over a tokenizer's vocabulary, the table
// tgx_automaton_create takes (include/tgx.h).  The device then masks and steps a row without the host (kernels/logit_proc.h); this runs once per request.
//
// The supported subset — the WHOLE output must match, anchors are implicit:
//   literals (UTF-8 included, as their byte sequences), escapes \d \w \s (ASCII: [0-9], [A-Za-z0-9_], [ \t\n\r\f\v]) \n \t \r \f \v \\ and escaped punctuation,
//   classes [a-z0-9_] and negated classes [^...] over ASCII members, `.`, `|`, `( )` and `(?: )`, `? * +`, `{m}`, `{m,n}`, `{m,}`.
//   `.` and negated classes match well-formed UTF-8 code points (`.`: all but newline), never stray bytes.
// Anything else fails with a message that names the byte position: backreferences, lookaround and other `(?` groups, lazy and possessive quantifiers,
// non-ASCII class members, \D \W \S \b and the other escapes, `^` and `$`, an empty alternative or group, malformed UTF-8 in the pattern.
//
// Pipeline: a small recursive-descent parser of this subset (host/regex.cpp is a backtracking matcher whose parser builds its matcher's program and knows
// Unicode categories this subset does not have: sharing it would be more code, not less) -> Thompson NFA over bytes -> subset construction to a byte DFA ->
// states that cannot reach acceptance dropped -> Moore's partition refinement (the DFA IS minimised: a table row costs 2 * vocab bytes on the device) ->
// for every state and every ordinary token, the walk of the token's bytes (Tokenizer::id2Token: raw bytes for byte-level tokens).  A token is allowed iff the
// walk stays inside the live DFA, its target the state reached.  Added / special tokens and tokens without bytes are never allowed; in ACCEPTING states every
// stop id the caller passes gets the state itself as its target, so that the row can end there and nowhere else.
// The compile FAILS with a message, never a partial table: a state left with no allowed token (only a vocabulary that lacks single-byte tokens, or an
// accepting state without continuation when no stop id was passed), more states than maxStates, a table above maxTableBytes.
//
// Scope: tokenizers whose decoder is ByteLevel (GPT-2, Llama 3, Qwen), where decode(ids) is the concatenation of the tokens' bytes.  A Metaspace / ByteFallback
// tokenizer is refused: its first-token space handling makes "the decoded text matches" a different problem.
// If maxNewTokens ends a row before the automaton reaches a stop, the output is a PREFIX of a match (engine.h SamplerConfig::regex).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "tokenizer.h"

namespace tgxh {

struct ByteDfa {
  int32_t nStates = 0, start = 0;
  std::vector<int32_t> next;      // [nStates][256]; -1: no match can follow
  std::vector<char> accept;       // [nStates]
  bool matches(const std::string& bytes) const {
    int32_t s = start;
    for (unsigned char c : bytes) { s = next[(size_t)s * 256 + c]; if (s < 0) return false; }
    return accept[(size_t)s] != 0;
  }
};

struct TokenAutomaton {           // what tgx_automaton_create takes
  int32_t nStates = 0, start = 0, vocab = 0;
  std::vector<uint16_t> next;     // [nStates][vocab]; 0xFFFF: not allowed
  std::vector<char> accept;       // [nStates]: the stop ids are allowed here
};

struct ConstraintLimits {
  int maxStates = 4096;
  size_t maxTableBytes = (size_t)256 << 20;
};

// pattern -> the minimal byte DFA of its language without dead states; false + err (with the position) on a pattern outside the subset or beyond maxStates
bool compileByteDfa(const std::string& pattern, ByteDfa& out, std::string& err, int maxStates = 4096);

// the token table of `dfa` over a vocabulary given as bytes per id (an empty string: never allowed), `vocab` entries wide (ids beyond tokens.size() are never
// allowed, tokens beyond vocab are dropped); stopIds: allowed in accepting states
bool compileTokenTable(const ByteDfa& dfa, const std::vector<std::string>& tokens, int32_t vocab, const std::vector<int32_t>& stopIds, TokenAutomaton& out,
                       std::string& err, const ConstraintLimits& lim = ConstraintLimits());

// the vocabulary of a ByteLevel tokenizer as compileTokenTable takes it; false + err for a tokenizer outside the scope above
inline bool constraintVocabulary(const Tokenizer& tok, std::vector<std::string>& out, std::string& err) {
  if (!tok.byteLevelDecoder()) { err = "constrained decoding needs a ByteLevel tokenizer (GPT-2, Llama 3, Qwen): a Metaspace / ByteFallback decoder is not supported"; return false; }
  out.assign(tok.vocabSize(), std::string());
  for (size_t i = 0; i < out.size(); i++)
    if (!tok.isAddedToken((int32_t)i)) out[i] = tok.id2Token((int32_t)i);
  return true;
}

inline bool compileConstraint(const std::string& pattern, const Tokenizer& tok, int32_t vocab, const std::vector<int32_t>& stopIds, TokenAutomaton& out, std::string& err,
                              const ConstraintLimits& lim = ConstraintLimits()) {
  std::vector<std::string> tokens;
  ByteDfa dfa;
  return constraintVocabulary(tok, tokens, err) && compileByteDfa(pattern, dfa, err, lim.maxStates) && compileTokenTable(dfa, tokens, vocab, stopIds, out, err, lim);
}

}  // namespace tgxh
