// automaton.h — the host-side checks of a token automaton's table (include/tgx.h tgx_automaton_create / tgx_set_row_automaton).  Host-only and free of HIP, so
// that tests/constraint_check.cpp audits it under the sanitizers without a GPU: abi.hip calls validate() before anything is allocated or copied, and the pattern
// compiler (host/constraint.cpp) holds its own output to the same rule.
//
// A table is next[n_states][vocab] of 16-bit words: the state after token t in state s, or NONE (the token is not allowed there).  The kernels index the table
// with a row's state word and trust it (kernels/logit_proc.h), so every entry a row can reach must be a state of the table, and a state without an allowed token
// would leave a row with logits of -inf throughout: both are refused here, once, instead of being tested on the device at every step.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace automaton {

constexpr uint16_t NONE = 0xFFFFu;        // == TGX_AUTOMATON_NONE
constexpr int MAX_STATES = 65535;         // == TGX_MAX_AUTOMATON_STATES: state ids 0 .. 65534
constexpr int MAX_TABLES = 16;            // == TGX_MAX_AUTOMATA

inline size_t table_bytes(int n_states, int vocab) { return (size_t)n_states * (size_t)vocab * sizeof(uint16_t); }

// nullptr when (n_states, start, next) is a table the kernels may walk over a vocabulary of `vocab` ids, else the reason in msg (cap bytes, always terminated)
inline const char* validate(int n_states, int start, const uint16_t* next, int vocab, char* msg, size_t cap) {
  if (cap) msg[0] = 0;
  if (!next) { snprintf(msg, cap, "null table"); return msg; }
  if (vocab < 1) { snprintf(msg, cap, "vocabulary %d < 1", vocab); return msg; }
  if (n_states < 1 || n_states > MAX_STATES) { snprintf(msg, cap, "n_states %d out of range [1,%d]", n_states, MAX_STATES); return msg; }
  if (start < 0 || start >= n_states) { snprintf(msg, cap, "start state %d out of range [0,%d)", start, n_states); return msg; }
  for (int s = 0; s < n_states; s++) {
    const uint16_t* row = next + (size_t)s * (size_t)vocab;
    bool any = false;
    for (int t = 0; t < vocab; t++) {
      const uint16_t e = row[t];
      if (e == NONE) continue;
      if ((int)e >= n_states) { snprintf(msg, cap, "next[%d][%d] = %u is neither a state below %d nor NONE", s, t, (unsigned)e, n_states); return msg; }
      any = true;
    }
    if (!any) { snprintf(msg, cap, "state %d allows no token (a dead end)", s); return msg; }
  }
  return nullptr;
}

// a row's setting: state -1 is the table's start
inline bool state_ok(int n_states, int state) { return state >= -1 && state < n_states; }

}  // namespace automaton
