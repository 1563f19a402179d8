// constraint_check.cpp — the CPU audit of tinygpt_amd/csrc/automaton.h (the table validation of tgx_automaton_create) and of the pattern compiler
// tinygpt_amd/host/constraint.cpp (built and run by tests/test_constraint_compile.py under the address and undefined-behaviour sanitizers).  Parts: good tables are
// accepted and each refusal of include/tgx.h is given with a reason; random tables with out-of-range entries and dead-end states are refused, every table a heap
// block of exactly its size (a read outside it is an AddressSanitizer report); good patterns compile and decide a few strings; every malformed pattern is refused
// with a message that names a position or a cap, never a crash; random byte strings as patterns never crash and what compiles passes the table validation over
// a vocabulary of the 256 single bytes plus a few longer tokens.
#include "../tinygpt_amd/csrc/automaton.h"
#include "../tinygpt_amd/host/constraint.cpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define REQUIRE(cond)                                                                                   \
  do {                                                                                                  \
    if (!(cond)) { fprintf(stderr, "constraint_check: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// validate() on a heap copy of exactly the table's size
static bool table_ok(int n_states, int start, const std::vector<uint16_t>& t, int vocab, std::string* why = nullptr) {
  const size_t words = n_states > 0 && n_states <= automaton::MAX_STATES ? (size_t)n_states * (size_t)vocab : 0;
  uint16_t* p = static_cast<uint16_t*>(malloc(words ? words * 2 : 2));
  REQUIRE(p != nullptr);
  if (words) { REQUIRE(t.size() >= words); memcpy(p, t.data(), words * 2); }
  char msg[160];
  const char* r = automaton::validate(n_states, start, p, vocab, msg, sizeof(msg));
  REQUIRE((r == nullptr) == (msg[0] == 0));
  if (why) *why = msg;
  free(p);
  return r == nullptr;
}

static void check_tables() {
  const int V = 37, N = 5;
  std::vector<uint16_t> good((size_t)N * V, automaton::NONE);
  for (int s = 0; s < N; s++) { good[(size_t)s * V + (size_t)(s * 7 % V)] = (uint16_t)((s + 1) % N); good[(size_t)s * V + V - 1] = (uint16_t)s; }
  std::string why;
  REQUIRE(table_ok(N, 0, good, V) && table_ok(N, N - 1, good, V) && table_ok(1, 0, std::vector<uint16_t>((size_t)V, 0), V));
  REQUIRE(!table_ok(0, 0, good, V, &why) && why.find("n_states") != std::string::npos);
  REQUIRE(!table_ok(-3, 0, good, V) && !table_ok(automaton::MAX_STATES + 1, 0, good, V));
  REQUIRE(!table_ok(N, N, good, V, &why) && why.find("start") != std::string::npos);
  REQUIRE(!table_ok(N, -1, good, V));
  { char msg[64]; REQUIRE(automaton::validate(N, 0, nullptr, V, msg, sizeof(msg)) != nullptr); }
  { std::vector<uint16_t> t(good); t[(size_t)2 * V + 3] = (uint16_t)N; REQUIRE(!table_ok(N, 0, t, V, &why) && why.find("next[2][3]") != std::string::npos); }
  { std::vector<uint16_t> t(good); t[(size_t)4 * V + 0] = 0xFFFE; REQUIRE(!table_ok(N, 0, t, V)); }
  { std::vector<uint16_t> t(good); for (int k = 0; k < V; k++) t[(size_t)3 * V + (size_t)k] = automaton::NONE; REQUIRE(!table_ok(N, 0, t, V, &why) && why.find("state 3") != std::string::npos); }
  REQUIRE(automaton::state_ok(N, -1) && automaton::state_ok(N, 0) && automaton::state_ok(N, N - 1) && !automaton::state_ok(N, N) && !automaton::state_ok(N, -2));
  REQUIRE(automaton::table_bytes(64, 128256) == (size_t)64 * 128256 * 2);
  // random tables: an independent verdict (every entry a state or NONE, every state with an allowed token) must agree
  int accepted = 0, refused = 0;
  for (int it = 0; it < 4000; it++) {
    const int n = 1 + (int)(rnd() % 9), v = 1 + (int)(rnd() % 40), mode = (int)(rnd() % 4);
    std::vector<uint16_t> t((size_t)n * v);
    for (auto& e : t) {
      const uint64_t r = rnd();
      e = r % 3 == 0 ? automaton::NONE : (uint16_t)(r % (uint64_t)n);
      if (mode == 1 && r % 97 == 0) e = (uint16_t)(n + (int)(r % 5));           // out of range
      if (mode == 2 && r % 89 == 0) e = (uint16_t)(rnd() & 0xFFFF);             // anything
    }
    if (mode == 3) { const int s = (int)(rnd() % (uint64_t)n); for (int k = 0; k < v; k++) t[(size_t)s * v + (size_t)k] = automaton::NONE; }      // a dead end
    bool want = true;
    for (int s = 0; s < n && want; s++) {
      bool any = false;
      for (int k = 0; k < v; k++) { const uint16_t e = t[(size_t)s * v + (size_t)k]; if (e == automaton::NONE) continue; if (e >= n) want = false; any = true; }
      if (!any) want = false;
    }
    REQUIRE(table_ok(n, (int)(rnd() % (uint64_t)n), t, v) == want);
    (want ? accepted : refused)++;
  }
  REQUIRE(accepted > 200 && refused > 200);
}

static std::vector<std::string> byte_vocab() {
  std::vector<std::string> tok;
  for (int b = 0; b < 256; b++) tok.push_back(std::string(1, (char)b));
  for (const char* w : {"yes", "no", "may", "be", " the", "12", "2024", "-0", "\xc3\xa9", "\xe2\x82\xac", "ab", "abc", "{\"", "\": "}) tok.push_back(w);
  tok.push_back("");            // an added token: never allowed
  tok.push_back("<eos>");      // (listed without bytes below)
  tok.back().clear();
  return tok;
}

static bool compiles(const std::string& pat, std::string* err = nullptr, int max_states = 4096) {
  tgxh::ByteDfa d;
  std::string e;
  const bool ok = tgxh::compileByteDfa(pat, d, e, max_states);
  REQUIRE(ok == e.empty());
  if (ok) { REQUIRE(d.nStates >= 1 && d.nStates <= max_states && d.start >= 0 && d.start < d.nStates && d.next.size() == (size_t)d.nStates * 256 && d.accept.size() == (size_t)d.nStates); }
  if (err) *err = e;
  return ok;
}
static bool matches(const std::string& pat, const std::string& s) {
  tgxh::ByteDfa d;
  std::string e;
  REQUIRE(tgxh::compileByteDfa(pat, d, e));
  return d.matches(s);
}

static void check_patterns() {
  REQUIRE(matches("(yes|no|maybe)", "maybe") && !matches("(yes|no|maybe)", "mayb") && !matches("(yes|no|maybe)", "yesno"));
  REQUIRE(matches("\\d{4}-\\d{2}-\\d{2}", "2024-02-29") && !matches("\\d{4}-\\d{2}-\\d{2}", "2024-2-29"));
  REQUIRE(matches("\\{\"name\": \"[a-z]+\", \"age\": \\d+\\}", "{\"name\": \"bo\", \"age\": 7}"));
  REQUIRE(matches("a{2,}", "aaaa") && !matches("a{2,}", "a") && matches("a{0,2}b?", "") && matches("(?:ab)*c", "ababc"));
  REQUIRE(matches("caf\xc3\xa9.", "caf\xc3\xa9\xe2\x82\xac") && !matches("caf\xc3\xa9.", "caf\xc3\xa9\n") && !matches(".", "\xc3") && !matches(".", "\xc0\xaf") && !matches("[^a]", "\xed\xa0\x80"));
  REQUIRE(matches("[^a-c]+", "xyz\xc3\xa9\n") && !matches("[^a-c]+", "xbz") && matches("[\\d\\-x]+", "1-x") && matches("\\\\\\.", "\\."));
  // minimised: the three spellings of one language need the same number of states
  { tgxh::ByteDfa a, b; std::string e; REQUIRE(tgxh::compileByteDfa("(a|b)*abb", a, e) && tgxh::compileByteDfa("(b|a)*(abb)", b, e) && a.nStates == b.nStates && a.nStates == 4); }
  // malformed and unsupported: a clean refusal with a message
  const char* bad[] = {"", "(", "(ab", "ab)", "((a)", "a{5,2}", "a{", "a{2", "a{x}", "a{1001}", "*a", "a|", "|a", "(|a)", "()", "a||b", "[", "[]", "[a", "[z-a]", "[\xc3\xa9]", "[a-\xc3\xa9]",
                       "a\\", "\\1", "(a)\\1", "(?=a)b", "(?!a)b", "(?<=a)b", "(?P<n>a)", "a*?", "a+?", "a??", "a{2}?", "a*+", "a**", "\\D", "\\W", "\\S", "\\b", "\\x41", "\\pL", "^a", "a$",
                       "caf\xc3", "\xa9", "\xe2\x82", "\xc0\xaf", "\xed\xa0\x80", "\xf5\x80\x80\x80"};
  for (const char* p : bad) {
    std::string err;
    if (compiles(p, &err)) { fprintf(stderr, "constraint_check: pattern '%s' was accepted\n", p); exit(1); }
    REQUIRE(err.find("position") != std::string::npos);
  }
  // repeats that blow the caps: the DFA cap, the NFA cap, a small cap
  std::string err;
  REQUIRE(!compiles("(a|b)*a(a|b){14}", &err) && err.find("DFA states") != std::string::npos);
  REQUIRE(!compiles("((a|b){1000}){1000}", &err) && err.find("states") != std::string::npos);
  REQUIRE(compiles("(a|b)*a(a|b){3}") && !compiles("(a|b)*a(a|b){3}", &err, 8));
  { std::string deep; for (int k = 0; k < 5000; k++) deep += '('; REQUIRE(!compiles(deep, &err) && err.find("nested") != std::string::npos); }
  // token tables over the byte vocabulary: pass the device's validation; stop ids only where the match may end; caps and dead ends refused
  const std::vector<std::string> tok = byte_vocab();
  const int32_t V = (int32_t)tok.size() + 3, EOS = (int32_t)tok.size() - 1;      // three padding ids past the tokenizer's vocabulary
  for (const char* p : {"(yes|no|maybe)", "\\d{4}-\\d{2}-\\d{2}", "\\{\"name\": \"[a-z]+\", \"age\": \\d+\\}", ".*", "[^x]+\xe2\x82\xac"}) {
    tgxh::ByteDfa d;
    tgxh::TokenAutomaton a;
    REQUIRE(tgxh::compileByteDfa(p, d, err) && tgxh::compileTokenTable(d, tok, V, {EOS}, a, err));
    REQUIRE(a.nStates == d.nStates && a.vocab == V && table_ok(a.nStates, a.start, a.next, V));
    for (int s = 0; s < a.nStates; s++) {
      REQUIRE((a.next[(size_t)s * V + (size_t)EOS] != automaton::NONE) == (a.accept[(size_t)s] != 0));
      for (int t = EOS - 1; t < V; t++) if (t != EOS) REQUIRE(a.next[(size_t)s * V + (size_t)t] == automaton::NONE);      // the added token and the padding ids
    }
  }
  {
    tgxh::ByteDfa d;
    tgxh::TokenAutomaton a;
    REQUIRE(tgxh::compileByteDfa("(yes|no)", d, err));
    REQUIRE(!tgxh::compileTokenTable(d, tok, V, {}, a, err) && a.next.empty() && err.find("no allowed token") != std::string::npos);            // the match can only end
    REQUIRE(!tgxh::compileTokenTable(d, {"yes", "n"}, 4, {3}, a, err) && a.next.empty());                                                           // no single-byte tokens
    REQUIRE(!tgxh::compileTokenTable(d, tok, V, {V}, a, err) && !tgxh::compileTokenTable(d, tok, V, {-1}, a, err));
    tgxh::ConstraintLimits lim;
    lim.maxTableBytes = 64;
    REQUIRE(!tgxh::compileTokenTable(d, tok, V, {EOS}, a, err, lim) && err.find("exceeds the cap") != std::string::npos);
    lim = tgxh::ConstraintLimits(); lim.maxStates = 2;
    REQUIRE(!tgxh::compileTokenTable(d, tok, V, {EOS}, a, err, lim));
  }
  // random strings over the metacharacters as patterns: never a crash; what compiles yields a valid table or a clean refusal
  const char alphabet[] = "ab|()[]{}*+?.\\^-,019d\xc3\xa9";
  int ok = 0, no = 0;
  for (int it = 0; it < 3000; it++) {
    std::string p;
    const int n = 1 + (int)(rnd() % 12);
    for (int k = 0; k < n; k++) p += alphabet[rnd() % (sizeof(alphabet) - 1)];
    tgxh::ByteDfa d;
    if (!tgxh::compileByteDfa(p, d, err, 512)) { REQUIRE(!err.empty()); no++; continue; }
    tgxh::TokenAutomaton a;
    if (tgxh::compileTokenTable(d, tok, V, {EOS}, a, err)) REQUIRE(table_ok(a.nStates, a.start, a.next, V));
    ok++;
  }
  REQUIRE(ok > 100 && no > 100);
}

int main() {
  check_tables();
  check_patterns();
  printf("constraint_check: ok\n");
  return 0;
}
