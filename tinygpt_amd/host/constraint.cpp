// constraint.cpp — the pattern compiler of constraint.h: parser -> Thompson NFA -> byte DFA (pruned, minimised) -> token table.  Tokenizer-free, so that
// tests/constraint_check.cpp compiles it stand-alone under the sanitizers.
#include "constraint.h"

#include <algorithm>
#include <map>

namespace tgxh {
namespace {

struct ByteSet {
  uint64_t w[4] = {0, 0, 0, 0};
  void add(int b) { w[b >> 6] |= 1ull << (b & 63); }
  void addRange(int lo, int hi) { for (int b = lo; b <= hi; b++) add(b); }
  bool has(int b) const { return (w[b >> 6] >> (b & 63)) & 1; }
  void merge(const ByteSet& o) { for (int i = 0; i < 4; i++) w[i] |= o.w[i]; }
};

// ---- the syntax tree
struct Node {
  enum Kind { Set, Cat, Alt, Repeat } kind = Set;
  ByteSet set;                    // Set: one byte out of these
  std::vector<int> kids;          // Cat / Alt; Repeat: kids[0]
  int lo = 0, hi = 0;             // Repeat: hi < 0 = unbounded
};

constexpr int kMaxRepeat = 1000;           // {m,n}: counts beyond this are refused outright
constexpr size_t kMaxNodes = 1u << 16;
constexpr int kMaxDepth = 100;             // nested groups (the parser and the NFA builder recurse)

struct Parser {
  const std::string& p;
  size_t i = 0;
  int depth = 0;
  std::vector<Node> nodes;
  std::string err;

  explicit Parser(const std::string& pat) : p(pat) {}
  bool fail(size_t pos, const std::string& what) {
    if (err.empty()) err = "regex position " + std::to_string(pos) + ": " + what;
    return false;
  }
  int add(const Node& n) { nodes.push_back(n); return (int)nodes.size() - 1; }
  int setNode(const ByteSet& s) { Node n; n.kind = Node::Set; n.set = s; return add(n); }
  int seq(Node::Kind k, const std::vector<int>& kids) {
    if (kids.size() == 1) return kids[0];
    Node n; n.kind = k; n.kids = kids; return add(n);
  }
  int range(int lo, int hi) { ByteSet s; s.addRange(lo, hi); return setNode(s); }
  // every well-formed UTF-8 sequence of two to four bytes (no overlong forms, no surrogates, nothing above U+10FFFF)
  void multibyte(std::vector<int>& alts) {
    const int c = range(0x80, 0xBF);
    alts.push_back(seq(Node::Cat, {range(0xC2, 0xDF), c}));
    alts.push_back(seq(Node::Cat, {range(0xE0, 0xE0), range(0xA0, 0xBF), c}));
    alts.push_back(seq(Node::Cat, {range(0xE1, 0xEC), c, c}));
    alts.push_back(seq(Node::Cat, {range(0xED, 0xED), range(0x80, 0x9F), c}));
    alts.push_back(seq(Node::Cat, {range(0xEE, 0xEF), c, c}));
    alts.push_back(seq(Node::Cat, {range(0xF0, 0xF0), range(0x90, 0xBF), c, c}));
    alts.push_back(seq(Node::Cat, {range(0xF1, 0xF3), c, c, c}));
    alts.push_back(seq(Node::Cat, {range(0xF4, 0xF4), range(0x80, 0x8F), c, c}));
  }
  // any code point but the ASCII ones in `not_ascii`
  int codePointsBut(const ByteSet& not_ascii) {
    ByteSet a;
    for (int b = 0; b < 0x80; b++) if (!not_ascii.has(b)) a.add(b);
    std::vector<int> alts;
    if (a.w[0] | a.w[1]) alts.push_back(setNode(a));
    multibyte(alts);
    return seq(Node::Alt, alts);
  }
  static bool classEscape(char c, ByteSet& s) {
    switch (c) {
      case 'd': s.addRange('0', '9'); return true;
      case 'w': s.addRange('0', '9'); s.addRange('a', 'z'); s.addRange('A', 'Z'); s.add('_'); return true;
      case 's': s.add(' '); s.addRange('\t', '\r'); return true;
      default: return false;
    }
  }
  // the escape at p[i] (behind the backslash): a class (`cls`) or one byte (`byte`)
  bool escape(ByteSet& cls, int& byte, bool& is_class) {
    if (i >= p.size()) return fail(i - 1, "a backslash at the end of the pattern");
    const unsigned char c = (unsigned char)p[i];
    is_class = false;
    if (classEscape((char)c, cls)) { is_class = true; i++; return true; }
    switch (c) {
      case 'n': byte = '\n'; break;
      case 't': byte = '\t'; break;
      case 'r': byte = '\r'; break;
      case 'f': byte = '\f'; break;
      case 'v': byte = '\v'; break;
      default:
        if (c >= '1' && c <= '9') return fail(i - 1, "backreferences are not supported");
        if (c < 0x80 && !((c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))) { byte = c; break; }      // escaped punctuation
        return fail(i - 1, std::string("unsupported escape \\") + (c < 0x80 ? std::string(1, (char)c) : std::string("<non-ASCII>")));
    }
    i++;
    return true;
  }
  // one UTF-8 literal at p[i] as its bytes
  bool literal(std::vector<int>& bytes) {
    const unsigned char c = (unsigned char)p[i];
    int n = c < 0x80 ? 1 : (c >= 0xC2 && c <= 0xDF) ? 2 : (c >= 0xE0 && c <= 0xEF) ? 3 : (c >= 0xF0 && c <= 0xF4) ? 4 : 0;
    if (!n) return fail(i, "malformed UTF-8 in the pattern");
    if (i + (size_t)n > p.size()) return fail(i, "a truncated UTF-8 sequence in the pattern");
    for (int k = 1; k < n; k++) {
      const unsigned char d = (unsigned char)p[i + (size_t)k];
      int lo = 0x80, hi = 0xBF;
      if (k == 1) { if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
      if (d < lo || d > hi) return fail(i, "malformed UTF-8 in the pattern");
    }
    for (int k = 0; k < n; k++) bytes.push_back((unsigned char)p[i + (size_t)k]);
    i += (size_t)n;
    return true;
  }
  bool parseClass(int& out) {      // behind '['
    const size_t open = i - 1;
    bool neg = false;
    if (i < p.size() && p[i] == '^') { neg = true; i++; }
    ByteSet s;
    bool any = false;
    while (true) {
      if (i >= p.size()) return fail(open, "a class without its closing bracket");
      if (p[i] == ']' && any) { i++; break; }
      if (p[i] == ']') return fail(open, "an empty class");
      int lo = -1;
      if ((unsigned char)p[i] >= 0x80) return fail(i, "non-ASCII class members are not supported");
      if (p[i] == '\\') {
        i++;
        ByteSet cls; int b = 0; bool is_class = false;
        if (!escape(cls, b, is_class)) return false;
        if (is_class) { s.merge(cls); any = true; continue; }
        lo = b;
      } else lo = (unsigned char)p[i++];
      int hi = lo;
      if (i + 1 < p.size() && p[i] == '-' && p[i + 1] != ']') {
        i++;
        if ((unsigned char)p[i] >= 0x80) return fail(i, "non-ASCII class members are not supported");
        if (p[i] == '\\') {
          i++;
          ByteSet cls; int b = 0; bool is_class = false;
          if (!escape(cls, b, is_class)) return false;
          if (is_class) return fail(i - 2, "a class escape as the end of a range");
          hi = b;
        } else hi = (unsigned char)p[i++];
        if (hi < lo) return fail(i - 1, "a range with its ends out of order");
      }
      s.addRange(lo, hi);
      any = true;
    }
    out = neg ? codePointsBut(s) : setNode(s);
    return true;
  }
  bool parseAtom(int& out) {
    const size_t at = i;
    const char c = p[i];
    if (c == '(') {
      i++;
      if (i < p.size() && p[i] == '?') {
        if (i + 1 < p.size() && p[i + 1] == ':') i += 2;
        else return fail(at, "lookaround and other (? groups are not supported");
      }
      if (++depth > kMaxDepth) return fail(at, "groups nested deeper than " + std::to_string(kMaxDepth));
      if (!parseAlt(out, /*nested=*/true)) return false;
      depth--;
      if (i >= p.size() || p[i] != ')') return fail(at, "a group without its closing parenthesis");
      i++;
      return true;
    }
    if (c == '[') { i++; return parseClass(out); }
    if (c == '.') { i++; ByteSet nl; nl.add('\n'); out = codePointsBut(nl); return true; }
    if (c == '\\') {
      i++;
      ByteSet cls; int b = 0; bool is_class = false;
      if (!escape(cls, b, is_class)) return false;
      if (!is_class) cls.add(b);
      out = setNode(cls);
      return true;
    }
    if (c == '*' || c == '+' || c == '?' || c == '{') return fail(at, "nothing to repeat");
    if (c == '^' || c == '$') return fail(at, "anchors are implicit: the whole output must match");
    std::vector<int> bytes, kids;
    if (!literal(bytes)) return false;
    for (int b : bytes) { ByteSet s; s.add(b); kids.push_back(setNode(s)); }
    out = seq(Node::Cat, kids);
    return true;
  }
  bool number(int& v) {
    if (i >= p.size() || p[i] < '0' || p[i] > '9') return false;
    long long n = 0;
    while (i < p.size() && p[i] >= '0' && p[i] <= '9') { n = n * 10 + (p[i] - '0'); if (n > 1000000) n = 1000000; i++; }
    v = (int)n;
    return true;
  }
  bool parseRepeat(int& out) {
    if (!parseAtom(out)) return false;
    bool quantified = false;
    while (i < p.size()) {
      const size_t at = i;
      const char c = p[i];
      int lo, hi;
      if (c == '*') { lo = 0; hi = -1; i++; }
      else if (c == '+') { lo = 1; hi = -1; i++; }
      else if (c == '?') { lo = 0; hi = 1; i++; }
      else if (c == '{') {
        i++;
        if (!number(lo)) return fail(at, "a repeat count was expected");
        hi = lo;
        if (i < p.size() && p[i] == ',') { i++; if (!number(hi)) hi = -1; }
        if (i >= p.size() || p[i] != '}') return fail(at, "a repeat without its closing brace");
        i++;
        if (hi >= 0 && hi < lo) return fail(at, "a repeat {m,n} with n < m");
        if (lo > kMaxRepeat || hi > kMaxRepeat) return fail(at, "a repeat count above " + std::to_string(kMaxRepeat));
      } else break;
      if (quantified) return fail(at, c == '?' ? "lazy quantifiers are not supported" : c == '+' ? "possessive quantifiers are not supported" : "a repeat of a repeat: group it");
      quantified = true;
      Node n; n.kind = Node::Repeat; n.kids = {out}; n.lo = lo; n.hi = hi;
      out = add(n);
    }
    return true;
  }
  bool parseAlt(int& out, bool nested) {
    std::vector<int> alts;
    while (true) {
      std::vector<int> cat;
      const size_t at = i;
      while (i < p.size() && p[i] != '|' && p[i] != ')') {
        int r;
        if (!parseRepeat(r)) return false;
        cat.push_back(r);
        if (nodes.size() > kMaxNodes) return fail(i, "the pattern is too large");
      }
      if (cat.empty()) return fail(at, "an empty alternative");
      alts.push_back(seq(Node::Cat, cat));
      if (i < p.size() && p[i] == '|') { i++; continue; }
      break;
    }
    if (!nested && i < p.size()) return fail(i, "a closing parenthesis without its group");
    out = seq(Node::Alt, alts);
    return true;
  }
};

// ---- Thompson NFA over bytes
struct Nfa {
  struct State { ByteSet on; int to = -1; int eps[2] = {-1, -1}; };
  std::vector<State> st;
  size_t cap;
  bool over = false;
  explicit Nfa(size_t c) : cap(c) {}
  int fresh() {
    if (st.size() >= cap) { over = true; return 0; }
    st.emplace_back();
    return (int)st.size() - 1;
  }
  void eps(int a, int b) { if (over) return; State& s = st[(size_t)a]; if (s.eps[0] < 0) s.eps[0] = b; else s.eps[1] = b; }
};

// the fragment of node n between a fresh start and a fresh end (each state has at most one byte edge or two epsilon edges)
void build(const std::vector<Node>& nodes, int n, Nfa& f, int& s, int& e) {
  s = f.fresh(); e = f.fresh();
  if (f.over) return;
  const Node& nd = nodes[(size_t)n];
  switch (nd.kind) {
    case Node::Set: f.st[(size_t)s].on = nd.set; f.st[(size_t)s].to = e; break;
    case Node::Cat: {
      int cur = s;
      for (int k : nd.kids) { int a, b; build(nodes, k, f, a, b); if (f.over) return; f.eps(cur, a); cur = b; }
      f.eps(cur, e);
      break;
    }
    case Node::Alt: {
      // a chain of two-way forks: every state keeps at most two epsilon edges
      int fork = s;
      for (size_t k = 0; k < nd.kids.size(); k++) {
        int a, b; build(nodes, nd.kids[k], f, a, b); if (f.over) return;
        if (k + 1 < nd.kids.size()) { const int nextFork = f.fresh(); if (f.over) return; f.eps(fork, a); f.eps(fork, nextFork); fork = nextFork; }
        else f.eps(fork, a);
        f.eps(b, e);
      }
      break;
    }
    case Node::Repeat: {
      int cur = s;
      for (int k = 0; k < nd.lo; k++) { int a, b; build(nodes, nd.kids[0], f, a, b); if (f.over) return; f.eps(cur, a); cur = b; }
      if (nd.hi < 0) {      // cur -> (x)* -> e
        int a, b; build(nodes, nd.kids[0], f, a, b); if (f.over) return;
        const int loop = f.fresh(); if (f.over) return;
        f.eps(cur, loop); f.eps(loop, a); f.eps(loop, e); f.eps(b, loop);
      } else {
        for (int k = nd.lo; k < nd.hi; k++) {      // each optional copy may be skipped to the end
          int a, b; build(nodes, nd.kids[0], f, a, b); if (f.over) return;
          const int opt = f.fresh(); if (f.over) return;
          f.eps(cur, opt); f.eps(opt, a); f.eps(opt, e); cur = b;
        }
        f.eps(cur, e);
      }
      break;
    }
  }
}

void closure(const Nfa& f, std::vector<int>& set, std::vector<char>& mark) {
  std::vector<int> stack(set);
  for (int s : set) mark[(size_t)s] = 1;
  while (!stack.empty()) {
    const int s = stack.back(); stack.pop_back();
    for (int t : f.st[(size_t)s].eps)
      if (t >= 0 && !mark[(size_t)t]) { mark[(size_t)t] = 1; set.push_back(t); stack.push_back(t); }
  }
  for (int s : set) mark[(size_t)s] = 0;
  std::sort(set.begin(), set.end());
}

}  // namespace

bool compileByteDfa(const std::string& pattern, ByteDfa& out, std::string& err, int maxStates) {
  out = ByteDfa();
  if (maxStates < 1) { err = "maxStates < 1"; return false; }
  Parser ps(pattern);
  int root = -1;
  if (!ps.parseAlt(root, /*nested=*/false)) { err = ps.err; return false; }
  Nfa f((size_t)maxStates * 64 + 4096);
  int s0, e0;
  build(ps.nodes, root, f, s0, e0);
  if (f.over) { err = "regex: the pattern expands to more than " + std::to_string(f.cap) + " NFA states (cap of " + std::to_string(maxStates) + " DFA states)"; return false; }
  // ---- subset construction
  std::map<std::vector<int>, int32_t> ids;
  std::vector<std::vector<int>> sets;
  std::vector<int32_t> next;
  std::vector<char> mark(f.st.size(), 0);
  std::vector<int> start{s0};
  closure(f, start, mark);
  ids[start] = 0; sets.push_back(start);
  for (size_t d = 0; d < sets.size(); d++) {
    next.resize((d + 1) * 256, -1);
    ByteSet any;
    for (int s : sets[d]) if (f.st[(size_t)s].to >= 0) any.merge(f.st[(size_t)s].on);
    for (int b = 0; b < 256; b++) {
      if (!any.has(b)) continue;
      std::vector<int> to;
      for (int s : sets[d]) if (f.st[(size_t)s].to >= 0 && f.st[(size_t)s].on.has(b)) to.push_back(f.st[(size_t)s].to);
      std::sort(to.begin(), to.end());
      to.erase(std::unique(to.begin(), to.end()), to.end());
      closure(f, to, mark);
      auto it = ids.find(to);
      if (it == ids.end()) {
        if ((int)sets.size() >= maxStates) { err = "regex: the pattern needs more than " + std::to_string(maxStates) + " DFA states"; return false; }
        it = ids.emplace(to, (int32_t)sets.size()).first;
        sets.push_back(to);
      }
      next[d * 256 + (size_t)b] = it->second;
    }
  }
  const size_t n = sets.size();
  std::vector<char> accept(n, 0);
  for (size_t d = 0; d < n; d++) accept[d] = std::binary_search(sets[d].begin(), sets[d].end(), e0);
  // ---- states that cannot reach acceptance (none in this subset — every fragment reaches its end — but the rule is the contract's, so it is enforced)
  std::vector<char> live(accept);
  for (bool grew = true; grew;) {
    grew = false;
    for (size_t d = 0; d < n; d++) {
      if (live[d]) continue;
      for (int b = 0; b < 256 && !live[d]; b++) { const int32_t t = next[d * 256 + (size_t)b]; if (t >= 0 && live[(size_t)t]) { live[d] = 1; grew = true; } }
    }
  }
  if (!live[0]) { err = "regex: the pattern matches nothing"; return false; }
  // ---- Moore's refinement over the live states: classes by (accepting, the classes of the 256 successors)
  std::vector<int32_t> cls(n, -1);
  for (size_t d = 0; d < n; d++) if (live[d]) cls[d] = accept[d] ? 1 : 0;
  size_t n_cls = 0;
  while (true) {
    std::map<std::vector<int32_t>, int32_t> sig_ids;
    std::vector<int32_t> ncls(n, -1);
    std::vector<int32_t> sig(257);
    for (size_t d = 0; d < n; d++) {
      if (!live[d]) continue;
      sig[0] = cls[d];
      for (int b = 0; b < 256; b++) { const int32_t t = next[d * 256 + (size_t)b]; sig[(size_t)b + 1] = t >= 0 && live[(size_t)t] ? cls[(size_t)t] : -1; }
      auto it = sig_ids.find(sig);
      if (it == sig_ids.end()) it = sig_ids.emplace(sig, (int32_t)sig_ids.size()).first;
      ncls[d] = it->second;
    }
    const bool done = sig_ids.size() == n_cls;
    n_cls = sig_ids.size();
    cls.swap(ncls);
    if (done) break;
  }
  out.nStates = (int32_t)n_cls;
  out.start = cls[0];
  out.next.assign(n_cls * 256, -1);
  out.accept.assign(n_cls, 0);
  for (size_t d = 0; d < n; d++) {
    if (!live[d]) continue;
    const size_t c = (size_t)cls[d];
    out.accept[c] = accept[d];
    for (int b = 0; b < 256; b++) { const int32_t t = next[d * 256 + (size_t)b]; out.next[c * 256 + (size_t)b] = t >= 0 && live[(size_t)t] ? cls[(size_t)t] : -1; }
  }
  return true;
}

bool compileTokenTable(const ByteDfa& dfa, const std::vector<std::string>& tokens, int32_t vocab, const std::vector<int32_t>& stopIds, TokenAutomaton& out, std::string& err,
                       const ConstraintLimits& lim) {
  out = TokenAutomaton();
  if (vocab < 1) { err = "constraint: vocabulary < 1"; return false; }
  if (dfa.nStates < 1) { err = "constraint: an empty automaton"; return false; }
  if (dfa.nStates > lim.maxStates || dfa.nStates > 65535) { err = "constraint: " + std::to_string(dfa.nStates) + " states exceed the cap of " + std::to_string(std::min(lim.maxStates, 65535)); return false; }
  const size_t bytes = (size_t)dfa.nStates * (size_t)vocab * sizeof(uint16_t);
  if (bytes > lim.maxTableBytes) { err = "constraint: a table of " + std::to_string(bytes) + " bytes (" + std::to_string(dfa.nStates) + " states x " + std::to_string(vocab) + " ids) exceeds the cap of " + std::to_string(lim.maxTableBytes); return false; }
  for (int32_t id : stopIds) if (id < 0 || id >= vocab) { err = "constraint: stop id " + std::to_string(id) + " outside the vocabulary"; return false; }
  out.nStates = dfa.nStates; out.start = dfa.start; out.vocab = vocab;
  out.accept = dfa.accept;
  out.next.assign((size_t)dfa.nStates * (size_t)vocab, (uint16_t)0xFFFF);
  const size_t n_tok = std::min(tokens.size(), (size_t)vocab);
  for (int32_t s = 0; s < dfa.nStates; s++) {
    uint16_t* row = out.next.data() + (size_t)s * (size_t)vocab;
    bool any = false;
    for (size_t t = 0; t < n_tok; t++) {
      const std::string& tk = tokens[t];
      if (tk.empty()) continue;
      int32_t cur = s;
      for (size_t k = 0; k < tk.size() && cur >= 0; k++) cur = dfa.next[(size_t)cur * 256 + (unsigned char)tk[k]];
      if (cur >= 0) { row[t] = (uint16_t)cur; any = true; }
    }
    if (dfa.accept[(size_t)s]) for (int32_t id : stopIds) { row[(size_t)id] = (uint16_t)s; any = true; }
    if (!any) {
      out = TokenAutomaton();
      err = "constraint: state " + std::to_string(s) + " is left with no allowed token (a vocabulary without single-byte tokens, or a match that can only end with no stop id given)";
      return false;
    }
  }
  return true;
}

}  // namespace tgxh
