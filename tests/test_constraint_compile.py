"""The host side of constrained decoding without a GPU: the table validation of tgx_automaton_create (tinygpt_amd/csrc/automaton.h) and the pattern compiler
(tinygpt_amd/host/constraint.{h,cpp}), over the GPT-2 tokenizer fixture.
  * tests/constraint_check.cpp, a stand-alone program under the address and undefined-behaviour sanitizers: malformed patterns and tables get clean refusals;
  * differential: the byte DFA's verdict equals Python's re.fullmatch on random strings over a small alphabet, hand-written matches and near-misses — and stray
    bytes are never accepted;
  * soundness: random walks over the token automaton decode to full matches; completeness: encode(s) + EOS is a path for matching strings;
  * the tables pass the device's validation and never allow a special token outside the stop ids in accepting states;
  * the host engine bound to the CPU oracle, which has no automaton calls: a regex fails the generate call with a message, an empty one changes nothing."""
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from constraint_util import GPT2_DIR, GPT2_EOS, NONE, PATTERNS, bind, compile_table, dfa_match, fullmatch, validate, walk
from host_util import HostEngine, HostTokenizer, host_lib, write_model_dir
from tinygpt_amd import build

import os


@pytest.fixture(scope="module")
def lib():
    return bind(host_lib(test_hooks=True))


@pytest.fixture(scope="module")
def tok(lib):
    t = HostTokenizer(lib, GPT2_DIR)
    yield t
    t.close()


def test_constraint_check():
    exe = build.build_constraint_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "constraint_check: ok" in r.stdout


# pattern -> hand-written matches and near-misses (the random strings come on top)
CASES = {
    r"(yes|no|maybe)": ["yes", "no", "maybe", "", "ye", "yesno", "mayb", "maybee", "Yes"],
    r"\d{4}-\d{2}-\d{2}": ["2024-02-29", "0000-00-00", "2024-2-29", "2024-02-290", "202a-02-29", "2024--02-29"],
    r'\{"name": "[a-z]+", "age": \d+\}': ['{"name": "bo", "age": 7}', '{"name": "", "age": 7}', '{"name": "bo", "age": }', '{"name": "Bo", "age": 7}', '{"name": "bo","age": 7}'],
    r"a*": ["", "a", "aaaa", "b", "aab"],
    r"a+b?": ["a", "ab", "aab", "b", "abb", ""],
    r"(ab|a)(c|bc)": ["abc", "ac", "abbc", "ab", "abcc"],
    r"a{2,4}": ["a", "aa", "aaa", "aaaa", "aaaaa"],
    r"(a|b){3}": ["aba", "bbb", "ab", "abab", "abc"],
    r"a{2,}b{0,1}": ["aa", "aaab", "ab", "aabb"],
    r"[a-c0-1_]+": ["a0_c1", "abc", "d", "a-c", ""],
    r"[^a-c]+": ["xyz", "é€", "\n", "xbz", ""],
    r"[^\d\s]x": ["ax", "1x", " x", "éx", "\nx", "x"],
    r".": ["a", "é", "€", "\n", "", "ab", "\U0001F600"],
    r".*b": ["b", "aab", "a\nb", "é€b", "ba"],
    r"\w+\s\w+": ["ab cd", "a\tb", "a  b", "ab", "é b", "a_1 b_2"],
    r"caf(é|e)s?": ["café", "cafes", "cafés", "caf", "cafée"],
    r"€{2}\n\t\\": ["€€\n\t\\", "€\n\t\\", "€€\n\t"],
    r"\(\[\.\*\+\?\|\]\)\{\}": ["([.*+?|]){}", "([.*+?|])", "(([.*+?|]){}"],
    r"(?:ab)+|c{0,2}": ["ab", "abab", "", "c", "cc", "ccc", "abc"],
    r"((a|b)*c|d)+": ["c", "d", "abcd", "ababc", "ab", "dcabc", ""],
    r"[-a]+[b-]+": ["-a-b", "ab", "a", "-b-", "ba"],
}
ALPHABET = ["a", "b", "c", "d", "x", "y", "0", "1", "2", "-", "_", " ", "\n", "\t", "é", "€", "s", "e", "f"]


def test_byte_dfa_equals_python_fullmatch(lib):
    rng = np.random.default_rng(7)
    random_strings = ["".join(rng.choice(ALPHABET, size=int(rng.integers(0, 7)))) for _ in range(150)]
    stray = [b"\xc3", b"a\x80", b"\xe2\x82", b"\xc0\xaf", b"\xed\xa0\x80b", b"ab\xff", b"\xf4\x90\x80\x80"]
    assert len(CASES) >= 20
    for pat, hand in CASES.items():
        verdicts = set()
        for s in hand + random_strings:
            got = dfa_match(lib, pat, s.encode("utf-8"))
            assert got is fullmatch(pat, s), (pat, s, got)
            verdicts.add(got)
        assert verdicts == {True, False}, pat
        for b in stray:
            assert dfa_match(lib, pat, b) is False, (pat, b)
    for pat in ("(a", "a{5,2}", "a|", "(a)\\1", "a*?", "(?=a)", "[é]", "caf\xc3".encode("latin-1")):
        msg = dfa_match(lib, pat, b"a")
        assert isinstance(msg, str) and "position" in msg, (pat, msg)


def test_random_walks_decode_to_matches(lib, tok):
    """soundness.  A walk ends when it draws the stop id, which the table allows in accepting states alone; decode(ids) must then match.  Each step is, with equal
    probability, a uniform choice among the allowed tokens or a uniform choice among the allowed TRANSITIONS (target states, the stop id counted as one) followed by
    a uniform token with that target: over 50k tokens a uniform token alone leaves a state like [a-z]+ once in thousands of steps (three tokens begin with the
    closing quote), and a walk that never ends checks nothing"""
    rng = np.random.default_rng(11)
    for pat in PATTERNS + [r"[^a-c]{1,3}é?", r"(ab|a)(c|bc)\s\w+", r".{2,5}"]:
        table, start, accept = compile_table(lib, pat)
        ended = 0
        for _ in range(40):
            s, ids = start, []
            for _ in range(64):
                ok = np.flatnonzero(table[s] != NONE)
                assert len(ok) > 0 and (table[s, GPT2_EOS] != NONE) == accept[s]
                if rng.random() < 0.5:
                    t = int(rng.choice(ok))
                else:
                    key = np.where(ok == GPT2_EOS, -1, table[s, ok].astype(np.int64))
                    t = int(rng.choice(ok[key == rng.choice(np.unique(key))]))
                if t == GPT2_EOS:
                    ended += 1
                    text = tok._decode(ids, 0).decode("utf-8")        # strict: a match is well-formed UTF-8
                    assert fullmatch(pat, text), (pat, ids, text)
                    break
                ids.append(t)
                s = int(table[s, t])
        assert ended >= 20, (pat, ended)


def test_encodings_of_matches_are_paths(lib, tok):
    """completeness: the ids the tokenizer gives a matching string, followed by EOS, are a path; a near-miss's are not"""
    for pat in PATTERNS + [r"caf(é|e)s?", r"\w+\s\w+", r".*b", r"[^\d\s]x"]:
        table, start, accept = compile_table(lib, pat)
        n = 0
        for s in CASES[pat]:
            ids = tok.encode(s, allow_added=False) + [GPT2_EOS]
            end = walk(table, start, ids)
            assert (end is not None) == fullmatch(pat, s), (pat, s, ids)
            n += end is not None
        assert n >= 1, pat


def test_tables_pass_validation_and_never_allow_specials(lib):
    for pat in PATTERNS:
        table, start, accept = compile_table(lib, pat)
        assert table.shape[1] == 50257 and validate(lib, table, start)
        assert ((table[:, GPT2_EOS] != NONE) == accept).all() and accept.any() and not accept.all()
        wide, wstart, _ = compile_table(lib, pat, vocab=50304)                 # a model's padded vocabulary: the ids past the tokenizer's are never allowed
        assert wide.shape == (table.shape[0], 50304) and (wide[:, 50257:] == NONE).all() and (wide[:, :50257] == table).all() and wstart == start
    # a tokenizer with several special tokens, none of them a stop id: their columns are empty
    import json
    ldir = os.path.join(GOLDEN, "tokenizer", "llama3_style")
    added = [a["id"] for a in json.load(open(os.path.join(ldir, "tokenizer.json")))["added_tokens"]]
    table, start, accept = compile_table(lib, r"(yes|no)*", tokenizer_dir=ldir, stops=())
    assert len(added) >= 2 and (table[:, added] == NONE).all() and validate(lib, table, start)
    # refusals, each with a message: a match that can only end with no stop id given, the state cap, a Metaspace tokenizer, a stop id outside the vocabulary
    assert "no allowed token" in compile_table(lib, r"(yes|no)", stops=())
    assert "states" in compile_table(lib, r"(a|b)*a(a|b){8}", max_states=64)
    assert "ByteLevel" in compile_table(lib, r"a+", tokenizer_dir=os.path.join(GOLDEN, "tokenizer", "Mistral-7B-v0.3"), stops=(2,))
    assert "stop id" in compile_table(lib, r"a+", stops=(50257,))
    assert "position" in compile_table(lib, r"a{5,2}")
    bad = compile_table(lib, PATTERNS[0])[0].copy()
    bad[2, :] = NONE
    assert not validate(lib, bad, 0) and not validate(lib, bad[:2] + 0, 2)


def test_engine_on_a_backend_without_the_calls(lib, oracle_lib, tmp_path):
    """the CPU oracle exports no automaton calls: a regex FAILS the generate call with a message (never plain generation), and an empty one leaves it as it was"""
    cfg, g = load_golden("llama_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    e = HostEngine(lib, model_dir=str(tmp_path), backend_lib=oracle_lib.path, prefix="tgxo_", dtype=0, max_batch=2)
    assert e.prepare(), e.error()
    e.reconfigure(max_new=6)
    plain, new, fin = e.generate_sync([g["prompt"][0]])
    lib.tgxe_set_regex(e.h, b"(yes|no)")
    e.reconfigure(max_new=6)
    for call in (lambda: e.generate_sync([g["prompt"][0]]), lambda: e.generate_async(g["prompt"][0])):
        with pytest.raises(AssertionError, match="regex: the device shim lacks tgx_automaton_create"):
            call()
    lib.tgxe_set_regex(e.h, b"")
    e.reconfigure(max_new=6)
    again, new2, fin2 = e.generate_sync([g["prompt"][0]])
    np.testing.assert_array_equal(again, plain)
    assert (new2, fin2) == (new, fin)
    e.close()
