"""ctypes view of the pattern compiler's test entry points (tinygpt_amd/host/engine_c.cpp: tgxe_regex_dfa_match, tgxe_constraint_compile, tgxe_automaton_validate,
tgxe_set_regex) and the walks the constrained-decoding tests share."""
import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_int, c_int32, c_int64, c_uint8, c_uint16, c_void_p

import numpy as np

from conftest import GOLDEN

NONE = 0xFFFF
GPT2_DIR = os.path.join(GOLDEN, "tokenizer", "gpt2")
GPT2_EOS = 50256
PATTERNS = [r"(yes|no|maybe)", r"\d{4}-\d{2}-\d{2}", r'\{"name": "[a-z]+", "age": \d+\}']


def bind(lib):
    lib.tgxe_regex_dfa_match.argtypes = [c_char_p, c_char_p, c_int64, c_char_p, c_int]
    lib.tgxe_constraint_compile.restype = c_void_p
    lib.tgxe_constraint_compile.argtypes = [c_char_p, c_char_p, POINTER(c_int32), c_int, c_int32, c_int, c_char_p, c_int]
    lib.tgxe_constraint_info.argtypes = [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]
    lib.tgxe_constraint_copy.argtypes = [c_void_p, POINTER(c_uint16), POINTER(c_uint8)]
    lib.tgxe_constraint_destroy.argtypes = [c_void_p]
    lib.tgxe_automaton_validate.argtypes = [c_int32, c_int32, POINTER(c_uint16), c_int32, c_char_p, c_int]
    lib.tgxe_set_regex.argtypes = [c_void_p, c_char_p]
    return lib


def dfa_match(lib, pattern, data: bytes):
    """True / False, or the compiler's message (a str) when the pattern is refused"""
    err = ctypes.create_string_buffer(512)
    r = lib.tgxe_regex_dfa_match(pattern.encode("utf-8") if isinstance(pattern, str) else pattern, data, len(data), err, 512)
    return err.value.decode("utf-8", "replace") if r < 0 else bool(r)


def compile_table(lib, pattern, tokenizer_dir=GPT2_DIR, stops=(GPT2_EOS,), vocab=0, max_states=0):
    """(next uint16 [n_states][vocab], start, accept bool [n_states]), or the compiler's message (a str)"""
    err = ctypes.create_string_buffer(512)
    st = (c_int32 * max(1, len(stops)))(*stops)
    h = lib.tgxe_constraint_compile(tokenizer_dir.encode(), pattern.encode("utf-8") if isinstance(pattern, str) else pattern, st, len(stops), vocab, max_states, err, 512)
    if not h:
        return err.value.decode("utf-8", "replace")
    n, s, v = c_int32(), c_int32(), c_int32()
    lib.tgxe_constraint_info(h, ctypes.byref(n), ctypes.byref(s), ctypes.byref(v))
    table, accept = np.empty((n.value, v.value), np.uint16), np.empty(n.value, np.uint8)
    lib.tgxe_constraint_copy(h, table.ctypes.data_as(POINTER(c_uint16)), accept.ctypes.data_as(POINTER(c_uint8)))
    lib.tgxe_constraint_destroy(h)
    return table, s.value, accept.astype(bool)


def validate(lib, table, start):
    err = ctypes.create_string_buffer(256)
    t = np.ascontiguousarray(table, np.uint16)
    return lib.tgxe_automaton_validate(t.shape[0], start, t.ctypes.data_as(POINTER(c_uint16)), t.shape[1], err, 256) == 0


def walk(table, start, ids):
    """the state after ids, or None where an id is not allowed"""
    s = start
    for t in ids:
        s = int(table[s, int(t)])
        if s == NONE:
            return None
    return s


def fullmatch(pattern, text):
    """Python's verdict under the subset's reading of \\d \\w \\s (ASCII)"""
    return re.fullmatch(pattern, text, re.ASCII) is not None
