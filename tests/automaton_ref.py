"""The restatement of constrained decoding (include/tgx.h tgx_automaton_create: "Formula", "State word"; tinygpt_amd/csrc/kernels/logit_proc.h stage 4): the
float32 processor formula of tests/logit_proc_ref.py, then -inf on every entry the automaton's state does not allow — and a mirror of the state rule.

A table is a uint16 array [n_states][vocab]: next[s][t] = the state after token t in state s, or NONE."""
import numpy as np

from logit_proc_ref import process_np

NONE = 0xFFFF


def mask_np(logits, next_table, state):
    """processed fp32 logits [V] -> the same with -inf where next[state] is NONE"""
    v = np.array(logits, dtype=np.float32, copy=True)
    v[np.asarray(next_table)[int(state)] == NONE] = -np.inf
    return v


def process_auto_np(logits, next_table=None, state=0, words=None, repetition=1.0, presence=0.0, frequency=0.0, bias=None):
    """raw fp32 logits [V] -> what a row with these processors draws from: penalties, bias, then the automaton's mask (next_table None: no automaton)"""
    v = process_np(logits, words, repetition, presence, frequency, bias)
    return v if next_table is None else mask_np(v, next_table, state)


def advance(next_table, state, tok):
    """the state rule of a tgx_decode_rows step: the row consumes its current token; a token the state does not allow leaves it where it is"""
    n = int(np.asarray(next_table)[int(state), int(tok)])
    return int(state) if n == NONE else n


def allowed(next_table, state):
    return np.flatnonzero(np.asarray(next_table)[int(state)] != NONE)


def random_table(rng, n_states, V, max_allowed=None, force=()):
    """every state allows a random non-empty subset with random targets; force: ids every state allows (e.g. a stop id)"""
    t = np.full((n_states, V), NONE, np.uint16)
    for s in range(n_states):
        k = int(rng.integers(1, (max_allowed or V) + 1))
        ids = rng.choice(V, size=k, replace=False)
        t[s, ids] = rng.integers(0, n_states, size=k).astype(np.uint16)
        for i in force:
            t[s, int(i)] = rng.integers(0, n_states)
    return t


def forced_table(V, seq):
    """state i allows exactly seq[i] and moves to i + 1; the last state allows seq[-1] again (it must allow something) and stays"""
    n = len(seq)
    t = np.full((n, V), NONE, np.uint16)
    for i, tok in enumerate(seq):
        t[i, int(tok)] = min(i + 1, n - 1)
    return t
