"""The float32 numpy restatement of the per-row logit processors (include/tgx.h tgx_set_row_penalties: "Formula"; tinygpt_amd/csrc/kernels/logit_proc.h).
Every operation is one IEEE float32 operation (numpy float32 arrays never fuse a multiply into an add), so the device's bits can be demanded, not approximated.

A history is a uint32 vector of vocab words: bit 31 "occurs in the prompt", bits 0 .. 30 the number of times the row produced the id."""
import numpy as np

PROMPT_BIT = np.uint32(0x80000000)
COUNT_MASK = np.uint32(0x7FFFFFFF)


def history(V, prompt_ids=(), produced_ids=()):
    """the words tgx_set_row_history(prompt_ids, produced_ids) leaves"""
    w = np.zeros(V, np.uint32)
    for t in prompt_ids:
        w[int(t)] |= PROMPT_BIT
    for t in produced_ids:
        count(w, t)
    return w


def count(words, tok):
    """the counting step of a tgx_decode_rows step: the row's current token, saturating"""
    t = int(tok)
    if (words[t] & COUNT_MASK) < COUNT_MASK:
        words[t] += np.uint32(1)
    return words


def process_np(logits, words=None, repetition=1.0, presence=0.0, frequency=0.0, bias=None):
    """raw fp32 logits [V] -> processed fp32 logits [V]"""
    v = np.array(logits, dtype=np.float32, copy=True)
    V = v.shape[0]
    w = np.zeros(V, np.uint32) if words is None else np.asarray(words, np.uint32)
    n = (w & COUNT_MASK)
    rep, pres, freq = np.float32(repetition), np.float32(presence), np.float32(frequency)
    with np.errstate(invalid="ignore", over="ignore"):
        seen = w != 0
        div, mul = (v / rep).astype(np.float32), (v * rep).astype(np.float32)
        v = np.where(seen, np.where(v > 0, div, mul), v).astype(np.float32)
        v = (v - (freq * n.astype(np.float32)).astype(np.float32)).astype(np.float32)
        v = (v - np.where(n > 0, pres, np.float32(0))).astype(np.float32)
        for i, b in (bias.items() if isinstance(bias, dict) else (bias or ())):
            v[int(i)] = np.float32(v[int(i)] + np.float32(b))
    return v


def argmax_lowest(v):
    """argmax with ties to the lowest index (Sampler.cpp:28)"""
    return int(np.argmax(v))
