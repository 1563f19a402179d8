"""Helpers of the tgx_verify_row_sampled tests (include/tgx.h): the 2-layer cuts, and the draw of a sampled token restated in Python.

The draw is a pure function of (logits, sampler settings, key): kernels/common.h draw_key and oracle/tgx_oracle.c tgxo_sample — splitmix64 of
seed * 0x9E3779B97F4A7C15 + index * 0xD1342543DE82EF95 + row, the top 53 bits as a uniform variate, and an inverse CDF over the kept entries in index order with
the probabilities accumulated in double.  tests/test_verify_sampled_api.py holds the restatement against OracleModel.sample on the CPU before a GPU test uses it."""
import copy

import numpy as np

from tinygpt_amd import known_desc
from tinygpt_amd.ffi import Model, SamplerCfg

M64 = (1 << 64) - 1
CTX = 1024
V = 4096


def cut(name, dtype, max_batch=1, max_ctx=CTX, vocab=V):
    """tests/test_hip_verify_row.py::cut — 2 layers, a small vocabulary, an untied head where the family allows one (a peaked checkpoint needs it)"""
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 2, vocab, max_ctx, max_batch
    if d.n_positions > 0:
        d.n_positions = max(d.n_positions, max_ctx)
    peaked = name != "gpt2"
    if peaked:
        d.tied = False
    return d, peaked


def gpu_model(name, dtype, max_batch=1, budget=0, max_ctx=CTX, vocab=V):
    d, peaked = cut(name, dtype, max_batch, max_ctx, vocab)
    m = Model(d)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(1234, 0.02, peaked=peaked).finalize()


def splitmix64(s):
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_uniform(seed, index, row):
    """the uniform variate of the draw with key (seed, index of the produced token, row)"""
    s = (seed * 0x9E3779B97F4A7C15 + index * 0xD1342543DE82EF95 + row) & M64
    return float(splitmix64(s) >> 11) * (1.0 / 9007199254740992.0)


def draw_from_probs(probs, u):
    """tgx_oracle.c:775-777: walk the kept entries in index order, the first whose inclusive cumulative probability (double) exceeds u; none: the last kept entry"""
    kept = np.flatnonzero(probs > 0)
    if kept.size == 0:
        return -1
    cum = np.cumsum(probs[kept].astype(np.float64))      # sequential double adds, as the C loop
    i = int(np.searchsorted(cum, u, side="right"))       # first i with u < cum[i]
    return int(kept[min(i, kept.size - 1)])


def expected_draw(cfg: SamplerCfg, logits, seed, index, row):
    """(the id the settings draw from `logits` with the key, the final probabilities)"""
    from oracle.oracle_ffi import filter_logits
    _, p = filter_logits(cfg, logits)
    return draw_from_probs(p, draw_uniform(seed, index, row)), p


def top_p_band(cfg: SamplerCfg, logits):
    """tests/test_hip_sampler.py:129-131: the oracle accumulates the top-p cut's cumulative mass in float like torch.cumsum, the GPU in exact 2^-40 fixed point, so
    the two may disagree on the entries whose inclusive cumulative mass lies inside the oracle's accumulation error around top_p — and on nothing else.  That file
    bounds the error by ~V 2^-24 of the total; here it is MEASURED on the position's own probabilities: the largest distance between the float running sum the
    oracle forms (sequential float adds) and the same sum in double, plus 2^-22 for the GPU's side (its probabilities are floats e * inv, each within 2^-24
    relative of the fixed-point masses the cut was found on: at most 2^-24 of the cumulative mass; the fixed point itself resolves V 2^-40).  Returns the indices
    of the entries inside that band (empty without top-p)"""
    if not cfg.top_p < 1:
        return np.zeros(0, np.int64)
    from oracle.oracle_ffi import filter_logits
    only_k = SamplerCfg(cfg.temperature, cfg.top_k, 1.0, 0.0)
    _, p = filter_logits(only_k, logits)                  # the distribution top-p looks at
    order = np.lexsort((np.arange(p.size), -p))           # value descending, index ascending
    c64 = np.cumsum(p[order].astype(np.float64))
    c32 = np.cumsum(p[order], dtype=np.float32)           # np.cumsum adds one by one in the accumulator's type: the oracle's `cum += tmp[i]`
    eps = float(np.abs(c32.astype(np.float64) - c64).max()) + 2.0 ** -22
    assert eps <= 4 * p.size * 2.0 ** -24                 # inside that file's bound
    return order[np.abs(c64 - cfg.top_p) <= eps]


def walk(draws, draft):
    """the accept rule without stop conditions: draft[0 .. a - 1] followed by s[a]"""
    out = []
    for i, s in enumerate(draws):
        out.append(int(s))
        if i == len(draft) or int(draft[i]) != int(s):
            break
    return out
