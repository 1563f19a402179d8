"""Speculative decoding on rows with a logit processor on (include/tgx.h option verify.processors; kernels/logit_proc.h logit_proc_pos_kernel and
automaton_walk_kernel, kernels/verify.h: the processed choice and the commit).

Every expected token is restated from the PASS'S OWN logits (tgx_read_pass_logits): position i of a pass over the inputs in[0] = t0, in[1 ..] = draft is
processed by tests/logit_proc_ref.py with the row's history counted by in[0 .. i] and the automaton state moved by in[0 .. i] (both mirrored here in numpy), then
chosen by the lowest-index argmax or by tests/verify_sampled_util.py's draw with the key (seed, past + i + 1, row).  The comparison is exact: no tolerance,
nothing skipped.  A draft that the model should accept comes from a twin context that steps through tgx_decode_rows with the same processors on; whether the pass
agrees with the steps is not assumed anywhere (the two differ by summation order), only restated.

The tiny models: 2 layers, hidden 64; V = 256 (one tile, 16-byte paths) and V = 1030 (two tiles, V % 4 != 0: the entry-by-entry paths and a tile boundary)."""
import ctypes
import subprocess
from ctypes import POINTER, c_int, c_int64, c_void_p

import numpy as np
import pytest

from automaton_ref import NONE, advance, process_auto_np, random_table
from conftest import load_golden
from logit_proc_ref import argmax_lowest, count, history
from tinygpt_amd import build
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import ADV_FEED, ADV_STEP, GREEDY, Model, SamplerCfg, TgxError
from verify_sampled_util import expected_draw, top_p_band

pytestmark = pytest.mark.gpu

ST_INVALID, ST_UNSUPPORTED = 1, 2
NINF = float("-inf")
SAMPLED = SamplerCfg(0.8, 0, 0.9, 0.0)
S = 9                                     # prompt length
OPT = "verify.processors"


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def make(hip, V, B=1, dtype="bf16", paged=False, option=True):
    cfg, g = load_golden("llama_tiny")
    cfg = dict(cfg, vocab_size=V, hidden_size=64, intermediate_size=64, num_attention_heads=1, num_key_value_heads=1, num_hidden_layers=2)
    d = desc_from_hf_config(cfg, dtype, max_batch=B)
    d.max_ctx = 256
    m = Model(d, hip)
    if paged:
        m.set_option("kv.budget_tokens", 256 * B)
    m.load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    if option:
        m.set_option(OPT, 1)
    return m


def prompts(B, V, seed=0):
    return np.random.default_rng(seed).integers(0, V, size=(B, S)).astype(np.int64)


def raises(status, call):
    with pytest.raises(TgxError) as e:
        call()
    assert e.value.status == status, (e.value.status, str(e.value))


class Spec:
    """one row's processors and sampler"""

    def __init__(self, repetition=1.0, presence=0.0, frequency=0.0, bias=None, table=None, start=0, cfg=GREEDY, seed=0):
        self.pen, self.bias, self.table, self.start, self.cfg, self.seed = (repetition, presence, frequency), bias, table, start, cfg, seed

    @property
    def on(self):
        return self.pen != (1.0, 0.0, 0.0) or bool(self.bias) or self.table is not None


class Mirror:
    """the test's own copy of a row's history words and automaton state"""

    def __init__(self, V, prompt, spec, row):
        self.spec, self.row, self.words, self.state = spec, row, history(V, prompt_ids=prompt), spec.start

    def processed(self, raw, words, state):
        if not self.spec.on:
            return raw
        return process_auto_np(raw, self.spec.table, state, words, *self.spec.pen, self.spec.bias)

    def choose(self, v, index):
        """what the row's settings choose from the processed vector v for the token with index `index`"""
        if self.spec.cfg.greedy:
            return argmax_lowest(v)
        t, _ = expected_draw(self.spec.cfg, v, self.spec.seed, index, self.row)
        assert t not in top_p_band(self.spec.cfg, v)      # (a property of the test's inputs: no compared draw sits where the top-p cut is a rounding question)
        return t

    def positions(self, L, inputs, past):
        """g[i] and (w_i, s_i) of every position of a pass over `inputs` with the raw logits L [M][V]"""
        w, s, g, per = self.words.copy(), self.state, [], []
        for i, t in enumerate(inputs):
            count(w, t)
            if self.spec.table is not None:
                s = advance(self.spec.table, s, t)
            g.append(self.choose(self.processed(L[i], w, s), past + i + 1))
            per.append((w.copy(), s))
        return g, per

    def commit(self, per, n):
        self.words, self.state = per[n - 1][0].copy(), per[n - 1][1]

    def step(self, cur):
        """one tgx_decode_rows step consumes `cur`"""
        count(self.words, cur)
        if self.spec.table is not None:
            self.state = advance(self.spec.table, self.state, cur)


def walk(g, draft, stops=()):
    out = []
    for i, t in enumerate(g):
        out.append(int(t))
        if int(t) in stops or i == len(draft) or int(draft[i]) != int(t):
            break
    return out


def start_rows(m, P, specs):
    """prefill, every row's processors with its history seeded from its prompt, its first token through tgx_sample_row, its sampler -> (t0 per row, mirrors, aids)"""
    V = m.desc.vocab
    m.forward(P)
    raw = m.logits(rounded=False)
    t0, mirrors, aids = [], [], []
    for b, sp in enumerate(specs):
        aid = -1
        if sp.on:
            m.set_row_penalties(b, *sp.pen).set_row_logit_bias(b, sp.bias).set_row_history(b, prompt_ids=P[b])
            if sp.table is not None:
                aid = m.automaton_create(sp.table, start=sp.start)
                m.set_row_automaton(b, aid, sp.start)
        mir = Mirror(V, P[b], sp, b)
        t = int(m.sample_row(b, sp.cfg, sp.seed))
        assert t == mir.choose(mir.processed(raw[b], mir.words, mir.state), S), b      # the first token: processed, nothing counted
        m.set_row_sampler(b, sp.cfg, sp.seed)
        t0.append(t); mirrors.append(mir); aids.append(aid)
    return t0, mirrors, aids


def lookahead(hip, V, P, specs, k, **kw):
    """what k steps of tgx_decode_rows produce per row, from a twin context"""
    A = make(hip, V, B=len(specs), **kw)
    start_rows(A, P, specs)
    ids = A.decode_rows(k)[0]
    A.close()
    return [[int(t) for t in ids[:, b]] for b in range(len(specs))]


def wrong_at(ids, j, V, avoid=()):
    d = list(ids)
    if j is not None:
        d[j] = next(t for t in range(V) if t != d[j] and t not in avoid)
    return d


def check_pass(m, mir, row, t0, draft, got, past, L=None, stops=()):
    """the call's ids against the restatement of the pass's logits; the mirror then stands as the row must -> (n, the row's pass logits)"""
    ids, fin = got
    if L is None:
        L = m.pass_logits()
    assert L.shape[0] == len(draft) + 1
    inputs = [t0] + [int(t) for t in draft]
    g, per = mir.positions(L, inputs, past)
    want = walk(g, draft, stops)
    assert [int(t) for t in ids] == want, (row, list(ids), want, g)
    n = len(want)
    print(f"row {row}: draft {len(draft)} produced {n} fin {fin} g {g}")
    assert m.past_length_row(row) == past + n
    mir.commit(per, n)
    return n, L, want


def check_row_afterwards(m, mir, row, L, n, last, aid, steps=3):
    """case 5: the logits slot is the RAW vector of the producing position; tgx_sample_row repeats the last id; the automaton state is s_{n-1}; then `steps`
    tgx_decode_rows steps follow the restatement that counted exactly in[0 .. n-1] (greedy rows: the only view of the history words)"""
    sp = mir.spec
    np.testing.assert_array_equal(m.logits(rounded=False)[row], L[n - 1])
    assert int(m.sample_row(row, sp.cfg, sp.seed)) == last
    if sp.table is not None:
        assert m.read_row_automaton(row) == (aid, mir.state)
    cur = last
    for _ in range(steps if sp.cfg.greedy else 0):
        mir.step(cur)
        ids, _, _ = m.decode_rows(1)
        cur = int(ids[0, row])
        assert cur == argmax_lowest(mir.processed(m.logits(rounded=False)[row], mir.words, mir.state))
        if sp.table is not None:
            assert m.read_row_automaton(row) == (aid, mir.state)


# ---- 1. the option gates the feature -------------------------------------------------------------------------------------------------------------------------
def test_option_gates_the_feature(hip):
    V = 256
    m = make(hip, V, option=False)
    assert m.get_option(OPT) == 0
    P = prompts(1, V, 1)
    sp = Spec(bias={3: 2.5, 77: -1.0})
    t0, mirrors, _ = start_rows(m, P, [sp])
    draft = [5, 6, 7, 8]
    raises(ST_UNSUPPORTED, lambda: m.verify_row(0, draft))
    assert m.past_length_row(0) == S
    m.set_option(OPT, 1)
    assert m.get_option(OPT) == 1
    raises(ST_INVALID, lambda: m.set_option(OPT, 2))
    got = m.verify_row(0, draft)
    check_pass(m, mirrors[0], 0, t0[0], draft, got, S)
    m.set_option(OPT, 0)
    raises(ST_UNSUPPORTED, lambda: m.verify_row(0, draft))
    m.close()


# ---- 2. greedy, penalties: counts that differ by position -----------------------------------------------------------------------------------------------------
def penalty_spec(V, P):
    """three loudly biased ids whose order the counts keep changing: the row's choices repeat ids, and a count that is off by one picks another id.  b sits in
    the prompt (its word carries the prompt bit: the repetition penalty applies before it is ever produced)"""
    a, b, c = V - 3, int(P[0][2]), V // 2 + 1
    assert len({a, b, c}) == 3
    return Spec(repetition=1.1, presence=0.15, frequency=0.6, bias={a: 40.0, b: 39.9, c: 39.6, 5: -1.0}), (a, b, c)


@pytest.mark.parametrize("V,dtype,paged", [(256, "bf16", 0), (256, "bf16", 1), (1030, "bf16", 0), (1030, "bf16", 1), (1030, "fp32", 0)])
def test_greedy_penalties(hip, V, dtype, paged):
    P = prompts(1, V, 2)
    sp, loud = penalty_spec(V, P)
    look = lookahead(hip, V, P, [sp], 12, dtype=dtype, paged=paged)[0]
    for j in (None, 0, 6, 11):      # a draft token wrong at the first, a middle and the last index, or nowhere
        m = make(hip, V, dtype=dtype, paged=paged)
        t0, mirrors, _ = start_rows(m, P, [sp])
        draft = wrong_at(look, j, V, avoid=loud)
        assert t0[0] in loud and t0[0] in look and max(look.count(t) for t in loud) >= 2      # the draft holds t0 again and an id twice
        got = m.verify_row(0, draft)
        n, L, want = check_pass(m, mirrors[0], 0, t0[0], draft, got, S)
        assert n <= (j if j is not None else 12) + 1 and got[1] == 0
        check_row_afterwards(m, mirrors[0], 0, L, n, want[-1], -1)
        m.close()


# ---- 3. a bias of -inf on the token the raw argmax would pick -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [256, 1030])
def test_banned_raw_argmax(hip, V):
    """The raw choices come from a pass of the unprocessed row itself (g1: what it produced, the draft's accepted prefix and its own token behind it), so that
    "the raw argmax of position k" is a statement about the very logits the processed call sees: the same inputs in a pass of the same length."""
    P = prompts(1, V, 3)
    raw_look = lookahead(hip, V, P, [Spec()], 14)[0]
    m0 = make(hip, V)
    t0 = start_rows(m0, P, [Spec()])[0][0]
    g1 = [int(t) for t in m0.verify_row(0, raw_look)[0]]
    m0.close()
    k = next(i for i in range(len(g1)) if g1[i] not in [t0] + g1[:i])      # banning g1[k] leaves t0 and g1[0 .. k-1] as they are
    banned = g1[k]
    sp = Spec(bias={banned: NINF})
    outs = []
    for follow_processed in (False, True):
        m = make(hip, V)
        t, mirrors, _ = start_rows(m, P, [sp])
        assert t[0] == t0
        draft = g1[:k] + [outs[0][k] if follow_processed else banned] + raw_look[k + 1:]      # (the pass keeps its length)
        got = m.verify_row(0, draft)
        L = m.pass_logits()
        assert argmax_lowest(L[k]) == banned                               # the raw choice of position k is the banned id ...
        n, L, want = check_pass(m, mirrors[0], 0, t0, draft, got, S, L=L)
        assert want[k] != banned                                           # ... and the processed one is not
        outs.append(want)
        assert (n >= k + 2) if follow_processed else (n == k + 1), (n, k)  # the raw draft is rejected at k; the processed one is accepted there
        check_row_afterwards(m, mirrors[0], 0, L, n, want[-1], -1, steps=1)
        m.close()


# ---- 4. automaton ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,paged", [(256, 0), (1030, 1)])
def test_automaton(hip, V, paged):
    P = prompts(1, V, 4)
    table = random_table(np.random.default_rng(40 + V), 7, V, max_allowed=12)
    sp = Spec(table=table, start=2)
    look = lookahead(hip, V, P, [sp], 8, paged=paged)[0]
    for j in (None, 3):
        m = make(hip, V, paged=paged)
        t0, mirrors, aids = start_rows(m, P, [sp])
        draft = list(look)
        if j is not None:      # a token that s_j does not allow: acceptance ends there
            s = sp.start
            for t in [t0[0]] + draft[:j]:
                s = advance(table, s, t)
            draft[j] = int(np.flatnonzero(table[s] == NONE)[0])
        got = m.verify_row(0, draft)
        n, L, want = check_pass(m, mirrors[0], 0, t0[0], draft, got, S)
        s = sp.start
        for t in [t0[0]] + want:                                             # every produced id is one its state allows
            assert table[s, t] != NONE
            s = int(table[s, t])
        assert n <= (j if j is not None else 8) + 1
        check_row_afterwards(m, mirrors[0], 0, L, n, want[-1], aids[0])
        m.close()


# ---- 6. a sampled row with penalties and an automaton ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,paged", [(256, 1), (1030, 0)])
def test_sampled_penalties_automaton(hip, V, paged, oracle_lib):
    P = prompts(1, V, 6)
    table = random_table(np.random.default_rng(60 + V), 5, V, max_allowed=40)
    sp = Spec(repetition=1.2, presence=0.2, frequency=0.1, bias={7: 1.0}, table=table, start=1, cfg=SAMPLED, seed=33)
    look = lookahead(hip, V, P, [sp], 12, paged=paged)[0]
    m = make(hip, V, paged=paged)
    t0, mirrors, aids = start_rows(m, P, [sp])
    mir, cur, past, at, produced, off_argmax = mirrors[0], t0[0], S, 0, [], 0
    for n_draft, j in ((4, None), (3, 1), (5, None)):
        draft = wrong_at(look[at:at + n_draft], j, V) if look[at:at + n_draft] else [0]
        got = m.verify_row_sampled(0, draft)
        L = m.pass_logits()
        n, L, want = check_pass(m, mir, 0, cur, draft, got, past, L=L)
        off_argmax += sum(int(want[i] != argmax_lowest(L[i])) for i in range(n))
        np.testing.assert_array_equal(m.logits(rounded=False)[0], L[n - 1])
        assert int(m.sample_row(0, sp.cfg, sp.seed)) == want[-1]
        assert m.read_row_automaton(0) == (aids[0], mir.state)
        produced += want
        at = at + n if produced == look[:len(produced)] else len(look)     # (the steps' lookahead serves only while the pass agrees with it)
        cur, past = want[-1], past + n
    s = sp.start
    for t in [t0[0]] + produced:                                           # no produced id is ever one the automaton forbids
        assert table[s, t] != NONE
        s = int(table[s, t])
    assert off_argmax >= 1                                                  # (an argmax in place of the draw would not pass)
    m.close()


# ---- 7. a stop id inside the accepted prefix ------------------------------------------------------------------------------------------------------------------
def test_stop_inside_the_prefix(hip):
    V = 256
    P = prompts(1, V, 2)
    sp, loud = penalty_spec(V, P)
    table = random_table(np.random.default_rng(7), 6, V, force=loud)
    sp.table, sp.start = table, 0
    look = lookahead(hip, V, P, [sp], 8)[0]
    at = next(i for i in range(1, 8) if look[i] not in look[:i])         # the stop id first occurs inside the draft, behind its first token
    stop = look[at]
    m = make(hip, V)
    t0, mirrors, aids = start_rows(m, P, [sp])
    m.set_row_stop(0, 0, [stop])
    got = m.verify_row(0, look)
    n, L, want = check_pass(m, mirrors[0], 0, t0[0], look, got, S, stops=[stop])
    assert want[-1] == stop and got[1] == 1 and 2 <= n <= at + 1 < len(look)
    assert m.read_row_automaton(0) == (aids[0], mirrors[0].state)          # s_{n-1}: the stop id was produced, never consumed
    np.testing.assert_array_equal(m.logits(rounded=False)[0], L[n - 1])
    m.close()


# ---- 8. tgx_verify_rows over four rows ------------------------------------------------------------------------------------------------------------------------
def kv_all(m, row):
    return [m.read_kv(row, layer) for layer in range(m.desc.layers)]


def four_specs(V, P):
    pen, _ = penalty_spec(V, P)
    table = random_table(np.random.default_rng(80 + V), 5, V, max_allowed=40)
    return [pen, Spec(presence=0.3, table=table, start=1, cfg=SAMPLED, seed=44), Spec(), Spec(bias={9: 3.0, 11: NINF})]


@pytest.mark.parametrize("V,dtype,paged", [(256, "bf16", 0), (1030, "bf16", 1), (256, "fp32", 0)])
def test_verify_rows_four_rows(hip, V, dtype, paged, oracle_lib):
    P = prompts(4, V, 8)
    specs = four_specs(V, P)
    look = lookahead(hip, V, P, specs, 6, dtype=dtype, paged=paged)
    drafts = [wrong_at(look[0][:6], 4, V), look[1][:3], look[2][:5], []]
    m = make(hip, V, B=4, dtype=dtype, paged=paged)
    t0, mirrors, aids = start_rows(m, P, specs)
    got = m.verify_rows([0, 1, 2, 3], drafts)
    L = m.pass_logits()
    assert L.shape[0] == sum(len(d) + 1 for d in drafts)
    form = m.get_option("verify.last_form")
    assert form == (2 if dtype == "fp32" else 1)
    first, res = 0, []
    for b in range(4):
        Lb = L[first:first + len(drafts[b]) + 1]
        n, _, want = check_pass(m, mirrors[b], b, t0[b], drafts[b], got[b], S, L=Lb)
        res.append((n, Lb, want))
        first += len(drafts[b]) + 1
    slots = m.logits(rounded=False)
    for b in range(4):
        np.testing.assert_array_equal(slots[b], res[b][1][res[b][0] - 1])
    # the unprocessed row against the same call on a context that never heard of processors: the same bits
    twin = make(hip, V, B=4, dtype=dtype, paged=paged, option=False)
    tt, _, _ = start_rows(twin, P, [Spec(), Spec(cfg=SAMPLED, seed=44), Spec(), Spec()])
    assert tt[2] == t0[2]
    tgot = twin.verify_rows([0, 1, 2, 3], drafts)
    assert list(tgot[2][0]) == list(got[2][0]) and tgot[2][1] == got[2][1]
    np.testing.assert_array_equal(twin.logits(rounded=False)[2], slots[2])
    for (k1, v1), (k2, v2) in zip(kv_all(m, 2), kv_all(twin, 2)):
        np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    twin.close()
    # each processed row afterwards (the sampled one: its state and its repeated draw)
    for b in (3, 1, 0):      # (row 0 last: its follow-up step moves every row of the batch)
        check_row_afterwards(m, mirrors[b], b, res[b][1], res[b][0], res[b][2][-1], aids[b], steps=1 if b == 0 else 0)
    m.close()


# ---- 9. tgx_advance_rows: a processed STEP row and a FEED row -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [256, 1030])
def test_advance_rows_step_and_feed(hip, V):
    P = prompts(2, V, 9)
    pen, _ = penalty_spec(V, P)
    table = random_table(np.random.default_rng(90 + V), 6, V, max_allowed=30)
    pen.table, pen.start = table, 3
    look = lookahead(hip, V, P, [pen, Spec()], 5)
    feed = [int(t) for t in np.random.default_rng(91).integers(0, V, size=6)]
    outs = []
    for processors in (True, False):
        m = make(hip, V, B=2, option=processors)
        t0, mirrors, aids = start_rows(m, P, [pen if processors else Spec(), Spec()])
        got = m.advance_rows([0, 1], [ADV_STEP, ADV_FEED], [look[0][:5], feed])
        assert m.advance_last_form == 1
        if processors:
            L = m.pass_logits()
            n, L, want = check_pass(m, mirrors[0], 0, t0[0], look[0][:5], got[0], S, L=L)
            assert m.past_length_row(1) == S + len(feed)
            outs.append(m.logits(rounded=False)[1].copy())
            check_row_afterwards(m, mirrors[0], 0, L, n, want[-1], aids[0], steps=0)
        else:
            outs.append(m.logits(rounded=False)[1].copy())
        m.close()
    np.testing.assert_array_equal(outs[0], outs[1])                          # the FEED row's logits do not depend on the STEP row's processors


# ---- 10. refusals repeat and change nothing -------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(hip):
    V = 256
    P = prompts(1, V, 10)
    table = random_table(np.random.default_rng(10), 5, V, max_allowed=30)
    sp = Spec(bias={3: 2.5}, table=table, start=1)
    m = make(hip, V, paged=True, option=False)
    t0, mirrors, aids = start_rows(m, P, [sp])

    def state():
        return (m.past_length_row(0), m.read_row_automaton(0), m.get_option("kv.free_tokens"), m.get_option("mem.live_allocs"))
    before = state()
    for _ in range(2):
        raises(ST_UNSUPPORTED, lambda: m.verify_row(0, [1, 2, 3]))
        raises(ST_UNSUPPORTED, lambda: m.verify_row_sampled(0, [1, 2, 3]))
        raises(ST_UNSUPPORTED, lambda: m.verify_rows([0], [[1, 2]]))
        raises(ST_UNSUPPORTED, lambda: m.advance_rows([0], [ADV_STEP], [[1, 2]]))
        raises(ST_UNSUPPORTED, lambda: m.verify_tree(0, [1, 2, 3], [-1, -1, 0]))
        assert state() == before
    m.set_option(OPT, 1)
    for _ in range(2):      # a tree that is no chain stays refused, and the refusal leaves everything where it was
        raises(ST_UNSUPPORTED, lambda: m.verify_tree(0, [1, 2, 3], [-1, -1, 0]))
        assert state() == before
    got = m.verify_tree(0, [4, 5, 6], [-1, 0, 1])                           # a chain-shaped tree is the chain call
    check_pass(m, mirrors[0], 0, t0[0], [4, 5, 6], got, S)
    m.close()


def test_option_alone_allocates_nothing(hip):
    V = 256
    P = prompts(1, V, 11)
    live = []
    for option in (False, True):
        m = make(hip, V, option=option)
        start_rows(m, P, [Spec()])
        m.verify_row(0, [1, 2, 3])                                             # an unprocessed row: today's launches, today's workspace
        m.set_row_logit_bias(0, {3: 1.0})                                      # ... and a processor that is never verified
        live.append(m.get_option("mem.live_allocs"))
        m.close()
    assert live[0] == live[1]


# ---- 11. determinism; paged equals unpaged --------------------------------------------------------------------------------------------------------------------
def test_determinism_and_paged_equals_unpaged(hip):
    V = 1030
    P = prompts(1, V, 2)
    sp, _ = penalty_spec(V, P)
    sp.table, sp.start = random_table(np.random.default_rng(12), 6, V, max_allowed=200), 0
    look = lookahead(hip, V, P, [sp], 7)[0]
    runs = []
    for paged in (0, 0, 1):
        m = make(hip, V, paged=paged)
        start_rows(m, P, [sp])
        ids, fin = m.verify_row(0, look)
        runs.append(([int(t) for t in ids], fin, m.logits(rounded=False)[0].tobytes(), m.pass_logits().tobytes(), m.read_row_automaton(0)[1]))
        m.close()
    assert runs[0] == runs[1] == runs[2]


# ---- 12. the host engine and the CLI: GPTConfig::speculateProcessed -------------------------------------------------------------------------------------------
PATTERN = r"(yes, no, )+"


def spec_stats(e):
    buf = (c_int64 * 32)()
    e.lib.tgxe_spec_stats(e.h, buf, 32)
    return list(buf[:21])


def test_host_engine_speculate_processed():
    """a regex and a penalty on the GPT-2 geometry (V = 50257: fifty tiles, V % 4 != 0): the ids with speculate + speculateProcessed are those without speculate,
    through generateAsync and through generateSync with two prompts (tgx_verify_rows); verify passes ran; without the flag none, as before"""
    from constraint_util import GPT2_DIR, bind
    from host_util import HostEngine, HostTokenizer, host_lib
    lib = bind(host_lib())
    lib.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    lib.tgxe_set_speculate_processed.argtypes = [c_void_p, c_int]
    lib.tgxe_set_processors.argtypes = [c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, POINTER(ctypes.c_int32), POINTER(ctypes.c_float), c_int]
    lib.tgxe_spec_stats.restype = c_int
    lib.tgxe_spec_stats.argtypes = [c_void_p, POINTER(c_int64), c_int]
    e = HostEngine(lib, synthetic="gpt2", tokenizer_dir=GPT2_DIR, max_batch=2)
    assert e.prepare(), e.error()
    tok = HostTokenizer(lib, GPT2_DIR)
    stops = [50256]
    ps = [tok.encode("Answer: yes, no, yes, no, "), tok.encode("yes, no, yes, no, yes, no, ")]
    lib.tgxe_set_regex(e.h, PATTERN.encode())
    lib.tgxe_set_processors(e.h, 1.0, 0.0, 0.05, None, None, 0)
    runs = {}
    for mode, (spec, processed) in {"plain": (0, 0), "unflagged": (8, 0), "processed": (8, 1)}.items():
        lib.tgxe_set_speculate(e.h, spec)
        lib.tgxe_set_speculate_processed(e.h, processed)
        e.reconfigure(max_new=32, extra_stop=stops)
        before = spec_stats(e)
        aids, anew, afin, _ = e.generate_async(ps[0])
        e.reconfigure(max_new=32, extra_stop=stops)
        out, new, fin = e.generate_sync(ps, pad=stops[0])
        after = spec_stats(e)
        runs[mode] = (list(aids), anew, afin, out.tolist(), new, fin)
        passes = after[0] - before[0]
        assert (passes >= 1) if processed else (passes == 0), (mode, before, after)
    assert runs["plain"] == runs["unflagged"] == runs["processed"]
    e.close()
    tok.close()


def test_cli_speculate_processed():
    from constraint_util import GPT2_DIR
    _, cli = build.build_host()
    base = [cli, "--synthetic", "gpt2", "--tokenizer", GPT2_DIR, "--prompt", "Answer: yes, no, yes, no, ", "--regex", PATTERN, "--frequency-penalty", "0.05", "--stop-ids", "50256",
            "--max-tokens", "32", "--temperature", "0", "--top-p", "1"]
    outs = []
    for extra in ([], ["--speculate", "8"], ["--speculate", "8", "--speculate-processed"]):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        outs.append(out.stdout)
    rows = [[l for l in o.splitlines() if l.startswith("Output:")] for o in outs]
    assert rows[0] == rows[1] == rows[2] and len(rows[0]) == 1
    lines = [[l for l in o.splitlines() if l.startswith("speculate:")] for o in outs]
    assert not lines[0] and int(lines[1][0].split()[1]) == 0 and int(lines[2][0].split()[1]) >= 1, lines      # "speculate: N verify passes, ..."
