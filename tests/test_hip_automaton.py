"""Constrained decoding: per-row token automata stepped on the device (include/tgx.h tgx_automaton_create / tgx_set_row_automaton; kernels/logit_proc.h stage 4
and automaton_advance_kernel).  Held to:
  * the kernel against the float32 restatement (tests/automaton_ref.py), model-free, on one tile, on a vocabulary that is no multiple of 4 and on one with a
    partial last tile: ids and probability bits, a disallowed id at probability exactly 0;
  * a forced sequence: an automaton whose every state allows one token spells its ids whatever the model says, and the row stops on the device;
  * greedy rows under seeded random automata: every id is the argmax of the restatement over the step's raw logits and the test's mirror state, one step per call
    and across the multi-step graph; the state word equals the mirror; unconstrained neighbours are bit-identical to a context that never created a table;
  * sampled rows: never a disallowed id, every step's probability vector the one a scratch context gives for the restatement's logits;
  * the lifecycle calls and the refusals the header names."""
import ctypes

import numpy as np
import pytest

from automaton_ref import NONE, advance, forced_table, mask_np, process_auto_np, random_table
from conftest import load_golden
from logit_proc_ref import argmax_lowest, count, history
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import ADV_STEP, GREEDY, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu

ST_INVALID, ST_UNSUPPORTED, ST_STATE = 1, 2, 4
NINF = float("-inf")
MIX = [GREEDY, SamplerCfg(0.8, 0, 0.9, 0.0), SamplerCfg(1.0, 50, 1.0, 0.0), SamplerCfg(0.9, 40, 0.95, 0.05)]
SEEDS = [11, 22, 33, 44]


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def make(hip, B, budget=0, max_ctx=256, **over):
    cfg, g = load_golden("llama_tiny")
    cfg = dict(cfg, **over)
    d = desc_from_hf_config(cfg, "bf16", max_batch=B)
    d.max_ctx = max_ctx
    m = Model(d, hip)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(int(g["seed"]), float(g["std"])).finalize()


def prompts(B, S=9, seed=0, V=256):
    return np.random.default_rng(seed).integers(0, V, size=(B, S)).astype(np.int64)


def raises(status, call):
    with pytest.raises(TgxError) as e:
        call()
    assert e.value.status == status, (e.value.status, str(e.value))


# ---- 1. the kernel against the restatement, model-free -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [256, 2503, 3080])
def test_kernel_matches_restatement(hip, V):
    """set_logits(L) + automaton (+ penalties + bias) + sample_row == processors off + set_logits(restatement(L)) + sample_row: the same id and the same
    probability bits.  The four states' allowed sets: a single id; everything but one id; the two ids either side of a tile boundary; the last id alone"""
    m = make(hip, 2, vocab_size=V, hidden_size=64, intermediate_size=64, num_attention_heads=1, num_key_value_heads=1, num_hidden_layers=1)
    rng = np.random.default_rng(V)
    peaked = (rng.standard_normal((2, V)) * 2.5).astype(np.float32)
    tied = (np.round(peaked * 2) / 2).astype(np.float32)
    boundary = [1023, 1024] if V > 1024 else [127, 128]
    hole = int(np.argmax(peaked[0]))
    single = next(i for i in range(V // 3, V) if i not in boundary + [hole, V - 1])
    banned = next(i for i in range(V // 2, V) if i not in boundary + [hole, single, V - 1])
    table = np.full((4, V), NONE, np.uint16)
    table[0, single] = 1
    table[1, :] = rng.integers(0, 4, size=V).astype(np.uint16)
    table[1, hole] = NONE
    table[2, boundary] = [3, 0]
    table[3, V - 1] = 2
    aid = m.automaton_create(table, start=0)
    assert m.read_row_automaton(0) == (-1, -1)
    # row 0: penalties and a bias list beside the automaton (one bias on an allowed id of every state, one -inf); row 1: the automaton alone
    pen = dict(repetition=1.3, presence=0.4, frequency=0.3, bias={single: 1.5, boundary[0]: -0.75, V - 1: 0.25, banned: NINF})
    hist = dict(prompt=[single, boundary[1], 3, 4], produced=[V - 1, V - 1, boundary[0], 7])
    words = history(V, hist["prompt"], hist["produced"])
    for L in (peaked, tied):
        for rot in range(4):
            st = [rot, (rot + 1) % 4]
            want = np.stack([process_auto_np(L[0], table, st[0], words, pen["repetition"], pen["presence"], pen["frequency"], pen["bias"]),
                             process_auto_np(L[1], table, st[1])])
            for b in range(2):
                off = table[st[b]] == NONE
                assert (want[b][off] == NINF).all() and np.isfinite(want[b][~off]).any()
            for k, cfg in enumerate(MIX):
                m.set_logits(L)
                m.set_row_penalties(0, pen["repetition"], pen["presence"], pen["frequency"]).set_row_logit_bias(0, pen["bias"])
                m.set_row_history(0, hist["prompt"], hist["produced"])
                got = []
                for b in range(2):
                    m.set_row_automaton(b, aid, st[b])
                    t = m.sample_row(b, cfg, 5 + k)
                    got.append((t, None if cfg.greedy else m.probs()[b].copy()))
                    assert m.read_row_automaton(b) == (aid, st[b])        # tgx_sample_row advances nothing
                m.set_row_penalties(0).set_row_logit_bias(0, None)
                for b in range(2):
                    m.set_row_automaton(b, -1)
                m.set_logits(want)
                for b in range(2):
                    t = m.sample_row(b, cfg, 5 + k)
                    assert t == got[b][0], (V, rot, k, b)
                    assert table[st[b], t] != NONE
                    if cfg.greedy:
                        assert t == argmax_lowest(want[b])
                        continue
                    p = m.probs()[b]
                    assert p.tobytes() == got[b][1].tobytes(), (V, rot, k, b)
                    assert p[t] > 0 and (got[b][1][table[st[b]] == NONE] == 0.0).all()


# ---- 2. a forced sequence ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [0, 1024])
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("B", [2, 8])
def test_forced_sequence(hip, B, sampled, budget):
    """every state allows exactly one token: the row spells [5, 9, 5, 9, stop] whatever the model says, and finishes on the device at the stop id, inside one
    16-step call.  B = 2: the GEMV step; B = 8: the matrix-core batched step, the other rows unconstrained"""
    STOP = 200
    seq = [5, 9, 5, 9, STOP]
    m = make(hip, B, budget=budget)
    V = m.desc.vocab
    P = prompts(B, seed=20 + B)
    m.forward(P)
    aid = m.automaton_create(forced_table(V, seq))
    other = m.automaton_create(forced_table(V, [17, 3, 3, 3, 3, 17, STOP]))
    rows = {0: seq, B - 3 if B > 2 else 1: [17, 3, 3, 3, 3, 17, STOP]}
    cfg = MIX[1] if sampled else GREEDY
    for b in range(B):
        if b in rows:
            m.set_row_automaton(b, aid if rows[b] is seq else other)
            m.set_row_stop(b, 0, [STOP])
        t = m.sample_row(b, cfg, 3 + b)
        assert b not in rows or t == rows[b][0], (b, t)
        m.set_row_sampler(b, cfg, 3 + b)
    ids, new, fin = m.decode_rows(16)
    for b in range(B):
        if b not in rows:
            assert new[b] == 16 and fin[b] == 0 and (ids[:, b] >= 0).all()
            continue
        n = len(rows[b]) - 1
        assert ids[:n, b].tolist() == rows[b][1:], (b, ids[:, b])
        assert new[b] == n and fin[b] == 1 and (ids[n:, b] == -1).all()
        assert m.read_row_automaton(b) == (aid if rows[b] is seq else other, n)      # the stop id was produced, never consumed


# ---- 3. greedy rows under random automata --------------------------------------------------------------------------------------------------------------------
class Batch:
    """B rows after a prefill; `on[b]` = (table index, start state) of the constrained rows, row `pen_row` with a repetition penalty beside its automaton"""

    def __init__(self, hip, B, P, tables, on, pen_row=None, cfg_of=lambda b: 0, create=True, **kw):
        self.m = m = make(hip, B, **kw)
        self.B, self.V, self.tables, self.on, self.pen_row = B, m.desc.vocab, tables, on, pen_row
        m.forward(P)
        self.raw0 = m.logits(rounded=False)
        self.aids = [m.automaton_create(t) for t in tables] if create else []
        self.state = {b: s for b, (_, s) in on.items()}
        self.words = history(self.V, prompt_ids=P[pen_row]) if pen_row is not None else None
        if create:
            for b, (ti, s) in on.items():
                m.set_row_automaton(b, self.aids[ti], s)
            if pen_row is not None:
                m.set_row_penalties(pen_row, 1.3, 0.2, 0.1).set_row_history(pen_row, prompt_ids=P[pen_row])
        self.k = [cfg_of(b) for b in range(B)]
        self.cur = []
        for b in range(B):
            self.cur.append(m.sample_row(b, MIX[self.k[b]], SEEDS[self.k[b]]))
            m.set_row_sampler(b, MIX[self.k[b]], SEEDS[self.k[b]])

    def consume(self):
        """the next step's advance (and the counting step of the penalised row), on the mirror"""
        for b in self.on:
            self.state[b] = advance(self.tables[self.on[b][0]], self.state[b], self.cur[b])
        if self.pen_row is not None:
            count(self.words, self.cur[self.pen_row])

    def processed(self, b, raw_b):
        if b not in self.on:
            return raw_b
        t = self.tables[self.on[b][0]]
        if b == self.pen_row:
            return process_auto_np(raw_b, t, self.state[b], self.words, 1.3, 0.2, 0.1)
        return mask_np(raw_b, t, self.state[b])

    def check_states(self):
        for b in self.on:
            assert self.m.read_row_automaton(b) == (self.aids[self.on[b][0]], self.state[b]), b


def two_tables(V, seed):
    rng = np.random.default_rng(seed)
    return [random_table(rng, 7, V, max_allowed=12), random_table(rng, 7, V)]


@pytest.mark.parametrize("B", [2, 8])
def test_greedy_rows_follow_the_restatement(hip, B):
    P = prompts(B, seed=30 + B)
    tables = two_tables(256, B)
    on = {0: (0, 0), 1: (1, 4)} if B == 2 else {0: (0, 0), 2: (1, 4), 3: (0, 5), 5: (1, 0), 6: (0, 2)}
    pen_row = 0 if B == 2 else 6
    r = Batch(hip, B, P, tables, on, pen_row)
    tw = Batch(hip, B, P, tables, on, create=False)             # a context that never creates a table
    m = r.m
    for b in range(B):
        assert r.cur[b] == argmax_lowest(r.processed(b, r.raw0[b])), b
    r.check_states()
    first, single = list(r.cur), []
    changed = False
    for step in range(20):
        r.consume()
        ids, new, fin = m.decode_rows(1)
        it, _, _ = tw.m.decode_rows(1)
        assert (new == 1).all() and not fin.any()
        raw, lt = m.logits(rounded=False), tw.m.logits(rounded=False)
        for b in range(B):
            assert int(ids[0, b]) == argmax_lowest(r.processed(b, raw[b])), (step, b)
            if b in on:
                assert tables[on[b][0]][r.state[b], int(ids[0, b])] != NONE
                changed = changed or int(ids[0, b]) != argmax_lowest(raw[b])
            else:
                assert ids[0, b] == it[0, b] and raw[b].tobytes() == lt[b].tobytes(), (step, b)
            r.cur[b] = int(ids[0, b])
        r.check_states()
        single.append(ids[0].copy())
    assert changed                                              # the constraint changed what some row did
    single = np.stack(single)
    # a fresh identical context, one call of 20 steps (the multi-step graph, then single steps): the same ids and the same state words, no host in between
    r2 = Batch(hip, B, P, tables, on, pen_row)
    assert r2.cur == first
    ids, new, fin = r2.m.decode_rows(20)
    assert (new == 20).all()
    np.testing.assert_array_equal(ids, single)
    for b in on:
        assert r2.m.read_row_automaton(b) == m.read_row_automaton(b)
    assert tw.m.get_option("mem.live_allocs") < m.get_option("mem.live_allocs")


# ---- 4. sampled rows -----------------------------------------------------------------------------------------------------------------------------------------
def test_sampled_rows_never_leave_the_automaton(hip):
    B = 3
    P = prompts(B, seed=40)
    tables = two_tables(256, 41)
    on = {0: (0, 1), 1: (1, 3), 2: (0, 6)}
    r = Batch(hip, B, P, tables, on, cfg_of=lambda b: b + 1)
    m = r.m
    scratch = make(hip, 1)
    for step in range(64):
        r.consume()
        ids, new, fin = m.decode_rows(1)
        raw, pm = m.logits(rounded=False), m.probs()
        for b in range(B):
            t, cfg = int(ids[0, b]), MIX[r.k[b]]
            tb = tables[on[b][0]]
            assert tb[r.state[b], t] != NONE, (step, b)
            scratch.set_logits(r.processed(b, raw[b])[None])
            scratch.sample(cfg, SEEDS[r.k[b]])
            assert scratch.probs()[0].tobytes() == pm[b].tobytes(), (step, b)
            assert pm[b][t] > 0 and (pm[b][tb[r.state[b]] == NONE] == 0.0).all()
            r.cur[b] = t
    r.check_states()


def test_sampled_rows_across_the_multi_step_graph(hip):
    """64 steps in one call: every id is allowed in the state the mirror reaches by consuming the ids before it"""
    B = 8
    P = prompts(B, seed=42)
    tables = two_tables(256, 43)
    on = {b: (b % 2, b % 7) for b in range(B) if b != 4}
    r = Batch(hip, B, P, tables, on, cfg_of=lambda b: 1 + b % 3)
    ids, new, fin = r.m.decode_rows(64)
    assert (new == 64).all()
    for s in range(64):
        r.consume()
        for b in on:
            assert tables[on[b][0]][r.state[b], int(ids[s, b])] != NONE, (s, b)
        r.cur = [int(t) for t in ids[s]]
    r.check_states()


# ---- 5. lifecycle and refusals -------------------------------------------------------------------------------------------------------------------------------
def test_fork_copies_id_and_state(hip):
    P = prompts(1, seed=50)
    tables = two_tables(256, 51)
    m = make(hip, 3)
    m.forward_row(0, P[0])
    aid = m.automaton_create(tables[1])
    m.set_row_automaton(0, aid, 2)
    cfg = MIX[1]
    cur = m.sample_row(0, cfg, 9)
    m.set_row_sampler(0, cfg, 9)
    state = 2
    for _ in range(5):
        state = advance(tables[1], state, cur)
        cur = int(m.decode_rows(1)[0][0, 0])
    m.fork_row(0, [1, 2])
    assert m.read_row_automaton(0) == m.read_row_automaton(1) == m.read_row_automaton(2) == (aid, state)
    m.set_row_sampler(1, cfg, 101).set_row_sampler(2, cfg, 202)
    st, cu = [state] * 3, [cur] * 3
    seen = []
    for step in range(10):
        st = [advance(tables[1], st[b], cu[b]) for b in range(3)]
        ids, _, _ = m.decode_rows(1)
        for b in range(3):
            assert tables[1][st[b], int(ids[0, b])] != NONE, (step, b)
            assert m.read_row_automaton(b) == (aid, st[b])
        cu = [int(t) for t in ids[0]]
        seen.append(ids[0].copy())
    seen = np.stack(seen)
    assert (seen[:, 1] != seen[:, 0]).any() or (seen[:, 2] != seen[:, 0]).any()      # the same constraint, their own draws


def test_reset_extend_truncate_and_retired_rows(hip):
    B = 2
    P = prompts(B, seed=52)
    tables = two_tables(256, 53)
    r = Batch(hip, B, P, tables, {0: (0, 3), 1: (1, 1)})
    m = r.m
    got = []
    for _ in range(6):
        r.consume()
        ids, _, _ = m.decode_rows(1)
        r.cur = [int(t) for t in ids[0]]
        got.append(ids[0].copy())
    got = np.stack(got)
    r.check_states()
    # truncate and extend keep id and state
    n = m.past_length_row(0)
    m.truncate_row(0, n - 2)
    assert m.read_row_automaton(0) == (r.aids[0], r.state[0])
    m.extend_row(0, got[-3:-1, 0])
    assert m.read_row_automaton(0) == (r.aids[0], r.state[0])
    t = m.sample_row(0, GREEDY)
    assert t == argmax_lowest(r.processed(0, m.logits(rounded=False)[0]))
    # destroy in use: refused; reset switches the row off and the table lives on
    raises(ST_STATE, lambda: m.automaton_destroy(r.aids[1]))
    m.reset_row(1)
    assert m.read_row_automaton(1) == (-1, -1)
    m.automaton_destroy(r.aids[1])
    raises(ST_INVALID, lambda: m.set_row_automaton(1, r.aids[1]))
    # a setting on the retired row: kept, not advanced while the slot rides along, in force with the admission
    m.set_row_automaton(1, r.aids[0], 5)
    raises(ST_STATE, lambda: m.automaton_destroy(r.aids[0]))
    ids, _, _ = m.decode_rows(3)
    assert (ids[:, 1] == -1).all() and m.read_row_automaton(1) == (r.aids[0], 5)
    m.forward_row(1, P[1])
    t = m.sample_row(1, GREEDY)
    assert t == argmax_lowest(mask_np(m.logits(rounded=False)[1], tables[0], 5))
    m.reset_row(0)
    m.decode_rows(1)
    assert m.read_row_automaton(1) == (r.aids[0], advance(tables[0], 5, t))
    m.reset_cache()
    assert m.read_row_automaton(0) == m.read_row_automaton(1) == (-1, -1)
    m.automaton_destroy(r.aids[0])


def test_memory_and_tables_without_rows(hip):
    B = 2
    P = prompts(B, seed=54)
    tables = two_tables(256, 55)
    m, tw = make(hip, B), make(hip, B)
    for x in (m, tw):
        x.forward(P)
    allocs, kib = m.get_option("mem.live_allocs"), m.get_option("mem.live_kib")
    aid = m.automaton_create(tables[0])
    assert m.get_option("mem.live_allocs") == allocs + 1 and kib + 3 <= m.get_option("mem.live_kib") <= kib + 4      # 7 * 256 * 2 bytes
    # tables but no row using one: nothing else is allocated and the rows decode like the twin's, bit for bit; tgx_decode ignores a setting altogether
    for x in (m, tw):
        for b in range(B):
            x.sample_row(b, MIX[1], 7)
            x.set_row_sampler(b, MIX[1], 7)
    a, _, _ = m.decode_rows(20)
    b_, _, _ = tw.decode_rows(20)
    np.testing.assert_array_equal(a, b_)
    assert m.logits(rounded=False).tobytes() == tw.logits(rounded=False).tobytes() and m.probs().tobytes() == tw.probs().tobytes()
    assert m.get_option("mem.live_allocs") == tw.get_option("mem.live_allocs") + 1
    m.automaton_destroy(aid)
    assert m.get_option("mem.live_allocs") == tw.get_option("mem.live_allocs") and m.get_option("mem.live_kib") == tw.get_option("mem.live_kib")
    aid = m.automaton_create(tables[1])
    m.set_row_automaton(0, aid, 2)
    np.testing.assert_array_equal(m.decode(4, GREEDY), tw.decode(4, GREEDY))
    assert m.read_row_automaton(0) == (aid, 2)
    assert m.logits(rounded=False).tobytes() == tw.logits(rounded=False).tobytes()


def test_refusals(hip):
    B = 3
    P = prompts(B, seed=56)
    cfg, g = load_golden("llama_tiny")
    tables = two_tables(256, 57)
    early = Model(desc_from_hf_config(cfg, "bf16", max_batch=1), hip)
    for call in (lambda: early.automaton_create(tables[0]), lambda: early.automaton_destroy(0), lambda: early.set_row_automaton(0, -1), lambda: early.read_row_automaton(0)):
        raises(ST_STATE, call)
    early.close()
    r = Batch(hip, B, P, tables, {0: (0, 0)})
    m, V = r.m, r.V
    kib = m.get_option("mem.live_kib")
    u16p = ctypes.POINTER(ctypes.c_uint16)
    out = ctypes.c_int32(-7)

    def create(n_states, start, arr):
        m._check(m.be.automaton_create(m._ctx, n_states, start, arr.ctypes.data_as(u16p) if arr is not None else None, ctypes.byref(out)))

    good = tables[1]
    high, dead = good.copy(), good.copy()
    high[3, 100] = 7                 # neither a state (0 .. 6) nor NONE
    dead[5, :] = NONE
    bad = [lambda: create(0, 0, good), lambda: create(-1, 0, good), lambda: create(65536, 0, good), lambda: create(7, 7, good), lambda: create(7, -1, good),
           lambda: create(7, 0, high), lambda: create(7, 0, dead), lambda: create(7, 0, None),
           lambda: m._check(m.be.automaton_create(m._ctx, 7, 0, good.ctypes.data_as(u16p), None)),
           lambda: m.automaton_destroy(-1), lambda: m.automaton_destroy(16), lambda: m.automaton_destroy(9),
           lambda: m.set_row_automaton(-1, r.aids[0]), lambda: m.set_row_automaton(B, r.aids[0]), lambda: m.set_row_automaton(1, 9), lambda: m.set_row_automaton(1, 16),
           lambda: m.set_row_automaton(1, -2), lambda: m.set_row_automaton(1, r.aids[0], 7), lambda: m.set_row_automaton(1, r.aids[0], -2),
           lambda: m.read_row_automaton(B)]
    for i, call in enumerate(bad):
        with pytest.raises(TgxError) as e:
            call()
        assert e.value.status == ST_INVALID, i
    assert out.value == -7 and m.get_option("mem.live_kib") == kib and m.read_row_automaton(1) == (-1, -1)
    more = [m.automaton_create(good) for _ in range(16 - len(r.aids))]
    raises(ST_INVALID, lambda: m.automaton_create(good))          # a 17th live table
    for a in more:
        m.automaton_destroy(a)
    assert m.get_option("mem.live_kib") == kib
    # an automaton is a processor on: the verify calls and a STEP row of tgx_advance_rows refuse the row, and nothing changes
    n0 = m.past_length_row(0)
    for call in (lambda: m.verify_row(0, [1, 2, 3]), lambda: m.verify_row_sampled(0, [1, 2, 3]), lambda: m.verify_rows([1, 0], [[1, 2], [3]]),
                 lambda: m.advance_rows([0, 1], [ADV_STEP, ADV_STEP], [[1], [2]])):
        raises(ST_UNSUPPORTED, call)
    assert m.past_length_row(0) == n0 and m.past_length_row(1) == n0 and m.read_row_automaton(0) == (r.aids[0], 0)
    out1, fin = m.verify_row(1, [1, 2, 3])                        # the unconstrained neighbour verifies
    assert 1 <= len(out1) <= 4
    r.cur[1] = int(out1[-1])
    # nothing above changed row 0's settings or poisoned the context
    for step in range(3):
        r.consume()
        ids, _, _ = m.decode_rows(1)
        assert int(ids[0, 0]) == argmax_lowest(r.processed(0, m.logits(rounded=False)[0]))
        r.cur = [int(t) for t in ids[0]]
    r.check_states()


# ---- 6. the host engine: a regular expression compiled over the GPT-2 tokenizer ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    """the GPT-2 geometry the CLI tests run with the GPT-2 ids (--synthetic gpt2), beside the GPT-2 tokenizer fixture"""
    from constraint_util import GPT2_DIR, bind
    from host_util import HostEngine, HostTokenizer, host_lib
    lib = bind(host_lib())
    e = HostEngine(lib, synthetic="gpt2", tokenizer_dir=GPT2_DIR, max_batch=2)
    assert e.prepare(), e.error()
    tok = HostTokenizer(lib, GPT2_DIR)
    yield lib, e, tok
    e.close()
    tok.close()


def check_row(pat, table, start, tok, new_ids, stops, must_stop=False):
    """a row's new tokens: up to a stop id they decode to a full match; without one they are a path through the table (a prefix of a match)"""
    from constraint_util import fullmatch, walk
    cut = next((i for i, t in enumerate(new_ids) if int(t) in stops), None)
    assert cut is not None or not must_stop
    if cut is None:
        assert walk(table, start, new_ids) is not None, (pat, list(new_ids))
        return False
    assert walk(table, start, new_ids[:cut + 1]) is not None, (pat, list(new_ids))
    text = tok._decode([int(t) for t in new_ids[:cut]], 0).decode("utf-8")
    assert fullmatch(pat, text), (pat, text)
    return True


@pytest.mark.parametrize("sampler", [dict(temperature=0.0), dict(temperature=0.8, top_p=0.9)])
def test_engine_output_matches_the_pattern(engine, sampler):
    from constraint_util import PATTERNS, compile_table
    lib, e, tok = engine
    stops = [50256]                                                    # the fixture's tokenizer_config names no EOS: the request's stop id, as a server passes it
    vocab = 50257
    prompts = [tok.encode("Answer:"), tok.encode("The date of the launch, as JSON or text:")]
    stopped = 0
    for pat in PATTERNS:
        table, start, accept = compile_table(lib, pat, stops=tuple(stops), vocab=vocab)
        lib.tgxe_set_regex(e.h, pat.encode())
        e.reconfigure(max_new=40, extra_stop=stops, **sampler)
        assert e.eos_ids() == stops
        ids, new, fin, seen = e.generate_async(prompts[0])
        assert new <= 40 and len(ids) == len(prompts[0]) + new
        stopped += check_row(pat, table, start, tok, ids[len(prompts[0]):], stops, must_stop=fin == "stop")
        e.reconfigure(max_new=40, extra_stop=stops, **sampler)             # (a row that finished on the device is reset by the next reconfigure, as on every per-row path; the same pattern compiles once)
        out, new, fin = e.generate_sync(prompts, pad=stops[0])           # two rows of unequal length, each with the automaton from its admission
        S = out.shape[1] - new
        done = [check_row(pat, table, start, tok, out[b, S:], stops) for b in range(2)]
        assert (fin == "stop") == all(done)
        stopped += sum(done)
    assert stopped >= 3                                                   # (yes|no|maybe) and the date are finite: they end inside 40 tokens
    # switched off, the engine's plain loop is back: the ids of an engine that never had a pattern
    lib.tgxe_set_regex(e.h, b"")
    e.reconfigure(max_new=6)
    plain, _, _ = e.generate_sync([prompts[0]], pad=stops[0])
    assert len(plain[0]) == len(prompts[0]) + 6


def test_cli_regex():
    import subprocess
    from constraint_util import GPT2_DIR, fullmatch
    from tinygpt_amd import build
    _, cli = build.build_host()
    pat = r"\d{4}-\d{2}-\d{2}"
    out = subprocess.run([cli, "--synthetic", "gpt2", "--tokenizer", GPT2_DIR, "--prompt", "The date:", "--regex", pat, "--stop-ids", "50256", "--max-tokens", "24", "--temperature", "0", "--top-p", "1"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    line = next(l for l in out.stdout.splitlines() if l.startswith("Output:"))
    assert fullmatch(pat, line[len("Output:"):].strip()[1:-1]), line
    bad = subprocess.run([cli, "--synthetic", "gpt2", "--tokenizer", GPT2_DIR, "--prompt", "The date:", "--regex", "a{5,2}", "--stop-ids", "50256", "--max-tokens", "4"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "regex position" in bad.stderr
