"""Beam search on the device (include/tgx.h tgx_beam_select / tgx_beam_advance; kernels/beam.h, csrc/beam_plan.h).  Held to:
  * select on injected logits == tests/beam_ref.py (numpy float64 log_softmax of the fp32 logits read back, plus the scores, in the stable joint order): beams and
    ids EXACTLY — the reference's adjacent candidates are tied by construction or >= 1e-3 apart, asserted on the reference before the GPU is looked at — lp within
    2e-5 (tests/test_hip_logprobs.py's derived bound), score within 2e-5 + 2^-23 |ref| (the fp32 rounding of the key), the same call twice the same bits;
  * select on real logits (2-layer, vocabulary-4096 cuts of four geometries, slabs and paged) after a prefill and after steps; under an automaton and a -inf bias
    only allowed ids come back, lp normalised over the allowed set;
  * advance: out_rows == the pinned placement; every placed row's cache rows [0, past) == the parent's, read BEFORE the call, bit for bit; kv.free_tokens exact at
    past 5 / 128 / 200; childless rows read length 0; a bystander row keeps logits and cache bit for bit; every refusal changes nothing;
  * advance + one step == tgx_fork_row + tgx_extend_row of one token (logits rel 1e-3, the new cache position within one ulp of the storage dtype);
  * a search of K = 4 over 6 steps driven through the two calls on the golden tiny families: every surviving row's logits against OracleModel.forward of its full
    sequence (rel 1e-2), every chosen candidate's lp within 2 x 1e-2 x max |oracle logit| of the oracle's (log-softmax moves at most twice the sup-norm change);
  * a context that never makes the new calls holds what its twin holds (mem.live_allocs / mem.live_kib)."""
import numpy as np
import pytest

import beam_ref
from conftest import GPU_FAMILIES, load_golden, rel_err
from test_hip_fork_row import BLK, MODELS, free, prompt, real, refused
from test_hip_logprobs import close, make
from test_hip_verify_row import check_kv, kv_all
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, MAX_BEAM_CAND, Model, TgxError

pytestmark = pytest.mark.gpu

TOL = 2e-5
ST_INVALID, ST_STATE, ST_CONTEXT = 1, 4, 8


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def check_cands(got, want, what):
    """got = Model.beam_select's arrays against the reference prefix `want`, exactly in beams and ids"""
    beam, tok, score, lp = got
    assert len(beam) == len(want), (what, len(beam), len(want))
    np.testing.assert_array_equal(beam, [c[1] for c in want], err_msg=str(what))
    np.testing.assert_array_equal(tok, [c[3] for c in want], err_msg=str(what))
    worst = 0.0
    for j, c in enumerate(want):
        worst = max(worst, close(lp[j], c[4], TOL, str(what)))
        assert abs(float(score[j]) - c[0]) <= TOL + 2.0 ** -23 * abs(c[0]), (what, j, float(score[j]), c[0])
    return worst


# ---- 1. injected logits -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [320, 5003, 70001])
def test_select_injected(hip, V):
    """one tile; a ragged last tile with V % 4 != 0; many tiles — n 1 / 3 / 8, k 1 / 4 / 8, 0 / 1 / 8 end ids, mixed rows and rows identical in pairs"""
    cases = beam_ref.cases(V)
    for (n, kind, pattern, vecs, scores, k, ends) in cases:      # the reference alone, before the GPU is looked at: nothing is skipped
        gap = beam_ref.min_gap(vecs, scores, k, ends)
        assert gap >= beam_ref.GAP, (V, n, kind, pattern, k, len(ends), gap)
    m = make(hip, 8, num_hidden_layers=1, vocab_size=V)
    worst, loaded, ties = 0.0, None, 0
    for (n, kind, pattern, vecs, scores, k, ends) in cases:
        if loaded != (n, kind):
            m.reset_cache()
            m.forward_rows(range(n), [np.arange(3 + r) % V for r in range(n)])      # live rows; their logits are replaced
            m.set_logits(np.stack(vecs))
            back = m.logits(rounded=False)
            for i in range(n):
                np.testing.assert_array_equal(back[i], vecs[i])
            loaded = (n, kind)
        what = (V, n, kind, pattern, k, len(ends))
        want, _ = beam_ref.select(vecs, scores, k, ends)
        got = m.beam_select(range(n), scores, k, ends)
        worst = max(worst, check_cands(got, want, what))
        live = sum(t not in ends for t in got[1])
        assert live == k or len(got[0]) == MAX_BEAM_CAND or live == sum(np.isfinite(v).sum() for v in vecs), what      # it ends at the k-th live candidate
        again = m.beam_select(range(n), scores, k, ends)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes(), what
        if kind == "twins":      # exact ties between rows: compared above, and counted here — they came out in (array index, rank) order
            ties += sum(want[j][0] == want[j + 1][0] and want[j][1] < want[j + 1][1] for j in range(len(want) - 1))
    assert ties > 0
    print(f"injected V={V}: {len(cases)} cases, max |lp - ref| = {worst:.3e}")
    m.close()


# ---- 2. real logits -----------------------------------------------------------------------------------------------------------------------------------------
def check_real(m, rows, scores, k, ends, what):
    """the call against the reference of the logits read back, without an assumption on gaps: every returned (beam, token) carries the reference's lp and key, the
    keys do not increase (beyond the bound on two of them), nothing left out beats the last one, and the prefix ends where it should"""
    lg = m.logits(rounded=False)
    vecs = [lg[r] for r in rows]
    beam, tok, score, lp = m.beam_select(rows, scores, k, ends)
    ref_lp = [beam_ref.log_softmax64(v) for v in vecs]
    keys = []
    for j in range(len(beam)):
        r = ref_lp[beam[j]][tok[j]]
        close(lp[j], r, TOL, str(what))
        keys.append(float(np.float64(np.float32(scores[beam[j]])) + r))
        assert abs(float(score[j]) - keys[-1]) <= TOL + 2.0 ** -23 * abs(keys[-1]), what
    assert all(keys[j] >= keys[j + 1] - 2 * TOL for j in range(len(keys) - 1)), what
    assert len(set(zip(beam.tolist(), tok.tolist()))) == len(beam), what
    live = [t not in ends for t in tok]
    assert sum(live) == k and live[-1], what
    taken = set(zip(beam.tolist(), tok.tolist()))
    for i, r in enumerate(ref_lp):
        best = max(float(np.float64(np.float32(scores[i])) + r[t]) for t in np.argsort(-r)[: len(beam) + 1] if (i, int(t)) not in taken)
        assert best <= keys[-1] + 2 * TOL, (what, i)
    return beam, tok, score, lp


@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("name,dtype", MODELS)
def test_select_real_logits(name, dtype, paged):
    """after a prefill of three prompts of different lengths, and again after steps"""
    m = real(name, dtype, 4, 512, 12 * BLK if paged else 0)
    m.forward_rows([0, 1, 2], [prompt(5, 1), prompt(130, 2), prompt(40, 3)])
    scores = np.array([-0.5, 0.0, -1.25], np.float32)
    lg = m.logits(rounded=False)
    ends = [int(np.argmax(lg[1]))]
    check_real(m, [0, 1, 2], scores, 4, ends, (name, "prefill"))
    check_real(m, [2, 0], scores[:2], 8, [], (name, "prefill, two rows"))
    for r in range(3):
        m.sample_row(r, GREEDY)
    m.decode_rows(3)
    check_real(m, [0, 1, 2], scores, 4, ends, (name, "steps"))
    check_real(m, [1], scores[:1], 8, ends, (name, "steps, one row"))
    m.close()


def test_select_under_processors(hip):
    """row 0 under an automaton that allows 12 ids and a bias of -inf on two of them, row 1 plain: row 0 returns allowed ids only, its lp normalised over them"""
    m = make(hip, 2)
    V = m.desc.vocab
    m.forward_rows([0, 1], [np.arange(7) % V, np.arange(11) % V])
    allowed = list(range(5, V, V // 12))[:12]
    table = np.full((1, V), 0xFFFF, np.uint16)
    table[0, allowed] = 0
    aid = m.automaton_create(table)
    m.set_row_automaton(0, aid)
    m.set_row_logit_bias(0, {allowed[0]: -np.inf, allowed[1]: -np.inf, allowed[2]: 1.5})
    lg = m.logits(rounded=False)
    v0 = np.full(V, -np.inf, np.float32)
    v0[allowed[2:]] = lg[0][allowed[2:]]
    v0[allowed[2]] += np.float32(1.5)
    scores = np.zeros(2, np.float32)
    want, _ = beam_ref.select([v0], scores[:1], 8)
    got = m.beam_select([0], scores[:1], 8)
    assert set(got[1].tolist()) <= set(allowed[2:]) and len(got[1]) == 8
    np.testing.assert_array_equal(got[1], [c[3] for c in want])
    close(got[3], [c[4] for c in want], TOL)
    assert abs(np.exp(np.asarray(m.beam_select([0], scores[:1], 8, allowed[2:10])[3], np.float64)).sum() - 1.0) < 1e-4      # all ten of them: one distribution
    beam, tok, _, lp = m.beam_select([0, 1], scores, 8)
    for j in range(len(beam)):
        if beam[j] == 0:
            assert tok[j] in allowed[2:]
            close(lp[j], beam_ref.log_softmax64(v0)[tok[j]], TOL)
        else:
            close(lp[j], beam_ref.log_softmax64(lg[1])[tok[j]], TOL)
    assert m.read_row_automaton(0) == (aid, 0)      # no state move
    m.close()


# ---- 3. advance -----------------------------------------------------------------------------------------------------------------------------------------------
def same_kv(a, b, what):
    for layer, (x, y) in enumerate(zip(a, b)):
        for p, q in zip(x, y):
            np.testing.assert_array_equal(p, q, err_msg=str((what, layer)))


def advance_checked(m, rows, parent, tokens, want_rows, what):
    """the call; out_rows == the pinned placement; every placed row holds its parent's length and cache rows as read before the call"""
    before = {r: (m.past_length_row(r), kv_all(m, r)) for r in set(rows[p] for p in parent)}
    out = m.beam_advance(rows, parent, tokens)
    assert out.tolist() == want_rows, (what, out.tolist())
    for j, r in enumerate(out):
        n, kv = before[rows[parent[j]]]
        assert m.past_length_row(int(r)) == n, (what, j)
        same_kv(kv_all(m, int(r)), kv, (what, j))
    for r in rows:
        if r not in out:
            assert m.past_length_row(r) == 0, (what, r)
    return out


@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("P", [5, 128, 200])
@pytest.mark.parametrize("name,dtype", [MODELS[0], MODELS[3]])
def test_advance_placement_cache_and_blocks(name, dtype, P, paged):
    """row 0 a bystander of 40 tokens, the group in rows 1 .. 4: 1 -> 4 from a fresh prefill, a step, the identity, a step, a permutation with a repeated parent, all
    children of one parent, a shrink; kv.free_tokens after each (tail at 5, no tail at 128, a tail behind a shared block at 200)"""
    budget = 24 * BLK if paged else 0
    m = real(name, dtype, 6, 512, budget)
    G = [1, 2, 3, 4]
    m.forward_rows([0, 1], [prompt(40, 9), prompt(P, 10)])
    m.sample_row(0, GREEDY)
    by = (m.logits(rounded=False)[0].copy(), kv_all(m, 0))
    tail = 1 if P % BLK else 0
    f = budget - (1 + (P + BLK - 1) // BLK) * BLK
    assert not paged or free(m) == f
    advance_checked(m, G, [0, 0, 0, 0], [11, 12, 13, 14], [1, 2, 3, 4], "1 -> 4")
    f -= 3 * tail * BLK
    assert not paged or free(m) == f
    lg = m.logits(rounded=False)
    for r in (2, 3, 4):
        np.testing.assert_array_equal(lg[r], lg[1])      # the logits travelled with the copy
    np.testing.assert_array_equal(lg[0], by[0])
    same_kv(kv_all(m, 0), by[1], "bystander")
    ids, new, fin = m.decode_rows(1)
    assert list(new) == [1] * 5 and [m.past_length_row(r) for r in G] == [P + 1] * 4
    f -= 0 if tail else 4 * BLK          # at 128 every row of the group writes position 128 into a block of its own
    assert not paged or free(m) == f
    lg = m.logits(rounded=False)
    assert not np.array_equal(lg[1], lg[2])      # four different tokens went in
    by = (lg[0].copy(), kv_all(m, 0))
    advance_checked(m, G, [0, 1, 2, 3], [21, 22, 23, 24], [1, 2, 3, 4], "identity")
    assert not paged or free(m) == f
    m.decode_rows(1)
    by = (m.logits(rounded=False)[0].copy(), kv_all(m, 0))
    advance_checked(m, G, [2, 0, 2, 1], [31, 32, 33, 34], [3, 1, 4, 2], "a repeated parent")      # row 4 retires and takes the second child of row 3
    assert not paged or free(m) == f            # its private tail block went back and came again
    np.testing.assert_array_equal(m.logits(rounded=False)[0], by[0])
    same_kv(kv_all(m, 0), by[1], "bystander")
    advance_checked(m, G, [1, 1, 1, 1], [41, 42, 43, 44], [2, 1, 3, 4], "all children of one parent")
    assert not paged or free(m) == f
    m.decode_rows(1)
    advance_checked(m, G, [2, 0], [51, 52], [3, 1], "a shrink")
    f += 2 * BLK                                 # rows 2 and 4 gave back the blocks only they mapped: their tails
    assert not paged or free(m) == f
    ids, new, fin = m.decode_rows(1)
    assert list(new) == [1, 1, 0, 1, 0] and list(ids[0, [2, 4]]) == [-1, -1]
    advance_checked(m, G, [0, 0, 2], [61, 62, 63], [1, 2, 3], "regrown through the retired rows")
    m.decode_rows(1)
    assert [m.past_length_row(r) for r in range(5)] == [45, P + 5, P + 5, P + 5, 0]
    m.close()


def test_refusals_change_nothing():
    """every refusal of the two calls returns its status and leaves kv.free_tokens and every row's length as they were; afterwards one step equals, bit for bit, that
    of a control that never made the calls"""
    budget = 7 * BLK
    m, ctrl = real("llama-3.2-1b", "bf16", 6, 768, budget), real("llama-3.2-1b", "bf16", 6, 768, budget)
    for x in (m, ctrl):
        x.forward_rows([0, 1, 2, 3], [prompt(300, 1), prompt(200, 2), prompt(5, 3), prompt(20, 4)])      # 3 + 2 + 1 + 1 blocks
        for r in range(4):
            x.sample_row(r, GREEDY)
        x.reset_row(2)                                               # row 2 retired
        x.set_row_stop(1, max_new=1)
        assert x.decode_rows(2)[2][1] == 2                           # row 1 finished
    assert free(m) == BLK
    adv = [(ST_INVALID, [], [], []),                     # n_rows < 1
           (ST_INVALID, list(range(9)), [0], [1]),       # n_rows > TGX_MAX_BEAMS (and rows out of range)
           (ST_INVALID, [0, 2], [], []),                 # n_next < 1
           (ST_INVALID, [0, 2], [0, 0, 0], [1, 1, 1]),   # n_next > n_rows
           (ST_INVALID, [0, 6], [0, 0], [1, 1]), (ST_INVALID, [0, -1], [0, 0], [1, 1]),      # a row out of range
           (ST_INVALID, [0, 0], [0, 0], [1, 1]),         # a row named twice
           (ST_INVALID, [0, 2], [0, 2], [1, 1]), (ST_INVALID, [0, 2], [-1, 0], [1, 1]),      # a parent out of range
           (ST_INVALID, [0, 2], [0, 0], [1, 4096]), (ST_INVALID, [0, 2], [0, 0], [-1, 1]),   # a token out of range
           (ST_INVALID, [0, 5], [0, 0], [1, 1]),         # a gap in the new rows (4 is next)
           (ST_STATE, [0, 1], [0, 0], [1, 1]),           # a finished row named
           (ST_STATE, [1, 2], [0], [1]),                 # ... as the parent
           (ST_STATE, [0, 2], [1, 0], [1, 1]),           # a retired row as parent
           (ST_STATE, [0, 4], [1], [1]),                 # a new row as parent
           (ST_CONTEXT, [0, 2, 4], [0, 0, 0], [1, 1, 1])]      # two tail blocks, one free
    for status, rows, parent, tokens in adv:
        refused(m, status, lambda: m.beam_advance(rows, parent, tokens), 6)
    m.truncate_row(3, 10); ctrl.truncate_row(3, 10)                  # row 3 holds no logits
    refused(m, ST_STATE, lambda: m.beam_advance([0, 3], [0, 0], [1, 1]), 6)
    refused(m, ST_STATE, lambda: m.beam_select([3], [0.0], 1), 6)
    m.extend_row(3, [7, 8]); ctrl.extend_row(3, [7, 8])
    m.sample_row(3, GREEDY); ctrl.sample_row(3, GREEDY)
    sel = [(ST_INVALID, [], [], 1, []), (ST_INVALID, list(range(9)), [0.0] * 9, 1, []),      # n
           (ST_INVALID, [0], [0.0], 0, []), (ST_INVALID, [0], [0.0], 9, []),                   # k
           (ST_INVALID, [0], [0.0], 1, list(range(9))),                                        # n_end
           (ST_INVALID, [0], [np.nan], 1, []), (ST_INVALID, [0, 3], [0.0, -np.inf], 1, []),    # a score that is not finite
           (ST_INVALID, [0, 0], [0.0, 0.0], 1, []),                                            # a row named twice
           (ST_INVALID, [6], [0.0], 1, []), (ST_INVALID, [-1], [0.0], 1, []),                  # a row out of range
           (ST_STATE, [2], [0.0], 1, []),                                                      # a retired row
           (ST_STATE, [0, 1], [0.0, 0.0], 1, []),                                              # a finished row
           (ST_STATE, [4], [0.0], 1, [])]                                                      # an empty row beyond the batch
    for status, rows, scores, k, ends in sel:
        refused(m, status, lambda: m.beam_select(rows, scores, k, ends), 6)
    early = Model(m.desc)                                            # before tgx_finalize
    for call in (lambda: early.beam_select([0], [0.0], 1), lambda: early.beam_advance([0, 1], [0, 0], [1, 1])):
        with pytest.raises(TgxError) as ei:
            call()
        assert ei.value.status == ST_STATE
    early.close()
    (ia, na, fa), (ib, nb, fb) = m.decode_rows(1), ctrl.decode_rows(1)
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(m.logits(rounded=False)[[0, 3]], ctrl.logits(rounded=False)[[0, 3]])
    out = m.beam_advance([0, 2, 4], [0, 0], [1, 1])                  # what fits, fits: one tail block
    assert out.tolist() == [0, 2] and free(m) == 0 and m.batch == 4
    m.close(); ctrl.close()


# ---- 4. equivalence -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("name,dtype", MODELS)
def test_advance_and_step_equal_fork_and_extend(name, dtype, paged):
    """A: tgx_beam_advance 1 -> 4 + tgx_decode_rows(1); B: tgx_fork_row + tgx_extend_row(row, [token], 1) per row.  Logits rel 1e-3 (GPU against GPU), the cache rows
    [0, past) bit for bit and the new position within one ulp of the storage dtype (check_kv)"""
    P, toks = 200, [17, 4001, 902, 33]
    budget = 16 * BLK if paged else 0
    A, B = real(name, dtype, 4, 512, budget), real(name, dtype, 4, 512, budget)
    p = prompt(P, 77)
    A.forward_row(0, p); B.forward_row(0, p)
    assert A.beam_advance([0, 1, 2, 3], [0, 0, 0, 0], toks).tolist() == [0, 1, 2, 3]
    A.decode_rows(1)
    B.fork_row(0, [1, 2, 3])
    for r in range(4):
        B.extend_row(r, [toks[r]])
    la, lb = A.logits(rounded=False), B.logits(rounded=False)
    for r in range(4):
        assert A.past_length_row(r) == B.past_length_row(r) == P + 1
        err = rel_err(la[r][None, :], lb[r][None, :])
        assert err < 1e-3, (name, r, err)
        ka, kb = kv_all(A, r), kv_all(B, r)
        for layer in range(2):
            for x, y in zip(ka[layer], kb[layer]):
                np.testing.assert_array_equal(x[:P], y[:P])
        check_kv(ka, kb, dtype, (name, r))
    A.close(); B.close()


# ---- 5. the oracle ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("fam", GPU_FAMILIES)
def test_search_against_the_oracle(hip, oracle_lib, fam, paged):
    """K = 4, 6 steps, the GPU makes every choice: after each step every row's logits against the oracle's forward of its full sequence, every chosen candidate's lp
    against the oracle's log_softmax of its parent's logits"""
    from oracle.oracle_ffi import OracleModel
    K, STEPS = 4, 6
    cfg, g = load_golden(fam)
    m = make(hip, K, fam=fam, budget=8 * BLK if paged else 0)
    d = desc_from_hf_config(cfg, "bf16", max_batch=K)
    d.max_ctx = m.desc.max_ctx
    ref = OracleModel(d).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    p = np.asarray(g["prompt"], np.int64).reshape(-1)[:9]

    def oracle_logits(seqs):
        ref.reset_cache()
        ref.forward(np.stack(seqs))
        return ref.logits(rounded=False)

    m.forward_row(0, p)
    seqs, rows, scores = [list(p)], [0], np.zeros(1, np.float32)
    group = list(range(K))
    for step in range(STEPS + 1):
        want = oracle_logits([np.asarray(s, np.int64) for s in seqs])
        got = m.logits(rounded=False)
        for i, r in enumerate(rows):
            err = rel_err(got[r][None, :], want[i][None, :])
            assert err < 1e-2, (fam, step, i, err)
        if step == STEPS:
            break
        beam, tok, score, lp = m.beam_select(rows, scores, K)
        assert len(beam) == K
        for j in range(K):
            o = want[beam[j]]
            assert abs(float(lp[j]) - beam_ref.log_softmax64(o)[tok[j]]) <= 2 * 1e-2 * np.abs(o).max(), (fam, step, j)
        out = m.beam_advance(rows if step else group, beam, tok)
        seqs = [seqs[beam[j]] + [int(tok[j])] for j in range(K)]
        rows, scores = [int(r) for r in out], score.copy()
        assert sorted(rows) == group
        m.decode_rows(1)
        assert [m.past_length_row(r) for r in rows] == [len(p) + step + 1] * K
    ref.close(); m.close()


# ---- 6. memory --------------------------------------------------------------------------------------------------------------------------------------------------
def test_nothing_allocated_until_the_first_call(hip):
    """twin contexts through a prefill, a sample and steps hold the same buffers; tgx_beam_advance allocates nothing, the first tgx_beam_select one workspace, the
    second nothing"""
    def mem(x):
        return x.get_option("mem.live_allocs"), x.get_option("mem.live_kib")
    a, b = make(hip, 4), make(hip, 4)
    for x in (a, b):
        x.forward_row(0, np.arange(9)); x.sample_row(0, GREEDY); x.decode_rows(2)
    assert mem(a) == mem(b)
    a.beam_advance([0, 1, 2, 3], [0, 0, 0, 0], [1, 2, 3, 4])
    assert mem(a) == mem(b)
    a.decode_rows(1)                     # (a four-row step may size a workspace of its own)
    before = mem(a)
    a.beam_select([0, 1, 2, 3], np.zeros(4, np.float32), 4)
    after = mem(a)
    assert after[0] == before[0] + 1 and after[1] >= before[1]
    a.beam_select([0, 1], np.zeros(2, np.float32), 8, [3])
    assert mem(a) == after
    a.close(); b.close()
