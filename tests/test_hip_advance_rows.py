"""tgx_advance_rows (include/tgx.h): prompt chunks (FEED / FEED_MORE) and live rows' steps (STEP) in ONE ragged pass.  The contract is "equal to tgx_verify_rows over
the STEP rows, tgx_extend_row for a FEED on a row that holds positions, tgx_forward_row for a FEED into an empty or new row, up to the order of the fp32 sums", with
the project's numbers: GPU against GPU logits rel_err < 1e-3, live cache rows by tests/test_hip_verify_row.py's check_kv, greedy ids equal where the CPU oracle's
top-2 gap clears that file's BAND (asserted, so no id comparison is skipped), sampled ids restated from the call's OWN pass logits with the row's key
(tests/verify_sampled_util.py: expected_draw, walk; the cap on compared draws inside the top-p band is 0).  Every context is a 2-layer cut of
tests/verify_sampled_util.py (vocabulary 4096, max_batch 2 - 7, max_ctx 512).

The prompt seeds were picked with the CPU oracle alone, the way tests/test_hip_verify_rows.py describes: per model the first seed (1, 2, ..) whose compared greedy
steps all clear BAND — test 1: past 63 (7 steps: the row's token, the two calls, four steps), the 329-token prompt of row 2 (129 held + 200 fed; 5 steps) and the
200-token prompt of row 3 (130 + 70; 5 steps); test 2: pasts 63, 129 and the 84-token prompt (64 + 20); test 5: the 150-token prompt (100 + 50; 9 steps) — and for
the sampled row of test 1 (past 200, T 0.8 / top-p 0.9, key (977, ., 1)) the first seed at which none of the ten draws of the oracle's own trajectory lands in the
top-p band.  They are recorded in SEEDS_1 / SEEDS_2 / SEED_5 below; every test asserts the gaps again before it compares an id."""
import numpy as np
import pytest

from conftest import rel_err
from test_hip_verify_row import BAND, check_kv, kv_all, oracle_run
from tinygpt_amd import synth
from tinygpt_amd.ffi import ADV_FEED, ADV_FEED_MORE, ADV_STEP, GREEDY, SamplerCfg, TgxError
from verify_sampled_util import V, expected_draw, gpu_model, top_p_band, walk

pytestmark = pytest.mark.gpu
BLK = 128
CTX = 512
SAMPLED = SamplerCfg(0.8, 0, 0.9, 0.0)
# test 1: (past 63 greedy, past 200 sampled with row seed 977, the 329-token prompt, the 200-token prompt)
SEEDS_1 = {"llama-3.2-1b": (1, 1, 1, 1), "mistral-7b-v0.3": (1, 1, 1, 1), "gpt2": (2, 1, 1, 1)}
SEEDS_2 = (1, 1, 1)          # test 2, Llama bf16: past 63, past 129, the 84-token prompt
SEED_5 = 1                   # test 5, Llama bf16: the 150-token prompt


def assert_gaps(name, dtype, past, seed, steps):
    """the CPU oracle's top-2 gap of the first `steps` free-running greedy steps of the prompt clears BAND; returns the oracle's ids"""
    ids, gaps = oracle_run(name, dtype, past, seed)
    assert min(gaps[:steps]) >= BAND, (name, dtype, past, seed, gaps[:steps])
    return ids


def ints(a):
    return [int(t) for t in a]


def setup(m, prompts, cfgs):
    """every row holds its prompt, its settings and a current token drawn with them"""
    m.reset_cache()
    for r, p in enumerate(prompts):
        m.forward_row(r, p)
    for r, (cfg, seed) in enumerate(cfgs):
        m.set_row_sampler(r, cfg, seed)
    return [int(m.sample_row(r, cfg, seed)) for r, (cfg, seed) in enumerate(cfgs)]


def same_rows(a, b, rows, dtype, what, logits=True, b_rows=None):
    la, lb = a.logits(rounded=False), b.logits(rounded=False)
    for r, rb in zip(rows, b_rows or rows):
        if logits:
            e = rel_err(la[r][None, :], lb[rb][None, :])
            print(what, "row", r, "logits rel_err", e)
            assert e < 1e-3, (what, r, e)
        assert a.past_length_row(r) == b.past_length_row(rb), (what, r)
        check_kv(kv_all(a, r), kv_all(b, rb), dtype, (what, r))


def bits_equal(a, b, rows, what, logits=True):
    la, lb = a.logits(rounded=False), b.logits(rounded=False)
    for r in rows:
        if logits:
            np.testing.assert_array_equal(la[r], lb[r], err_msg=str((what, r)))
        assert a.past_length_row(r) == b.past_length_row(r), (what, r)
        for (k1, v1), (k2, v2) in zip(kv_all(a, r), kv_all(b, r)):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)


def sampled_check(cfg, seed, row, past, L, got, draft, what):
    """every produced id of a sampled STEP row is the draw of the call's own pass logits L [positions][V] with the key (seed, past + i + 1, row); returns the
    compared draws that lie inside the top-p band"""
    draws = [expected_draw(cfg, L[i], seed, past + i + 1, row)[0] for i in range(L.shape[0])]
    assert ints(got) == walk(draws, draft), (what, ints(got), draws, draft)
    return sum(int(draws[i] in top_p_band(cfg, L[i])) for i in range(len(got)))


def case1(name):
    """test 1's rows: prompts, settings, and the pieces fed by the two calls"""
    s = SEEDS_1[name]
    p2, p3 = synth.synth_prompt(V, 329, s[2]), synth.synth_prompt(V, 200, s[3])
    prompts = [synth.synth_prompt(V, 63, s[0]), synth.synth_prompt(V, 200, s[1]), p2[:129]]
    cfgs = [(GREEDY, 0), (SAMPLED, 977), (GREEDY, 0)]
    return prompts, cfgs, ints(p2[129:]), ints(p3[:130]), ints(p3[130:]), p3


def call1(m, draft, feed2, more3):
    return m.advance_rows([0, 1, 2, 3], [ADV_STEP, ADV_STEP, ADV_FEED, ADV_FEED_MORE], [[], draft, feed2, more3])


@pytest.mark.parametrize("name,dtype", [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16"), ("gpt2", "bf16")])
@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("tiles", [0, 1])
def test_joint_equals_piecewise_tiled(name, dtype, paged, tiles, oracle_lib):
    """call 1 (M = 339, the tiled route): row 0 STEP with no draft at past 63; row 1 STEP with 7 drafts, the first wrong one at index 3, sampled, at past 200; row 2
    FEED of 200 ids at past 129 (two query blocks, keys to 329, across the page at 256); row 3 FEED_MORE of 130 ids into a new row (query block 1 holds two
    queries).  Call 2: row 3 FEED of the 70 that remain, rows 0 and 1 STEP again.  Twin B makes the equivalent calls; twin C admits row 3's 200 ids at once"""
    budget = 4 * CTX if paged else 0
    A, B, C = (gpu_model(name, dtype, 4, budget, CTX) for _ in range(3))
    A.advance_attn_tiles = tiles
    assert A.advance_attn_tiles == tiles and A.advance_last_form == 0
    prompts, cfgs, feed2, more3, rest3, p3 = case1(name)
    s = SEEDS_1[name]
    o0 = assert_gaps(name, dtype, 63, s[0], 7)
    o2 = assert_gaps(name, dtype, 329, s[2], 5)
    o3 = assert_gaps(name, dtype, 200, s[3], 5)
    t0 = setup(A, prompts, cfgs)
    cont = A.decode_rows(8)[0]                                            # row 1's true continuation under its own settings
    draft = ints(cont[:7, 1])
    draft[3] = (draft[3] + 1) % V
    assert setup(A, prompts, cfgs) == t0 and setup(B, prompts, cfgs) == t0
    assert t0[0] == o0[0]
    what = (name, dtype, paged, tiles)
    # ---- call 1
    got = call1(A, draft, feed2, more3)
    assert A.advance_last_form == 1 and A.get_option("advance.last_tiles") == tiles
    L = A.pass_logits()
    assert L.shape == (9, V)
    ref = B.verify_rows([0, 1], [[], draft])
    B.extend_row(2, feed2); B.forward_row(3, more3)
    for r in (0, 1):
        assert len(got[r][0]) == len(ref[r][0]) and got[r][1] == ref[r][1] == 0, (what, r, got[r], ref[r])
    assert [(len(i), f) for i, f in got[2:]] == [(0, 0), (0, 0)]
    assert [A.past_length_row(r) for r in range(4)] == [64, 200 + len(got[1][0]), 329, 130]
    assert A.get_option("kv.free_tokens") == B.get_option("kv.free_tokens")
    same_rows(A, B, (0, 1, 2), dtype, what)
    same_rows(A, B, (3,), dtype, what, logits=False)                      # FEED_MORE: no logits, the cache rows
    assert ints(got[0][0]) == ints(ref[0][0]) == o0[1:2], (what, got[0], ref[0], o0[:2])
    band = sampled_check(SAMPLED, 977, 1, 200, L[1:9], got[1][0], draft, what)
    assert len(got[1][0]) == 4                                            # three right drafts and the row's own draw at the wrong one
    la = A.logits(rounded=False)
    np.testing.assert_array_equal(la[0], L[0])                            # a STEP row's slot: its producing position's row, bit for bit
    np.testing.assert_array_equal(la[1], L[1 + len(got[1][0]) - 1])
    # ---- call 2
    got2 = A.advance_rows([3, 0, 1], [ADV_FEED, ADV_STEP, ADV_STEP], [rest3, [], []])
    assert A.advance_last_form == 1
    L2 = A.pass_logits()
    assert L2.shape == (2, V)
    B.extend_row(3, rest3)
    ref2 = B.verify_rows([0, 1], [[], []])
    assert (len(got2[0][0]), got2[0][1]) == (0, 0)
    assert ints(got2[1][0]) == ints(ref2[0][0]) == o0[2:3] and got2[1][1] == ref2[0][1] == 0, (what, got2[1], ref2[0], o0[:3])
    assert len(got2[2][0]) == len(ref2[1][0]) == 1
    band += sampled_check(SAMPLED, 977, 1, 204, L2[1:2], got2[2][0], [], what)
    assert band == 0, band
    assert [A.past_length_row(r) for r in range(4)] == [65, 205, 329, 200]
    assert A.get_option("kv.free_tokens") == B.get_option("kv.free_tokens")
    same_rows(A, B, range(4), dtype, what + ("call 2",))
    la = A.logits(rounded=False)
    np.testing.assert_array_equal(la[0], L2[0]); np.testing.assert_array_equal(la[1], L2[1])
    # ---- twin C: the chunking contract
    for r, p in enumerate(prompts):
        C.forward_row(r, p)
    C.forward_row(3, p3)
    same_rows(A, C, (3,), dtype, what + ("one shot",))
    # ---- then four steps on A and B: the fed rows take their first token
    for m in (A, B):
        assert [int(m.sample_row(r, GREEDY)) for r in (2, 3)] == [o2[0], o3[0]], what
    oa, ob = A.decode_rows(4)[0], B.decode_rows(4)[0]
    same_rows(A, B, range(4), dtype, what + ("steps",))
    np.testing.assert_array_equal(oa[:, [0, 2, 3]], ob[:, [0, 2, 3]])
    assert ints(oa[:, 0]) == o0[3:7] and ints(oa[:, 2]) == o2[1:5] and ints(oa[:, 3]) == o3[1:5], (what, oa.T, o0[3:7], o2[1:5], o3[1:5])
    A.close(); B.close(); C.close()


def llama(max_batch, budget=0, dtype="bf16"):
    return gpu_model("llama-3.2-1b", dtype, max_batch, budget, CTX)


def case2():
    p2 = synth.synth_prompt(V, 84, SEEDS_2[2])
    prompts = [synth.synth_prompt(V, 63, SEEDS_2[0]), synth.synth_prompt(V, 129, SEEDS_2[1]), p2[:64]]
    return prompts, ints(p2[64:]), ints(synth.synth_prompt(V, 9, 5))


@pytest.mark.parametrize("paged", [0, 1])
def test_skinny_route(paged, oracle_lib):
    """M = 34: STEP with 0 and with 3 (right) drafts, FEED of 20 at past 64, FEED_MORE of 9 into the new row 3 (row == batch)"""
    name, dtype = "llama-3.2-1b", "bf16"
    budget = 4 * CTX if paged else 0
    A, B = llama(4, budget), llama(4, budget)
    prompts, feed2, more3 = case2()
    o0 = assert_gaps(name, dtype, 63, SEEDS_2[0], 2)
    o1 = assert_gaps(name, dtype, 129, SEEDS_2[1], 5)
    o2 = assert_gaps(name, dtype, 84, SEEDS_2[2], 1)
    for m in (A, B):
        assert setup(m, prompts, [(GREEDY, 0)] * 3)[:2] == [o0[0], o1[0]]
    draft = o1[1:4]
    got = A.advance_rows([0, 1, 2, 3], [ADV_STEP, ADV_STEP, ADV_FEED, ADV_FEED_MORE], [[], draft, feed2, more3])
    assert A.advance_last_form == 1
    L = A.pass_logits()
    assert L.shape == (5, V)
    ref = B.verify_rows([0, 1], [[], draft])
    B.extend_row(2, feed2); B.forward_row(3, more3)
    assert ints(got[0][0]) == ints(ref[0][0]) == o0[1:2] and ints(got[1][0]) == ints(ref[1][0]) == o1[1:5], (got, ref, o0[:2], o1[:5])
    assert [g[1] for g in got] == [0, 0, 0, 0] and [len(g[0]) for g in got[2:]] == [0, 0]
    assert [A.past_length_row(r) for r in range(4)] == [64, 133, 84, 9]
    assert A.get_option("kv.free_tokens") == B.get_option("kv.free_tokens")
    same_rows(A, B, (0, 1, 2), dtype, ("skinny", paged))
    same_rows(A, B, (3,), dtype, ("skinny", paged), logits=False)
    la = A.logits(rounded=False)
    np.testing.assert_array_equal(la[0], L[0]); np.testing.assert_array_equal(la[1], L[4])
    assert int(A.sample_row(2, GREEDY)) == int(B.sample_row(2, GREEDY)) == o2[0]
    A.close(); B.close()


@pytest.mark.parametrize("dtype,mfma", [("fp32", 1), ("bf16", 0)])
def test_piecewise_forms(dtype, mfma):
    """fp32 storage, and prefill.mfma 0: advance.last_form 2, and every row ends bit for bit as the one-after-another calls leave it in a twin"""
    A, B = llama(4, 0, dtype), llama(4, 0, dtype)
    prompts, feed2, more3 = case2()
    cfgs = [(GREEDY, 0), (SAMPLED, 8), (GREEDY, 0)]
    for m in (A, B):
        m.set_option("prefill.mfma", mfma)
        setup(m, prompts, cfgs)
    drafts = [[], [9, 8, 7]]
    got = A.advance_rows([2, 0, 3, 1], [ADV_FEED, ADV_STEP, ADV_FEED_MORE, ADV_STEP], [feed2, drafts[0], more3, drafts[1]])
    assert A.advance_last_form == 2
    ref = B.verify_rows([0, 1], drafts)
    np.testing.assert_array_equal(A.pass_logits(), B.pass_logits())
    B.extend_row(2, feed2); B.forward_row(3, more3)
    assert [(ints(i), f) for i, f in (got[1], got[3])] == [(ints(i), f) for i, f in ref]
    assert [(len(i), f) for i, f in (got[0], got[2])] == [(0, 0), (0, 0)]
    bits_equal(A, B, (0, 1, 2), "piecewise")
    bits_equal(A, B, (3,), "piecewise", logits=False)
    with pytest.raises(TgxError) as ei:                                   # the FEED_MORE row is in the no-logits state here as well
        A.sample_row(3, GREEDY)
    assert ei.value.status == 4
    A.close(); B.close()


@pytest.mark.parametrize("paged", [0, 1])
def test_bystanders_keep_their_bits(paged):
    """rows 0 and 2 are live and not named, a FEED goes into row 1 between them and row 3 steps: logits, cache rows and length of the bystanders as in a twin that
    made no call; the next step of both gives the same ids and bits for them"""
    budget = 4 * CTX if paged else 0
    A, T = llama(4, budget), llama(4, budget)
    prompts = [synth.synth_prompt(V, p, 40 + r) for r, p in enumerate((50, 63, 330, 64))]      # (row 2 stays the longest row: the step's forms are the twin's)
    cfgs = [(GREEDY, 0), (GREEDY, 0), (SAMPLED, 5), (SAMPLED, 6)]
    for m in (A, T):
        setup(m, prompts, cfgs)
    got = A.advance_rows([1, 3], [ADV_FEED, ADV_STEP], [ints(synth.synth_prompt(V, 140, 7)), [1, 2, 3, 4, 5]])
    assert A.advance_last_form == 1
    assert [A.past_length_row(r) for r in range(4)] == [50, 203, 330, 64 + len(got[1][0])]
    bits_equal(A, T, (0, 2), "bystanders")
    A.sample_row(1, GREEDY)
    oa, ot = A.decode_rows(1)[0], T.decode_rows(1)[0]
    np.testing.assert_array_equal(oa[:, [0, 2]], ot[:, [0, 2]])
    bits_equal(A, T, (0, 2), "bystanders after a step")
    A.close(); T.close()


def refused(m, status, fn):
    with pytest.raises(TgxError) as ei:
        fn()
    assert ei.value.status == status, (status, str(ei.value))


def test_row_states(oracle_lib):
    name, dtype = "llama-3.2-1b", "bf16"
    o = assert_gaps(name, dtype, 150, SEED_5, 9)
    prompt = ints(synth.synth_prompt(V, 150, SEED_5))
    m, T = llama(4, 8 * BLK), llama(4, 8 * BLK)
    p0 = synth.synth_prompt(V, 40, 3)
    t0 = setup(m, [p0], [(GREEDY, 0)])
    cont = m.decode_rows(3)[0]
    assert int(cont[0, 0]) != int(cont[1, 0])
    assert setup(m, [p0], [(GREEDY, 0)]) == t0
    m.set_row_stop(0, 0, [int(cont[1, 0])])
    _, new, fin = m.decode_rows(3)
    assert (int(new[0]), int(fin[0])) == (2, 1) and m.past_length_row(0) == 42      # row 0 finished on its stop id
    # a FEED on the finished row clears the state; FEED_MORE admits the first 100 ids into the new row 1
    got = m.advance_rows([0, 1], [ADV_FEED, ADV_FEED_MORE], [[5, 6, 7], prompt[:100]])
    assert m.advance_last_form == 1 and [(len(i), f) for i, f in got] == [(0, 0), (0, 0)]
    assert [m.past_length_row(r) for r in (0, 1)] == [45, 100]
    m.set_row_stop(0, 0, [])
    m.sample_row(0, GREEDY)                                               # row 0 runs again: it has logits and takes a token
    # the no-logits state of row 1
    refused(m, 4, lambda: m.sample_row(1, GREEDY))
    refused(m, 4, lambda: m.decode_rows(1))
    refused(m, 4, lambda: m.fork_row(1, [2]))
    refused(m, 4, lambda: m.advance_rows([1], [ADV_STEP], [[]]))
    assert [m.past_length_row(r) for r in (0, 1)] == [45, 100]
    blob = m.save_row(1)                                                  # the prefix-only snapshot round-trips
    m.restore_row(2, blob)
    assert m.past_length_row(2) == 100
    for (k1, v1), (k2, v2) in zip(kv_all(m, 1), kv_all(m, 2)):
        np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    refused(m, 4, lambda: m.sample_row(2, GREEDY))
    m.reset_row(2)
    # the closing FEED: the row then samples and steps as the one-shot twin's
    m.advance_rows([1], [ADV_FEED], [prompt[100:]])
    T.forward_row(0, prompt)
    assert int(m.sample_row(1, GREEDY)) == int(T.sample_row(0, GREEDY)) == o[0]
    same_rows(m, T, (1,), dtype, "closing feed", b_rows=(0,))
    om, ot = m.decode_rows(8)[0], T.decode_rows(8)[0]
    assert ints(om[:, 1]) == ints(ot[:, 0]) == o[1:9], (om[:, 1], ot[:, 0], o[:9])
    m.close(); T.close()


def test_refusals_change_nothing():
    """each refused call leaves lengths, kv.free_tokens and the logits as they were, and the next legal call gives the results of a twin that never made the
    refused calls, bit for bit"""
    m, T = llama(6, 24 * BLK), llama(6, 24 * BLK)
    lens = (30, 31, 32, 33, 34)
    prompts = [synth.synth_prompt(V, p, 11 + r) for r, p in enumerate(lens)]
    for x in (m, T):
        setup(x, prompts, [(GREEDY, 0)] * 5)
        x.extend_row(4, [5, 6])                                           # row 4: no current token

    def state():
        return ([m.past_length_row(r) for r in range(6)], m.get_option("kv.free_tokens"), m.logits(rounded=False).copy())

    def no(status, rows, kinds, ids):
        s0 = state()
        refused(m, status, lambda: m.advance_rows(rows, kinds, ids))
        s1 = state()
        assert s0[:2] == s1[:2], (rows, kinds, s0[:2], s1[:2])
        np.testing.assert_array_equal(s0[2], s1[2])

    no(1, [0, 1], [ADV_STEP, 3], [[1], [2]])                              # a bad kind
    no(1, [0, 1, 0], [ADV_STEP, ADV_FEED, ADV_STEP], [[1], [2], [3]])     # a row named twice
    no(4, [0, 4], [ADV_STEP, ADV_STEP], [[1], [1]])                       # a STEP on a row without a token
    no(1, [0, 5], [ADV_STEP, ADV_FEED], [[1], [1, 2, V]])                 # a FEED id out of range in the last row of the array
    m.sample_row(4, GREEDY); T.sample_row(4, GREEDY)
    no(1, [0, 1, 2, 3, 4], [ADV_STEP] * 5, [[1] * 12] * 5)                # 65 STEP positions
    no(1, [0, 5], [ADV_FEED, ADV_FEED], [[1] * 4097, [1] * 4096])         # 8193 positions
    no(8, [0, 1], [ADV_STEP, ADV_FEED], [[1], [1] * (CTX - 30)])          # past + len > max_ctx
    m.set_row_penalties(2, repetition=1.3)
    no(2, [0, 2], [ADV_STEP, ADV_STEP], [[1], [1]])                       # a STEP row with a penalty on
    m.set_row_penalties(2)
    args = ([0, 5, 1], [ADV_STEP, ADV_FEED_MORE, ADV_FEED], [[1, 2], ints(synth.synth_prompt(V, 40, 9)), [7, 8, 9]])
    gm, gt = m.advance_rows(*args), T.advance_rows(*args)
    assert [(ints(i), f) for i, f in gm] == [(ints(i), f) for i, f in gt]
    assert m.get_option("kv.free_tokens") == T.get_option("kv.free_tokens")
    np.testing.assert_array_equal(m.pass_logits(), T.pass_logits())
    bits_equal(m, T, (0, 1, 2, 3, 4), "after the refusals")
    bits_equal(m, T, (5,), "after the refusals", logits=False)
    m.close(); T.close()
    # a paged cache: two rows whose blocks fit separately but not together
    p = llama(2, 3 * BLK)
    setup(p, [synth.synth_prompt(V, 126, 3), synth.synth_prompt(V, 126, 4)], [(GREEDY, 0)] * 2)
    assert p.get_option("kv.free_tokens") == BLK
    s0 = ([p.past_length_row(r) for r in range(2)], p.logits(rounded=False).copy())
    refused(p, 8, lambda: p.advance_rows([0, 1], [ADV_STEP, ADV_FEED], [[1, 2, 3], [4, 5, 6]]))      # each reaches position 129: one more block each, one is free
    assert p.get_option("kv.free_tokens") == BLK and s0[0] == [p.past_length_row(r) for r in range(2)]
    np.testing.assert_array_equal(s0[1], p.logits(rounded=False))
    ids, fin = p.advance_rows([0], [ADV_STEP], [[1, 2, 3]])[0]            # separately each fits (a wrong draft: the extra block comes back)
    assert 1 <= len(ids) <= 2 and p.get_option("kv.free_tokens") == BLK
    p.advance_rows([1], [ADV_FEED], [[4, 5, 6]])
    assert p.past_length_row(1) == 129 and p.get_option("kv.free_tokens") == 0
    p.close()


def test_which_refusal_wins():
    """calls that break two rules: the status and the message of the refusal that comes first, and lengths and kv.free_tokens as they were"""
    m = llama(7, 24 * BLK)
    prompts = [synth.synth_prompt(V, p, 11 + r) for r, p in enumerate((30, 31, 32, 33, 34))]
    setup(m, prompts, [(GREEDY, 0)] * 5)
    m.extend_row(4, [5, 6])                                               # row 4: no current token; rows 5 and 6 are new

    def no(x, status, text, rows, kinds, ids):
        s0 = ([x.past_length_row(r) for r in range(x.desc.max_batch)], x.get_option("kv.free_tokens"))
        with pytest.raises(TgxError) as ei:
            x.advance_rows(rows, kinds, ids)
        assert ei.value.status == status and text in str(ei.value), (status, text, str(ei.value))
        assert s0 == ([x.past_length_row(r) for r in range(x.desc.max_batch)], x.get_option("kv.free_tokens")), (rows, kinds)

    no(m, 1, "kinds[1] = 3", [4, 0], [ADV_STEP, 3], [[1], [2]])             # the call's own checks come before any row's
    no(m, 1, "65 step positions", [0, 1, 2, 3, 4], [ADV_STEP] * 5, [[1] * 12] * 5)
    no(m, 4, "row 4 has no current token", [4, 0], [ADV_STEP, ADV_FEED], [[1], [1, V]])      # the rows in array order
    no(m, 1, "token id out of range", [0, 4], [ADV_FEED, ADV_STEP], [[1, V], [1]])
    no(m, 8, "context size exceeded: row 1", [1, 6], [ADV_FEED, ADV_FEED], [[1] * (CTX - 30), [1, 2]])      # the rows' checks come before the new rows' order
    no(m, 1, "the new rows of a call must be 5..5", [6], [ADV_FEED], [[1, 2]])
    m.close()
    prompts = [synth.synth_prompt(V, 126, 3), synth.synth_prompt(V, 126, 4)]
    p = llama(2, 3 * BLK)                                                 # paged: one block free, each row would take one
    setup(p, prompts, [(GREEDY, 0)] * 2)
    p.set_row_penalties(1, repetition=1.3)
    no(p, 2, "row 1 has a logit processor on", [0, 1], [ADV_STEP, ADV_STEP], [[1, 2, 3], [4, 5, 6]])      # the budget is checked last
    p.set_row_penalties(1)
    no(p, 8, "1 free or held by its admissions' rows of", [0, 1], [ADV_STEP, ADV_STEP], [[1, 2, 3], [4, 5, 6]])
    p.close()


def test_same_bits_from_run_to_run():
    """test 1's call 1 on two fresh contexts with advance.attn_tiles 1 (every query block of more than one key tile split and merged)"""
    name = "llama-3.2-1b"
    prompts, cfgs, feed2, more3, _, _ = case1(name)
    outs = []
    for _ in range(2):
        m = llama(4)
        m.advance_attn_tiles = 1
        setup(m, prompts, cfgs)
        got = call1(m, [1, 2, 3, 4, 5, 6, 7], feed2, more3)
        assert m.advance_last_form == 1 and m.get_option("advance.last_tiles") == 1
        outs.append(([(ints(i), f) for i, f in got], m.pass_logits(), m.logits(rounded=False)[:3].copy(), [kv_all(m, r) for r in range(4)]))
        m.close()
    x, y = outs
    assert x[0] == y[0]
    np.testing.assert_array_equal(x[1], y[1]); np.testing.assert_array_equal(x[2], y[2])
    for ka, kb in zip(x[3], y[3]):
        for (k1, v1), (k2, v2) in zip(ka, kb):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
