"""tgx_verify_rows (include/tgx.h): the drafts of several rows verified in ONE joint pass and ONE accept launch.  The contract is "equal to n calls of
tgx_verify_row_sampled in array order, up to the order of the fp32 sums", with the project's numbers: GPU against GPU rel_err < 1e-3 (tests/test_hip_verify_row.py),
live cache rows by that file's check_kv, greedy ids equal where the CPU oracle's top-2 gap clears that file's BAND (asserted, so no id comparison is skipped), sampled
ids restated from the call's OWN pass logits with the row's key (tests/test_hip_verify_sampled.py: expected_draw, the top-p band's exclusion, its cap of 0 positions).
Every context is a 2-layer cut of tests/verify_sampled_util.py (vocabulary 4096, max_batch 4 - 6, max_ctx 512).

The prompt seeds of test 1 were picked with the CPU oracle alone: per model the first seed whose greedy steps all clear BAND (pasts 63 and 129), and for the sampled
rows (pasts 64 and 200, T 0.8 / top-p 0.9, keys (11, ., 1) and (977, ., 3)) the first seed at which no draw of the oracle's own trajectory lands in the top-p band:
seed 1 everywhere but GPT-2 at past 63 (2).  A row with n_draft 0 has no one-row verify call to compare with: its twin takes tgx_extend_row of the current token and
tgx_sample_row, which is what one step is."""
import numpy as np
import pytest

from conftest import rel_err
from test_hip_verify_row import BAND, SEEDS, check_kv, kv_all, oracle_run
from tinygpt_amd import synth
from tinygpt_amd.ffi import GREEDY, SamplerCfg, TgxError
from verify_sampled_util import V, expected_draw, gpu_model, top_p_band, walk

pytestmark = pytest.mark.gpu
BLK = 128
CTX = 512
SAMPLED = SamplerCfg(0.8, 0, 0.9, 0.0)
PASTS = [63, 64, 129, 200]           # a key-tile boundary, a page boundary, several tiles
N_DRAFT = [0, 1, 7, 15]              # M = 27
CFGS = [(GREEDY, 0), (SAMPLED, 11), (GREEDY, 0), (SAMPLED, 977)]      # (settings, row seed) of rows 0 .. 3
WRONG = [None, 0, None, 7]           # the first wrong draft index: acceptance none (row 1), all (row 2), part-way (row 3)
PROMPT_SEEDS = {"llama-3.2-1b": [1, 1, 1, 1], "mistral-7b-v0.3": [1, 1, 1, 1], "gpt2": [2, 1, 1, 1]}
FIRST = [0, 1, 3, 11]                # row i's slice of the pass: sum of the M_j before it


def wrong_at(ids, j):
    d = [int(t) for t in ids]
    if j is not None:
        d[j] = (d[j] + 1) % V
    return d


def setup(m, prompts, cfgs):
    """every row holds its prompt, its settings and a current token drawn with them"""
    m.reset_cache()
    for r, p in enumerate(prompts):
        m.forward_row(r, p)
    for r, (cfg, seed) in enumerate(cfgs):
        m.set_row_sampler(r, cfg, seed)
    return [int(m.sample_row(r, cfg, seed)) for r, (cfg, seed) in enumerate(cfgs)]


def assert_gaps(name, dtype, past, seed, steps):
    """the CPU oracle's top-2 gap of the first `steps` free-running greedy steps of the prompt clears BAND; returns the oracle's ids"""
    ids, gaps = oracle_run(name, dtype, past, seed)
    assert min(gaps[:steps]) >= BAND, (name, dtype, past, seed, gaps[:steps])
    return ids


def twin_step_row(m, row, t0):
    """one greedy step of ONE row of the twin: the input t0 through the row's own pass, then its token"""
    m.extend_row(row, [t0])
    return [int(m.sample_row(row, GREEDY))]


def same_rows(a, b, rows, dtype, what):
    la, lb = a.logits(rounded=False), b.logits(rounded=False)
    for r in rows:
        e = rel_err(la[r][None, :], lb[r][None, :])
        print(what, "row", r, "logits rel_err", e)
        assert e < 1e-3, (what, r, e)
        assert a.past_length_row(r) == b.past_length_row(r), (what, r)
        check_kv(kv_all(a, r), kv_all(b, r), dtype, (what, r))


@pytest.mark.parametrize("name,dtype", [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16"), ("gpt2", "bf16")])
@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("splits", [0, 3])
def test_joint_equals_row_by_row(name, dtype, paged, splits, oracle_lib):
    budget = 4 * CTX if paged else 0
    A, B = gpu_model(name, dtype, 4, budget, CTX), gpu_model(name, dtype, 4, budget, CTX)
    for m in (A, B):
        m.set_option("extend.attn_splits", splits)
    prompts = [synth.synth_prompt(V, p, s) for p, s in zip(PASTS, PROMPT_SEEDS[name])]
    # the greedy rows' compared steps all clear BAND on the oracle: t0, the call's tokens, four steps
    o0 = assert_gaps(name, dtype, PASTS[0], PROMPT_SEEDS[name][0], 1 + 1 + 4)
    o2 = assert_gaps(name, dtype, PASTS[2], PROMPT_SEEDS[name][2], 1 + 8 + 4)
    t0 = setup(A, prompts, CFGS)
    cont = A.decode_rows(15)[0]                                           # every row's true continuation under its own settings
    drafts = [wrong_at(cont[:n, r], j) for r, (n, j) in enumerate(zip(N_DRAFT, WRONG))]
    assert setup(A, prompts, CFGS) == t0 and setup(B, prompts, CFGS) == t0
    assert t0[0] == o0[0] and t0[2] == o2[0]
    got = A.verify_rows([0, 1, 2, 3], drafts)
    assert A.get_option("verify.last_form") == 1
    L = A.pass_logits()
    assert L.shape == (27, V)
    ref = [(twin_step_row(B, 0, t0[0]), 0)] + [B.verify_row_sampled(r, drafts[r]) for r in (1, 2, 3)]
    what = (name, dtype, paged, splits)
    for r in range(4):
        assert len(got[r][0]) == len(ref[r][0]) and got[r][1] == ref[r][1] == 0, (what, r, got[r], ref[r])
    assert A.get_option("kv.free_tokens") == B.get_option("kv.free_tokens")
    same_rows(A, B, range(4), dtype, what)
    # greedy rows: equal ids (and the oracle's); row 2's right draft is accepted whole
    assert list(got[0][0]) == list(ref[0][0]) == o0[1:2], (what, got[0], ref[0], o0[:2])
    assert list(got[2][0]) == list(ref[2][0]) == o2[1:9], (what, got[2], ref[2], o2[:9])
    # sampled rows: every produced id is the draw of the call's own pass logits with the row's key; no expected draw inside the top-p band
    band = 0
    for r in (1, 3):
        cfg, seed = CFGS[r]
        Lr = L[FIRST[r]:FIRST[r] + N_DRAFT[r] + 1]
        draws = [expected_draw(cfg, Lr[i], seed, PASTS[r] + i + 1, r)[0] for i in range(Lr.shape[0])]
        band += sum(int(draws[i] in top_p_band(cfg, Lr[i])) for i in range(Lr.shape[0]))
        assert list(got[r][0]) == walk(draws, drafts[r]), (what, r, list(got[r][0]), draws, drafts[r])
        np.testing.assert_array_equal(A.logits(rounded=False)[r], Lr[len(got[r][0]) - 1])      # the slot: the producing position's row, bit for bit
    assert band == 0, band
    assert len(got[1][0]) == 1                                            # draft[0] is not the draw: nothing accepted
    # then four steps on both contexts
    oa, ob = A.decode_rows(4)[0], B.decode_rows(4)[0]
    same_rows(A, B, range(4), dtype, what + ("steps",))
    np.testing.assert_array_equal(oa[:, [0, 2]], ob[:, [0, 2]])
    assert [int(t) for t in oa[:, 0]] == o0[2:6] and [int(t) for t in oa[:, 2]] == o2[9:13], (what, oa[:, [0, 2]].T, o0[2:6], o2[9:13])
    A.close(); B.close()


def llama(max_batch, budget=0):
    return gpu_model("llama-3.2-1b", "bf16", max_batch, budget, CTX)


def bits_equal(a, b, rows, what):
    la, lb = a.logits(rounded=False), b.logits(rounded=False)
    for r in rows:
        np.testing.assert_array_equal(la[r], lb[r], err_msg=str((what, r)))
        assert a.past_length_row(r) == b.past_length_row(r), (what, r)
        for (k1, v1), (k2, v2) in zip(kv_all(a, r), kv_all(b, r)):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)


@pytest.mark.parametrize("paged", [0, 1])
def test_bystanders_keep_their_bits(paged):
    """rows 0 and 2 are live and not named: logits, cache rows and length as in a twin that made no call; the next step of both gives the same ids and bits for
    them (the token and position words were not touched, the rows have not stepped)"""
    budget = 4 * CTX if paged else 0
    A, T = llama(4, budget), llama(4, budget)
    prompts = [synth.synth_prompt(V, p, 40 + r) for r, p in enumerate((50, 63, 130, 64))]
    cfgs = [(GREEDY, 0), (GREEDY, 0), (SAMPLED, 5), (SAMPLED, 6)]
    for m in (A, T):
        setup(m, prompts, cfgs)
    got = A.verify_rows([3, 1], [[1, 2, 3, 4, 5], [7, 8, 9]])
    assert A.get_option("verify.last_form") == 1
    assert [A.past_length_row(r) for r in range(4)] == [50, 63 + len(got[1][0]), 130, 64 + len(got[0][0])]
    bits_equal(A, T, (0, 2), "bystanders")
    oa, ot = A.decode_rows(1)[0], T.decode_rows(1)[0]
    np.testing.assert_array_equal(oa[:, [0, 2]], ot[:, [0, 2]])
    bits_equal(A, T, (0, 2), "bystanders after a step")
    A.close(); T.close()


def test_all_n_draft_zero_is_one_step(oracle_lib):
    name, dtype = "llama-3.2-1b", "bf16"
    pasts = [63, 129, 5, 126]
    seeds = [1, 1, SEEDS[(name, dtype, 5)], SEEDS[(name, dtype, 126)]]
    want = [assert_gaps(name, dtype, p, s, 2) for p, s in zip(pasts, seeds)]
    A, T = llama(4), llama(4)
    prompts = [synth.synth_prompt(V, p, s) for p, s in zip(pasts, seeds)]
    for m in (A, T):
        assert setup(m, prompts, [(GREEDY, 0)] * 4) == [w[0] for w in want]
    got = A.verify_rows([0, 1, 2, 3], [[], [], [], []])
    assert A.pass_logits().shape == (4, V)
    ot, _, _ = T.decode_rows(1)
    for r in range(4):
        assert got[r][1] == 0 and list(got[r][0]) == [int(ot[0, r])] == want[r][1:2], (r, got[r], ot[0, r], want[r][:2])
    same_rows(A, T, range(4), dtype, "n_draft 0")
    oa, ot = A.decode_rows(1)[0], T.decode_rows(1)[0]                      # ... and both go on alike
    same_rows(A, T, range(4), dtype, "n_draft 0, next step")
    A.close(); T.close()


def test_stop_conditions_per_row():
    m = llama(4, 4 * CTX)
    prompts = [synth.synth_prompt(V, p, 70 + r) for r, p in enumerate((40, 63, 100))]
    cfgs = [(GREEDY, 0)] * 3
    t0 = setup(m, prompts, cfgs)
    cont = m.decode_rows(7)[0]
    assert len(set(int(t) for t in cont[:3, 1])) == 3
    assert setup(m, prompts, cfgs) == t0
    m.set_row_stop(0, 3, [])                                              # max_new inside the accepted prefix
    m.set_row_stop(1, 0, [int(cont[2, 1])])                               # a stop id at accepted index 2
    got = m.verify_rows([0, 1, 2], [[int(t) for t in cont[:7, r]] for r in range(3)])
    assert m.get_option("verify.last_form") == 1
    assert (list(got[0][0]), got[0][1]) == ([int(t) for t in cont[:3, 0]], 2)
    assert (list(got[1][0]), got[1][1]) == ([int(t) for t in cont[:3, 1]], 1)
    assert got[2][1] == 0 and len(got[2][0]) == 8 and list(got[2][0][:7]) == [int(t) for t in cont[:7, 2]]      # the third row runs on
    assert [m.past_length_row(r) for r in range(3)] == [43, 66, 100 + len(got[2][0])]
    # a later call naming a finished row: TGX_ERR_STATE, nothing changes (the running row named beside it included)
    s0 = ([m.past_length_row(r) for r in range(3)], m.get_option("kv.free_tokens"), m.logits(rounded=False).copy())
    with pytest.raises(TgxError) as ei:
        m.verify_rows([2, 0], [[1, 2], [3]])
    assert ei.value.status == 4
    assert s0[0] == [m.past_length_row(r) for r in range(3)] and s0[1] == m.get_option("kv.free_tokens")
    np.testing.assert_array_equal(s0[2], m.logits(rounded=False))
    got = m.verify_rows([2], [[1, 2]])                                    # the running row alone goes on
    assert got[0][1] == 0 and len(got[0][0]) >= 1
    m.close()


def test_every_refusal_changes_nothing():
    m = llama(6)
    lens = (30, 31, 32, 33, CTX - 4)
    prompts = [synth.synth_prompt(V, p, 11 + r) for r, p in enumerate(lens)]
    setup(m, prompts, [(GREEDY, 0)] * 5)

    def state():
        return ([m.past_length_row(r) for r in range(5)], m.get_option("kv.free_tokens"), m.get_option("mem.live_kib"), m.logits(rounded=False).copy())

    def refused(status, rows, drafts):
        s0 = state()
        with pytest.raises(TgxError) as ei:
            m.verify_rows(rows, drafts)
        assert ei.value.status == status, (status, rows, str(ei.value))
        s1 = state()
        assert s0[:3] == s1[:3], (rows, s0[:3], s1[:3])
        np.testing.assert_array_equal(s0[3], s1[3])

    refused(1, [0, 1, 0], [[1], [2], [3]])                                # a row named twice
    refused(1, [0, 1, 2, 3, 4], [[1] * 15] * 4 + [[]])                    # M = 65
    refused(1, [0], [[1] * 16])                                           # n_draft 16
    refused(1, [0, 6], [[1], [1]]); refused(1, [-1], [[1]])               # a row out of range
    refused(1, [0], [[V]])                                                # a draft id out of range
    refused(1, [], [])                                                    # n < 1
    refused(8, [0, 4], [[1], [1, 2, 3, 4]])                               # past + M_i > max_ctx
    refused(4, [0, 5], [[1], [1]])                                        # an empty row
    m.extend_row(1, [5, 6])
    refused(4, [0, 1], [[1], [1]])                                        # a row without a current token
    m.sample_row(1, GREEDY)
    m.set_row_penalties(2, repetition=1.3)
    refused(2, [0, 2], [[1], [1]])                                        # a logit processor on a named row
    m.set_row_penalties(2)
    got = m.verify_rows([0, 4], [[1], [1, 2, 3]])                         # past + 4 == max_ctx fits
    assert len(got) == 2 and all(len(ids) >= 1 for ids, _ in got)
    m.close()
    # a paged cache: two rows whose blocks fit separately but not together
    p = llama(2, 3 * BLK)
    setup(p, [synth.synth_prompt(V, 126, 3), synth.synth_prompt(V, 126, 4)], [(GREEDY, 0)] * 2)
    assert p.get_option("kv.free_tokens") == BLK
    s0 = ([p.past_length_row(r) for r in range(2)], p.get_option("mem.live_kib"), p.logits(rounded=False).copy())
    with pytest.raises(TgxError) as ei:
        p.verify_rows([0, 1], [[1, 2, 3], [4, 5, 6]])                     # each reaches position 129: one more block each, one is free
    assert ei.value.status == 8
    assert p.get_option("kv.free_tokens") == BLK and s0[0] == [p.past_length_row(r) for r in range(2)] and s0[1] == p.get_option("mem.live_kib")
    np.testing.assert_array_equal(s0[2], p.logits(rounded=False))
    for r in (0, 1):                                                      # separately each fits (a wrong draft: one token taken, the extra block comes back)
        ids, fin = p.verify_rows([r], [[(r + 1) % V, 2, 3]])[0]
        assert 1 <= len(ids) <= 2 and p.get_option("kv.free_tokens") == BLK
    p.close()


def test_which_refusal_wins():
    """calls that break two rules: the status and the message of the refusal that comes first, and lengths and kv.free_tokens as they were"""
    m = llama(6, 24 * BLK)
    prompts = [synth.synth_prompt(V, p, 11 + r) for r, p in enumerate((30, 31, 32, 33, 34))]
    setup(m, prompts, [(GREEDY, 0)] * 5)
    m.extend_row(4, [5, 6])                                               # row 4: no current token

    def no(status, text, rows, drafts):
        s0 = ([m.past_length_row(r) for r in range(6)], m.get_option("kv.free_tokens"))
        with pytest.raises(TgxError) as ei:
            m.verify_rows(rows, drafts)
        assert ei.value.status == status and text in str(ei.value), (status, text, str(ei.value))
        assert s0 == ([m.past_length_row(r) for r in range(6)], m.get_option("kv.free_tokens")), rows

    no(4, "row 4 has no current token", [0, 1, 2, 3, 4], [[1] * 12] * 5)      # 65 positions: every row's checks come before the call's limit
    no(4, "row 4 has no current token", [4, 0], [[1], [1] * 16])          # the rows in array order
    no(1, "n_draft 16 out of range", [0, 4], [[1] * 16, [1]])
    no(1, "row 0 named twice", [0, 1, 0], [[1], [2], [V]])                # ahead of the second naming's own checks
    m.close()


def test_the_same_call_twice_gives_the_same_bits():
    outs = []
    prompts = [synth.synth_prompt(V, p, 90 + r) for r, p in enumerate((63, 200, 129))]
    cfgs = [(GREEDY, 0), (SAMPLED, 3), (SAMPLED, 4)]
    for _ in range(2):
        m = llama(4)
        m.set_option("extend.attn_splits", 3)
        setup(m, prompts, cfgs)
        got = m.verify_rows([0, 1, 2], [[1, 2, 3], [4, 5, 6, 7, 8, 9, 10], []])
        assert m.get_option("verify.last_form") == 1
        outs.append(([(list(i), f) for i, f in got], m.pass_logits(), m.logits(rounded=False).copy(), [kv_all(m, r) for r in range(3)]))
        m.close()
    x, y = outs
    assert x[0] == y[0]
    np.testing.assert_array_equal(x[1], y[1]); np.testing.assert_array_equal(x[2], y[2])
    for ka, kb in zip(x[3], y[3]):
        for (k1, v1), (k2, v2) in zip(ka, kb):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)


@pytest.mark.parametrize("dtype,mfma", [("fp32", 1), ("bf16", 0)])
def test_row_by_row_form(dtype, mfma):
    """fp32 storage, and prefill.mfma 0: verify.last_form 2, and each row with a draft ends bit for bit as its own tgx_verify_row_sampled call in a twin; the
    n_draft 0 row as its twin's one-row pass of the current token"""
    A, B = gpu_model("llama-3.2-1b", dtype, 4, 0, CTX), gpu_model("llama-3.2-1b", dtype, 4, 0, CTX)
    prompts = [synth.synth_prompt(V, p, 20 + r) for r, p in enumerate((63, 64, 129))]
    cfgs = [(GREEDY, 0), (SAMPLED, 8), (GREEDY, 0)]
    for m in (A, B):
        m.set_option("prefill.mfma", mfma)
        t0 = setup(m, prompts, cfgs)
    drafts = [[1, 2, 3, 4, 5, 6, 7], [9, 8, 7], []]
    got = A.verify_rows([0, 1, 2], drafts)
    assert A.get_option("verify.last_form") == 2
    L = A.pass_logits()
    assert L.shape == (8 + 4 + 1, V)
    ref = []
    for r in (0, 1):
        ref.append(B.verify_row_sampled(r, drafts[r]))
        np.testing.assert_array_equal(B.pass_logits(), L[(0, 8)[r]:(8, 12)[r]])
    ref.append((twin_step_row(B, 2, t0[2]), 0))
    for r in range(3):
        assert (list(got[r][0]), got[r][1]) == (list(ref[r][0]), ref[r][1]), (r, got[r], ref[r])
    bits_equal(A, B, (0, 1), "row by row")
    same_rows(A, B, (2,), dtype, "row by row, n_draft 0")
    A.close(); B.close()


def test_memory():
    m = llama(4)
    prompts = [synth.synth_prompt(V, p, 50 + r) for r, p in enumerate((63, 64, 129))]
    cfgs = [(GREEDY, 0), (SAMPLED, 8), (GREEDY, 0)]
    counts = []
    for _ in range(2):                                                    # prefill + decode: after the first round nothing new
        setup(m, prompts, cfgs); m.decode_rows(2)
        counts.append(m.get_option("mem.live_allocs"))
    assert counts[0] == counts[1]
    drafts = [[1, 2, 3, 4, 5, 6, 7], [9, 8, 7], []]
    setup(m, prompts, cfgs)
    m.verify_rows([0, 1, 2], drafts)
    first = m.get_option("mem.live_allocs")
    assert first > counts[1]
    setup(m, prompts, cfgs)
    m.verify_rows([0, 1, 2], drafts)
    assert m.get_option("mem.live_allocs") == first
    m.close()


def test_forked_rows_leave_the_source_alone():
    m = llama(4, 8 * BLK)
    prompt = synth.synth_prompt(V, 200, 9)                                # one full block, shared by the forks, and a tail of 72
    setup(m, [prompt], [(GREEDY, 0)])
    m.fork_row(0, [1, 2])
    free = m.get_option("kv.free_tokens")
    src_l, src_kv = m.logits(rounded=False)[0].copy(), kv_all(m, 0)
    got = m.verify_rows([1, 2], [[1, 2, 3, 4, 5, 6, 7], [11, 12, 13]])
    assert m.get_option("verify.last_form") == 1 and m.get_option("kv.free_tokens") == free
    assert m.past_length_row(0) == 200
    np.testing.assert_array_equal(m.logits(rounded=False)[0], src_l)
    for (k1, v1), (k2, v2) in zip(kv_all(m, 0), src_kv):
        np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    for r in (1, 2):                                                      # the forks still hold the source's 200 positions, the shared block included
        assert m.past_length_row(r) == 200 + len(got[r - 1][0])
        for (k1, v1), (k2, v2) in zip(kv_all(m, r), src_kv):
            np.testing.assert_array_equal(k1[:200], k2); np.testing.assert_array_equal(v1[:200], v2)
    # the two forks saw the same first input: their first produced token is the same greedy token
    assert got[0][0][0] == got[1][0][0]
    m.close()
