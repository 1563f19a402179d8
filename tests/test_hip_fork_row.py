"""tgx_fork_row (include/tgx.h): a live row copied into other rows — on a paged cache its full 128-token blocks shared by reference (a host count per block), only
the partial tail block copied; on slabs the prefix [0, past) copied — by ONE kv_fork_kernel launch (kernels/kv_fork.h) that also carries the per-row state.  Held to:
  * a fork == the same prompt admitted separately into every row, BIT for bit: lengths, logits, every cache row, and 40 steps of tgx_decode_rows afterwards
    (greedy next to T 0.8 / top-p 0.9 with distinct seeds), prompts of 5 / 128 / 200 / 1100 tokens, slabs and paged, four geometries;
  * shared blocks outlive the source row; kv.free_tokens after every call (a fork of a 300-token row into three rows costs 3 blocks, not 9; of a 256-token row none);
    prefill + fork fits a budget that four admissions do not;
  * refusals change nothing, and a tgx_forward_rows call is refused, with nothing moved, when only blocks that siblings still map could make room for it;
  * a fork mid-generation, row against row; the CPU oracle; bystander rows; tgx_write_kv refuses a shared block."""
import copy

import numpy as np
import pytest

from conftest import rel_err
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import GREEDY, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu

MODELS = [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16"), ("qwen3-1.7b", "bf16"), ("gpt2", "bf16")]
WARM = SamplerCfg(0.8, 0, 0.9, 0.0)
BLK = 128


def cut(name, dtype, max_batch, max_ctx, peaked=False):
    """the two-layer, vocabulary-4096 cut of a real geometry"""
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 2, 4096, max_ctx, max_batch
    if d.n_positions:
        d.n_positions = max(d.n_positions, max_ctx)      # GPT-2: the 1100-token prompt needs rows of the learned position table beyond the released 1024
    if peaked:
        d.tied = False                    # the peaked checkpoint's loud rows live in an untied lm_head (tinygpt_amd/synth.py)
    return d


def real(name, dtype, max_batch, max_ctx, budget=0, peaked=False):
    m = Model(cut(name, dtype, max_batch, max_ctx, peaked))
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(1234, 0.02, peaked=peaked).finalize()


def prompt(n, seed):
    return synth.synth_prompt(4096, n, seed)


def free(m):
    return m.get_option("kv.free_tokens")


def assert_same_bits(a, b, rows, what):
    """logits and every layer's cache rows of `rows`, context a against context b"""
    np.testing.assert_array_equal(a.logits(rounded=False)[rows], b.logits(rounded=False)[rows], err_msg=str(what))
    for r in rows:
        assert a.past_length_row(r) == b.past_length_row(r), (what, r)
        for layer in range(2):
            for x, y in zip(a.read_kv(r, layer), b.read_kv(r, layer)):
                np.testing.assert_array_equal(x, y, err_msg=str(what + (r, layer)))


def refused(m, status, call, rows):
    """`call` is refused with `status` and leaves kv.free_tokens, every row's length and the longest length as they were"""
    def state():
        return free(m), [m.past_length_row(r) for r in range(rows)], m.past_length
    before = state()
    with pytest.raises(TgxError) as ei:
        call()
    assert ei.value.status == status, str(ei.value)
    assert state() == before


@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("name,dtype", MODELS)
def test_fork_equals_separate_admission_bit_for_bit(name, dtype, paged):
    """context A: tgx_forward_row(0, p) + tgx_fork_row(0, [1, 2, 3]); context B: tgx_forward_row(r, p) for r = 0..3.  Right after: the same lengths, logits and cache rows
    in every row; then per-row samplers (row 0 greedy, rows 1-3 T 0.8 / top-p 0.9 with their own seeds), tgx_sample_row and 40 steps of tgx_decode_rows (128 -> 168 and
    1100 -> 1140 cross a block boundary; 5 runs by steps, 128 / 200 on the skinny or tiled route by geometry, 1100 tiled): the same ids, logits and cache rows"""
    lens = (5, 128, 200, 1100)
    ctx = max(lens) + 64
    budget = 4 * ((ctx + BLK - 1) // BLK) * BLK if paged else 0
    A, B = real(name, dtype, 4, ctx, budget), real(name, dtype, 4, ctx, budget)
    for P in lens:
        p = prompt(P, 300 + P)
        A.reset_cache(); B.reset_cache()
        A.forward_row(0, p); A.fork_row(0, [1, 2, 3])
        for r in range(4):
            B.forward_row(r, p)
        assert [A.past_length_row(r) for r in range(4)] == [P] * 4
        if paged:       # the full blocks once, a tail block per row
            assert free(A) == budget - (P // BLK + (4 if P % BLK else 0)) * BLK
        assert_same_bits(A, B, range(4), (P, "fork"))
        first = []
        for m in (A, B):
            for r in range(4):
                m.set_row_sampler(r, WARM if r else GREEDY, 100 + r)
            first.append([m.sample_row(r, WARM if r else GREEDY, seed=100 + r) for r in range(4)])
        assert first[0] == first[1]
        (ia, na, fa), (ib, nb, fb) = A.decode_rows(40), B.decode_rows(40)
        np.testing.assert_array_equal(ia, ib, err_msg=str(P))
        np.testing.assert_array_equal(na, nb)
        np.testing.assert_array_equal(fa, fb)
        assert list(na) == [40] * 4 and list(fa) == [0] * 4
        assert_same_bits(A, B, range(4), (P, "decoded"))
    A.close(); B.close()


@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("name,dtype", [MODELS[0], MODELS[2]])
def test_shared_blocks_outlive_the_source(name, dtype, paged):
    """fork, then the source row is reset and refilled with another prompt (on a paged cache the refill takes blocks from the free list: a shared block freed too early
    would be overwritten): rows 1-3 keep decoding, and the refilled row decodes, bit-identically to a control whose rows were admitted one by one"""
    budget = 12 * BLK if paged else 0
    A, B = real(name, dtype, 4, 512, budget), real(name, dtype, 4, 512, budget)
    p, q = prompt(300, 21), prompt(260, 22)
    A.forward_row(0, p); A.fork_row(0, [1, 2, 3])
    for r in range(4):
        B.forward_row(r, p)
    out = []
    for m in (A, B):
        for r in range(4):
            m.sample_row(r, GREEDY)
        ids = [m.decode(5, GREEDY).copy()]
        m.reset_row(0)
        if paged and m is A:
            assert free(m) == budget - (2 + 3) * BLK          # the source's tail block came back; the two shared blocks stay with rows 1-3
        m.forward_row(0, q); m.sample_row(0, GREEDY)
        ids.append(m.decode(40, GREEDY).copy())
        out.append(np.concatenate(ids))
    np.testing.assert_array_equal(out[0], out[1])
    assert_same_bits(A, B, range(4), ("refilled",))
    A.close(); B.close()


def test_block_accounting():
    """kv.free_tokens after every call: a 300-token admission takes 3 blocks, its fork into three rows 3 more (one tail each), tgx_reset_row of the source gives 1 back,
    of each sibling 1, of the last one the shared blocks as well; a 256-token row forks for nothing.  A 10-block budget refuses the fourth of four 380-token admissions
    (status 8) while prefill + fork fits and decodes past the next block boundary"""
    budget = 16 * BLK
    m = real("llama-3.2-1b", "bf16", 4, 512, budget)
    assert free(m) == budget
    m.forward_row(0, prompt(300, 5)); assert free(m) == budget - 3 * BLK
    m.fork_row(0, [1, 2, 3]); assert free(m) == budget - 6 * BLK
    m.reset_row(0); assert free(m) == budget - 5 * BLK
    m.reset_row(2); assert free(m) == budget - 4 * BLK
    m.reset_row(1); assert free(m) == budget - 3 * BLK
    m.reset_row(3); assert free(m) == budget
    m.forward_row(0, prompt(256, 6)); assert free(m) == budget - 2 * BLK
    m.fork_row(0, [1, 2, 3]); assert free(m) == budget - 2 * BLK
    for r in range(4):
        m.sample_row(r, GREEDY)
    m.decode(1, GREEDY); assert free(m) == budget - 6 * BLK          # every row writes position 256 into a block of its own
    m.reset_cache(); assert free(m) == budget
    m.close()
    budget = 10 * BLK
    p = prompt(380, 7)
    ctrl = real("llama-3.2-1b", "bf16", 4, 512, budget)
    for r in range(3):
        ctrl.forward_row(r, p)
    with pytest.raises(TgxError) as ei:
        ctrl.forward_row(3, p)
    assert ei.value.status == 8
    ctrl.close()
    m = real("llama-3.2-1b", "bf16", 4, 512, budget)
    m.forward_row(0, p); m.fork_row(0, [1, 2, 3])
    assert free(m) == budget - 6 * BLK
    for r in range(4):
        m.sample_row(r, GREEDY)
    ids = m.decode(8, GREEDY)                                         # 380 -> 388: a fourth block per row
    assert free(m) == 0 and [m.past_length_row(r) for r in range(4)] == [388] * 4
    assert (ids == ids[:, :1]).all()                                  # four greedy copies of one sequence
    m.close()


def test_refusals_change_nothing():
    """every refused call returns its status, leaves kv.free_tokens and every row's length as they were, and the next decode step equals, bit for bit, that of a control
    that never made the call; a retired forked row gives back its tail block only, so a tgx_forward_rows call that needs the shared blocks too is refused"""
    budget = 8 * BLK
    m, ctrl = real("llama-3.2-1b", "bf16", 6, 768, budget), real("llama-3.2-1b", "bf16", 6, 768, budget)
    for x in (m, ctrl):
        x.forward_rows([0, 1, 2, 3], [prompt(300, 1), prompt(200, 2), prompt(5, 3), prompt(20, 4)])      # 3 + 2 + 1 + 1 blocks
        for r in range(4):
            x.sample_row(r, GREEDY)
        x.reset_row(2)                                               # row 2 retired
        x.set_row_stop(1, max_new=1)
        assert x.decode_rows(2)[2][1] == 2                           # row 1 finished
    assert free(m) == 2 * BLK
    calls = [(8, 0, [2, 4, 5]),      # three tail blocks, two free
             (1, 0, []),             # n < 1
             (1, -1, [2]), (1, 6, [2]),      # source out of range
             (4, 2, [4]),            # retired source
             (4, 1, [2]),            # finished source
             (4, 4, [2]),            # a source beyond the batch holds no sequence
             (1, 0, [0]), (1, 0, [2, 0]),    # the source among the destinations
             (1, 0, [2, 2]),         # a destination named twice
             (4, 0, [3]),            # live destination
             (4, 0, [1]),            # finished destination
             (1, 0, [5]),            # a gap in the new rows (4 is next)
             (1, 0, [6]), (1, 0, [-1])]      # destination out of range
    for status, src, dst in calls:
        refused(m, status, lambda: m.fork_row(src, dst), 6)
        (ia, na, fa), (ib, nb, fb) = m.decode_rows(1), ctrl.decode_rows(1)
        np.testing.assert_array_equal(ia, ib, err_msg=str((src, dst)))
        np.testing.assert_array_equal(m.logits(rounded=False)[[0, 3]], ctrl.logits(rounded=False)[[0, 3]], err_msg=str((src, dst)))
    m.fork_row(0, [2, 4])                                            # what fits, fits: two tail blocks
    assert free(m) == 0 and m.batch == 5 and [m.past_length_row(r) for r in (2, 4)] == [m.past_length_row(0)] * 2
    m.close(); ctrl.close()
    # tgx_forward_rows on a pool that holds shared blocks.  Rows 1-3 share row 0's two full blocks; row 1 retired gives ONE block back (its tail): 3 are free.  A
    # release that ignored the counts would put the two shared blocks on the free list as well (5 free), and a 513-token prompt (5 blocks) would be admitted onto
    # blocks that rows 0, 2, 3 still read.  (No state reachable through the entry points separates admit_rows' own "blocks the target rows give back" sum from the
    # parent's: a row that may be admitted into — retired, or holding no position — has released its blocks and holds none.  What is held here is the release path.)
    m = real("llama-3.2-1b", "bf16", 4, 768, budget)
    m.forward_row(0, prompt(300, 1)); m.fork_row(0, [1, 2, 3])
    for r in range(4):
        m.sample_row(r, GREEDY)
    m.reset_row(1)
    assert free(m) == 3 * BLK
    refused(m, 8, lambda: m.forward_rows([1], [prompt(513, 9)]), 4)
    m.forward_rows([1], [prompt(380, 9)])                            # three blocks fit
    assert free(m) == 0
    for layer in range(2):                                           # ... and took none of the shared ones
        for x, y in zip(m.read_kv(0, layer), m.read_kv(2, layer)):
            np.testing.assert_array_equal(x, y)
    m.sample_row(1, GREEDY)
    ids = m.decode(3, GREEDY)
    assert (ids[:, 0] == ids[:, 2]).all() and (ids[:, 0] == ids[:, 3]).all()
    m.close()


@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("name,dtype", MODELS)
def test_fork_mid_generation(name, dtype, paged):
    """the source has decoded 10 greedy steps (it carries a current token): the destination is ready for tgx_decode at once, and 20 steps (110 -> 130, across a block
    boundary) give it the ids and logits of the source, bit for bit, row against row"""
    m = real(name, dtype, 2, 256, 4 * BLK if paged else 0)
    m.forward_row(0, prompt(100, 31)); m.sample_row(0, GREEDY)
    m.decode(10, GREEDY)
    m.fork_row(0, [1])
    assert m.past_length_row(1) == 110
    lg = m.logits(rounded=False)
    np.testing.assert_array_equal(lg[0], lg[1])
    for step in range(20):
        ids = m.decode(1, GREEDY)
        lg = m.logits(rounded=False)
        assert ids[0, 0] == ids[0, 1], step
        np.testing.assert_array_equal(lg[0], lg[1], err_msg=str(step))
    for layer in range(2):
        for x, y in zip(m.read_kv(0, layer), m.read_kv(1, layer)):
            np.testing.assert_array_equal(x, y)
    m.close()


# prompt seeds found with the CPU oracle alone (the loop of the test below without the GPU): with these the oracle's top-2 gap exceeds 2e-3 of its largest logit on at
# least 6 of the 8 teacher-forced steps — llama 8 / 8, mistral 8 / 8, qwen3 8 / 8, gpt2 8 / 8
ORACLE_SEED = {"llama-3.2-1b": 8, "mistral-7b-v0.3": 8, "qwen3-1.7b": 8, "gpt2": 8}


def oracle_steps(d, p, steps, peaked):
    """the CPU oracle alone on prompt p, free-running greedy: its logits before each of steps + 1 tokens, and the tokens"""
    from oracle.oracle_ffi import OracleModel
    ref = OracleModel(d)
    for name, bits in synth.synth_checkpoint(d, 1234, 0.02, peaked=peaked):
        ref.upload(name, bits)
    ref.finalize()
    ref.forward(p[None, :])
    logits, toks = [], []
    for step in range(steps + 1):
        logits.append(ref.logits(rounded=False)[0].copy())
        t = ref.sample(GREEDY)
        toks.append(int(t[0]))
        if step < steps:
            ref.forward(t[None, :])
    ref.close()
    return logits, toks


def clear_gap(l):
    top2 = np.partition(l, -2)[-2:]
    return (top2[1] - top2[0]) > 2e-3 * np.abs(l).max()


@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("name,dtype", MODELS)
def test_forked_row_against_the_cpu_oracle(name, dtype, paged, oracle_lib):
    """peaked checkpoint: the source and its forked row, teacher-forced with the oracle's tokens over 8 steps, stay within 1e-3 of the oracle run alone on the same prompt
    and pick its ids wherever its top-2 gap is clear — on at least 6 of the 8 steps for every row"""
    STEPS, P = 8, 150
    peaked = name != "gpt2"        # GPT-2's head is tied: it has no peaked checkpoint (tinygpt_amd/synth.py) and runs the plain one
    d = cut(name, dtype, 2, 256, peaked=peaked)
    p = prompt(P, ORACLE_SEED[name])
    ref_logits, ref_toks = oracle_steps(cut(name, dtype, 1, 256, peaked=peaked), p, STEPS, peaked)
    m = Model(d)
    if paged:
        m.set_option("kv.budget_tokens", 4 * BLK)
    m.load_synthetic(1234, 0.02, peaked=peaked).finalize()
    m.forward_row(0, p); m.fork_row(0, [1])
    compared = [0, 0]
    V = d.vocab
    for step in range(STEPS + 1):
        lg = m.logits(rounded=False)
        for r in range(2):
            err = rel_err(lg[r][None, :], ref_logits[step][None, :])
            assert err < 1e-3, (step, r, err)
            if step > 0 and clear_gap(ref_logits[step]):
                compared[r] += 1
                assert int(np.argmax(lg[r])) == ref_toks[step], (step, r)
        if step < STEPS:          # the oracle's token into both rows (one-hot logits -> greedy sample), one decode step
            onehot = np.full((2, V), -1.0, np.float32); onehot[:, ref_toks[step]] = 1.0
            m.set_logits(onehot)
            assert list(m.sample(GREEDY)) == [ref_toks[step]] * 2
            m.decode(1, GREEDY)
    assert min(compared) >= 6, compared
    assert [m.past_length_row(r) for r in range(2)] == [P + STEPS] * 2
    m.close()


@pytest.mark.parametrize("paged", [0, 1])
def test_bystanders_keep_their_bits(paged):
    """two other live rows of different lengths in the batch: their ids and logits over 16 steps equal, as bits, those of a control in which the new rows were admitted by
    tgx_forward_row instead of one admission and a fork"""
    budget = 12 * BLK if paged else 0
    out = []
    for fork in (True, False):
        m = real("llama-3.2-1b", "bf16", 4, 512, budget)
        m.forward_rows([0, 1], [prompt(150, 41), prompt(40, 42)])
        m.sample_row(0, GREEDY); m.sample_row(1, GREEDY)
        ids = [m.decode(3, GREEDY).copy()]
        p = prompt(200, 43)
        m.forward_row(2, p)
        if fork:
            m.fork_row(2, [3])
        else:
            m.forward_row(3, p)
        m.sample_row(2, GREEDY); m.sample_row(3, GREEDY)
        lg = []
        for step in range(16):
            ids.append(m.decode(1, GREEDY).copy())
            lg.append(m.logits(rounded=False).copy())
        out.append((np.concatenate([i[:, :2] for i in ids]), np.concatenate([i for i in ids[1:]]), np.stack(lg)))
        m.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][2], out[1][2])


def test_write_kv_refuses_a_shared_block():
    """tgx_write_kv on a range inside a block that forked siblings map is TGX_ERR_STATE (status 4) and changes nothing; a row whose positions all lie in its private tail
    block is written as before and its sibling does not change; tgx_read_kv works on shared blocks throughout"""
    m = real("llama-3.2-1b", "bf16", 4, 512, 12 * BLK)
    m.forward_row(0, prompt(300, 51)); m.fork_row(0, [1])
    k, v = m.read_kv(1, 0)
    for row, n in ((1, 300), (1, 128), (1, 1), (0, 200)):
        with pytest.raises(TgxError) as ei:
            m.write_kv(row, 0, k[:n] + 1.0, v[:n] + 1.0)
        assert ei.value.status == 4, str(ei.value)
    for r in (0, 1):
        for x, y in zip(m.read_kv(r, 0), (k, v)):
            np.testing.assert_array_equal(x, y)
    m.forward_row(2, prompt(100, 52)); m.fork_row(2, [3])            # 100 tokens: nothing but a private tail
    k, v = m.read_kv(3, 1)
    m.write_kv(3, 1, k * 0.5, v * 0.5)                               # (a power of two: exact in the storage dtype)
    for x, y in zip(m.read_kv(3, 1), (k * 0.5, v * 0.5)):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(m.read_kv(2, 1), (k, v)):
        np.testing.assert_array_equal(x, y)
    m.reset_row(0)                                                   # the last sibling of row 1 is gone: its blocks are its own again
    k, v = m.read_kv(1, 0)
    m.write_kv(1, 0, k * 0.5, v * 0.5)
    np.testing.assert_array_equal(m.read_kv(1, 0)[0], k * 0.5)
    m.close()
