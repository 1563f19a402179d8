"""tgx_forward_rows (include/tgx.h): several prompts into rows of a live batch in ONE ragged prefill pass — the GEMMs once over all their rows, ONE RoPE / cache
append launch and ONE attention launch per layer for all prompts (kernels/prefill.h rope_kv_split_rg_kernel / attn_prefill_rg_kernel, attn_prefill_dma.h).  Held to:
  * equal lengths into rows 0..n-1 == tgx_forward on the same prompts, BIT for bit (logits and every cache row), across the attention forms and on a paged cache;
  * ragged prompts (1..600 tokens) into scattered retired rows plus new rows == each prompt run alone (the batch-invariance bound of tests/test_hip_rows.py) and its
    CPU oracle, over 8 decode steps; the rows not named stay bit-identical to a batch that never admitted anything;
  * a serving continuation (per-row samplers, tgx_decode_rows) gives the ids of the same requests admitted one by one;
  * refusals change nothing (paged budget counted for the whole call, every argument check); several passes when the prompts exceed 8192 workspace rows."""
import copy

import numpy as np
import pytest

from conftest import load_golden, rel_err
from tinygpt_amd import known_desc, synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def make(fam, hip, dtype="bf16", max_batch=1, max_ctx=None, budget=0):
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(cfg, dtype, max_batch=max_batch)
    if max_ctx:
        d.max_ctx = max_ctx
    m = Model(d, hip)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(int(g["seed"]), float(g["std"])).finalize(), g


def real(name, dtype, max_batch, max_ctx, budget=0, peaked=False):
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 2, 4096, max_ctx, max_batch
    if peaked:
        d.tied = False                    # the peaked checkpoint's loud rows live in an untied lm_head (tinygpt_amd/synth.py)
    m = Model(d)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(1234, 0.02, peaked=peaked).finalize()


def check_row(lb, tok_b, l1, tok_1):
    assert rel_err(lb[None, :], l1[None, :]) < 1e-3, rel_err(lb[None, :], l1[None, :])
    top2 = np.sort(l1)[-2:]
    if (top2[1] - top2[0]) > 2e-3 * np.abs(l1).max():
        assert int(tok_b) == int(tok_1)


def force(m, toks):
    """make `toks` [rows] the current tokens of all rows (one-hot logits -> greedy sample), then one decode step"""
    V = m.desc.vocab
    onehot = np.full((len(toks), V), -1.0, np.float32); onehot[np.arange(len(toks)), toks] = 1.0
    m.set_logits(onehot)
    np.testing.assert_array_equal(m.sample(GREEDY), toks)
    return m.decode(1, GREEDY)[0].copy()


# (model, dtype, prompt lengths, attention option sets): head_dim 64 under both key-split settings and the LDS-DMA form, head_dim 128, Qwen3's q / k norm, GPT-2
EQUAL = [("llama-3.2-1b", "bf16", (24, 200, 1100), ((0, 0), (0, 2), (2, 0), (2, 2))),
         ("mistral-7b-v0.3", "fp16", (24, 200, 1100), ((0, 0), (0, 2))),
         ("qwen3-1.7b", "bf16", (24, 200, 1100), ((0, 0), (0, 2))),
         ("gpt2", "bf16", (24, 200, 900), ((0, 0), (0, 2)))]


@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("name,dtype,lens,forms", EQUAL)
def test_equal_lengths_equal_tgx_forward_bit_for_bit(name, dtype, lens, forms, paged, hip):
    """n equal-length prompts into rows 0..n-1 of a fresh context: the same GEMMs over the same stacked rows as tgx_forward, RoPE / append and attention as ONE
    work-list launch each that picks the per-row form's key split -> the same bits in the logits and in every cache row of every layer"""
    ctx = max(lens) + 64
    budget = 4 * ((ctx + 127) // 128) * 128 if paged else 0
    joint, twin = real(name, dtype, 4, ctx, budget), real(name, dtype, 4, ctx, budget)
    for S in lens:
        for n in (2, 4):
            prompts = np.stack([synth.synth_prompt(4096, S, 500 + 7 * b + S) for b in range(n)])
            for ks, dma in forms:
                for m in (joint, twin):
                    m.set_option("prefill.attn_ksplit", ks); m.set_option("prefill.attn_dma", dma)
                    m.reset_cache()
                twin.forward(prompts)
                joint.forward_rows(range(n), list(prompts))
                assert [joint.past_length_row(r) for r in range(n)] == [S] * n
                what = (S, n, ks, dma)
                np.testing.assert_array_equal(joint.logits(rounded=False)[:n], twin.logits(rounded=False), err_msg=str(what))
                for r in range(n):
                    for layer in range(2):
                        for a, b in zip(joint.read_kv(r, layer), twin.read_kv(r, layer)):
                            np.testing.assert_array_equal(a, b, err_msg=str(what + (r, layer)))
    joint.close(); twin.close()


def solo_run(fam, hip, dtype, prompt, steps, ctx):
    m, _ = make(fam, hip, dtype, 1, ctx)
    m.forward(prompt[None, :])
    logits = [m.logits(rounded=False)[0].copy()]
    toks = [int(m.sample(GREEDY)[0])]
    for _ in range(steps):
        toks.append(int(m.decode(1, GREEDY)[0, 0]))
        logits.append(m.logits(rounded=False)[0].copy())
    m.close()
    return toks, logits


@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("fam,dtype", [("llama_tiny", "bf16"), ("qwen3_tiny", "bf16"), ("mistral_tiny", "fp16")])
def test_ragged_admission_equals_each_prompt_alone_and_leaves_the_others_alone(fam, dtype, paged, hip, oracle_lib):
    """prompts of 600 / 2 / 130 / 37 / 1 tokens into retired rows 6, 1, 4 and new rows 8, 9 of a running 8-row batch: each admitted row == the prompt run alone on
    the GPU (1e-3, greedy ids where the top-2 gap is clear) and near its CPU oracle, over 8 forced decode steps; rows 0, 2, 3, 5, 7 == a control batch bit for bit"""
    from oracle.oracle_ffi import OracleModel
    STEPS, B, CTX = 8, 8, 640
    budget = 24 * 128 if paged else 0
    gpu, g = make(fam, hip, dtype, 10, CTX, budget)
    ctrl, _ = make(fam, hip, dtype, 10, CTX, budget)
    V = gpu.desc.vocab
    p = g["prompt"][0]
    ids = np.stack([(p + 3 * b + 1) % V for b in range(B)])
    for m in (gpu, ctrl):
        m.forward(ids); m.sample(GREEDY); m.decode(2, GREEDY)
    for r in (6, 1, 4):
        gpu.reset_row(r)
    rows, lens = [6, 1, 8, 4, 9], [600, 2, 130, 37, 1]
    rng = np.random.default_rng(11)
    prompts = [rng.integers(0, V, n).astype(np.int64) for n in lens]
    free0 = gpu.get_option("kv.free_tokens")
    gpu.forward_rows(rows, prompts)
    assert gpu.batch == 10 and [gpu.past_length_row(r) for r in rows] == lens
    if paged:
        assert gpu.get_option("kv.free_tokens") == free0 - sum((n + 127) // 128 for n in lens) * 128
    cfg, _ = load_golden(fam)
    d1 = desc_from_hf_config(cfg, dtype, max_batch=1); d1.max_ctx = CTX
    solos = [solo_run(fam, hip, dtype, pr, STEPS, CTX) for pr in prompts]
    lg = gpu.logits(rounded=False)
    others = [0, 2, 3, 5, 7]
    np.testing.assert_array_equal(lg[others], ctrl.logits(rounded=False)[others])
    for i, (r, pr) in enumerate(zip(rows, prompts)):
        check_row(lg[r], gpu.sample_row(r, GREEDY), solos[i][1][0], solos[i][0][0])
        ref = OracleModel(d1).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
        ref.forward(pr[None, :])
        lr = ref.logits(rounded=False)[0]
        assert rel_err(lg[r][None, :], lr[None, :]) < 1e-2, (r, rel_err(lg[r][None, :], lr[None, :]))
        top2 = np.sort(lr)[-2:]
        if (top2[1] - top2[0]) > 4e-3 * np.abs(lr).max():
            assert int(np.argmax(lg[r])) == int(np.argmax(lr))
    cur_c = ctrl.sample(GREEDY).copy()
    cur_b = np.zeros(10, dtype=np.int64)
    cur_b[others] = cur_c[others]
    for step in range(STEPS):
        for i, r in enumerate(rows):
            cur_b[r] = solos[i][0][step]
        nxt_b, nxt_c = force(gpu, cur_b), force(ctrl, cur_c)
        lb, lc = gpu.logits(rounded=False), ctrl.logits(rounded=False)
        for i, r in enumerate(rows):
            check_row(lb[r], nxt_b[r], solos[i][1][step + 1], solos[i][0][step + 1])
            assert gpu.past_length_row(r) == lens[i] + step + 1
        np.testing.assert_array_equal(lb[others], lc[others])
        np.testing.assert_array_equal(nxt_b[others], nxt_c[others])
        cur_b, cur_c = nxt_b, nxt_c
    for r, n in zip(rows, lens):
        assert gpu.read_kv(r, 0)[0].shape[0] == n + STEPS


def test_serving_continuation_equals_one_by_one_admission(hip):
    """a joint admission, then per-row sampler settings (greedy next to T 0.8 / top-p 0.9), tgx_sample_row and 16 steps of tgx_decode_rows: every row's ids equal
    those of the same requests admitted by tgx_forward_row (peaked synthetic checkpoint: no draw sits on a tie)"""
    lens = [300, 40, 7, 129, 64, 3]
    cfgs = [GREEDY, SamplerCfg(0.8, 0, 0.9, 0.0)] * 3
    out = []
    for joint in (True, False):
        m = real("llama-3.2-1b", "bf16", 6, 512, peaked=True)
        prompts = [synth.synth_prompt(4096, n, 40 + i) for i, n in enumerate(lens)]
        if joint:
            m.forward_rows(range(6), prompts)
        else:
            for r, pr in enumerate(prompts):
                m.forward_row(r, pr)
        first = []
        for r in range(6):
            m.set_row_sampler(r, cfgs[r], 100 + r)
            first.append(m.sample_row(r, cfgs[r], seed=100 + r))
        ids, new, fin = m.decode_rows(16)
        out.append((first, ids.copy(), new.copy()))
        m.close()
    assert out[0][0] == out[1][0]
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][2], out[1][2])


def test_refusals_change_nothing(hip):
    """all or nothing: a paged call whose later prompt exhausts the budget returns TGX_ERR_CONTEXT with kv.free_tokens, every row's length and the batch size as
    they were, and a smaller call then succeeds; every refused argument returns its status and changes nothing"""
    m, g = make("llama_tiny", hip, "bf16", 6, 512, budget=8 * 128)
    V = m.desc.vocab
    rng = np.random.default_rng(3)
    P = lambda n: rng.integers(0, V, n).astype(np.int64)
    m.forward_rows([0, 1], [P(200), P(50)])                  # 2 + 1 blocks
    m.sample_row(0, GREEDY); m.sample_row(1, GREEDY)

    def state():
        return m.get_option("kv.free_tokens"), [m.past_length_row(r) for r in range(6)], m.past_length

    def refused(status, rows, prompts):
        before, batch = state(), m.batch
        with pytest.raises(TgxError) as ei:
            m.forward_rows(rows, prompts)
        assert ei.value.status == status, (rows, str(ei.value))
        m.batch = batch
        assert state() == before

    assert state()[0] == 5 * 128
    refused(8, [2, 3, 4], [P(300), P(100), P(250)])          # 3 + 1 + 2 blocks > 5 free: the last prompt does not fit
    m.decode(1, GREEDY)                                      # not poisoned: the live rows step on
    m.forward_rows([3, 2], [P(100), P(300)])                 # 1 + 3 blocks fit
    assert state()[0] == 1 * 128 and m.batch == 4
    m.sample_row(2, GREEDY); m.sample_row(3, GREEDY)
    refused(1, [4, 4], [P(3), P(3)])                         # duplicate row
    refused(4, [0], [P(5)])                                  # live row
    refused(1, [5], [P(5)])                                  # a gap in the new rows (4 is next)
    refused(1, [4], [P(0)])                                  # length 0
    refused(1, [4], [np.array([V], dtype=np.int64)])         # id out of range
    refused(1, [], [])                                       # n = 0
    refused(4, [4, 1], [P(5), P(5)])                         # a new row next to a live one
    m.set_row_stop(1, max_new=1)
    _, _, fin = m.decode_rows(2)
    assert fin[1] == 2
    refused(4, [1], [P(5)])                                  # finished row
    m.reset_row(1)
    m.forward_rows([1, 4], [P(5), P(9)])
    assert [m.past_length_row(r) for r in (1, 4)] == [5, 9] and m.batch == 5


def test_prompts_beyond_8192_rows_run_as_several_passes(hip):
    """3 x 3000 tokens on a 2-layer Llama-3.2-1B: two passes (6000 + 3000 rows); every row == the same prompt admitted by tgx_forward_row (the per-row bound)"""
    lens = [3000, 3000, 3000]
    prompts = [synth.synth_prompt(4096, n, 70 + i) for i, n in enumerate(lens)]
    joint, one = real("llama-3.2-1b", "bf16", 3, 3072), real("llama-3.2-1b", "bf16", 3, 3072)
    joint.forward_rows(range(3), prompts)
    for r, pr in enumerate(prompts):
        one.forward_row(r, pr)
    la, lb = joint.logits(rounded=False), one.logits(rounded=False)
    for r in range(3):
        check_row(la[r], int(np.argmax(la[r])), lb[r], int(np.argmax(lb[r])))
