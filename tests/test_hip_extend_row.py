"""tgx_extend_row / tgx_truncate_row (include/tgx.h): a live row grows by several positions in ONE causal pass over its cache, or is rolled back — prefix reuse without
a second prefill.  The numerics contract is "equal up to summation order", with the project's numbers: GPU against GPU rel_err < 1e-3 and equal greedy ids where the
top-2 gap exceeds 2e-3 max|logit| (check_row); against the CPU oracle 1e-2 and 4e-3 (tests/test_hip_forward_rows.py).  Held to:
  * forward_row(A) + extend_row(B) == forward_row(A + B) on every route (by steps, skinny, tiled, fp32), the per-row prompt attention and the key-split form
    (kernels/attn_extend.h, option extend.attn_splits) with 2 / 3 / 7 splits, paged and unpaged, logits and every cache row, then over 4 forced decode steps;
  * the same extend twice gives the same bits for every split count; paged == unpaged bit for bit; truncation leaves the kept cache rows bit for bit;
  * the CPU oracle given the whole sequence in one forward;
  * a running batch: the rows not named stay bit-identical to a control, a finished row runs again;
  * fork, then extend (shared paged blocks stay shared; the tails cost exactly their blocks); truncation into a shared block copies before anything can write;
  * every refusal changes nothing, and the no-logits state after a truncation refuses sampling, stepping and forking until tgx_extend_row lifts it."""
import copy

import numpy as np
import pytest

from conftest import load_golden, rel_err
from tinygpt_amd import known_desc, synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model, TgxError

pytestmark = pytest.mark.gpu
BLK = 128


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def make(fam, hip, dtype="bf16", max_batch=1, max_ctx=None, budget=0):
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(cfg, dtype, max_batch=max_batch)
    if max_ctx:
        d.max_ctx = max_ctx
        if d.n_positions > 0:
            d.n_positions = max(d.n_positions, max_ctx)
    m = Model(d, hip)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(int(g["seed"]), float(g["std"])).finalize(), g


def real(name, dtype, max_batch, max_ctx, budget=0):
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 2, 4096, max_ctx, max_batch
    if d.n_positions > 0:
        d.n_positions = max(d.n_positions, max_ctx)      # GPT-2: a (synthetic) position table as long as the test's context
    m = Model(d)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(1234, 0.02).finalize()


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


def kv_all(m, row, layers=2):
    return [m.read_kv(row, layer) for layer in range(layers)]


def check_kv(got, ref, dtype, what):
    """cache rows within one ulp of the storage dtype (tests/test_hip_parity.py's form): one ulp of the entry, plus a floor for the entries near zero, which carry the
    fp32 difference of two summation orders that an ulp of their own magnitude does not resolve — 4e-6 of the largest entry in layer 0 (identical inputs), a tenth of an
    ulp of the largest entry in layer 1 (its inputs differ by layer 0's one-ulp flips)"""
    ulp = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10, "fp32": 2.0 ** -23}[dtype]
    for layer, (g, r) in enumerate(zip(got, ref)):
        floor = 4e-6 if layer == 0 else max(4e-6, 0.1 * ulp)
        for g_, r_ in zip(g, r):
            assert g_.shape == r_.shape, what
            bad = np.abs(g_ - r_) > ulp * np.abs(r_) + floor * np.abs(r_).max()
            assert not bad.any(), (what, layer, int(bad.sum()), float(np.abs(g_ - r_).max()))


# (|A|, |B|): a by-steps extension; the diagonal inside a tile; a page boundary at the join (and a one-token extension); a full query block; the S > 128 fallback;
# a partially live wave (33 queries); a full block over 18 key tiles.  At (100, 40) there are three key tiles: 7 splits exercise the clamp, 2 / 3 put a split wholly
# behind the early queries' causal range
PAIRS = [(1, 5), (63, 2), (100, 40), (127, 1), (128, 128), (200, 129), (700, 33), (1100, 128)]
SPLITS = [0, 2, 3, 7, -1]      # -1: the automatic rule (the default) — above its threshold at (700, 33) and (1100, 128), the per-row kernel below it
FORCED = [17, 4001, 902, 33]
CTX = 1280
MODELS = [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16"), ("qwen3-1.7b", "bf16"), ("gpt2", "bf16"), ("llama-3.2-1b", "fp32")]


def run_steps(m):
    """first greedy id, then FORCED teacher-forced steps -> (ids, logits)"""
    toks, logits = [int(m.sample_row(0, GREEDY))], []
    for t in FORCED:
        toks.append(int(force(m, np.array([t]))[0]))
        logits.append(m.logits(rounded=False)[0].copy())
    return toks, logits


# (paged KV serves the 16-bit storage dtypes: tgx_finalize refuses it with fp32)
@pytest.mark.parametrize("name,dtype,paged", [(n, d, p) for n, d in MODELS for p in (0, 1) if not (p and d == "fp32")])
def test_extend_equals_one_shot_on_every_route_and_form(name, dtype, paged, hip):
    """forward_row(0, A) + extend_row(0, B) against forward_row(0, A + B) (the same context, reset in between): the logits by check_row, every cache row of both layers
    within one storage ulp, then 4 forced decode steps the same way — for the per-row prompt attention (0), 2 / 3 / 7 key splits and the automatic choice (-1)"""
    m = real(name, dtype, 1, CTX, CTX if paged else 0)
    for a, b in PAIRS:
        seq = synth.synth_prompt(4096, a + b, 900 + a)
        m.reset_cache(); m.forward_row(0, seq)
        ref_l, ref_kv = m.logits(rounded=False)[0].copy(), kv_all(m, 0)
        ref_t, ref_ls = run_steps(m)
        for ns in SPLITS:
            what = (name, dtype, paged, a, b, ns)
            m.set_option("extend.attn_splits", ns)
            m.reset_cache(); m.forward_row(0, seq[:a]); m.extend_row(0, seq[a:])
            assert m.past_length_row(0) == a + b and m.past_length == a + b, what
            got_l = m.logits(rounded=False)[0].copy()
            check_kv(kv_all(m, 0), ref_kv, dtype, what)
            got_t, got_ls = run_steps(m)
            check_row(got_l, got_t[0], ref_l, ref_t[0])
            for i in range(len(FORCED)):
                check_row(got_ls[i], got_t[i + 1], ref_ls[i], ref_t[i + 1])
            assert m.past_length_row(0) == a + b + len(FORCED), what
    m.close()


@pytest.mark.parametrize("name,dtype", [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16")])
def test_extend_is_deterministic_paged_equals_unpaged_and_truncation_keeps_the_prefix(name, dtype, hip):
    """the same extend twice (truncate_row back to |A| in between): bit-identical logits and cache rows for every forced split count; paged == unpaged bit for bit on
    the same options; read_kv after truncate_row(L) == the first L rows before it, bit for bit"""
    a, b = 300, 77
    seq = synth.synth_prompt(4096, a + b, 31)
    flat, paged = real(name, dtype, 1, 512), real(name, dtype, 1, 512, budget=512)
    for ns in (0, 1, 2, 3, 7):
        runs = []
        for m in (flat, paged):
            m.set_option("extend.attn_splits", ns)
            m.reset_cache(); m.forward_row(0, seq[:a])
            kv_a = kv_all(m, 0)
            m.extend_row(0, seq[a:])
            l1, kv1 = m.logits(rounded=False)[0].copy(), kv_all(m, 0)
            m.sample_row(0, GREEDY)
            m.truncate_row(0, a)
            assert m.past_length_row(0) == a
            for (k0, v0), (k1, v1), (kf, vf) in zip(kv_a, kv_all(m, 0), kv1):
                np.testing.assert_array_equal(k0, k1); np.testing.assert_array_equal(v0, v1)
                np.testing.assert_array_equal(kf[:a], k1); np.testing.assert_array_equal(vf[:a], v1)
            m.extend_row(0, seq[a:])
            np.testing.assert_array_equal(m.logits(rounded=False)[0], l1, err_msg=str((name, ns)))
            for (k1, v1), (k2, v2) in zip(kv1, kv_all(m, 0)):
                np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
            runs.append((l1, kv1))
        np.testing.assert_array_equal(runs[0][0], runs[1][0], err_msg=str((name, ns, "paged vs unpaged")))
        for (k1, v1), (k2, v2) in zip(runs[0][1], runs[1][1]):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    flat.close(); paged.close()


@pytest.mark.parametrize("fam,dtype", [("llama_tiny", "bf16"), ("qwen2_tiny", "bf16"), ("qwen3_tiny", "bf16"), ("gpt2_hd64", "bf16"), ("mistral_tiny", "fp16")])
def test_extend_against_the_oracle(fam, dtype, hip, oracle_lib):
    """the GPU prefills A (9 tokens) and extends twice (6 and 17 tokens); the oracle gets each whole sequence in ONE forward"""
    from oracle.oracle_ffi import OracleModel
    gpu, g = make(fam, hip, dtype, 1, 64)
    cfg, _ = load_golden(fam)
    d1 = desc_from_hf_config(cfg, dtype, max_batch=1); d1.max_ctx = 64
    if d1.n_positions > 0:
        d1.n_positions = max(d1.n_positions, 64)
    V = gpu.desc.vocab
    seq = np.random.default_rng(5).integers(0, V, 9 + 6 + 17).astype(np.int64)
    gpu.forward_row(0, seq[:9])
    at = 9
    for n in (6, 17):
        gpu.extend_row(0, seq[at:at + n]); at += n
        assert gpu.past_length_row(0) == at
        lg = gpu.logits(rounded=False)[0]
        ref = OracleModel(d1).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
        ref.forward(seq[None, :at])
        lr = ref.logits(rounded=False)[0]
        assert rel_err(lg[None, :], lr[None, :]) < 1e-2, (fam, n, rel_err(lg[None, :], lr[None, :]))
        top2 = np.sort(lr)[-2:]
        if (top2[1] - top2[0]) > 4e-3 * np.abs(lr).max():
            assert int(np.argmax(lg)) == int(np.argmax(lr))
    gpu.close()


@pytest.mark.parametrize("paged", [0, 1])
def test_extend_in_a_running_batch_leaves_the_other_rows_alone(paged, hip):
    """6 rows live and decoding; row 2 extended by 37 tokens, row 4 — finished on a stop id in tgx_decode_rows — by 5: rows 0, 1, 3, 5 == a control batch bit for bit
    over 4 more steps; row 4's finish flag is cleared and its count restarted; the lengths are exact; row 2 == its solo run"""
    budget = 12 * BLK if paged else 0
    gpu, ctrl = real("llama-3.2-1b", "bf16", 6, 256, budget), real("llama-3.2-1b", "bf16", 6, 256, budget)
    prompts = np.stack([synth.synth_prompt(4096, 50, 60 + r) for r in range(6)])
    for m in (gpu, ctrl):
        m.forward(prompts); first = m.sample(GREEDY).copy(); d2 = m.decode(2, GREEDY).copy()
    nxt = ctrl.decode(1, GREEDY)[0].copy()
    gpu.set_row_stop(4, max_new=3, stop_ids=[int(nxt[4])])   # row 4 of gpu stops on the id it is about to produce; the control lets it run
    ids, new, fin = gpu.decode_rows(1)
    np.testing.assert_array_equal(ids[0], nxt)
    assert fin[4] == 1 and new[4] == 1 and all(fin[r] == 0 for r in (0, 1, 2, 3, 5))
    len4 = gpu.past_length_row(4)
    e2, e4 = synth.synth_prompt(4096, 37, 71), synth.synth_prompt(4096, 5, 72)
    gpu.extend_row(2, e2); gpu.extend_row(4, e4)
    assert gpu.past_length_row(2) == 53 + 37 and gpu.past_length_row(4) == len4 + 5 and gpu.past_length == 53 + 37
    others = [0, 1, 3, 5]
    assert [gpu.past_length_row(r) for r in others] == [ctrl.past_length_row(r) for r in others] == [53] * 4
    np.testing.assert_array_equal(gpu.logits(rounded=False)[others], ctrl.logits(rounded=False)[others])
    with pytest.raises(TgxError) as ei:      # no current token in rows 2 and 4 yet
        gpu.decode(1, GREEDY)
    assert ei.value.status == 4
    # row 2 alone: the same 90 tokens in one prefill (its prompt, the three ids it consumed, the extension)
    solo = real("llama-3.2-1b", "bf16", 1, 256)
    solo.forward_row(0, np.concatenate([prompts[2], [first[2], d2[0, 2], d2[1, 2]], e2]))
    t2 = gpu.sample_row(2, GREEDY)
    check_row(gpu.logits(rounded=False)[2], t2, solo.logits(rounded=False)[0], solo.sample_row(0, GREEDY))
    gpu.sample_row(4, GREEDY)
    cur_c = nxt.copy()
    cur_g = nxt.copy(); cur_g[2] = t2; cur_g[4] = 7
    for step in range(4):
        ng, nc = force(gpu, cur_g), force(ctrl, cur_c)
        np.testing.assert_array_equal(gpu.logits(rounded=False)[others], ctrl.logits(rounded=False)[others])
        np.testing.assert_array_equal(ng[others], nc[others])
        cur_g, cur_c = ng, nc
    assert gpu.past_length_row(4) == len4 + 5 + 4 and gpu.past_length_row(2) == 53 + 37 + 4
    # the count restarted with the extension: max_new 3 lets row 4 produce three more (had the one token from before still counted, two)
    ids, new, fin = gpu.decode_rows(3)
    assert (fin[4] == 2 and new[4] == 3) or (fin[4] == 1 and ids[new[4] - 1, 4] == nxt[4]), (fin, new)
    gpu.close(); ctrl.close(); solo.close()


def free(m):
    return m.get_option("kv.free_tokens")


def forked(budget_blocks=16):
    """paged: a 300-token prefix in row 0, forked into rows 1 and 2 (two full blocks shared, one tail block each)"""
    m = real("llama-3.2-1b", "bf16", 3, 512, budget=budget_blocks * BLK)
    prefix = synth.synth_prompt(4096, 300, 81)
    m.forward_row(0, prefix); m.fork_row(0, [1, 2])
    return m, prefix


def test_fork_then_extend(hip):
    """each fork extended with its own text (20 and 45 tokens) == a solo forward_row(prefix + text); row 0's cache and logits are bit-identical to before; the two full
    blocks stay shared and kv.free_tokens drops by exactly what the tails need"""
    m, prefix = forked()
    assert free(m) == (16 - 5) * BLK                        # 2 shared + 3 tails
    l0, kv0 = m.logits(rounded=False)[0].copy(), kv_all(m, 0)
    texts = {1: synth.synth_prompt(4096, 20, 82), 2: synth.synth_prompt(4096, 45, 83)}
    m.extend_row(1, texts[1]); m.extend_row(2, texts[2])
    assert free(m) == (16 - 5) * BLK                        # 320 and 345 tokens still fit the rows' own tail blocks (384)
    assert [m.past_length_row(r) for r in range(3)] == [300, 320, 345]
    np.testing.assert_array_equal(m.logits(rounded=False)[0], l0)
    for (k0, v0), (k1, v1) in zip(kv0, kv_all(m, 0)):
        np.testing.assert_array_equal(k0, k1); np.testing.assert_array_equal(v0, v1)
    solo = real("llama-3.2-1b", "bf16", 1, 512)
    for r in (1, 2):
        solo.reset_cache(); solo.forward_row(0, np.concatenate([prefix, texts[r]]))
        check_row(m.logits(rounded=False)[r], m.sample_row(r, GREEDY), solo.logits(rounded=False)[0], solo.sample_row(0, GREEDY))
        check_kv(kv_all(m, r), kv_all(solo, 0), "bf16", ("fork+extend", r))
    m.extend_row(2, synth.synth_prompt(4096, 40, 84))       # 385 tokens: one more block, row 2's alone
    assert free(m) == (16 - 6) * BLK
    m.truncate_row(2, 345)                                  # ... which returns
    assert free(m) == (16 - 5) * BLK
    m.reset_row(1); m.reset_row(2)
    assert free(m) == (16 - 3) * BLK                        # the shared blocks are row 0's alone again
    np.testing.assert_array_equal(m.logits(rounded=False)[0], l0)
    m.close(); solo.close()


def test_truncation_into_a_shared_block_copies_first(hip):
    """truncate_row(1, 200) ends inside shared block 1: a fresh block is taken and rows 0 and 2 read back bit-identical, also after row 1 is extended; with the free list
    emptied the call is TGX_ERR_CONTEXT and changes nothing; truncate_row(1, 256) — a block boundary — takes no block"""
    m, prefix = forked()
    kv0, kv2 = kv_all(m, 0), kv_all(m, 2)
    f0 = free(m)
    m.truncate_row(1, 200)
    assert free(m) == f0 + BLK - BLK and m.past_length_row(1) == 200      # the tail block returned, a fresh one taken for rows [128, 200)
    text = synth.synth_prompt(4096, 90, 85)
    m.extend_row(1, text)                                                  # writes positions 200 .. 289: into the copy, not into block 1 of rows 0 / 2
    for r, ref in ((0, kv0), (2, kv2)):
        for (k0, v0), (k1, v1) in zip(ref, kv_all(m, r)):
            np.testing.assert_array_equal(k0, k1); np.testing.assert_array_equal(v0, v1)
    solo = real("llama-3.2-1b", "bf16", 1, 512)
    solo.forward_row(0, np.concatenate([prefix[:200], text]))
    check_row(m.logits(rounded=False)[1], m.sample_row(1, GREEDY), solo.logits(rounded=False)[0], solo.sample_row(0, GREEDY))
    check_kv(kv_all(m, 1), kv_all(solo, 0), "bf16", "cow")
    solo.close(); m.close()
    # a block boundary needs no copy: rows 0 .. 255 are two whole shared blocks, appends start a new one
    m, prefix = forked()
    f0 = free(m)
    m.truncate_row(1, 256)
    assert free(m) == f0 + BLK
    m.close()
    # no free block: refused, nothing moves
    m, prefix = forked(budget_blocks=5)
    assert free(m) == 0
    before = [kv_all(m, r) for r in range(3)]
    with pytest.raises(TgxError) as ei:
        m.truncate_row(1, 200)
    assert ei.value.status == 8
    assert free(m) == 0 and [m.past_length_row(r) for r in range(3)] == [300] * 3
    for r in range(3):
        for (k0, v0), (k1, v1) in zip(before[r], kv_all(m, r)):
            np.testing.assert_array_equal(k0, k1); np.testing.assert_array_equal(v0, v1)
    m.sample(GREEDY); m.decode(1, GREEDY)                                  # not poisoned, every row still has its logits
    m.close()


@pytest.mark.parametrize("paged", [0, 1])
def test_refusals_change_nothing(paged, hip):
    """every refusal of tgx_extend_row / tgx_truncate_row (but the poisoned context, which no test can bring about on purpose): the status, then lengths, logits of all
    rows, kv.free_tokens and a following decode step equal a control's; the no-logits state after truncate_row refuses sample_row, sample, decode, decode_rows,
    step_async and fork_row (TGX_ERR_STATE) until extend_row lifts it"""
    import ctypes
    budget = 5 * BLK if paged else 0
    m, g = make("llama_tiny", hip, "bf16", 5, 512, budget)
    ctrl, _ = make("llama_tiny", hip, "bf16", 5, 512, budget)
    V = m.desc.vocab
    rng = np.random.default_rng(9)
    P = lambda n: rng.integers(0, V, n).astype(np.int64)
    p0, p1, p2, p3 = P(200), P(100), P(30), P(10)
    for x in (m, ctrl):
        x.forward_rows([0, 1, 2, 3], [p0, p1, p2, p3])       # 2 + 1 + 1 + 1 blocks: the whole budget
        for r in range(4):
            x.sample_row(r, GREEDY)
        x.reset_row(3)                                       # row 3: retired (one block free); row 4: beyond the batch
    l1_0 = m.logits(rounded=False)[1].copy()

    def state(x):
        return x.get_option("kv.free_tokens"), [x.past_length_row(r) for r in range(5)], x.past_length

    def refused(status, fn):
        before = state(m)
        with pytest.raises(TgxError) as ei:
            fn()
        assert ei.value.status == status, str(ei.value)
        assert state(m) == before == state(ctrl)
        np.testing.assert_array_equal(m.logits(rounded=False), ctrl.logits(rounded=False))

    refused(4, lambda: m.extend_row(3, P(3)))                # retired row
    refused(4, lambda: m.extend_row(4, P(3)))                # row >= batch
    refused(1, lambda: m.extend_row(5, P(3)))                # outside [0, max_batch)
    refused(1, lambda: m.extend_row(-1, P(3)))
    refused(1, lambda: m.extend_row(0, P(0)))                # seq < 1
    refused(1, lambda: m.extend_row(0, np.array([3, V], dtype=np.int64)))      # id out of range
    assert m.be.extend_row(m._ctx, 0, None, 3) == 1 and state(m) == state(ctrl)      # null pointer
    refused(8, lambda: m.extend_row(0, P(313)))              # 200 + 313 > max_ctx 512
    if paged:
        refused(8, lambda: m.extend_row(2, P(300)))          # 330 tokens: two more blocks, one free
    refused(4, lambda: m.truncate_row(3, 1))                 # retired row
    refused(4, lambda: m.truncate_row(4, 1))
    refused(1, lambda: m.truncate_row(5, 1))
    refused(1, lambda: m.truncate_row(0, 0))                 # tgx_reset_row's job
    refused(1, lambda: m.truncate_row(0, 201))               # beyond what the row holds
    m.truncate_row(0, 200)                                   # the row as it is, logits and token in place: a no-op
    assert state(m) == state(ctrl)
    np.testing.assert_array_equal(m.decode(1, GREEDY), ctrl.decode(1, GREEDY))      # not poisoned, the same step
    np.testing.assert_array_equal(m.logits(rounded=False), ctrl.logits(rounded=False))
    # ---- the no-logits state
    m.truncate_row(1, 60)
    assert m.past_length_row(1) == 60 and m.past_length == 201
    for fn in (lambda: m.sample_row(1, GREEDY), lambda: m.sample(GREEDY), lambda: m.decode(1, GREEDY), lambda: m.decode_rows(1), lambda: m.fork_row(1, [3]),
               lambda: m.step_async(GREEDY)):
        with pytest.raises(TgxError) as ei:
            fn()
        assert ei.value.status == 4, str(ei.value)
    assert [m.past_length_row(r) for r in range(4)] == [201, 60, 31, 0]
    m.extend_row(1, p1[60:])                                 # the same 100 tokens again
    check_row(m.logits(rounded=False)[1], m.sample_row(1, GREEDY), l1_0, int(np.argmax(l1_0)))
    m.decode(1, GREEDY)
    assert [m.past_length_row(r) for r in range(3)] == [202, 101, 32]
    m.close(); ctrl.close()
