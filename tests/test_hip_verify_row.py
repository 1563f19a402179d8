"""tgx_verify_row (include/tgx.h): greedy speculative decoding — a row's draft tokens verified in ONE causal pass, the row left as after the accepted greedy
decode steps.  The contract is "equal to a + 1 steps of tgx_decode_rows up to summation order", with the project's numbers: GPU against GPU rel_err < 1e-3 and
equal greedy ids; against the CPU oracle 1e-2 and ids outside 4e-3 (tests/test_hip_forward_rows.py).  Held to:
  * equals stepping: drafts built from a control context's own greedy ids with the first wrong token at index j, for 2 / 4 / 5 / 8 / 16 positions (by steps, one
    full chunk, a chunk and a rest, the first skinny size, all 16 rows), a right-wrong-right draft, a page boundary inside the pass (new length exactly 128), the
    key-split attention form; ids, lengths, logits, every live cache row, then 4 forced steps.  Checkpoints are peaked (untied head; GPT-2's head is tied, so
    its checkpoint is the plain one) and every prompt seed was picked with the CPU oracle so that the top-2 gap of every compared free-running step is at least
    four times the 2e-3 band — asserted here from the oracle's own logits, so NO id comparison of those steps is skipped (the 4 forced steps behind them keep
    check_row's band: their trajectories are not the oracle's);
  * the CPU oracle given the whole accepted sequence in one forward;
  * the same call twice gives the same bits; paged == unpaged bit for bit;
  * stop ids and max_new end acceptance on the device; a finished row behaves as after tgx_decode_rows;
  * paged bookkeeping: kv.free_tokens after every call, an exhausted budget, a forked copy (shared blocks stay shared, the source bit-identical to a control);
  * a running batch: the rows not named are bit-identical to a control; every refusal changes nothing;
  * the host engine and tgx_cli with speculate = 7: the ids and callbacks of speculate = 0, and the fast path is known to have run."""
import copy
import os
import subprocess

import numpy as np
import pytest

from conftest import load_golden, rel_err
from tinygpt_amd import build, known_desc, synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu
BLK = 128
CTX = 1024
V = 4096
FORCED = [17, 4001, 902, 33]
K = 16                      # free-running control steps: the most a verify pass can produce
BAND = 4 * 2e-3             # every compared step's top-2 gap, relative to max |logit| (the margin of tests/test_hip_parity_bar.py)
MODELS = [("llama-3.2-1b", "bf16"), ("qwen3-1.7b", "bf16"), ("mistral-7b-v0.3", "fp16"), ("gpt2", "bf16"), ("llama-3.2-1b", "fp32")]
# prompt seeds per (model, dtype, past), found with the CPU oracle alone (tests/test_hip_verify_row.py::oracle_run over seeds 1, 2, ..): the first whose K + 1
# free-running steps all clear BAND
SEEDS = {
    ("llama-3.2-1b", "bf16", 5): 1, ("llama-3.2-1b", "bf16", 126): 1, ("llama-3.2-1b", "bf16", 700): 1,
    ("qwen3-1.7b", "bf16", 5): 1, ("qwen3-1.7b", "bf16", 126): 1,
    ("mistral-7b-v0.3", "fp16", 5): 1, ("mistral-7b-v0.3", "fp16", 126): 1,
    ("gpt2", "bf16", 5): 1, ("gpt2", "bf16", 126): 2,
    ("llama-3.2-1b", "fp32", 5): 1, ("llama-3.2-1b", "fp32", 126): 1, ("llama-3.2-1b", "fp32", 700): 1,
}


def cut(name, dtype, max_batch=1, max_ctx=CTX):
    """2-layer cut, vocab 4096, with an untied head where the family allows one (a peaked checkpoint needs it)"""
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 2, V, max_ctx, max_batch
    if d.n_positions > 0:
        d.n_positions = max(d.n_positions, max_ctx)
    peaked = name != "gpt2"
    if peaked:
        d.tied = False
    return d, peaked


def gpu_model(name, dtype, max_batch=1, budget=0, max_ctx=CTX):
    d, peaked = cut(name, dtype, max_batch, max_ctx)
    m = Model(d)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(1234, 0.02, peaked=peaked).finalize()


_oracle_runs = {}


def oracle_run(name, dtype, past, seed):
    """the CPU oracle's free-running greedy trajectory of the prompt: ids [K + 1] and each step's top-2 gap relative to max |logit| (computed once per case)"""
    key = (name, dtype, past, seed)
    if key not in _oracle_runs:
        from oracle.oracle_ffi import OracleModel
        d, peaked = cut(name, dtype)
        ref = OracleModel(d).load_synthetic(1234, 0.02, peaked=peaked).finalize()
        ref.forward(synth.synth_prompt(V, past, seed)[None, :])
        ids, gaps = [], []
        for step in range(K + 1):
            l = ref.logits(rounded=False)[0]
            top2 = np.sort(l)[-2:]
            gaps.append(float((top2[1] - top2[0]) / np.abs(l).max()))
            ids.append(int(ref.sample(GREEDY)[0]) if step == 0 else None)
            if step == K:
                break
            nxt = ref.decode(1, GREEDY)
            ids.append(int(nxt[0, 0]))
        ids = [i for i in ids if i is not None]
        ref.close()
        _oracle_runs[key] = (ids, gaps)
    return _oracle_runs[key]


def start(m, prompt, row=0):
    """a fresh row holding the prompt and its first greedy token"""
    m.reset_cache()
    m.forward_row(row, prompt)
    return int(m.sample_row(row, GREEDY))


def force(m, toks):
    onehot = np.full((len(toks), V), -1.0, np.float32); onehot[np.arange(len(toks)), toks] = 1.0
    m.set_logits(onehot)
    np.testing.assert_array_equal(m.sample(GREEDY), toks)
    return m.decode(1, GREEDY)[0].copy()


def kv_all(m, row, layers=2):
    return [m.read_kv(row, layer) for layer in range(layers)]


def check_kv(got, ref, dtype, what):
    """tests/test_hip_extend_row.py's check_kv: one ulp of the storage dtype plus the floor for entries near zero"""
    ulp = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10, "fp32": 2.0 ** -23}[dtype]
    for layer, (g, r) in enumerate(zip(got, ref)):
        floor = 4e-6 if layer == 0 else max(4e-6, 0.1 * ulp)
        for g_, r_ in zip(g, r):
            assert g_.shape == r_.shape, what
            bad = np.abs(g_ - r_) > ulp * np.abs(r_) + floor * np.abs(r_).max()
            assert not bad.any(), (what, layer, int(bad.sum()), float(np.abs(g_ - r_).max()))


def check_row(lb, tok_b, l1, tok_1):
    assert rel_err(lb[None, :], l1[None, :]) < 1e-3, rel_err(lb[None, :], l1[None, :])
    top2 = np.sort(l1)[-2:]
    if (top2[1] - top2[0]) > 2e-3 * np.abs(l1).max():
        assert int(tok_b) == int(tok_1)


def wrong_at(ids, j):
    """the draft `ids` with a token the model will not choose at index j (None: all right)"""
    d = list(ids)
    if j is not None:
        d[j] = (d[j] + 1) % V
    return d


# (past, n_draft, index of the first wrong draft token or None): 2 positions, a full 4-chunk, 4 + 1, the first skinny size, 16 rows; j = 0, the middle, none;
# past 126 with 7 drafts crosses a page inside the pass (j = 1: the new length is exactly 128); past 700 runs the key-split attention form at head_dim 64
def cases(name):
    cs = [(5, n, j) for n in (1, 3, 4, 7, 15) for j in sorted({0, n // 2}) + [None]]
    cs += [(126, 7, j) for j in (0, 1, 3, None)]
    if name == "llama-3.2-1b":
        cs += [(700, n, j) for n in (3, 7, 15) for j in (n // 2, None)]
    return cs


@pytest.mark.parametrize("name,dtype,paged", [(n, d, p) for n, d in MODELS for p in (0, 1) if not (p and d == "fp32")])
def test_verify_equals_stepping(name, dtype, paged):
    budget = 2 * CTX if paged else 0
    gpu, ctrl = gpu_model(name, dtype, 1, budget), gpu_model(name, dtype, 1, budget)
    for past in sorted({c[0] for c in cases(name)}):
        seed = SEEDS[(name, dtype, past)]
        prompt = synth.synth_prompt(V, past, seed)
        o_ids, o_gaps = oracle_run(name, dtype, past, seed)
        assert min(o_gaps) >= BAND, (name, dtype, past, seed, min(o_gaps))      # the oracle's own logits: no id comparison below is skipped
        c_ids = [start(ctrl, prompt)] + [int(t) for t in ctrl.decode_rows(K)[0][:, 0]]
        assert c_ids == o_ids, (name, dtype, past)
        todo = [c for c in cases(name) if c[0] == past]
        if past == 5:
            todo.append((5, 3, "rwr"))
        for _, n_draft, j in todo:
            what = (name, dtype, paged, past, n_draft, j)
            draft = wrong_at(c_ids[1:1 + n_draft], 1 if j == "rwr" else j)      # right, wrong, right: stops at the wrong one
            want = n_draft + 1 if j is None else (2 if j == "rwr" else j + 1)
            assert start(gpu, prompt) == c_ids[0], what
            ids, fin = gpu.verify_row(0, draft)
            assert len(ids) == want and fin == 0, (what, ids)
            assert list(ids) == c_ids[1:1 + want], (what, ids)
            assert gpu.past_length_row(0) == past + want == gpu.past_length, what
            if paged:
                assert gpu.get_option("kv.free_tokens") == budget - -(-(past + want) // BLK) * BLK, what
            assert start(ctrl, prompt) == c_ids[0]
            ctrl.decode_rows(want)
            lg, lc = gpu.logits(rounded=False)[0].copy(), ctrl.logits(rounded=False)[0].copy()
            assert rel_err(lg[None, :], lc[None, :]) < 1e-3, (what, rel_err(lg[None, :], lc[None, :]))
            assert int(np.argmax(lg)) == int(np.argmax(lc)) == c_ids[want], what      # never skipped: the oracle's gap is >= BAND
            check_kv(kv_all(gpu, 0), kv_all(ctrl, 0), dtype, what)
            for t in FORCED:
                tg, tc = force(gpu, np.array([t])), force(ctrl, np.array([t]))
                check_row(gpu.logits(rounded=False)[0], tg[0], ctrl.logits(rounded=False)[0], tc[0])
            assert gpu.past_length_row(0) == past + want + len(FORCED), what
    gpu.close(); ctrl.close()


@pytest.mark.parametrize("fam,dtype", [("llama_tiny", "bf16"), ("qwen3_tiny", "bf16"), ("gpt2_hd64", "bf16"), ("mistral_tiny", "fp16")])
def test_verify_against_the_oracle(fam, dtype, oracle_lib):
    """the oracle is given the whole accepted sequence in ONE forward: its last-position logits against the row's"""
    from oracle.oracle_ffi import OracleModel
    cfg, g = load_golden(fam)

    def desc():
        d = desc_from_hf_config(cfg, dtype, max_batch=1); d.max_ctx = 64
        if d.n_positions > 0:
            d.n_positions = max(d.n_positions, 64)
        return d
    gpu = Model(desc()).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    ctrl = Model(desc()).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    prompt = np.random.default_rng(5).integers(0, gpu.desc.vocab, 9).astype(np.int64)
    c_ids = [start(ctrl, prompt)] + [int(t) for t in ctrl.decode_rows(8)[0][:, 0]]
    for n_draft, j in ((6, None), (6, 2), (2, None)):
        t0 = start(gpu, prompt)
        ids, _ = gpu.verify_row(0, wrong_at([c_ids[1 + i] for i in range(n_draft)], j))
        seq = np.concatenate([prompt, [t0], ids[:-1]]).astype(np.int64)      # every input that produced a token
        assert gpu.past_length_row(0) == len(seq)
        lg = gpu.logits(rounded=False)[0]
        ref = OracleModel(desc()).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
        ref.forward(seq[None, :])
        lr = ref.logits(rounded=False)[0]
        assert rel_err(lg[None, :], lr[None, :]) < 1e-2, (fam, n_draft, j, rel_err(lg[None, :], lr[None, :]))
        top2 = np.sort(lr)[-2:]
        if (top2[1] - top2[0]) > 4e-3 * np.abs(lr).max():
            assert int(np.argmax(lg)) == int(np.argmax(lr)) == int(ids[-1])
        ref.close()
    gpu.close(); ctrl.close()


@pytest.mark.parametrize("name,dtype", [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16")])
def test_verify_is_deterministic_and_paged_equals_unpaged(name, dtype):
    flat, paged = gpu_model(name, dtype), gpu_model(name, dtype, 1, 2 * CTX)
    for past, n_draft, j in ((5, 3, 1), (126, 7, None), (600, 15, 9)):
        prompt = synth.synth_prompt(V, past, 77)
        runs = []
        for m in (flat, paged):
            start(m, prompt)
            steps = [int(t) for t in m.decode_rows(n_draft)[0][:, 0]]
            draft = wrong_at(steps, j)
            two = []
            for _ in range(2):
                start(m, prompt)
                ids, fin = m.verify_row(0, draft)
                two.append((list(ids), fin, m.logits(rounded=False)[0].copy(), kv_all(m, 0), int(m.decode_rows(1)[0][0, 0]), m.logits(rounded=False)[0].copy()))
            runs.append(two[0])
            for a, b in ((two[0], two[1]),):
                assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4]
                np.testing.assert_array_equal(a[2], b[2]); np.testing.assert_array_equal(a[5], b[5])
                for (k1, v1), (k2, v2) in zip(a[3], b[3]):
                    np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
        a, b = runs
        assert a[0] == b[0] and a[4] == b[4], (name, past, "paged vs unpaged")
        np.testing.assert_array_equal(a[2], b[2]); np.testing.assert_array_equal(a[5], b[5])
        for (k1, v1), (k2, v2) in zip(a[3], b[3]):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    flat.close(); paged.close()


def test_stop_conditions_end_acceptance_on_the_device():
    m = gpu_model("llama-3.2-1b", "bf16", 1, 2 * CTX)
    prompt = synth.synth_prompt(V, 40, 3)
    t0 = start(m, prompt)
    steps = [int(t) for t in m.decode_rows(8)[0][:, 0]]
    # a stop id at accepted index 2 of a fully correct 7-draft (its first occurrence among the produced tokens must be index 2)
    assert steps[2] not in steps[:2]
    assert start(m, prompt) == t0
    m.set_row_stop(0, 0, [steps[2]])
    ids, fin = m.verify_row(0, steps[:7])
    assert list(ids) == steps[:3] and fin == 1
    assert m.past_length_row(0) == 40 + 3
    assert m.get_option("kv.free_tokens") == 2 * CTX - BLK
    with pytest.raises(TgxError) as ei:                                   # as after any greedy step: no sampled row in the batch, nothing to read
        m.probs()
    assert ei.value.status == 4
    with pytest.raises(TgxError) as ei:                                   # the only live row is finished: as after tgx_decode_rows
        m.decode_rows(1)
    assert ei.value.status == 4
    with pytest.raises(TgxError) as ei:
        m.verify_row(0, steps[3:5])
    assert ei.value.status == 4
    m.extend_row(0, [steps[2], steps[3]])                                 # revives it: the stop token and one more into the cache
    assert m.past_length_row(0) == 40 + 5
    m.set_row_stop(0, 0, [])
    m.sample_row(0, GREEDY)
    out, new, f = m.decode_rows(1)
    assert new[0] == 1 and f[0] == 0
    # max_new = 2
    assert start(m, prompt) == t0
    m.set_row_stop(0, 2, [])
    ids, fin = m.verify_row(0, steps[:7])
    assert list(ids) == steps[:2] and fin == 2 and m.past_length_row(0) == 42
    # a stop id that is the token of the FIRST position: one token, finished
    assert start(m, prompt) == t0
    m.set_row_stop(0, 0, [steps[0]])
    ids, fin = m.verify_row(0, steps[:3])
    assert list(ids) == steps[:1] and fin == 1 and m.past_length_row(0) == 41
    m.close()


def test_paged_free_tokens_follow_the_new_length():
    """blocks are assigned for the whole pass and the ones beyond ceil(new length / 128) go back: kv.free_tokens is that of a row of the new length"""
    budget = 4 * BLK
    gpu, ctrl = gpu_model("llama-3.2-1b", "bf16", 1, budget), gpu_model("llama-3.2-1b", "bf16", 1, budget)
    prompt = synth.synth_prompt(V, 250, 9)                                # two blocks; a pass of 8 positions from 250 needs a third
    for m in (gpu, ctrl):
        start(m, prompt)
    steps = [int(t) for t in ctrl.decode_rows(9)[0][:, 0]]
    assert gpu.get_option("kv.free_tokens") == budget - 2 * BLK
    ids, fin = gpu.verify_row(0, wrong_at(steps[:7], 2))                  # 3 tokens: length 253 -> the third block goes back
    assert list(ids) == steps[:3] and gpu.get_option("kv.free_tokens") == budget - 2 * BLK
    ids, fin = gpu.verify_row(0, steps[3:8])                              # 6 tokens: length 259 -> three blocks
    assert list(ids) == steps[3:9] and gpu.past_length_row(0) == 259
    assert gpu.get_option("kv.free_tokens") == budget - 3 * BLK
    gpu.close(); ctrl.close()


def test_verify_on_a_forked_copy_leaves_the_source_alone():
    """verify on the copy: the source row's logits, cache rows and a following decode step are bit-identical to a control that never saw the call, and the
    shared block stays shared"""
    budget = 4 * BLK
    gpu, ctrl = gpu_model("llama-3.2-1b", "bf16", 2, budget), gpu_model("llama-3.2-1b", "bf16", 2, budget)
    prompt = synth.synth_prompt(V, 250, 9)
    for m in (gpu, ctrl):
        start(m, prompt)
        m.fork_row(0, [1])                                                # one full block shared, a tail block each: 3 blocks, 1 free
        assert m.get_option("kv.free_tokens") == budget - 3 * BLK
    steps = [int(t) for t in ctrl.decode_rows(3)[0][:, 1]]                # the copy's next ids, from a throw-away run of the control
    start(ctrl, prompt); ctrl.fork_row(0, [1])
    ids, fin = gpu.verify_row(1, wrong_at(steps + [0, 0, 0, 0], 1))       # 258 positions: the free block is taken, and goes back at length 252
    assert list(ids) == steps[:2] and gpu.past_length_row(1) == 252 and gpu.past_length_row(0) == 250
    assert gpu.get_option("kv.free_tokens") == budget - 3 * BLK
    np.testing.assert_array_equal(gpu.logits(rounded=False)[0], ctrl.logits(rounded=False)[0])
    for (k1, v1), (k2, v2) in zip(kv_all(gpu, 0), kv_all(ctrl, 0)):
        np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    k, v = gpu.read_kv(0, 0)
    with pytest.raises(TgxError) as ei:                                   # the full block is still shared: tgx_write_kv refuses a range inside it
        gpu.write_kv(0, 0, k[:BLK], v[:BLK])
    assert ei.value.status == 4
    og, oc = gpu.decode_rows(1)[0], ctrl.decode_rows(1)[0]
    assert og[0, 0] == oc[0, 0]
    np.testing.assert_array_equal(gpu.logits(rounded=False)[0], ctrl.logits(rounded=False)[0])
    gpu.close(); ctrl.close()


def test_budget_exhausted_is_refused_and_changes_nothing():
    budget = 3 * BLK
    gpu = gpu_model("llama-3.2-1b", "bf16", 2, budget)
    prompt = synth.synth_prompt(V, 250, 9)
    start(gpu, prompt)
    gpu.fork_row(0, [1])                                                  # 1 shared + 2 tails = 3 blocks: nothing free
    assert gpu.get_option("kv.free_tokens") == 0
    l0, kv0 = gpu.logits(rounded=False).copy(), [kv_all(gpu, r) for r in (0, 1)]
    with pytest.raises(TgxError) as ei:
        gpu.verify_row(1, [1, 2, 3, 4, 5, 6, 7])                          # 250 + 8 = 258: a third block for the row
    assert ei.value.status == 8
    assert gpu.get_option("kv.free_tokens") == 0 and gpu.past_length_row(1) == 250 and gpu.past_length_row(0) == 250
    np.testing.assert_array_equal(gpu.logits(rounded=False), l0)
    for r in (0, 1):
        for (k1, v1), (k2, v2) in zip(kv_all(gpu, r), kv0[r]):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    ids, fin = gpu.verify_row(1, [1, 2, 3, 4, 5])                         # 250 + 6 = 256 fits the row's own tail block
    assert len(ids) >= 1 and gpu.get_option("kv.free_tokens") == 0
    gpu.close()


def test_more_than_1024_blocks_per_row_is_unsupported_on_the_matrix_core_routes():
    m = gpu_model("llama-3.2-1b", "bf16", 1, 2 * BLK, max_ctx=1025 * BLK)
    start(m, synth.synth_prompt(V, 3, 4))                                 # (a prompt that goes by steps)
    l0 = m.logits(rounded=False).copy()
    with pytest.raises(TgxError) as ei:
        m.verify_row(0, [1, 2, 3, 4, 5, 6, 7])                            # 8 positions: the skinny route, whose attention holds the block table in LDS
    assert ei.value.status == 2 and m.past_length_row(0) == 3 and m.get_option("kv.free_tokens") == BLK
    np.testing.assert_array_equal(m.logits(rounded=False), l0)
    ids, fin = m.verify_row(0, [1])                                       # 2 positions go by steps: served
    assert len(ids) >= 1
    m.close()


@pytest.mark.parametrize("paged", [0, 1])
def test_verify_in_a_running_batch_leaves_the_other_rows_alone(paged):
    budget = 6 * BLK if paged else 0
    gpu, ctrl = gpu_model("llama-3.2-1b", "bf16", 3, budget), gpu_model("llama-3.2-1b", "bf16", 3, budget)
    prompts = np.stack([synth.synth_prompt(V, 50, 60 + r) for r in range(3)])
    for m in (gpu, ctrl):
        m.forward(prompts); m.sample(GREEDY); m.decode(2, GREEDY)
    look = ctrl.decode_rows(4)[0][:, 1].copy()                            # row 1's next ids, from a throw-away run of the control
    ctrl.reset_cache(); ctrl.forward(prompts); ctrl.sample(GREEDY); ctrl.decode(2, GREEDY)
    ids, fin = gpu.verify_row(1, wrong_at([int(t) for t in look[:3]], 2))
    assert list(ids) == [int(t) for t in look[:3]] and fin == 0
    assert [gpu.past_length_row(r) for r in range(3)] == [52, 55, 52]
    lg, lc = gpu.logits(rounded=False), ctrl.logits(rounded=False)
    for r in (0, 2):
        np.testing.assert_array_equal(lg[r], lc[r])
        for (k1, v1), (k2, v2) in zip(kv_all(gpu, r), kv_all(ctrl, r)):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    og, oc = gpu.decode_rows(2)[0], ctrl.decode_rows(2)[0]
    np.testing.assert_array_equal(og[:, [0, 2]], oc[:, [0, 2]])
    lg, lc = gpu.logits(rounded=False), ctrl.logits(rounded=False)
    for r in (0, 2):
        np.testing.assert_array_equal(lg[r], lc[r])
    assert [gpu.past_length_row(r) for r in range(3)] == [54, 57, 54]
    gpu.close(); ctrl.close()


def test_every_refusal_changes_nothing():
    import ctypes
    from ctypes import POINTER, c_int32, c_int64
    budget = 4 * BLK
    gpu, ctrl = gpu_model("llama-3.2-1b", "bf16", 4, budget), gpu_model("llama-3.2-1b", "bf16", 4, budget)
    prompts = np.stack([synth.synth_prompt(V, 30, 11 + r) for r in range(3)])
    for m in (gpu, ctrl):
        m.forward(prompts); m.sample(GREEDY)
        m.reset_row(2)                                                    # row 2 retired; row 3 never used

    def state():
        return ([gpu.past_length_row(r) for r in range(4)], gpu.get_option("kv.free_tokens"), gpu.logits(rounded=False).copy())

    def refused(status, row, draft, prepare=None):
        if prepare:
            prepare()
        s0 = state()
        with pytest.raises(TgxError) as ei:
            gpu.verify_row(row, draft)
        assert ei.value.status == status, (status, row, draft, str(ei.value))
        s1 = state()
        assert s0[0] == s1[0] and s0[1] == s1[1]
        np.testing.assert_array_equal(s0[2], s1[2])

    refused(1, -1, [1]); refused(1, 4, [1])                               # row outside [0, max_batch)
    refused(1, 0, []); refused(1, 0, [1] * 16)                            # n_draft outside [1, 15]
    refused(1, 0, [1, V]); refused(1, 0, [-1])                            # a draft id out of range
    n, f = c_int32(), c_int32()
    out = (c_int64 * 16)()
    d = (c_int64 * 2)(1, 2)
    be, ctx = gpu.be, gpu._ctx
    assert be.verify_row(ctx, 0, None, 2, out, ctypes.byref(n), ctypes.byref(f)) == 1      # null pointers
    assert be.verify_row(ctx, 0, d, 2, None, ctypes.byref(n), ctypes.byref(f)) == 1
    assert be.verify_row(ctx, 0, d, 2, out, None, ctypes.byref(f)) == 1
    assert be.verify_row(ctx, 0, d, 2, out, ctypes.byref(n), None) == 1
    refused(4, 2, [1]); refused(4, 3, [1])                                # a retired row, an empty one
    gpu.set_row_sampler(1, SamplerCfg(temperature=0.7), 3)
    refused(2, 1, [1, 2])                                                 # not greedy
    gpu.set_row_sampler(1, GREEDY, 0)
    # the state is the control's: a decode step on both gives the same bits
    np.testing.assert_array_equal(gpu.decode_rows(1)[0], ctrl.decode_rows(1)[0])
    np.testing.assert_array_equal(gpu.logits(rounded=False), ctrl.logits(rounded=False))
    # a finished row; a row fresh from tgx_extend_row (no current token); a truncated row (no logits)
    gpu.set_row_stop(0, 1, [])
    _, new, fin = gpu.decode_rows(1)
    assert fin[0] == 2
    refused(4, 0, [1])
    gpu.extend_row(1, [5, 6])
    refused(4, 1, [1])
    gpu.sample_row(1, GREEDY)
    gpu.truncate_row(1, 10)
    refused(4, 1, [1])
    gpu.close(); ctrl.close()
    # the context size
    m = gpu_model("llama-3.2-1b", "bf16", 1)
    start(m, synth.synth_prompt(V, CTX - 4, 5))
    l0 = m.logits(rounded=False).copy()
    with pytest.raises(TgxError) as ei:
        m.verify_row(0, [1, 2, 3, 4])                                     # past + 5 > max_ctx
    assert ei.value.status == 8 and m.past_length_row(0) == CTX - 4
    np.testing.assert_array_equal(m.logits(rounded=False), l0)
    ids, fin = m.verify_row(0, [1, 2, 3])                                 # past + 4 == max_ctx fits
    assert len(ids) >= 1
    m.close()


def test_which_refusal_wins():
    """calls that break two rules: the status and the message of the refusal that comes first, and lengths and kv.free_tokens as they were"""
    m = gpu_model("llama-3.2-1b", "bf16", 2, 10 * BLK)
    m.forward_row(0, synth.synth_prompt(V, CTX - 5, 5)); m.forward_row(1, synth.synth_prompt(V, 31, 12))
    for r in (0, 1):
        m.sample_row(r, GREEDY)

    def no(call, status, text, row, draft):
        s0 = ([m.past_length_row(r) for r in range(2)], m.get_option("kv.free_tokens"))
        with pytest.raises(TgxError) as ei:
            call(row, draft)
        assert ei.value.status == status and text in str(ei.value), (status, text, str(ei.value))
        assert s0 == ([m.past_length_row(r) for r in range(2)], m.get_option("kv.free_tokens")), (row, draft)

    m.set_row_stop(0, 1, [])
    fin = m.decode_rows(1)[2]
    assert fin[0] == 2 and m.past_length_row(0) == CTX - 4
    no(m.verify_row, 4, "row 0 finished", 0, [1, 2, 3, 4])                # past + 5 > max_ctx as well: the row's state before the context size
    m.set_row_sampler(1, SamplerCfg(temperature=0.7), 3)
    m.set_row_penalties(1, repetition=1.3)
    no(m.verify_row, 2, "row 1 does not sample greedily", 1, [1, 2])      # the row's sampler before its processors
    no(m.verify_row_sampled, 2, "tgx_verify_row_sampled: row 1 has a logit processor on", 1, [1, 2])
    m.close()


def spec_engine(tmp_path):
    from host_util import HostEngine, host_lib, write_model_dir
    from ctypes import POINTER, c_int, c_int64, c_void_p
    cfg, g = load_golden("llama_tiny")
    cfg = dict(cfg, tie_word_embeddings=False)
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]), peaked=True, eos=[cfg["vocab_size"] - 1])
    lib = host_lib()
    lib.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    lib.tgxe_spec_stats.restype = c_int
    lib.tgxe_spec_stats.argtypes = [c_void_p, POINTER(c_int64), c_int]
    e = HostEngine(lib, model_dir=str(tmp_path), device="mi355x", dtype=1)
    assert e.prepare(), e.error()
    return e, lib


# a prompt with a repeated span, so that the lookup has something to find from the first iteration on
SPEC_PROMPT = [11, 12, 13, 14, 15, 16, 7, 8, 11, 12, 13, 14, 15, 16, 9, 11, 12, 13]


def stats(e):
    from ctypes import c_int64
    buf = (c_int64 * 32)()
    e.lib.tgxe_spec_stats(e.h, buf, 32)
    return list(buf[:21])


def test_host_engine_speculate_equals_plain(tmp_path):
    e, lib = spec_engine(tmp_path)
    n_new = 40
    runs = {}
    for spec in (0, 7):
        lib.tgxe_set_speculate(e.h, spec)
        e.reconfigure(max_new=n_new)
        ids, new, fin = e.generate_sync([SPEC_PROMPT])
        e.reconfigure(max_new=n_new)
        aids, anew, afin, seen = e.generate_async(SPEC_PROMPT)
        runs[spec] = (ids.tolist(), new, fin, aids.tolist(), anew, afin, seen)
        if spec == 0:
            assert stats(e) == [0] * 21
    assert runs[0] == runs[7]
    s = stats(e)
    assert s[0] >= 1 and s[2] >= 1, s                                     # verify passes ran and at least one accepted a draft token
    assert sum(s[4 + 2:]) >= 1, s                                          # ... i.e. a pass produced two or more tokens
    # an extra stop id that the generation produces: Stop at that token on both paths, same callbacks
    gen = runs[0][3][len(SPEC_PROMPT):]
    stop = gen[len(gen) // 2]
    res = []
    for spec in (0, 7):
        lib.tgxe_set_speculate(e.h, spec)
        e.reconfigure(max_new=n_new, extra_stop=[stop])
        aids, anew, afin, seen = e.generate_async(SPEC_PROMPT)
        res.append((aids.tolist(), anew, afin, seen))
    assert res[0] == res[1] and res[0][2] == "stop"
    # a sampling configuration keeps the old loop
    before = stats(e)
    e.reconfigure(temperature=0.8, top_p=0.9, max_new=8)
    e.generate_sync([SPEC_PROMPT])
    assert stats(e) == before
    e.close()


def test_cli_speculate_equals_plain(tmp_path):
    from host_util import write_model_dir
    cfg, g = load_golden("llama_tiny")
    cfg = dict(cfg, tie_word_embeddings=False)
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]), peaked=True)
    _, cli = build.build_host()
    base = [cli, "--model", str(tmp_path), "--device", "mi355x", "--dtype", "bf16", "--max-tokens", "40", "--temperature", "0", "--top-p", "1",
            "--prompt-ids", ",".join(str(t) for t in SPEC_PROMPT)]
    outs = []
    for extra in ([], ["--speculate", "7"]):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        outs.append(out.stdout)
    rows = [[l for l in o.splitlines() if l.startswith("Output ids:")] for o in outs]
    assert rows[0] == rows[1] and len(rows[0]) == 1
    assert "speculate:" not in outs[0] and "speculate:" in outs[1]
    line = [l for l in outs[1].splitlines() if l.startswith("speculate:")][0].split()
    assert int(line[1]) >= 1 and int(line[4]) >= 1, line                  # "speculate: N verify passes, A of D draft tokens accepted, ..."
