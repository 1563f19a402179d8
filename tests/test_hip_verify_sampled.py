"""tgx_verify_row_sampled (include/tgx.h): a draft verified with the row's OWN sampler in one pass.  A sampled token is a pure function of its position's logits, the
row's settings and the draw key (kernels/common.h draw_key), so every check that involves a draw is made on the PASS'S OWN logits (tgx_read_pass_logits), where it
is exact: ids of two kernel paths cannot be compared step for step under sampling (at the temperatures at which draws leave the argmax, the CDF interval of a drawn
token is narrower than the project's path-to-path band).  Held to:
  * exact draws at every position, nothing skipped: s[i] restated from pass_logits[i] (oracle filter + tests/verify_sampled_util.py's draw), the accept rule
    walked in Python, out_n / out_ids / out_finish / the row's length asserted exactly; 2 / 4 / 5 / 8 / 16 positions, the wrong draft index at 0, the middle, nowhere,
    a page boundary inside the pass, rows 0 and 2 of a 3-row batch, two seeds, six sampler configurations, the greedy test's families and dtypes, one paged variant
    per family, GPT-2 at vocabulary 4099 (unaligned logits rows, the accept launch's scalar copy);
  * the row afterwards: its logits slot is pass_logits[out_n - 1] bit for bit, tgx_sample_row with the row's cfg and seed returns the last produced id again (same
    logits, same key: no tolerance), four forced steps equal a control, tgx_read_probs has no vector for the row;
  * the pass itself against a control row fed one token at a time (1e-3) and against the CPU oracle (1e-2), the live cache rows by check_kv;
  * greedy through the new entry == tgx_verify_row bit for bit; the same sampled call twice gives the same bits; paged == unpaged;
  * stop ids and max_new under sampling, log-probability records, every refusal, tgx_read_pass_logits' STATE / INVALID cases, memory, the other rows of a batch;
  * the host engine and tgx_cli with speculateSampled.
Top-p: a position whose expected draw lands on an entry inside the float-cumsum band around the cut (tests/test_hip_sampler.py:129-131) would not be compared; the
number of such positions over the committed case list is asserted to be 0."""
import ctypes
import subprocess
from ctypes import POINTER, c_float, c_int32, c_int64

import numpy as np
import pytest

from conftest import load_golden, rel_err
from test_hip_verify_row import BLK, FORCED, check_kv, check_row, force, kv_all
from tinygpt_amd import build, synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model, SamplerCfg, TgxError
from verify_sampled_util import CTX, V, draw_uniform, draw_from_probs, expected_draw, gpu_model, top_p_band, walk

pytestmark = pytest.mark.gpu
K = 16
# (family, dtype, vocabulary): the greedy test's MODELS (fp32 once), and GPT-2 at a vocabulary that is no multiple of 4
MODELS = [("llama-3.2-1b", "bf16", V), ("qwen3-1.7b", "bf16", V), ("mistral-7b-v0.3", "fp16", V), ("gpt2", "bf16", V), ("llama-3.2-1b", "fp32", V), ("gpt2", "bf16", 4099)]
# temperatures at which draws leave the argmax: the peaked cuts' logits reach several hundred (max |v| 500 - 800 on the CPU oracle: T <= 3 draws the argmax at
# every step, T = 100 leaves it at 6 - 17 of 17 steps); GPT-2's plain checkpoint is flat at any temperature
def temp(name):
    return 1.0 if name == "gpt2" else 100.0


def configs(name):
    T = temp(name)
    return {"T": SamplerCfg(T, 0, 1.0, 0.0), "top-k": SamplerCfg(T, 40, 1.0, 0.0), "top-p": SamplerCfg(T, 0, 0.9, 0.0), "top-k+top-p": SamplerCfg(T, 40, 0.9, 0.0),
            "min-p": SamplerCfg(T, 0, 1.0, 0.05), "all": SamplerCfg(T, 40, 0.9, 0.05)}


# (past, n_draft, index of the first wrong draft token or None): 2 / 4 / 5 / 8 / 16 positions (by steps, one chunk, a chunk and a rest, the first skinny size, all
# rows); past 126 with 7 drafts crosses a page inside the pass
CASES = [(5, n, j) for n in (1, 3, 4, 7, 15) for j in sorted({0, n // 2}) + [None]] + [(126, 7, j) for j in (0, 3, None)]
ROW_SEEDS = [(0, 11), (2, 977)]      # (row of a 3-row batch, the row's seed): the key's row word and seed word


def admit(m, prompts):
    """three rows, each with its prompt and a current token (rows other than the one under test stay greedy)"""
    m.reset_cache()
    for r, p in enumerate(prompts):
        m.forward_row(r, p)


def start_sampled(m, prompts, row, cfg, seed):
    admit(m, prompts)
    for r in range(len(prompts)):
        if r != row:
            m.sample_row(r, GREEDY)
    m.set_row_sampler(row, cfg, seed)
    return int(m.sample_row(row, cfg, seed))


def wrong_at(ids, j, vocab):
    d = list(ids)
    if j is not None:
        d[j] = (d[j] + 1) % vocab
    return d


def expected_from_pass(m, cfg, seed, past, row, draft, stats):
    """s[i] of every position from the pass's own logits, the accept rule walked in Python -> (ids the call must return, pass logits)"""
    L = m.pass_logits()
    assert L.shape[0] == len(draft) + 1
    draws = []
    for i in range(L.shape[0]):
        s, p = expected_draw(cfg, L[i], seed, past + i + 1, row)
        draws.append(s)
        stats["draws"] += 1
        stats["off_argmax"] += int(s != int(np.argmax(L[i])))
        stats["band"] += int(s in top_p_band(cfg, L[i]))
    return walk(draws, draft), L


@pytest.mark.parametrize("name,dtype,vocab,paged", [(n, d, v, p) for n, d, v in MODELS for p in (0, 1) if not (p and (d == "fp32" or v != V))])
def test_exact_draws_at_every_position(name, dtype, vocab, paged, oracle_lib):
    """Context A steps (tgx_decode_rows), context B — same kernels, same bits, same t0 — verifies A's ids as a draft, wrong at index j or nowhere.  What B must
    return is computed from B's own pass logits; nothing is skipped.  Per configuration at least 25 % of the compared draws differ from their position's argmax
    (a test that an argmax in place of the draw would pass shows nothing), and at least 80 % of the all-right drafts are accepted whole (the two paths differ by
    summation order alone).  No position's expected draw lands in the top-p band (module docstring): the count is asserted to be 0."""
    budget = 3 * CTX if paged else 0
    A, B = gpu_model(name, dtype, 3, budget, vocab=vocab), gpu_model(name, dtype, 3, budget, vocab=vocab)
    band_total = 0
    for cname, cfg in configs(name).items():
        stats = {"draws": 0, "off_argmax": 0, "band": 0}
        whole, whole_ok = 0, 0
        for row, seed in ROW_SEEDS:
            for past in sorted({c[0] for c in CASES}):
                prompts = [synth.synth_prompt(vocab, past if r == row else 5, 31 + r) for r in range(3)]
                t0 = start_sampled(A, prompts, row, cfg, seed)
                c_ids = [int(t) for t in A.decode_rows(K)[0][:, row]]
                for _, n_draft, j in [c for c in CASES if c[0] == past]:
                    what = (name, dtype, vocab, paged, cname, row, seed, past, n_draft, j)
                    assert start_sampled(B, prompts, row, cfg, seed) == t0, what
                    draft = wrong_at(c_ids[:n_draft], j, vocab)
                    ids, fin = B.verify_row_sampled(row, draft)
                    want, L = expected_from_pass(B, cfg, seed, past, row, draft, stats)
                    assert list(ids) == want and fin == 0, (what, list(ids), want)
                    assert B.past_length_row(row) == past + len(want), what
                    # the row afterwards: the logits of the position that produced the last id, bit for bit, and the same draw from them again
                    np.testing.assert_array_equal(B.logits(rounded=False)[row], L[len(want) - 1], err_msg=str(what))
                    assert int(B.sample_row(row, cfg, seed)) == want[-1], what
                    if j is None:
                        whole += 1
                        whole_ok += int(len(want) == n_draft + 1)
        assert stats["off_argmax"] >= 0.25 * stats["draws"], (name, cname, stats)
        assert whole_ok >= 0.8 * whole, (name, cname, whole_ok, whole)
        band_total += stats["band"]
    assert band_total == 0, band_total
    A.close(); B.close()


@pytest.mark.parametrize("fam,dtype", [("llama_tiny", "bf16"), ("qwen3_tiny", "bf16"), ("gpt2_hd64", "bf16"), ("mistral_tiny", "fp16")])
def test_the_pass_against_a_control_row_and_the_oracle(fam, dtype, oracle_lib):
    """every position's logits of the pass: against a control row fed the same inputs one token at a time (GPU to GPU: 1e-3) and against the CPU oracle given the
    whole sequence (1e-2); the live cache rows against the control's by check_kv"""
    from oracle.oracle_ffi import OracleModel
    cfg_, g = load_golden(fam)

    def desc():
        d = desc_from_hf_config(cfg_, dtype, max_batch=1); d.max_ctx = 64
        if d.n_positions > 0:
            d.n_positions = max(d.n_positions, 64)
        return d
    gpu = Model(desc()).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    ctrl = Model(desc()).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    ref = OracleModel(desc()).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    vocab = gpu.desc.vocab
    prompt = np.random.default_rng(5).integers(0, vocab, 9).astype(np.int64)
    cfg = SamplerCfg(1.0, 0, 0.95, 0.0)
    for n_draft, seed in ((6, 3), (15, 4), (2, 5)):
        gpu.reset_cache(); gpu.forward_row(0, prompt); gpu.set_row_sampler(0, cfg, seed)
        t0 = int(gpu.sample_row(0, cfg, seed))
        draft = np.random.default_rng(seed).integers(0, vocab, n_draft).astype(np.int64)
        ids, fin = gpu.verify_row_sampled(0, draft)
        L = gpu.pass_logits()
        inputs = [t0] + [int(t) for t in draft]
        ctrl.reset_cache(); ctrl.forward_row(0, prompt)
        ref.reset_cache(); ref.forward(prompt[None, :])
        for i, t in enumerate(inputs):
            ctrl.extend_row(0, [t]); ref.forward(np.array([[t]], dtype=np.int64))
            lc, lr = ctrl.logits(rounded=False)[0], ref.logits(rounded=False)[0]
            assert rel_err(L[i][None, :], lc[None, :]) < 1e-3, (fam, n_draft, i, rel_err(L[i][None, :], lc[None, :]))
            assert rel_err(L[i][None, :], lr[None, :]) < 1e-2, (fam, n_draft, i, rel_err(L[i][None, :], lr[None, :]))
            if i + 1 == len(ids):                                         # the control holds exactly the row's live positions now
                assert gpu.past_length_row(0) == ctrl.past_length_row(0) == len(prompt) + len(ids)
                check_kv(kv_all(gpu, 0), kv_all(ctrl, 0), dtype, (fam, n_draft))
    gpu.close(); ctrl.close(); ref.close()


def test_the_row_afterwards_steps_like_a_control():
    """at every rejection index: four forced steps equal a control that took the same ids by tgx_decode_rows-equivalent means (tgx_extend_row of the accepted
    inputs), and tgx_read_probs has no vector for the row"""
    name, dtype = "llama-3.2-1b", "bf16"
    gpu, ctrl = gpu_model(name, dtype), gpu_model(name, dtype)
    cfg, seed, past = configs(name)["top-p"], 5, 40
    prompt = synth.synth_prompt(V, past, 3)
    t0 = start_sampled(gpu, [prompt], 0, cfg, seed)
    c_ids = [int(t) for t in gpu.decode_rows(8)[0][:, 0]]
    for j in (0, 3, None):
        assert start_sampled(gpu, [prompt], 0, cfg, seed) == t0
        assert gpu.probs()[0].sum() > 0.99                                # the sampled first token left a vector ...
        ids, fin = gpu.verify_row_sampled(0, wrong_at(c_ids[:7], j, V))
        with pytest.raises(TgxError) as ei:                               # ... the verify pass leaves none (its scratch is not the row's)
            gpu.probs()
        assert ei.value.status == 4
        ctrl.reset_cache(); ctrl.forward_row(0, prompt)
        ctrl.extend_row(0, [t0] + [int(t) for t in ids[:-1]])             # every input that produced a token
        assert gpu.past_length_row(0) == ctrl.past_length_row(0) == past + len(ids)
        lg, lc = gpu.logits(rounded=False)[0], ctrl.logits(rounded=False)[0]
        assert rel_err(lg[None, :], lc[None, :]) < 1e-3
        check_kv(kv_all(gpu, 0), kv_all(ctrl, 0), dtype, j)
        gpu.set_row_sampler(0, GREEDY, 0)
        for t in FORCED:
            tg, tc = force(gpu, np.array([t])), force(ctrl, np.array([t]))
            check_row(gpu.logits(rounded=False)[0], tg[0], ctrl.logits(rounded=False)[0], tc[0])
        assert gpu.past_length_row(0) == past + len(ids) + len(FORCED)
    gpu.close(); ctrl.close()


def test_greedy_through_the_new_entry_is_verify_row(oracle_lib):
    """ids, logits slot, every cache row, kv.free_tokens and mem.live_allocs of a greedy call through tgx_verify_row_sampled are tgx_verify_row's, bit for bit"""
    a, b = gpu_model("llama-3.2-1b", "bf16", 1, 2 * CTX), gpu_model("llama-3.2-1b", "bf16", 1, 2 * CTX)
    for past, n_draft, j in ((5, 3, 1), (126, 7, None), (600, 15, 9)):
        prompt = synth.synth_prompt(V, past, 77)
        for m in (a, b):                                                   # (both contexts take the same calls: their allocation counts stay comparable)
            m.reset_cache(); m.forward_row(0, prompt); m.sample_row(0, GREEDY)
            steps = [int(t) for t in m.decode_rows(n_draft)[0][:, 0]]
        draft = wrong_at(steps, j, V)
        outs = []
        for m, call in ((a, a.verify_row), (b, b.verify_row_sampled)):
            m.reset_cache(); m.forward_row(0, prompt); m.sample_row(0, GREEDY)
            ids, fin = call(0, draft)
            outs.append((list(ids), fin, m.logits(rounded=False)[0].copy(), kv_all(m, 0), m.get_option("kv.free_tokens"), m.get_option("mem.live_allocs"), m.pass_logits()))
        x, y = outs
        assert x[0] == y[0] and x[1] == y[1] and x[4] == y[4] and x[5] == y[5], (past, n_draft, j, x[0], y[0], x[4:6], y[4:6])
        np.testing.assert_array_equal(x[2], y[2]); np.testing.assert_array_equal(x[6], y[6])
        for (k1, v1), (k2, v2) in zip(x[3], y[3]):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    a.close(); b.close()


@pytest.mark.parametrize("name,dtype", [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16")])
def test_sampled_verify_is_deterministic_and_paged_equals_unpaged(name, dtype):
    flat, paged = gpu_model(name, dtype), gpu_model(name, dtype, 1, 2 * CTX)
    cfg, seed = configs(name)["all"], 21
    for past, n_draft in ((5, 3), (126, 7), (600, 15)):
        prompt = synth.synth_prompt(V, past, 77)
        runs = []
        for m in (flat, paged):
            start_sampled(m, [prompt], 0, cfg, seed)
            draft = [int(t) for t in m.decode_rows(n_draft)[0][:, 0]]
            two = []
            for _ in range(2):
                start_sampled(m, [prompt], 0, cfg, seed)
                ids, fin = m.verify_row_sampled(0, draft)
                two.append((list(ids), fin, m.logits(rounded=False)[0].copy(), m.pass_logits(), kv_all(m, 0), int(m.decode_rows(1)[0][0, 0])))
            runs.append(two[0])
            for x, y in ((two[0], two[1]), ):
                assert x[0] == y[0] and x[1] == y[1] and x[5] == y[5]
                np.testing.assert_array_equal(x[2], y[2]); np.testing.assert_array_equal(x[3], y[3])
                for (k1, v1), (k2, v2) in zip(x[4], y[4]):
                    np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
        x, y = runs
        assert x[0] == y[0] and x[5] == y[5], (name, past, "paged vs unpaged")
        np.testing.assert_array_equal(x[2], y[2]); np.testing.assert_array_equal(x[3], y[3])
        for (k1, v1), (k2, v2) in zip(x[4], y[4]):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    flat.close(); paged.close()


def test_stop_conditions_end_the_walk_under_sampling(oracle_lib):
    name = "llama-3.2-1b"
    m = gpu_model(name, "bf16", 1, 2 * CTX)
    cfg, seed, past = configs(name)["T"], 9, 40
    prompt = synth.synth_prompt(V, past, 3)
    stats = {"draws": 0, "off_argmax": 0, "band": 0}
    t0 = start_sampled(m, [prompt], 0, cfg, seed)
    # an all-right draft built position by position from the passes' own draws (each pass reveals at least one more of them)
    steps = []
    while len(steps) < 7:
        assert start_sampled(m, [prompt], 0, cfg, seed) == t0
        draft = steps + [0] * (7 - len(steps))
        ids, _ = m.verify_row_sampled(0, draft)
        want, _ = expected_from_pass(m, cfg, seed, past, 0, draft, stats)
        assert list(ids) == want and want[:len(steps)] == steps
        steps = want[:len(steps) + 1]
    assert len(set(steps[:3])) == 3
    # a stop id at accepted index 2
    assert start_sampled(m, [prompt], 0, cfg, seed) == t0
    m.set_row_stop(0, 0, [steps[2]])
    ids, fin = m.verify_row_sampled(0, steps[:7])
    assert list(ids) == steps[:3] and fin == 1 and m.past_length_row(0) == past + 3
    assert m.get_option("kv.free_tokens") == 2 * CTX - BLK
    with pytest.raises(TgxError) as ei:                                   # finished: as after tgx_decode_rows
        m.verify_row_sampled(0, steps[3:5])
    assert ei.value.status == 4
    # max_new = 2
    assert start_sampled(m, [prompt], 0, cfg, seed) == t0
    m.set_row_stop(0, 2, [])
    ids, fin = m.verify_row_sampled(0, steps[:7])
    assert list(ids) == steps[:2] and fin == 2 and m.past_length_row(0) == past + 2
    # the first position's draw is a stop id
    assert start_sampled(m, [prompt], 0, cfg, seed) == t0
    m.set_row_stop(0, 0, [steps[0]])
    ids, fin = m.verify_row_sampled(0, steps[:3])
    assert list(ids) == steps[:1] and fin == 1 and m.past_length_row(0) == past + 1
    m.close()


def test_logprob_records_of_a_sampled_verify():
    """one record per produced token = the fp64 log-softmax of the pass's logits at the position that produced it (2e-5, the row fuzz's lp_tol): the model's
    distribution, whatever the sampler"""
    name = "llama-3.2-1b"
    m = gpu_model(name, "bf16")
    cfg, seed, past = configs(name)["top-k"], 13, 20
    prompt = synth.synth_prompt(V, past, 8)
    m.reset_cache(); m.forward_row(0, prompt); m.set_row_logprobs(0, 3); m.set_row_sampler(0, cfg, seed)
    m.sample_row(0, cfg, seed)
    draft = [int(t) for t in m.decode_rows(7)[0][:, 0]]
    m.reset_cache(); m.forward_row(0, prompt); m.set_row_logprobs(0, 3); m.set_row_sampler(0, cfg, seed)
    m.sample_row(0, cfg, seed)
    ids, fin = m.verify_row_sampled(0, draft[:5] + [(draft[5] + 1) % V, draft[6]])
    L = m.pass_logits().astype(np.float64)
    lp, top_ids, top_lp, top_n = m.row_logprobs(0, len(ids))
    for i, t in enumerate(ids):
        ls = L[i] - (L[i].max() + np.log(np.exp(L[i] - L[i].max()).sum()))
        assert abs(lp[i] - ls[t]) < 2e-5, (i, lp[i], ls[t])
        order = np.lexsort((np.arange(V), -L[i]))[:3]
        assert list(top_ids[i][:3]) == [int(o) for o in order] and top_n[i] == 3
        np.testing.assert_allclose(top_lp[i][:3], ls[order], atol=2e-5, rtol=0)
    m.close()


def test_every_refusal_is_repeated_and_changes_nothing():
    budget = 4 * BLK
    gpu, ctrl = gpu_model("llama-3.2-1b", "bf16", 4, budget), gpu_model("llama-3.2-1b", "bf16", 4, budget)
    prompts = np.stack([synth.synth_prompt(V, 30, 11 + r) for r in range(3)])
    for m in (gpu, ctrl):
        m.forward(prompts); m.sample(GREEDY)
        m.reset_row(2)                                                    # row 2 retired; row 3 never used
    allocs0 = gpu.get_option("mem.live_allocs")

    def state():
        return ([gpu.past_length_row(r) for r in range(4)], gpu.get_option("kv.free_tokens"), gpu.logits(rounded=False).copy(), gpu.get_option("mem.live_allocs"))

    def refused(status, row, draft, call=None):
        s0 = state()
        with pytest.raises(TgxError) as ei:
            (call or gpu.verify_row_sampled)(row, draft)
        assert ei.value.status == status, (status, row, draft, str(ei.value))
        s1 = state()
        assert s0[0] == s1[0] and s0[1] == s1[1] and s0[3] == s1[3]
        np.testing.assert_array_equal(s0[2], s1[2])

    with pytest.raises(TgxError) as ei:                                   # no verify pass yet
        gpu.pass_logits()
    assert ei.value.status == 4
    refused(1, -1, [1]); refused(1, 4, [1])                               # row outside [0, max_batch)
    refused(1, 0, []); refused(1, 0, [1] * 16)                            # n_draft outside [1, 15]
    refused(1, 0, [1, V]); refused(1, 0, [-1])                            # a draft id out of range
    n, f = c_int32(), c_int32()
    out = (c_int64 * 16)()
    d = (c_int64 * 2)(1, 2)
    be, ctx = gpu.be, gpu._ctx
    assert be.verify_row_sampled(ctx, 0, None, 2, out, ctypes.byref(n), ctypes.byref(f)) == 1      # null pointers
    assert be.verify_row_sampled(ctx, 0, d, 2, None, ctypes.byref(n), ctypes.byref(f)) == 1
    assert be.verify_row_sampled(ctx, 0, d, 2, out, None, ctypes.byref(f)) == 1
    assert be.verify_row_sampled(ctx, 0, d, 2, out, ctypes.byref(n), None) == 1
    refused(4, 2, [1]); refused(4, 3, [1])                                # a retired row, an empty one
    gpu.set_row_sampler(1, SamplerCfg(temperature=0.7), 3)
    refused(2, 1, [1, 2], call=gpu.verify_row)                            # tgx_verify_row on a sampled row: STILL unsupported
    gpu.set_row_penalties(1, repetition=1.3)
    allocs1 = gpu.get_option("mem.live_allocs")                           # (the processors' buffers)
    refused(2, 1, [1, 2])                                                 # a logit processor on
    gpu.set_row_penalties(1); gpu.set_row_sampler(1, GREEDY, 0)
    assert allocs1 >= allocs0 and gpu.get_option("mem.live_allocs") == allocs1      # no refusal allocated anything
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
    # the context size, under sampling
    m = gpu_model("llama-3.2-1b", "bf16", 1)
    cfg = SamplerCfg(100.0, 0, 0.9, 0.0)
    start_sampled(m, [synth.synth_prompt(V, CTX - 4, 5)], 0, cfg, 1)
    l0 = m.logits(rounded=False).copy()
    with pytest.raises(TgxError) as ei:
        m.verify_row_sampled(0, [1, 2, 3, 4])                             # past + 5 > max_ctx
    assert ei.value.status == 8 and m.past_length_row(0) == CTX - 4
    np.testing.assert_array_equal(m.logits(rounded=False), l0)
    ids, fin = m.verify_row_sampled(0, [1, 2, 3])                         # past + 4 == max_ctx fits
    assert len(ids) >= 1
    m.close()


def test_read_pass_logits_state_and_memory():
    """TGX_ERR_STATE before any pass, after tgx_score_row's group form and after tgx_reset_cache; cap_rows below the pass's positions is TGX_ERR_INVALID and writes
    nothing; a context that never calls the new entry on a sampled row keeps its mem.live_allocs, the first such call allocates four buffers, later ones none"""
    name = "llama-3.2-1b"
    m = gpu_model(name, "bf16", 2)
    cfg, seed = configs(name)["top-p"], 2
    prompt = synth.synth_prompt(V, 20, 4)
    for n in (5, 15, 3):                                                  # the greedy entry's workspaces at every size used below
        m.reset_cache(); m.forward_row(0, prompt); m.sample_row(0, GREEDY)
        m.verify_row(0, list(range(1, n + 1)))
    base = m.get_option("mem.live_allocs")
    assert m.pass_logits().shape == (4, V)
    m.reset_cache(); m.forward_row(0, prompt); m.sample_row(0, GREEDY)
    m.verify_row_sampled(0, [1, 2, 3])                                   # greedy through the new entry: nothing new
    assert m.get_option("mem.live_allocs") == base
    buf = np.full((3, V), 7.0, np.float32)
    rows = c_int32(-1)
    assert m.be.read_pass_logits(m._ctx, buf.ctypes.data_as(POINTER(c_float)), 3, ctypes.byref(rows)) == 1      # 3 < 4
    assert (buf == 7.0).all() and rows.value == -1
    assert m.be.read_pass_logits(m._ctx, None, 16, ctypes.byref(rows)) == 1
    assert m.be.read_pass_logits(m._ctx, buf.ctypes.data_as(POINTER(c_float)), 16, None) == 1
    start_sampled(m, [prompt], 0, cfg, seed)
    m.verify_row_sampled(0, [1, 2, 3, 4, 5])
    assert m.get_option("mem.live_allocs") == base + 4                   # scratch, two lists, the draws
    assert m.pass_logits().shape == (6, V)
    start_sampled(m, [prompt], 0, cfg, seed)
    m.verify_row_sampled(0, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])
    assert m.get_option("mem.live_allocs") == base + 4
    m.score_row(1, synth.synth_prompt(V, 9, 6))                          # 9 positions: the group form uses the workspace
    if m.get_option("score.last_form") == 2:
        with pytest.raises(TgxError) as ei:
            m.pass_logits()
        assert ei.value.status == 4
    m.reset_cache()
    with pytest.raises(TgxError) as ei:
        m.pass_logits()
    assert ei.value.status == 4
    m.close()


@pytest.mark.parametrize("paged", [0, 1])
def test_sampled_verify_in_a_running_batch_leaves_the_other_rows_alone(paged):
    name = "llama-3.2-1b"
    budget = 6 * BLK if paged else 0
    gpu, ctrl = gpu_model(name, "bf16", 3, budget), gpu_model(name, "bf16", 3, budget)
    prompts = np.stack([synth.synth_prompt(V, 50, 60 + r) for r in range(3)])
    cfg, seed = configs(name)["top-k+top-p"], 6
    for m in (gpu, ctrl):
        m.forward(prompts); m.sample(GREEDY); m.decode(2, GREEDY)
        m.set_row_sampler(1, cfg, seed)
    look = [int(t) for t in ctrl.decode_rows(4)[0][:, 1]]                 # row 1's next ids, from a throw-away run of the control
    ctrl.reset_cache(); ctrl.forward(prompts); ctrl.sample(GREEDY); ctrl.decode(2, GREEDY); ctrl.set_row_sampler(1, cfg, seed)
    ids, fin = gpu.verify_row_sampled(1, look[:3])
    assert 1 <= len(ids) <= 4 and fin == 0
    assert [gpu.past_length_row(r) for r in range(3)] == [52, 52 + len(ids), 52]
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
    gpu.close(); ctrl.close()


# ---- the host engine and the CLI: GPTConfig::speculateSampled
SPEC_PROMPT = [11, 12, 13, 14, 15, 16, 7, 8, 11, 12, 13, 14, 15, 16, 9, 11, 12, 13]      # a repeated span: the lookup finds a draft from the first iteration on


def spec_engine(tmp_path):
    from ctypes import c_int, c_void_p
    from host_util import HostEngine, host_lib, write_model_dir
    cfg, g = load_golden("llama_tiny")
    cfg = dict(cfg, tie_word_embeddings=False)
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]), peaked=True, eos=[cfg["vocab_size"] - 1])
    lib = host_lib()
    lib.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    lib.tgxe_set_speculate_sampled.argtypes = [c_void_p, c_int]
    lib.tgxe_spec_stats.restype = c_int
    lib.tgxe_spec_stats.argtypes = [c_void_p, POINTER(c_int64), c_int]
    lib.tgxe_ctx.restype = c_void_p
    lib.tgxe_ctx.argtypes = [c_void_p]
    e = HostEngine(lib, model_dir=str(tmp_path), device="mi355x", dtype=1)
    assert e.prepare(), e.error()
    return e, lib, cfg["vocab_size"]


def stats(e):
    buf = (c_int64 * 32)()
    e.lib.tgxe_spec_stats(e.h, buf, 32)
    return list(buf[:21])


def test_host_engine_speculate_sampled(tmp_path, oracle_lib):
    """the CLI's default sampler (T 0.8 / top-p 0.9, the engine's seed) with speculate = 7.  speculateSampled off: the run of today, nothing drafted.  On: verify
    passes ran and the ids are the plain loop's — compared up to the first position at which the two paths' draws differ, which in this committed case is the
    end of the sequence (asserted).  The last pass is also restated from its own logits, read through the engine's context: the ids it produced are the draws
    of (the engine's seed, past + i + 1, row 0) from those logits."""
    from tinygpt_amd.ffi import product_backend
    e, lib, vocab = spec_engine(tmp_path)
    n_new = 40
    sampler = dict(temperature=0.8, top_p=0.9)
    runs = {}
    for on in (0, 1):
        lib.tgxe_set_speculate(e.h, 7)
        lib.tgxe_set_speculate_sampled(e.h, on)
        e.reconfigure(max_new=n_new, **sampler)
        ids, new, fin = e.generate_sync([SPEC_PROMPT])
        last = None
        if on:                                                            # the last verify pass, before anything else uses the workspace
            be = product_backend()
            L = np.empty((16, vocab), np.float32)
            m = c_int32(0)
            assert be.read_pass_logits(lib.tgxe_ctx(e.h), L.ctypes.data_as(POINTER(c_float)), 16, ctypes.byref(m)) == 0
            last = L[:m.value].copy()
        e.reconfigure(max_new=n_new, **sampler)
        aids, anew, afin, seen = e.generate_async(SPEC_PROMPT)
        runs[on] = (ids.tolist(), new, fin, aids.tolist(), anew, afin, seen)
        if not on:
            assert stats(e) == [0] * 21
    s = stats(e)
    assert s[0] >= 1, s                                                   # verify passes ran
    first_diff = next((i for i, (a, b) in enumerate(zip(runs[0][0][0], runs[1][0][0])) if a != b), len(runs[0][0][0]))
    assert first_diff == len(runs[0][0][0]) == len(runs[1][0][0]), first_diff      # the end of the sequence
    assert runs[0] == runs[1]
    # the last pass from its own logits: for some produced count n <= M, the sequence's last n tokens are the draws of its first n positions
    seq = runs[1][0][0]
    cfg = SamplerCfg(0.8, 0, 0.9, 0.0)
    seed = 0                                                              # GPTConfig::seed's default (host/engine.h)
    ok = []
    for n in range(1, last.shape[0] + 1):
        past = len(seq) - 1 - n                                           # the pass's first input sat at index `past`; its n produced tokens end the sequence
        draws = [expected_draw(cfg, last[i], seed, past + i + 1, 0)[0] for i in range(n)]
        ok.append(draws == seq[len(seq) - n:])
    assert any(ok), ok
    e.close()


def test_cli_speculate_sampled(tmp_path):
    from host_util import write_model_dir
    cfg, g = load_golden("llama_tiny")
    cfg = dict(cfg, tie_word_embeddings=False)
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]), peaked=True)
    _, cli = build.build_host()
    base = [cli, "--model", str(tmp_path), "--device", "mi355x", "--dtype", "bf16", "--max-tokens", "40", "--temperature", "0.8", "--top-p", "0.9",
            "--prompt-ids", ",".join(str(t) for t in SPEC_PROMPT), "--speculate", "7"]
    outs = []
    for extra in ([], ["--speculate-sampled"]):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        outs.append(out.stdout)
    rows = [[l for l in o.splitlines() if l.startswith("Output ids:")] for o in outs]
    assert rows[0] == rows[1] and len(rows[0]) == 1
    lines = [[l for l in o.splitlines() if l.startswith("speculate:")][0].split() for o in outs]
    assert int(lines[0][1]) == 0 and int(lines[1][1]) >= 1, lines        # "speculate: N verify passes, ..."
