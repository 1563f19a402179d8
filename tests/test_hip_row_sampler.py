"""Per-row sampler settings and device-side stop in batched decode (include/tgx.h: tgx_set_row_sampler / tgx_set_row_stop / tgx_decode_rows) — the request
half of continuous batching: the reference reconfigures its engine per request (server/HttpServer.cpp:118-163 -> src/engine/GPTEngine.cpp:67-84) and checks
EOS per token (GPTEngine.cpp:196-217).  Held to:
  * draw identity: a row of a mixed batch == tgx_decode with that row's cfg and seed on the whole batch (a "twin" context on the same prompts), bit for bit —
    ids, fp32 logits and the probability vector — on the GEMV step (2 rows) and the matrix-core step (8 / 32 rows), one step per call and across graphs;
  * the oracle's ids for a 4-row batch under per-row settings (unpaged and paged);
  * a changed setting takes effect in the next call (no stale captured value);
  * stops on the device: counts, finish reasons, -1 after the finish, lengths, the cache of a stopped row, untouched neighbours;
  * lifecycle (reset / refill of a stopped row), paged blocks returned after a stop, and the error statuses the header names."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu

ST_INVALID, ST_STATE = 1, 4
# greedy, the CLI default T 0.8 / top-p 0.9, T 1.0 / top-k 50, T 0.7 / min-p 0.05, and all four filters
MIX = [GREEDY, SamplerCfg(0.8, 0, 0.9, 0.0), SamplerCfg(1.0, 50, 1.0, 0.0), SamplerCfg(0.7, 0, 1.0, 0.05), SamplerCfg(0.9, 40, 0.95, 0.05)]
SEEDS = [11, 22, 33, 44, 55]


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def make(hip, B, fam="llama_tiny", budget=0, max_ctx=256):
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(cfg, "bf16", max_batch=B)
    d.max_ctx = max_ctx
    m = Model(d, hip)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(int(g["seed"]), float(g["std"])).finalize()


def prompts(B, S=9, seed=0, V=256):
    return np.random.default_rng(seed).integers(0, V, size=(B, S)).astype(np.int64)


def start_rows(m, P, k_of):
    """prefill the batch, then every row's first token under its own settings (what a server does per request)"""
    m.forward(P)
    for b in range(P.shape[0]):
        k = k_of(b)
        m.sample_row(b, MIX[k], SEEDS[k])
        m.set_row_sampler(b, MIX[k], SEEDS[k])


def twin(hip, B, P, k, **kw):
    t = make(hip, B, **kw)
    t.forward(P)
    t.sample(MIX[k], SEEDS[k])
    return t


def check_probs(pm, pt, b, k):
    if MIX[k].greedy:
        assert not pm[b].any()
    else:
        np.testing.assert_array_equal(pm[b], pt[b])


@pytest.mark.parametrize("B,per_call", [(2, 1), (2, 20), (8, 1), (8, 20), (32, 5)])
def test_mixed_configs_equal_uniform_twins(hip, B, per_call):
    """every row of a mixed batch == the twin decoding the whole batch with that row's cfg / seed; 20 steps per call cross the 16-step graph"""
    P = prompts(B, seed=B)
    k_of = lambda b: b % len(MIX)
    m = make(hip, B)
    start_rows(m, P, k_of)
    ks = sorted({k_of(b) for b in range(B)})
    tw = {k: twin(hip, B, P, k) for k in ks}
    n_calls = 20 // per_call if B < 32 else 2
    for _ in range(n_calls):
        ids, new, fin = m.decode_rows(per_call)
        assert (new == per_call).all() and not fin.any()
        lm, pm = m.logits(rounded=False), m.probs()
        for k, t in tw.items():
            it = t.decode(per_call, MIX[k], SEEDS[k])
            lt = t.logits(rounded=False)
            pt = t.probs() if not MIX[k].greedy else None
            for b in range(B):
                if k_of(b) != k:
                    continue
                np.testing.assert_array_equal(ids[:, b], it[:, b])
                np.testing.assert_array_equal(lm[b], lt[b])
                check_probs(pm, pt, b, k)


@pytest.mark.parametrize("budget", [0, 1024])
def test_per_row_settings_match_oracle(hip, oracle_lib, budget):
    """4 equal-length rows with 4 different settings: row b == row b of the oracle decoding the whole batch with cfg_b / seed_b"""
    from oracle.oracle_ffi import OracleModel
    cfg, g = load_golden("llama_tiny")
    d = desc_from_hf_config(cfg, "bf16", max_batch=4)
    P = prompts(4, seed=7)
    m = make(hip, 4, budget=budget)
    k_of = lambda b: b + 1            # the four sampled settings
    start_rows(m, P, k_of)
    ids, new, _ = m.decode_rows(12)
    assert (new == 12).all()
    for b in range(4):
        k = k_of(b)
        ref = OracleModel(d).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
        ref.forward(P)
        ref.sample(MIX[k], SEEDS[k])
        np.testing.assert_array_equal(ids[:, b], ref.decode(12, MIX[k], SEEDS[k])[:, b])


def test_setting_change_takes_effect(hip):
    """changing a row's temperature / top-k between calls: the second call equals the twin under the new cfg (no captured value survives)"""
    B = 8
    P = prompts(B, seed=3)
    m = make(hip, B)
    start_rows(m, P, lambda b: 2)
    t = twin(hip, B, P, 2)
    ids, _, _ = m.decode_rows(6)
    np.testing.assert_array_equal(ids, t.decode(6, MIX[2], SEEDS[2]))
    new_cfg = SamplerCfg(0.6, 20, 1.0, 0.0)
    for b in range(B):
        m.set_row_sampler(b, new_cfg, 99)
    ids, _, _ = m.decode_rows(6)
    np.testing.assert_array_equal(ids, t.decode(6, new_cfg, 99))
    np.testing.assert_array_equal(m.logits(rounded=False), t.logits(rounded=False))


@pytest.mark.parametrize("B", [2, 8])
def test_device_stop(hip, B):
    """rows finish at step 1, mid-call, across the 16-step graph boundary, by max_new, or never; counts, -1, lengths, caches and neighbours"""
    P = prompts(B, seed=5 + B)
    k_of = lambda b: (b + 1) % len(MIX)
    n = 24
    ref = make(hip, B)
    start_rows(ref, P, k_of)
    r_ids, _, _ = ref.decode_rows(n)
    m = make(hip, B)
    start_rows(m, P, k_of)
    before = [m.past_length_row(b) for b in range(B)]
    # step index (0-based) at which the row stops on a stop id: the first step, mid-call, across the graph boundary; row 2 by max_new only; the rest never
    want_step = {0: 0} if B == 2 else {0: 0, 1: 9, 3: 17, 5: 3}
    expect_new, expect_fin = {}, {}
    for b in range(B):
        s = want_step.get(b)
        if b == 2 and B > 2:                     # max_new only
            m.set_row_stop(b, max_new=7)
            expect_new[b], expect_fin[b] = 7, 2
        elif s is not None:
            tok = int(r_ids[s, b])
            first = int(np.nonzero(r_ids[:, b] == tok)[0][0])   # the first occurrence of that id is where the row stops
            m.set_row_stop(b, stop_ids=[tok, 100000])
            expect_new[b], expect_fin[b] = first + 1, 1
        else:
            expect_new[b], expect_fin[b] = n, 0
    ids, new, fin = m.decode_rows(n)
    for b in range(B):
        e = expect_new[b]
        assert new[b] == e and fin[b] == expect_fin[b], (b, new[b], fin[b], e, expect_fin[b])
        np.testing.assert_array_equal(ids[:e, b], r_ids[:e, b])
        assert (ids[e:, b] == -1).all()
        assert m.past_length_row(b) == before[b] + e
        if e < n:
            k, v = m.read_kv(b, 1)
            kr, vr = ref.read_kv(b, 1)
            np.testing.assert_array_equal(k, kr[:len(k)])
            np.testing.assert_array_equal(v, vr[:len(v)])
            assert len(k) == before[b] + e
    # unstopped rows continue bit-identically; stopped rows stay at -1 with their length
    ids2, new2, fin2 = m.decode_rows(5)
    r2, _, _ = ref.decode_rows(5)
    for b in range(B):
        if expect_new[b] < n:
            assert (ids2[:, b] == -1).all() and new2[b] == 0 and fin2[b] == expect_fin[b]
            assert m.past_length_row(b) == before[b] + expect_new[b]
        else:
            np.testing.assert_array_equal(ids2[:, b], r2[:, b])


def test_stopped_row_refill_and_paged_blocks(hip):
    """a stopped row is reset, refilled and decodes like its solo run; with a paged cache the stopped rows' surplus blocks go back to the pool"""
    B, budget = 8, 8192
    P = prompts(B, S=100, seed=9)
    m = make(hip, B, budget=budget)
    start_rows(m, P, lambda b: 0)
    for b in range(0, B, 2):
        m.set_row_stop(b, max_new=5 + b)
    ids, new, fin = m.decode_rows(40)
    lens = [m.past_length_row(b) for b in range(B)]
    assert lens == [100 + (5 + b if b % 2 == 0 else 40) for b in range(B)]
    blocks = sum((L + 127) // 128 for L in lens)
    assert m.get_option("kv.free_tokens") == budget // 128 * 128 - blocks * 128
    # refill row 2 with a fresh prompt; it decodes like the same prompt alone (batch-invariance bound of tests/test_hip_rows.py)
    q = prompts(1, S=13, seed=77)[0]
    with pytest.raises(TgxError) as ei:
        m.forward_row(2, q)
    assert ei.value.status == ST_STATE
    m.reset_row(2)
    m.forward_row(2, q)
    m.sample_row(2, GREEDY)
    solo = make(hip, 1)
    solo.forward(q[None, :])
    solo.sample(GREEDY)
    for _ in range(6):
        ids, new, _ = m.decode_rows(1)
        assert new[2] == 1 and new[0] == 0
        lb = m.logits(rounded=False)[2]
        s = solo.decode(1, GREEDY)[0, 0]
        l1 = solo.logits(rounded=False)[0]
        assert rel_err(lb[None, :], l1[None, :]) < 1e-3
        top2 = np.sort(l1)[-2:]
        if top2[1] - top2[0] > 2e-3 * np.abs(l1).max():
            assert ids[0, 2] == s
    assert m.past_length_row(2) == 13 + 6


def test_errors_leave_context_usable(hip):
    B = 2
    P = prompts(B, seed=12)
    m = make(hip, B)
    start_rows(m, P, lambda b: 1)
    t = twin(hip, B, P, 1)
    for call, status in [(lambda: m.set_row_sampler(5, MIX[1]), ST_INVALID), (lambda: m.set_row_sampler(-1, MIX[1]), ST_INVALID),
                         (lambda: m.set_row_stop(0, stop_ids=list(range(9))), ST_INVALID), (lambda: m.set_row_sampler(0, None), ST_INVALID),
                         (lambda: m.set_row_stop(2, max_new=1), ST_INVALID)]:
        with pytest.raises(TgxError) as ei:
            call()
        assert ei.value.status == status
    ids, _, _ = m.decode_rows(3)
    np.testing.assert_array_equal(ids, t.decode(3, MIX[1], SEEDS[1]))
    # row 0 finishes; uniform calls refuse, a refill into it refuses, decode_rows goes on with row 1
    m.set_row_stop(0, max_new=1)
    ids, new, fin = m.decode_rows(2)
    it = t.decode(2, MIX[1], SEEDS[1])
    assert new.tolist() == [1, 2] and fin.tolist() == [2, 0]
    np.testing.assert_array_equal(ids[:, 1], it[:, 1])
    for call in (lambda: m.decode(1, MIX[1], SEEDS[1]), lambda: m.step_async(MIX[1], SEEDS[1]), lambda: m.forward_row(0, P[0])):
        with pytest.raises(TgxError) as ei:
            call()
        assert ei.value.status == ST_STATE
    m.set_row_stop(1, max_new=1)
    ids, new, fin = m.decode_rows(1)
    assert fin.tolist() == [2, 2]
    with pytest.raises(TgxError) as ei:
        m.decode_rows(1)
    assert ei.value.status == ST_STATE
    # everything reset: the context decodes like its twin again
    m.reset_cache()
    t.reset_cache()
    m.forward(P); t.forward(P)
    np.testing.assert_array_equal(m.sample(MIX[1], 5), t.sample(MIX[1], 5))
    for b in range(B):
        m.set_row_sampler(b, MIX[1], 5)
    ids, new, fin = m.decode_rows(4)
    np.testing.assert_array_equal(ids, t.decode(4, MIX[1], 5))
