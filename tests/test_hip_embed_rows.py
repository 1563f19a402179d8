"""tgx_embed_rows (include/tgx.h; kernels/embed_pool.h): the pooled final-norm hidden state of several texts in one ragged pass without lm_head.

Section 1 holds the vectors to the CPU oracle WITHOUT touching it: an untied checkpoint whose lm_head is the identity on its first H rows (tests/embed_ref.py) makes the
oracle's unrounded logits [:H] its final-normed hidden row; the oracle is teacher-forced once per model over the shared 200 tokens and every text is a prefix of them.
Bound: conftest.rel_err < 1e-3, the project's bar for HIP against the oracle; the floor f of the existing path on the same quantity (tgx_forward_row logits [:H] on the
identity-head checkpoint against the oracle) is measured in the same test, and were f > 5e-4 the bound would be 2 f.  Normalised / truncated outputs: twice that bound
(the doubling test_hip_score_row.py uses for derived quantities).
Observed on an MI355X (profiles/embed_rows.txt): f = 1.89e-4 (llama_tiny bf16), 9.07e-5 (qwen3_tiny bf16), 3.91e-5 (qwen3_tiny fp16), slab and paged alike, so the
bound is 1e-3; the pooled vectors' own worst errors were 1.96e-4 / 9.35e-5 / 4.01e-5 (LAST), 1.22e-4 / 7.43e-5 / 1.92e-5 (MEAN), 3.84e-6 / 2.29e-6 / 2.44e-7 (FIRST).

Sections 2-6: every family (tied heads, GPT-2's ln_f, fp32 storage on both of its routes, prefill.mfma 0, real geometry) through W_head @ e == the plain pass's logits;
MEAN == the float64 mean of the prefixes' LAST vectors; bit reproducibility; batch invariance; live rows untouched; row state with and without release; refusals."""
import copy
import ctypes
from ctypes import POINTER, c_float, c_int32, c_int64

import numpy as np
import pytest

from conftest import GPU_FAMILIES, load_golden, rel_err
from embed_ref import POOLS, identity_head, pool_ref
from tinygpt_amd import synth
from tinygpt_amd.desc import desc_from_hf_config, known_desc
from tinygpt_amd.ffi import GREEDY, EmbedCfg, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu

ST_INVALID, ST_STATE, ST_CONTEXT = 1, 4, 8
BAR = 1e-3
LENS = (1, 3, 5, 31, 33, 130, 200)      # one below and one above each route and tile boundary, one across a 128-token KV block
N = 200


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def describe(fam, dtype, B, max_ctx=256, untie=False, **over):
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(dict(cfg, **over), dtype, max_batch=B)
    d.max_ctx = min(max_ctx, d.n_positions) if d.n_positions > 0 else max_ctx
    if untie:
        d.tied = False
    return d, g


def make(hip, B, fam="llama_tiny", dtype="bf16", budget=0, max_ctx=256, ident=False, options=(), **over):
    d, g = describe(fam, dtype, B, max_ctx, untie=ident, **over)
    m = Model(d, hip)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    if ident:
        m.load_state(identity_head(d, dict(synth.synth_checkpoint(d, int(g["seed"]), float(g["std"]))))).finalize()
    else:
        m.load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    for k, v in options:
        m.set_option(k, v)
    return m


def tokens(V, n=N, seed=7):
    return np.random.default_rng(seed + V).integers(0, V, n).astype(np.int64)


_hidden = {}


def oracle_hidden(oracle_lib, fam, dtype):
    """[N][H] float64: the oracle's final-normed hidden row of every position of tokens(V), once per model (read-only)"""
    if (fam, dtype) not in _hidden:
        from oracle.oracle_ffi import OracleModel
        d, g = describe(fam, dtype, 1, untie=True)
        ref = OracleModel(d).load_state(identity_head(d, dict(synth.synth_checkpoint(d, int(g["seed"]), float(g["std"]))))).finalize()
        ids = tokens(d.vocab)
        rows = []
        for t in range(N):
            ref.forward(ids[None, t:t + 1])
            v = ref.logits(rounded=False)[0]
            assert (v[d.hidden:] == 0).all()
            rows.append(v[:d.hidden].astype(np.float64))
        ref.close()
        h = np.stack(rows)
        h.setflags(write=False)
        _hidden[(fam, dtype)] = h
    return _hidden[(fam, dtype)]


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,dtype,budget", [("llama_tiny", "bf16", 0), ("llama_tiny", "bf16", 2048), ("qwen3_tiny", "bf16", 0), ("qwen3_tiny", "bf16", 2048),
                                              ("qwen3_tiny", "fp16", 0)])
def test_against_the_oracle(hip, oracle_lib, fam, dtype, budget):
    hid = oracle_hidden(oracle_lib, fam, dtype)
    H = hid.shape[1]
    one = make(hip, 1, fam, dtype, ident=True)
    ids = tokens(one.desc.vocab)
    f = 0.0
    for L in LENS:                                # the floor of the existing path on this quantity
        one.reset_cache()
        one.forward_row(0, ids[:L])
        f = max(f, rel_err(one.logits(rounded=False)[0, :H], hid[L - 1]))
    one.close()
    bound = BAR if f <= 5e-4 else 2 * f
    print(f"{fam} {dtype} paged={bool(budget)}: floor f = {f:.3e} -> bound {bound:.3e}")
    m = make(hip, 9, fam, dtype, budget, ident=True)
    m.forward_rows([0, 1, 2, 3], [ids[:9], ids[:4], ids[:40], ids[:2]])
    m.reset_row(1); m.reset_row(3)
    rows = [3, 4, 1, 5, 6, 8, 7]                  # scattered: two retired rows and the five next new ones
    texts = [ids[:L] for L in LENS]
    worst = {}
    for pool in POOLS:
        e = m.embed_rows(rows, texts, pool, normalize=False, release=True)
        assert e.shape == (len(LENS), H) and e.dtype == np.float32
        en = m.embed_rows(rows, texts, pool, normalize=True, release=True)
        et = m.embed_rows(rows, texts, pool, normalize=True, dims=64, release=True)
        assert et.shape == (len(LENS), 64)
        for i, L in enumerate(LENS):
            w = rel_err(e[i], pool_ref(hid[:L], pool, False))
            wn = rel_err(en[i], pool_ref(hid[:L], pool, True))
            wt = rel_err(et[i], pool_ref(hid[:L], pool, True, 64))
            print(f"  {pool} len {L}: raw {w:.3e} normalised {wn:.3e} truncated {wt:.3e}")
            worst[pool] = max(worst.get(pool, 0.0), w)
            assert w < bound, (pool, L, w)
            assert wn < 2 * bound and wt < 2 * bound, (pool, L, wn, wt)
            for v in (en[i], et[i]):
                assert abs(np.sqrt((v.astype(np.float64) ** 2).sum()) - 1) < 1e-5, (pool, L)
    print(f"  worst raw: {worst}")
    assert [m.past_length_row(r) for r in (0, 2)] == [9, 40]      # the live rows kept their sequences
    m.close()


# ---- 2. every family: W_head @ e == the plain pass's logits -------------------------------------------------------------------------------------------------
def head_matrix(d, seed, std):
    t = dict(synth.synth_checkpoint(d, seed, std))
    name = "lm_head.weight" if "lm_head.weight" in t else ("wte.weight" if "wte.weight" in t else "model.embed_tokens.weight")
    return synth.bf16_bits_to_f32(t[name]).astype(np.float64)


def check_head_identity(m, twin, W, prompts, what):
    rows = list(range(len(prompts)))
    e = m.embed_rows(rows, prompts, "last", normalize=False, release=True)
    for i, p in enumerate(prompts):
        twin.reset_cache()
        twin.forward_row(0, p)
        err = rel_err(W @ e[i].astype(np.float64), twin.logits(rounded=False)[0])
        print(f"{what} len {len(p)}: W_head @ e vs tgx_forward_row logits {err:.3e}")
        assert err < BAR, (what, len(p), err)


@pytest.mark.parametrize("fam", GPU_FAMILIES)
def test_every_family(hip, fam):
    over = dict(n_positions=256, n_ctx=256) if fam.startswith("gpt2") else {}
    d, g = describe(fam, "bf16", 4, **over)
    W = head_matrix(d, int(g["seed"]), float(g["std"]))
    m, twin = make(hip, 4, fam, **over), make(hip, 1, fam, **over)
    ids = tokens(d.vocab)
    check_head_identity(m, twin, W, [ids[:3], ids[:37], ids[:130], ids[:5]], fam)
    m.close(); twin.close()


def test_gpt2_fp32_storage_both_routes(hip):
    """gpt2_hd64 (the GPT-2 fixture the device library builds: head_dim 64) in fp32 storage, one length below and one above prefill.f32_min_rows: prefill by steps
    (the staged slices) and the fp32 matrix-core route"""
    over = dict(n_positions=256, n_ctx=256)
    d, g = describe("gpt2_hd64", "fp32", 2, **over)
    W = head_matrix(d, int(g["seed"]), float(g["std"]))
    m, twin = make(hip, 2, "gpt2_hd64", "fp32", **over), make(hip, 1, "gpt2_hd64", "fp32", **over)
    fmin = 40                                     # (the default is 16; 40 puts a whole staged slice and a ragged one below the threshold)
    m.set_option("prefill.f32_min_rows", fmin)
    ids = tokens(d.vocab)
    check_head_identity(m, twin, W, [ids[:fmin - 1], ids[:fmin + 1]], "gpt2_hd64 fp32")
    # MEAN over the staged slices (prefill by steps) against the LAST vectors of the prefixes, each embedded alone
    L = min(fmin - 1, 37)
    mean = m.embed_rows([0], [ids[:L]], "mean", normalize=False, release=True)[0]
    last = np.stack([m.embed_rows([0], [ids[:k]], "last", normalize=False, release=True)[0] for k in range(1, L + 1)]).astype(np.float64)
    assert rel_err(mean, last.mean(axis=0)) < BAR
    m.close(); twin.close()


def test_prefill_mfma_off(hip):
    d, g = describe("llama_tiny", "bf16", 2)
    W = head_matrix(d, int(g["seed"]), float(g["std"]))
    m, twin = make(hip, 2, options=[("prefill.mfma", 0)]), make(hip, 1)
    ids = tokens(d.vocab)
    check_head_identity(m, twin, W, [ids[:37], ids[:70]], "prefill.mfma 0")
    mean = m.embed_rows([0], [ids[:70]], "mean", normalize=False, release=True)[0]      # three staged slices: 32 + 32 + 6
    ref = make(hip, 1)
    assert rel_err(mean, ref.embed_rows([0], [ids[:70]], "mean", normalize=False, release=True)[0]) < BAR
    m.close(); twin.close(); ref.close()


@pytest.mark.parametrize("name", ["llama-3.2-1b", "qwen3-1.7b"])
def test_real_geometry_slice(hip, name):
    """2 layers and vocabulary 4096 of the real geometry (tests/test_hip_forward_rows.py::real): head_dim 64, and head_dim 128 with q/k norm"""
    d = copy.deepcopy(known_desc(name, "bf16"))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 2, 4096, 256, 3
    d1 = copy.deepcopy(d); d1.max_batch = 1
    W = head_matrix(d, 1234, 0.02)
    m, twin = Model(d, hip).load_synthetic(1234, 0.02).finalize(), Model(d1, hip).load_synthetic(1234, 0.02).finalize()
    ids = tokens(d.vocab)
    check_head_identity(m, twin, W, [ids[:33], ids[:130], ids[:3]], name)
    m.close(); twin.close()


# ---- 3. self-consistency of MEAN ----------------------------------------------------------------------------------------------------------------------------
def test_mean_is_the_mean_of_the_prefixes_last(hip):
    m = make(hip, 4)
    ids = tokens(m.desc.vocab)[:37]
    mean = m.embed_rows([0], [ids], "mean", normalize=False, release=True)[0]
    last = [m.embed_rows([0], [ids[:k]], "last", normalize=False, release=True)[0] for k in range(1, 38)]
    err = rel_err(mean, np.stack(last).astype(np.float64).mean(axis=0))
    print(f"MEAN of 37 tokens vs the float64 mean of its prefixes' LAST: {err:.3e}")
    assert err < BAR
    first = m.embed_rows([0], [ids], "first", normalize=False, release=True)[0]
    assert rel_err(first, last[0]) < BAR
    m.close()


# ---- 4. reproducibility and isolation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [0, 2048])
def test_same_bits_and_batch_invariance(hip, budget):
    m = make(hip, 5, budget=budget)
    V = m.desc.vocab
    rng = np.random.default_rng(5)
    texts = [rng.integers(0, V, L).astype(np.int64) for L in (70, 3, 33, 130, 9)]
    for pool in POOLS:
        a = m.embed_rows(range(5), texts, pool, release=True)
        b = m.embed_rows(range(5), texts, pool, release=True)
        np.testing.assert_array_equal(a, b, err_msg=pool)
        for i in (0, 3):                          # alone and inside the group of five
            alone = m.embed_rows([2], [texts[i]], pool, release=True)[0]
            assert rel_err(a[i], alone) < BAR, (pool, i)
    launches = m.get_option("embed.last_pool_launches")
    assert launches == 2                          # a one-row matrix-core pass: one partials launch, one finish
    m.embed_rows(range(5), texts, "mean", release=True)
    assert m.get_option("embed.last_pool_launches") == 2      # ... and so for five texts in one ragged pass
    m.close()


def test_rows_not_named_stay_bit_identical(hip):
    V = 256
    rng = np.random.default_rng(9)
    P = lambda n: rng.integers(0, V, n).astype(np.int64)
    p = [P(20), P(140), P(5), P(6)]
    texts = [P(50), P(131)]
    seeded = SamplerCfg(0.8, 40, 0.95, 0.0)
    obs = []
    for embeds in (True, False):
        x = make(hip, 4, budget=2048)
        x.forward_rows([0, 1, 2, 3], p)
        for r in range(4):
            x.set_row_sampler(r, seeded if r == 1 else GREEDY, 11 + r)
            x.sample_row(r, GREEDY)
        x.decode_rows(3)
        x.reset_row(2); x.reset_row(3)
        free = x.get_option("kv.free_tokens")
        if embeds:
            for pool in POOLS:
                x.embed_rows([3, 2], texts, pool, release=True)
            assert x.get_option("kv.free_tokens") == free
        o = {"logits": x.logits(rounded=False)[:2].copy(), "kv": [x.read_kv(r, layer) for r in (0, 1) for layer in range(2)],
             "len": [x.past_length_row(r) for r in range(4)]}
        o["next"] = x.decode_rows(4)[0][:, :2].copy()
        o["logits_after"] = x.logits(rounded=False)[:2].copy()
        obs.append(o)
        x.close()
    a, b = obs
    for k in ("logits", "len", "next", "logits_after"):
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
    for (k0, v0), (k1, v1) in zip(a["kv"], b["kv"]):
        np.testing.assert_array_equal(k0, k1); np.testing.assert_array_equal(v0, v1)


# ---- 5. row state -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [0, 2048])
def test_row_state_without_release(hip, budget):
    m, plain, twin = make(hip, 3, budget=budget), make(hip, 3, budget=budget), make(hip, 1)
    V = m.desc.vocab
    rng = np.random.default_rng(21)
    texts = [rng.integers(0, V, L).astype(np.int64) for L in (40, 3, 131)]
    tail = rng.integers(0, V, 3).astype(np.int64)
    m.embed_rows([0, 1, 2], texts, "mean")
    plain.forward_rows([0, 1, 2], texts)
    assert [m.past_length_row(r) for r in range(3)] == [40, 3, 131]
    assert m.get_option("kv.free_tokens") == plain.get_option("kv.free_tokens")
    for r in range(3):                            # the same pass: the same cache rows, bit for bit
        for layer in range(2):
            (k0, v0), (k1, v1) = m.read_kv(r, layer), plain.read_kv(r, layer)
            np.testing.assert_array_equal(k0, k1); np.testing.assert_array_equal(v0, v1)
    for r in range(3):
        with pytest.raises(TgxError) as ei:
            m.sample_row(r, GREEDY)
        assert ei.value.status == ST_STATE
    with pytest.raises(TgxError) as ei:
        m.decode_rows(1)
    assert ei.value.status == ST_STATE
    blob = m.save_row(0)                          # tgx_save_row works on a row without logits
    assert len(blob) > 0
    for r in range(3):
        m.extend_row(r, tail)
        twin.reset_cache()
        twin.forward_row(0, np.concatenate([texts[r], tail]))
        assert m.past_length_row(r) == len(texts[r]) + 3
        assert rel_err(m.logits(rounded=False)[r], twin.logits(rounded=False)[0]) < BAR, r
    for r in range(3):
        m.sample_row(r, GREEDY)
    m.decode_rows(2)
    m.truncate_row(1, 2); m.reset_row(1)
    m.close(); plain.close(); twin.close()


@pytest.mark.parametrize("budget", [0, 1024])
def test_row_state_with_release(hip, budget):
    m = make(hip, 4, budget=budget)
    V = m.desc.vocab
    rng = np.random.default_rng(22)
    texts = [rng.integers(0, V, L).astype(np.int64) for L in (40, 130)]
    m.forward_row(0, texts[0])
    m.sample_row(0, GREEDY)
    free = m.get_option("kv.free_tokens")
    m.embed_rows([1, 2], texts, "last", release=True)
    assert m.get_option("kv.free_tokens") == free
    assert [m.past_length_row(r) for r in range(3)] == [40, 0, 0]
    with pytest.raises(TgxError):                 # retired rows of a batch that grew to three: row 3 is the next new one
        m.forward_rows([1, 2, 4], texts + [texts[0]])
    m.forward_rows([1, 2], texts)
    assert [m.past_length_row(r) for r in range(3)] == [40, 40, 130]
    for r in (1, 2):
        m.sample_row(r, GREEDY)
    m.decode_rows(2)
    m.close()


# ---- 6. refusals change nothing -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [0, 1])
def test_refusals_change_nothing(hip, paged):
    V = 256
    rng = np.random.default_rng(31)
    P = lambda n: rng.integers(0, V, n).astype(np.int64)
    budget = 4 * 128 if paged else 0
    m, ctrl = make(hip, 5, budget=budget), make(hip, 5, budget=budget)
    p0, p1, p2 = P(140), P(20), P(3)
    for x in (m, ctrl):
        x.forward_rows([0, 1, 2], [p0, p1, p2])        # 2 + 1 + 1 blocks: the whole budget
        x.sample_row(0, GREEDY); x.sample_row(1, GREEDY)
        x.reset_row(2)                                # one retired row, one block free again
    H = m.desc.hidden

    def state(x):
        return x.get_option("kv.free_tokens"), [x.past_length_row(r) for r in range(5)], x.past_length

    def refused(status, rows, prompts, pool=0, dims=0, null_out=False, null_cfg=False):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        lens = np.ascontiguousarray([len(p) for p in prompts], dtype=np.int32)
        ids = np.ascontiguousarray(np.concatenate(prompts), dtype=np.int64)
        out = np.full((len(rows), max(dims, H)), 7.5, np.float32)
        cfg = EmbedCfg(pool, 1, dims, 0)
        before = state(m)
        st = m.be.embed_rows(m._ctx, len(rows), rows.ctypes.data_as(POINTER(c_int32)), ids.ctypes.data_as(POINTER(c_int64)), lens.ctypes.data_as(POINTER(c_int32)),
                             None if null_cfg else ctypes.byref(cfg), None if null_out else out.ctypes.data_as(POINTER(c_float)))
        assert st == status, (st, m.be.last_error(m._ctx))
        assert state(m) == before == state(ctrl)
        assert (out == 7.5).all()
        np.testing.assert_array_equal(m.logits(rounded=False), ctrl.logits(rounded=False))

    refused(ST_STATE, [0], [P(5)])                    # a live target row
    refused(ST_STATE, [2, 1], [P(5), P(5)])
    refused(ST_INVALID, [2, 2], [P(5), P(5)])         # duplicate rows
    refused(ST_INVALID, [2, 4], [P(5), P(5)])         # the new rows of a call are batch .. in order: row 3 is next
    refused(ST_INVALID, [2], [np.array([3, V, 1])])   # an id out of range
    refused(ST_INVALID, [2], [np.array([-1])])
    refused(ST_INVALID, [2], [P(5)], dims=H + 1)
    refused(ST_INVALID, [2], [P(5)], dims=-1)
    refused(ST_INVALID, [2], [P(5)], pool=3)          # a bad pool
    refused(ST_INVALID, [2], [P(5)], pool=-1)
    refused(ST_INVALID, [2], [P(5)], null_out=True)
    refused(ST_INVALID, [2], [P(5)], null_cfg=True)
    refused(ST_CONTEXT, [2], [P(257)])                # beyond the context size
    if paged:
        refused(ST_CONTEXT, [2, 3], [P(100), P(5)])   # one block short for the whole call: two needed, one free
        refused(ST_CONTEXT, [2], [P(129)])
    # the batch is still three rows (row 4 is not the next new one, row 3 is) and the context is not poisoned
    with pytest.raises(TgxError) as ei:
        m.forward_row(4, P(3))
    assert ei.value.status == ST_INVALID
    e = m.embed_rows([2], [P(100)], "mean", release=True)
    assert e.shape == (1, H) and np.isfinite(e).all()
    np.testing.assert_array_equal(m.decode_rows(1)[0][:, :2], ctrl.decode_rows(1)[0][:, :2])
    m.close(); ctrl.close()


# ---- 7. host ------------------------------------------------------------------------------------------------------------------------------------------------
def test_engine_embed_batches_into_calls(hip, tmp_path):
    """GPTEngine::embed over 6 texts on a 4-row engine: two tgx_embed_rows calls, the vectors those calls return through Model.embed_rows"""
    from ctypes import c_int, c_void_p
    from host_util import HostEngine, host_lib, write_model_dir
    cfg, g = load_golden("qwen2_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    lib = host_lib()
    lib.tgxe_embed.argtypes = [c_void_p, c_int, POINTER(c_int32), POINTER(c_int32), c_int, c_int, c_int, POINTER(c_float), POINTER(c_int64)]
    e = HostEngine(lib, model_dir=str(tmp_path), device="mi355x", max_batch=4)
    assert e.prepare(), e.error()
    m = make(hip, 4, "qwen2_tiny")
    V, H = m.desc.vocab, m.desc.hidden
    rng = np.random.default_rng(41)
    texts = [rng.integers(0, V, L).astype(np.int32) for L in (9, 40, 3, 131, 33, 5)]
    flat, lens = np.ascontiguousarray(np.concatenate(texts)), np.ascontiguousarray([len(t) for t in texts], dtype=np.int32)
    for pool, name in enumerate(POOLS):
        out, calls = np.zeros((6, H), np.float32), c_int64()
        rc = lib.tgxe_embed(e.h, 6, flat.ctypes.data_as(POINTER(c_int32)), lens.ctypes.data_as(POINTER(c_int32)), pool, 1, 0, out.ctypes.data_as(POINTER(c_float)), ctypes.byref(calls))
        assert rc == 0, e.error()
        assert calls.value == 2
        kept = [t[-128:] for t in texts]              # the engine's context is the checkpoint's 128 positions: of the 131-token text its tail, like a prompt
        same = np.concatenate([m.embed_rows(range(4), kept[:4], name, release=True), m.embed_rows(range(2), kept[4:], name, release=True)])
        np.testing.assert_array_equal(out, same, err_msg=name)
        for i in (1, 3, 5):
            assert rel_err(out[i], m.embed_rows([0], [kept[i]], name, release=True)[0]) < BAR, (name, i)
    e.reconfigure(max_new=3)
    ids, new, _ = e.generate_sync([[5, 6, 7]])        # the engine generates afterwards: the cache was left empty
    assert new == 3
    e.close(); m.close()


def test_cli_embed_prints_vectors(hip, tmp_path):
    import json
    import subprocess
    from host_util import write_model_dir
    from tinygpt_amd import build
    cfg, g = load_golden("qwen2_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    _, cli = build.build_host()
    prompts = [[5, 6, 7, 8, 9], [1, 2, 3], [4] * 40]
    out = subprocess.run([cli, "--model", str(tmp_path), "--embed", "--pool", "mean", "--embed-dims", "16", "--prompt-ids", ";".join(",".join(map(str, p)) for p in prompts)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    vecs = [json.loads(line) for line in out.stdout.splitlines()]
    assert len(vecs) == 3 and all(len(v) == 16 for v in vecs)
    m = make(hip, 4, "qwen2_tiny")
    ref = m.embed_rows(range(3), prompts, "mean", dims=16, release=True)
    np.testing.assert_array_equal(np.asarray(vecs, np.float32), ref)      # %.9g round-trips fp32
    m.close()
