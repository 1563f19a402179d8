"""The oracle hooks behind the attention key-range tests (oracle/tgx_oracle.c: tgxo_write_kv, tgxo_set_past, tgxo_set_ablate_key) and the planted caches of
tests/kv_plant.py, on the CPU alone.

The sweep at the end is the reason the GPU tests of tests/test_hip_attn_keyrange.py mean something: for every model, every length of kv_plant.LENGTHS and every key p
of boundary_keys(L), the oracle that loses key p moves its own logits by at least 10x the bound the GPU is held to against the oracle.  A kernel that drops, doubles or
misplaces one key at a tile, split, block or range edge therefore cannot pass.  The rows planted into HERE are synthetic (N(0, 1), what the synthetic checkpoints'
caches look like: the oracle never prefills); tests/test_hip_attn_keyrange.py repeats the whole sweep on the rows a GPU prefill wrote, which are what it plants into.  On the caches a model fills itself the same measure reads 1e-4 .. 1e-2 at contexts
of 1000 .. 4400 and the GPU bound is blind to it; measured here on the planted one: >= 8.4e-2 for all 245 (L, p) of each model (least: Llama-3.2-1B cut 1.35e-1 at
(645, 64), Mistral-7B cut 8.4e-2 at (129, 64), Qwen2.5-0.5B cut 1.16e-1 at (645, 64)).  The choice made here: K factor 4 (2 leaves the scaled keys under the 3x of
test_the_scaled_keys_make_the_softmax_uneven), and no scaled key that is also a boundary key — with 447 and 512 scaled AND loud the sweep read 1.1e-3 at (513, 64);
the loud amplitude beyond L max|v| changes nothing (the loud keys already carry the output).
CPU time of the sweep: one oracle step per (L, p), 245 + 24 steps per model — 1.0 s / 5.0 s / 0.2 s on 8 threads; the whole file 12 s."""
import ctypes
import time

import numpy as np
import pytest

import kv_plant as kp
from conftest import load_golden, rel_err
from tinygpt_amd import synth
from tinygpt_amd.desc import desc_from_hf_config

TOL_GPU = 1e-3          # the loosest bound tests/test_hip_attn_keyrange.py may hold the GPU to against the oracle (the project's TOL_ORACLE); it uses 1e-4 where it can
SENSITIVITY = 10 * TOL_GPU
TOK = 17                # the token every step feeds (inside the tiny fixture's vocabulary too)


@pytest.fixture(scope="module")
def oracle_model(oracle_lib):
    from oracle.oracle_ffi import OracleModel
    return OracleModel


def tiny(oracle_model, dtype, layers=2, zero_k=False):
    cfg, g = load_golden("llama_tiny")
    d = desc_from_hf_config(cfg, dtype, max_batch=1)
    d.layers, d.max_ctx = layers, 96
    m = oracle_model(d)
    for name, bits in synth.synth_checkpoint(d, int(g["seed"]), float(g["std"])):
        m.upload(name, np.zeros_like(bits) if zero_k and name.endswith("k_proj.weight") else bits)
    return m.finalize()


def step(m, L, ablate=-1):
    """one step on TOK over a context of L written positions"""
    m.set_ablate_key(ablate).set_past(L)
    m.forward(np.array([[TOK]]))
    return m.logits(rounded=False).copy()


# ------------------------------------------------------------------------------------------------ the helper itself (no oracle)
def test_boundary_keys():
    assert kp.boundary_keys(1) == [0] and kp.boundary_keys(2) == [0, 1] and kp.boundary_keys(3) == [0, 1, 2]
    assert kp.boundary_keys(64) == [0, 62, 63]                                   # 64 is no multiple BELOW 64
    assert kp.boundary_keys(65) == [0, 63, 64]
    assert kp.boundary_keys(130) == [0, 63, 64, 127, 128, 129]
    assert kp.boundary_keys(645) == sorted({0, 643, 644} | {b + o for b in range(64, 645, 64) for o in (-1, 0)})
    for L in kp.LENGTHS:
        bk = kp.boundary_keys(L)
        assert all(0 <= p < L for p in bk) and len(set(bk)) == len(bk)
        assert not set(bk) & set(kp.scaled_keys(L))


def test_plant_and_poison_are_exact_in_every_storage_dtype():
    rng = np.random.default_rng(3)
    for L in (1, 2, 65, 645):
        k = synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(rng.standard_normal((L, 2, 64)).astype(np.float32))).reshape(L, 2, 64)
        v = synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(rng.standard_normal((L, 2, 64)).astype(np.float32))).reshape(L, 2, 64)
        pk, pv = kp.plant(k, v, L)
        A = kp.loud_amplitude(v, L)
        assert A >= L * np.abs(v).max() and A < 2 * kp.LOUD_GAIN * L * np.abs(v).max() + 2 and A < 65504      # proportional to L max|v|, finite in fp16
        bk, sk = kp.boundary_keys(L), kp.scaled_keys(L)
        assert (np.abs(pv[bk]) == A).all()
        signs = np.sign(pv[bk]).reshape(len(bk), -1)
        assert (np.abs(signs.sum(axis=1)) < 0.5 * signs.shape[1]).all()                                       # both signs within a row ...
        assert len({s.tobytes() for s in signs}) == len(bk)                                                    # ... and no two positions alike
        rest = np.setdiff1d(np.arange(L), bk)
        np.testing.assert_array_equal(pv[rest], v[rest])
        np.testing.assert_array_equal(pk[sk], k[sk] * np.float32(kp.K_FACTOR))
        np.testing.assert_array_equal(np.delete(pk, sk, axis=0), np.delete(k, sk, axis=0))
        for a in (pk, pv, kp.poison((5, 2, 64))):
            np.testing.assert_array_equal(synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(a)).reshape(a.shape), a)
            with np.errstate(over="raise"):
                assert np.isfinite(a.astype(np.float16)).all()
        np.testing.assert_array_equal(pv.astype(np.float16).astype(np.float32), pv)                          # +-A in fp16 too (the K rows start as bf16 values here)
    p = kp.poison((3, 2, 4))
    assert p.shape == (3, 2, 4) and (np.abs(p) == 4096).all() and (p.reshape(-1)[::2] > 0).all() and (p.reshape(-1)[1::2] < 0).all()


# ------------------------------------------------------------------------------------------------ the hooks
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_write_kv_rounds_once_and_read_kv_returns_it(dtype, oracle_model):
    m = tiny(oracle_model, dtype)
    d = m.desc
    rng = np.random.default_rng(11)
    n = d.max_ctx                                                # the whole allocation may be written
    k = (rng.standard_normal((n, d.kv_heads, d.head_dim)) * 3).astype(np.float32)
    v = (rng.standard_normal((n, d.kv_heads, d.head_dim)) * 300).astype(np.float32)

    def stored(a):
        if dtype == "fp32":
            return a
        if dtype == "fp16":
            return a.astype(np.float16).astype(np.float32)
        return synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(a)).reshape(a.shape)

    for layer in range(d.layers):
        m.write_kv(0, layer, k + layer, v - layer)
    m.set_past(n)
    assert m.past_length == n
    for layer in range(d.layers):
        gk, gv = m.read_kv(0, layer)
        np.testing.assert_array_equal(gk, stored(k + layer)); np.testing.assert_array_equal(gv, stored(v - layer))
        m.write_kv(0, layer, gk, gv)                                # stored values are fixed points of the rounding
        k2, v2 = m.read_kv(0, layer)
        np.testing.assert_array_equal(k2, gk); np.testing.assert_array_equal(v2, gv)
    m.write_kv(0, 0, k[:5] * 2, v[:5] * 2)                          # a prefix write leaves the rows behind it alone
    gk, gv = m.read_kv(0, 0)
    np.testing.assert_array_equal(gk[:5], stored(k[:5] * 2)); np.testing.assert_array_equal(gk[5:], stored(k)[5:]); np.testing.assert_array_equal(gv[5:], stored(v)[5:])
    m.set_past(7)
    assert m.read_kv(0, 0)[0].shape[0] == 7
    big = np.zeros((n + 1, d.kv_heads, d.head_dim), np.float32)
    assert m.be.write_kv(m._ctx, 0, 0, big.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None, n + 1) == 1      # beyond max_ctx: refused
    assert m.be.set_past(m._ctx, n + 1) == 1 and m.be.set_past(m._ctx, -1) == 1 and m.past_length == 7
    m.close()


def test_a_step_on_a_written_cache_equals_a_step_after_a_prefill(oracle_model):
    """write_kv + set_past reproduce a prefilled context bit for bit: the rows read back from one context, written into a fresh one"""
    a, b = tiny(oracle_model, "bf16"), tiny(oracle_model, "bf16")
    prompt = synth.synth_prompt(a.desc.vocab, 21, 5)[None, :]
    a.forward(prompt)
    for layer in range(a.desc.layers):
        b.write_kv(0, layer, *a.read_kv(0, layer))
    a.forward(np.array([[TOK]]))
    np.testing.assert_array_equal(step(b, 21), a.logits(rounded=False))
    for layer in range(a.desc.layers):
        for x, y in zip(a.read_kv(0, layer), b.read_kv(0, layer)):
            np.testing.assert_array_equal(x, y)
    a.close(); b.close()


def test_ablating_a_key_outside_the_range_changes_nothing(oracle_model):
    m = tiny(oracle_model, "bf16")
    L = 20
    for layer, (k, v) in enumerate(kp.synthetic_rows(m.desc, L, 1)):
        m.write_kv(0, layer, k, v)
    base = step(m, L)
    for p in (L + 1, L + 2, 95, 10 ** 6):                          # the step sees keys [0, L]: nkeys = L + 1
        np.testing.assert_array_equal(step(m, L, p), base)
    np.testing.assert_array_equal(step(m, L, -1), base)
    for p in (0, L - 1, L):                                        # ... and every key inside it counts, the step's own among them
        assert rel_err(step(m, L, p), base) > 1e-4
    m.close()


def test_ablation_equals_replacing_the_value_by_the_mean_of_the_others(oracle_model):
    """fp32, one layer, k_proj = 0 and the K rows written as zeros: every score is exactly 0, the softmax exactly uniform over the L + 1 keys (the step's own key is 0 as
    well, which a written cache alone could not arrange).  Losing key p then gives mean_{j != p} v_j; so does keeping it with v_p := that mean.  Both are evaluated in
    float64 numpy per head; they differ by the fp32 rounding of the written mean only.  The bound on the logits: each fp32 evaluation of the (L + 1)-term sum is within
    (L + 3) u sum|p_j v_j| <= (L + 3) u max|v| of the exact one (u = 2^-24; L + 1 products and adds, exp and the normaliser), taken relative to the largest output entry;
    the rest of the layer (o_proj, residual, RMSNorm, MLP, lm_head) is smooth and is granted a factor 8 on that relative perturbation.  A wrong ablation — another key, no
    renormalisation, one head or layer left out — is off by ~1 / L of the output: asserted to be 100x the bound."""
    m = tiny(oracle_model, "fp32", layers=1, zero_k=True)
    d, L, u = m.desc, 37, 2.0 ** -24
    rng = np.random.default_rng(7)
    v = rng.standard_normal((L, d.kv_heads, d.head_dim)).astype(np.float32)
    zeros = np.zeros_like(v)
    m.write_kv(0, 0, zeros, v)
    base = step(m, L)
    k_all, v_all = m.read_kv(0, 0)                                 # L + 1 rows: the step appended its own
    assert not k_all.any()
    v64 = v_all.astype(np.float64)
    for p in (0, 17, L - 1):
        others = np.delete(v64, p, axis=0)
        lost = others.mean(axis=0)                                  # float64: the ablated head output (per kv head; the query heads of a group share it)
        v_new = v.copy(); v_new[p] = lost[None].astype(np.float32)
        kept = np.concatenate([np.delete(v64, p, axis=0), v_new[p:p + 1].astype(np.float64)]).mean(axis=0)
        d64 = np.abs(kept - lost).max() / np.abs(lost).max()
        assert d64 < u                                              # the two constructions are one and the same in exact arithmetic
        bound = 8 * (d64 + 2 * (L + 3) * u * np.abs(v64).max() / np.abs(lost).max())
        m.write_kv(0, 0, zeros, v)
        la = step(m, L, p)
        m.write_kv(0, 0, zeros, v_new)
        lb = step(m, L)
        print("p %d: ablate vs mean %.2e (bound %.2e), ablate vs full %.2e" % (p, rel_err(la, lb), bound, rel_err(la, base)))
        assert rel_err(la, lb) <= bound, (p, rel_err(la, lb), bound)
        assert rel_err(la, base) > 100 * bound and rel_err(la, step(m, L, (p + 1) % L)) > 100 * bound
    m.close()


# ------------------------------------------------------------------------------------------------ the planted cache: chosen here, on the CPU
@pytest.fixture(scope="module", params=kp.MODELS)
def planted(request, oracle_model):
    d = kp.cut_desc(request.param, "bf16", 768)
    m = oracle_model(d).load_synthetic(1234, 0.02).finalize()
    yield request.param, m, kp.synthetic_rows(d, max(kp.LENGTHS), 77)
    m.close()


def write_planted(m, base, L):
    for layer, (k, v) in enumerate(base):
        m.write_kv(0, layer, *kp.plant(k, v, L))


def test_every_boundary_key_of_every_length_counts(planted):
    """the sweep: none of the (L, p) left out"""
    name, m, base = planted
    t0, worst, n = time.time(), (np.inf, None), 0
    for L in kp.LENGTHS:
        write_planted(m, base, L)
        full = step(m, L)
        for p in kp.boundary_keys(L):
            e = rel_err(step(m, L, p), full); n += 1
            worst = min(worst, (e, (L, p)))
            assert e >= SENSITIVITY, (name, L, p, e)
    print("%s: %d (L, p), least sensitivity %.2e at %s, %.1f s" % (name, n, worst[0], worst[1], time.time() - t0))


@pytest.mark.parametrize("L", [65, 257, 645])
def test_the_scaled_keys_make_the_softmax_uneven(L, planted):
    """every scaled key s whose neighbour s + 1 is a plain key (neither scaled nor loud): losing s against losing s + 1.  Both carry plain V rows, so the move is the key's
    softmax weight.  EVERY pair cannot be held to 3x — in a head where the query's score on s is negative the factor makes s LIGHTER — so the condition is put on the
    pairs of a length together: the summed moves and the median pair >= 3x (measured: sums 16 .. 274x, medians 11 .. 198x), at least nine pairs in ten >= 3x, and no
    pair below 1x (measured: 95 .. 100 % of the pairs, least pair 1.19x).  Why nine in ten: the move is carried by the heaviest of the >= 28 (head, layer) attentions
    a key takes part in; with plain scores ~N(0, 0.9^2) the scaled key's heaviest weight is e^(4 max s), and that it stays under 3x the neighbour's e^(max s') in
    all of them has probability ~Phi(0.8)^28 ~ 1e-3 per pair for independent heads; heads of one kv group are not independent and the rest of the network is not
    linear, which is what the tenth is granted for."""
    name, m, base = planted
    write_planted(m, base, L)
    full = step(m, L)
    bk = set(kp.boundary_keys(L))
    pairs = [s for s in kp.scaled_keys(L) if s + 1 < L and s + 1 not in bk]
    assert len(pairs) >= 4
    es = np.array([rel_err(step(m, L, s), full) for s in pairs]); en = np.array([rel_err(step(m, L, s + 1), full) for s in pairs])
    share = float((es >= 3 * en).mean())
    print("%s L %d: %d pairs, sum ratio %.1f, median %.1f, least %.2f, share at 3x %.2f" % (name, L, len(pairs), es.sum() / en.sum(), np.median(es / en), (es / en).min(), share))
    assert es.sum() >= 3 * en.sum() and np.median(es / en) >= 3
    assert share >= 0.9 and (es / en).min() >= 1, (share, (es / en).min())
