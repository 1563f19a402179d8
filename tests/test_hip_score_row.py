"""tgx_score_row (include/tgx.h; kernels/score.h): a prompt pass that also returns the log-probability of every token the caller supplied.

The reference of section 1 is an OracleModel with the same description and synthetic seed, teacher-forced one token at a time, and float64 log_softmax of its fp32
logits at each position (computed once per model, shared by the cases that score prefixes or continuations of the same 200 tokens).  Held to:
  * |lp - ref| <= 2 * 1e-3 * max |oracle logits of that position|: 1e-3 is the project's bar for HIP logits against the oracle's (test_hip_parity.py), and
    |d lp| <= |d v_t| + |d lse| <= 2 max |d v|;
  * top ids are not compared exactly (values inside the band may swap): for every rank k the oracle lp of the returned id is >= the oracle's k-th largest lp minus
    the band, and the returned lp matches the oracle lp of THAT id within the bound;
  * exact on the device's own values: strict (lp, -id) order, out_lp equal to the top list's entry of the same id, -1 / -inf beyond top_n;
  * bit identity across score.rows / score.vocab_chunk, runs, paged / unpaged and top_n;
  * the call is the plain pass plus outputs: logits, KV rows, sampled ids, lengths, free blocks and eight following steps equal a twin's that made the plain call;
  * no buffer of seq x V; refusals change nothing."""
import ctypes
from ctypes import POINTER, c_float, c_int32, c_int64

import numpy as np
import pytest

from conftest import load_golden
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, MAX_LOGPROBS, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu

ST_INVALID, ST_STATE, ST_CONTEXT = 1, 4, 8
BAR = 2 * 1e-3
SEEDED = SamplerCfg(0.8, 40, 0.95, 0.0)
N = 200                       # the shared token sequence's length
GPT2_LONG = dict(n_positions=256, n_ctx=256)      # gpt2_hd64's fixture has 64 learned positions: the seq-200 case needs 256 (synthetic weights, both sides)


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def describe(fam, dtype, B, max_ctx=256, **over):
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(dict(cfg, **over), dtype, max_batch=B)
    d.max_ctx = min(max_ctx, d.n_positions) if d.n_positions > 0 else max_ctx
    return d, g


def make(hip, B, fam="llama_tiny", dtype="bf16", budget=0, max_ctx=256, **over):
    """tests/test_hip_logprobs.py::make"""
    d, g = describe(fam, dtype, B, max_ctx, **over)
    m = Model(d, hip)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(int(g["seed"]), float(g["std"])).finalize()


def tokens(V, n=N, seed=7):
    return np.random.default_rng(seed + V).integers(0, V, n).astype(np.int64)


_refs = {}


def oracle_ref(oracle_lib, fam, dtype, n=N, **over):
    """(float64 log_softmax [n][V], max |logit| [n]) of the oracle teacher-forced over tokens(V, n), once per model"""
    key = (fam, dtype, n, tuple(sorted(over.items())))
    if key not in _refs:
        from oracle.oracle_ffi import OracleModel
        d, g = describe(fam, dtype, 1, **over)
        ref = OracleModel(d).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
        ids = tokens(d.vocab, n)
        lps, mags = [], []
        for t in range(n):
            ref.forward(ids[None, t:t + 1])
            v = ref.logits(rounded=False)[0].astype(np.float64)
            mx = v.max()
            lps.append(v - (mx + np.log(np.exp(v - mx).sum())))
            mags.append(np.abs(v).max())
        ref.close()
        lp, mag = np.stack(lps), np.array(mags)
        lp.setflags(write=False); mag.setflags(write=False)
        _refs[key] = (lp, mag)
    return _refs[key]


def check_scores(out, ids, ref_lp, ref_mag, top_n, what):
    """scores `out` of the pass over `ids` against the reference rows of the same positions; returns the worst |lp - ref| / bound"""
    lp, tid, tlp = out
    n = len(ids) - 1
    assert lp.shape == (n,) and tid.shape == (n, MAX_LOGPROBS) and tlp.shape == (n, MAX_LOGPROBS), what
    bound = BAR * ref_mag[:n]
    rows = np.arange(n)
    err = np.abs(lp.astype(np.float64) - ref_lp[rows, ids[1:]])
    assert (err <= bound).all(), (what, float((err / bound).max()))
    worst = float((err / bound).max()) if n else 0.0
    assert (tid[:, top_n:] == -1).all() and np.isneginf(tlp[:, top_n:]).all(), what
    if top_n and n:
        got = tid[:, :top_n]
        assert ((got >= 0) & (got < ref_lp.shape[1])).all(), what
        of_id = ref_lp[rows[:, None], got]                             # the oracle's lp of the returned ids
        kth = -np.sort(-ref_lp[:n], axis=1)[:, :top_n]                 # the oracle's k-th largest
        assert (of_id >= kth - bound[:, None]).all(), (what, "rank")
        e2 = np.abs(tlp[:, :top_n].astype(np.float64) - of_id)
        assert (e2 <= bound[:, None]).all(), (what, float((e2 / bound[:, None]).max()))
        worst = max(worst, float((e2 / bound[:, None]).max()))
        for i in range(n):
            assert len(set(got[i].tolist())) == top_n, (what, i)
    return worst


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------------------------------------
#        fam          dtype   V     seq  opts (score.rows, score.vocab_chunk)  past  budget  form  over
CASES = [("llama_tiny", "bf16", 5003, 200, None, 0, 0, 1, {}),                # TILED: two row tiles with a ragged second; five vocabulary tiles with a ragged last; V % 4 != 0
         ("llama_tiny", "bf16", 5003, 200, (64, 1024), 0, 0, 1, {}),          # groups and chunks with ragged tails
         ("llama_tiny", "bf16", 256, 200, None, 0, 0, 1, {}),                 # one tile that is smaller than a chunk
         ("llama_tiny", "fp16", 5003, 130, None, 0, 0, 1, {}),                # fp16 storage
         ("llama_tiny", "bf16", 5003, 37, None, 0, 0, 2, {}),                 # skinny route, groups 16 + 16 + 5
         ("llama_tiny", "bf16", 5003, 3, None, 0, 0, 2, {}),                  # steps route
         ("gpt2_hd64", "fp32", 320, 40, None, 0, 0, 2, {}),                   # fp32 storage route
         ("gpt2_hd64", "bf16", 320, 200, None, 0, 0, 1, GPT2_LONG),           # GPT-2's LayerNorm and biased final norm on the matrix-core form
         ("llama_tiny", "bf16", 5003, 150, None, 50, 0, 1, {}),               # extend form: tgx_forward_row of 50, then tgx_score_row of 150
         ("llama_tiny", "bf16", 5003, 150, None, 50, 2048, 1, {})]            # ... paged


@pytest.mark.parametrize("fam,dtype,V,seq,opts,past,budget,form,over", CASES)
def test_against_the_oracle(hip, oracle_lib, fam, dtype, V, seq, opts, past, budget, form, over):
    over = dict(over, vocab_size=V)
    ref_lp, ref_mag = oracle_ref(oracle_lib, fam, dtype, N if fam == "llama_tiny" or over.get("n_positions") else 40, **over)
    ids = tokens(V, len(ref_mag))
    m = make(hip, 1, fam, dtype, budget, **over)
    assert m.get_option("score.last_form") == 0
    if opts:
        m.set_option("score.rows", opts[0]); m.set_option("score.vocab_chunk", opts[1])
    worst = 0.0
    for top_n in (0, 1, 20):
        m.reset_cache()
        if past:
            m.forward_row(0, ids[:past])
        out = m.score_row(0, ids[past:past + seq], top_n)
        assert m.get_option("score.last_form") == form
        assert m.past_length_row(0) == past + seq
        worst = max(worst, check_scores(out, ids[past:past + seq], ref_lp[past:past + seq], ref_mag[past:past + seq], top_n, f"top_n={top_n}"))
    print(f"{fam} {dtype} V={V} seq={seq} past={past} opts={opts} paged={bool(budget)}: worst |lp - ref| / bound = {worst:.3f}")
    m.close()


# ---- 2. exact on the device's own values --------------------------------------------------------------------------------------------------------------------
def test_exact_on_the_devices_own_values(hip):
    V = 5003
    m = make(hip, 1, vocab_size=V)
    ids = tokens(V)
    for p in (0, 127, 198):                      # make position p's target one of its own alternatives (causal: the earlier positions' distributions stay)
        m.reset_cache()
        _, tid, _ = m.score_row(0, ids, 20)
        ids[p + 1] = tid[p, 2]
    m.reset_cache()
    lp, tid, tlp = m.score_row(0, ids, 20)
    m.reset_cache()
    lp5, tid5, tlp5 = m.score_row(0, ids, 5)
    for p in (0, 127, 198):
        a, i = tlp[p].astype(np.float64), tid[p].astype(np.int64)
        assert ((a[:-1] > a[1:]) | ((a[:-1] == a[1:]) & (i[:-1] < i[1:]))).all(), p      # strictly descending in (lp, -id)
        assert ids[p + 1] == tid[p, 2] and lp[p] == tlp[p, 2], p
        np.testing.assert_array_equal(tid5[p, :5], tid[p, :5]); np.testing.assert_array_equal(tlp5[p, :5], tlp[p, :5])
        assert (tid5[p, 5:] == -1).all() and np.isneginf(tlp5[p, 5:]).all()
    hit = 0
    for p in range(N - 1):                       # ... and wherever else a target is among the ids
        k = np.flatnonzero(tid[p] == ids[p + 1])
        if len(k):
            assert lp[p] == tlp[p, k[0]], p
            hit += 1
    assert hit >= 3
    m.close()


# ---- 3. bit identity ----------------------------------------------------------------------------------------------------------------------------------------
def test_bit_identity(hip):
    V = 5003
    ids = tokens(V)
    m = make(hip, 1, vocab_size=V)
    rows0, chunk0 = m.get_option("score.rows"), m.get_option("score.vocab_chunk")
    assert (rows0, chunk0) == (2048, 16384)

    def run(x, top_n=20):
        x.reset_cache()
        return x.score_row(0, ids, top_n)
    base = run(m)
    for chunk in (1024, 2048, chunk0):
        for rows in (64, 128, rows0):
            m.set_option("score.vocab_chunk", chunk); m.set_option("score.rows", rows)
            for a, b in zip(run(m), base):
                np.testing.assert_array_equal(a, b, err_msg=f"rows {rows} chunk {chunk}")
    for a, b in zip(run(m), base):               # a second run
        np.testing.assert_array_equal(a, b)
    for top_n in (0, 1):
        np.testing.assert_array_equal(run(m, top_n)[0], base[0])
    paged = make(hip, 1, budget=2048, vocab_size=V)
    for a, b in zip(run(paged), base):
        np.testing.assert_array_equal(a, b, err_msg="paged")
    m.close(); paged.close()


# ---- 4. the call is the plain pass plus outputs -------------------------------------------------------------------------------------------------------------
def observe(x, row, layers=2):
    """what a twin must hold bit for bit after the pass: logits of all rows, the row's KV, length, free blocks, a greedy and a seeded draw, eight following steps"""
    obs = {"logits": x.logits(rounded=False).copy(), "len": [x.past_length_row(r) for r in range(x.batch)], "free": x.get_option("kv.free_tokens")}
    obs["kv"] = [x.read_kv(row, layer) for layer in range(layers)]
    obs["greedy"] = x.sample_row(row, GREEDY)
    obs["seeded"] = x.sample_row(row, SEEDED, 99)
    obs["next"] = x.decode_rows(8)[0].copy()
    obs["logits_after"] = x.logits(rounded=False).copy()
    return obs


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if k == "kv":
            for (k0, v0), (k1, v1) in zip(a[k], b[k]):
                np.testing.assert_array_equal(k0, k1, err_msg=what); np.testing.assert_array_equal(v0, v1, err_msg=what)
        else:
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=f"{what}: {k}")


@pytest.mark.parametrize("budget", [0, 2048])
def test_the_call_is_the_plain_pass_plus_outputs(hip, budget):
    V = 5003
    ids = tokens(V)
    rng = np.random.default_rng(3)
    p0, p2 = rng.integers(0, V, 33).astype(np.int64), rng.integers(0, V, 140).astype(np.int64)
    twins = [make(hip, 3, budget=budget, vocab_size=V) for _ in range(2)]
    obs = []
    for k, x in enumerate(twins):                # k == 0 scores, k == 1 makes the plain calls
        score = k == 0
        x.forward_rows([0, 1, 2], [p0, ids[:9], p2])
        for r in range(3):
            x.set_row_sampler(r, SEEDED if r == 2 else GREEDY, 5 + r)
            x.sample_row(r, GREEDY)
        x.decode_rows(3)
        # ---- admission into a retired row of the running batch (150 tokens: the matrix-core form)
        x.reset_row(1)
        if score:
            x.score_row(1, ids[:150], 20)
        else:
            x.forward_row(1, ids[:150])
        x.set_row_logprobs(1, 2)
        o = {"admit": observe(x, 1)}
        # ---- extension of the live row, whose ring holds the ten records of observe()'s two draws and eight steps
        n_rec = 10
        x.row_logprobs(1, n_rec)
        with pytest.raises(TgxError):
            x.row_logprobs(1, n_rec + 1)
        if score:
            x.score_row(1, ids[:40], 3)
        else:
            x.extend_row(1, ids[:40])
        x.row_logprobs(1, n_rec)                 # the record count did not move
        with pytest.raises(TgxError) as ei:
            x.row_logprobs(1, n_rec + 1)
        assert ei.value.status == ST_INVALID
        o["extend"] = observe(x, 1)
        # ---- extension of a row that finished on the device
        x.set_row_stop(1, 2)
        _, _, fin = x.decode_rows(4)
        assert fin[1] == 2
        x.set_row_stop(1, 0)
        if score:
            x.score_row(1, ids[:5], 0)
        else:
            x.extend_row(1, ids[:5])
        o["finished"] = observe(x, 1)
        obs.append(o)
    for what in obs[0]:
        same(obs[0][what], obs[1][what], what)
    for x in twins:
        x.close()


# ---- 5. memory ----------------------------------------------------------------------------------------------------------------------------------------------
def test_no_buffer_of_seq_times_vocabulary(hip):
    V = 5003
    ids = tokens(V)
    a, b, never = make(hip, 1, vocab_size=V), make(hip, 1, vocab_size=V), make(hip, 1, vocab_size=V)
    a.set_option("score.rows", 64); a.set_option("score.vocab_chunk", 1024)
    a.score_row(0, ids, 20)
    b.forward_row(0, ids)
    never.set_option("score.rows", 64)
    never.forward_row(0, ids)
    extra = a.get_option("mem.live_kib") - b.get_option("mem.live_kib")
    print(f"tgx_score_row holds {extra} KiB more than tgx_forward_row ([200][5003] fp32 = 3908 KiB)")
    assert 0 < extra < 1954
    assert never.get_option("mem.live_allocs") == b.get_option("mem.live_allocs")
    for x in (a, b, never):
        x.close()


# ---- 6. refusals change nothing -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [0, 1])
def test_refusals_change_nothing(hip, paged):
    """TGX_ERR_INVALID, TGX_ERR_CONTEXT (context size and paged budget) and TGX_ERR_STATE (before tgx_finalize) of the two underlying calls, the call's own argument
    checks and the options' refusals.  NOT covered, because neither can be reached at max_ctx 256 / V 5003: TGX_ERR_UNSUPPORTED of tgx_extend_row on a paged block table
    of more than 1024 entries (max_ctx > 131072), and the scoring workspace's refusal of a vocabulary of more than 1024 tiles (V > 2^20).  The poisoned context
    (TGX_ERR_STATE after a pass failed half-way) cannot be brought about on purpose either."""
    V = 5003
    rng = np.random.default_rng(11)
    P = lambda n: rng.integers(0, V, n).astype(np.int64)
    m = make(hip, 4, budget=3 * 128 if paged else 0, vocab_size=V)
    ctrl = make(hip, 4, budget=3 * 128 if paged else 0, vocab_size=V)
    p0, p1 = P(140), P(20)
    for x in (m, ctrl):
        x.forward_rows([0, 1], [p0, p1])         # 2 + 1 blocks: the whole budget
        x.sample_row(0, GREEDY); x.sample_row(1, GREEDY)

    def state(x):
        return x.get_option("kv.free_tokens"), [x.past_length_row(r) for r in range(4)], x.past_length, x.get_option("score.last_form")

    def refused(status, row, ids, top_n=0, null_lp=False, seq=None):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        n = max(len(ids), 2)
        lp, tid, tlp = np.full(n, 7.5, np.float32), np.full((n, MAX_LOGPROBS), -7, np.int32), np.full((n, MAX_LOGPROBS), 7.5, np.float32)
        before = state(m)
        st = m.be.score_row(m._ctx, row, ids.ctypes.data_as(POINTER(c_int64)) if len(ids) else (c_int64 * 1)(), len(ids) if seq is None else seq, top_n,
                            None if null_lp else lp.ctypes.data_as(POINTER(c_float)), tid.ctypes.data_as(POINTER(c_int32)), tlp.ctypes.data_as(POINTER(c_float)))
        assert st == status, (st, m.be.last_error(m._ctx))
        assert state(m) == before == state(ctrl)
        assert (lp == 7.5).all() and (tid == -7).all() and (tlp == 7.5).all()
        np.testing.assert_array_equal(m.logits(rounded=False), ctrl.logits(rounded=False))

    refused(ST_INVALID, 4, P(5))                 # outside [0, max_batch)
    refused(ST_INVALID, -1, P(5))
    refused(ST_INVALID, 3, P(5))                 # admission: the batch grows in order (row 2 is next)
    refused(ST_INVALID, 2, P(0))                 # admission: seq < 1
    refused(ST_INVALID, 0, P(0))                 # extension: seq < 1
    refused(ST_INVALID, 2, np.array([3, V, 1]))  # admission: id out of range
    refused(ST_INVALID, 0, np.array([3, -1]))    # extension: id out of range
    refused(ST_CONTEXT, 2, P(5), seq=257)        # admission: beyond the context size (refused before the ids are read)
    refused(ST_CONTEXT, 0, P(117))               # extension: 140 + 117 > 256
    refused(ST_INVALID, 2, P(5), top_n=-1)       # the call's own arguments
    refused(ST_INVALID, 0, P(5), top_n=MAX_LOGPROBS + 1)
    refused(ST_INVALID, 2, P(5), null_lp=True)
    refused(ST_INVALID, 0, P(2), null_lp=True)
    assert m.be.score_row(m._ctx, 0, None, 3, 0, None, None, None) == ST_INVALID and state(m) == state(ctrl)
    if paged:
        refused(ST_CONTEXT, 2, P(5))             # admission: no block free
        refused(ST_CONTEXT, 1, P(110))           # extension: 130 tokens need a second block
    for key, bad in (("score.rows", 0), ("score.rows", 96), ("score.rows", -64), ("score.vocab_chunk", 0), ("score.vocab_chunk", 1536), ("score.vocab_chunk", 64)):
        before = m.get_option(key)
        with pytest.raises(TgxError) as ei:
            m.set_option(key, bad)
        assert ei.value.status == ST_INVALID and m.get_option(key) == before
    fresh = Model(describe("llama_tiny", "bf16", 1, vocab_size=V)[0], hip)      # before tgx_finalize: tgx_forward_row's status
    one = np.zeros(2, np.int64)
    lp = np.zeros(2, np.float32)
    assert fresh.be.score_row(fresh._ctx, 0, one.ctypes.data_as(POINTER(c_int64)), 2, 0, lp.ctypes.data_as(POINTER(c_float)), None, None) == ST_STATE
    fresh.close()
    # not poisoned: the next step is the control's, and a legal call of one position writes nothing
    np.testing.assert_array_equal(m.decode_rows(1)[0], ctrl.decode_rows(1)[0])
    if not paged:
        lp, tid, tlp = m.score_row(2, P(1), 5)
        assert lp.shape == (0,) and m.past_length_row(2) == 1
        assert m.get_option("score.last_form") == 0              # a call that scored no position is not a form
    m.close(); ctrl.close()
