"""Per-token log-probabilities on the device (include/tgx.h: tgx_set_row_logprobs / tgx_read_row_logprobs; kernels/logprobs.h).  The reference everywhere is numpy
float64 log_softmax of the fp32 logits read back with tgx_read_logits(rounded = 0) — what the argmax and the sampler look at.  Held to:
  * top ids == numpy's stable order (value descending, index ascending) EXACTLY: the same fp32 values, no band;
  * |lp - ref| <= 2e-5 for every finite value.  Derived, not measured: for |lp| < 128 two fp32 roundings of at most 3.8e-6 each plus the relative error of a double
    sum of fp32 exp terms (< 1e-6) stay below 1e-5; the bound is doubled;
  * the produced token's id is not part of what tgx_read_row_logprobs returns, so "the record belongs to out_ids' token" is checked through its value: lp == ref[out_id]
    to 2e-5 — an INDIRECT check, which cannot tell tokens of equal logits apart — and, exactly, for greedy rows with top_n >= 1: top id 0 == out_id;
  * recording perturbs nothing: ids and fp32 logits bit-identical to a twin context with logprobs off;
  * the lifecycle of the record count and every error status the header names."""
import numpy as np
import pytest

from conftest import load_golden
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, LOGPROB_RING, MAX_LOGPROBS, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu

ST_INVALID, ST_STATE = 1, 4
TOL = 2e-5
MIX = [GREEDY, SamplerCfg(0.8, 0, 0.9, 0.0), SamplerCfg(1.0, 50, 1.0, 0.0), SamplerCfg(0.7, 0, 1.0, 0.05), SamplerCfg(0.9, 40, 0.95, 0.05)]
SEEDS = [11, 22, 33, 44, 55]


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def ref_logprobs(v):
    """float64 log_softmax and the stable order (value descending, index ascending) of fp32 logits v"""
    v = np.asarray(v, np.float64)
    m = v.max()
    with np.errstate(divide="ignore"):
        lse = m + np.log(np.exp(v - m).sum())
    return v - lse, np.argsort(-v, kind="stable")


def close(a, b, tol, what=""):
    """|a - b| <= tol where b is finite, the same infinity elsewhere; returns the largest finite difference"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    fin = np.isfinite(b)
    np.testing.assert_array_equal(a[~fin], b[~fin], err_msg=what)
    err = float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0
    assert err <= tol, (what, err, tol)
    return err


def check_record(rec, i, logits, tok, top_n, tol=TOL, what="", greedy=False):
    """record i of rec = (lp, ids, tlp, tn) against the reference of `logits` for produced token `tok`"""
    lp, ids, tlp, tn = rec
    ref, order = ref_logprobs(logits)
    assert tn[i] == top_n, what
    assert 0 <= tok < len(ref), what
    err = close(lp[i], ref[tok], tol, what)
    np.testing.assert_array_equal(ids[i, :top_n], order[:top_n], err_msg=what)
    if top_n:
        err = max(err, close(tlp[i, :top_n], ref[order[:top_n]], tol, what))
        assert not greedy or ids[i, 0] == tok, what              # a greedy row produced the first entry of the order
    assert (ids[i, top_n:] == -1).all() and np.isneginf(tlp[i, top_n:]).all(), what
    return err


def make(hip, B, fam="llama_tiny", dtype="bf16", budget=0, max_ctx=256, **over):
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(dict(cfg, **over), dtype, max_batch=B)
    d.max_ctx = min(max_ctx, d.n_positions) if d.n_positions > 0 else max_ctx      # (GPT-2: the learned position table bounds the context)
    m = Model(d, hip)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(int(g["seed"]), float(g["std"])).finalize()


def prompts(B, S=9, seed=0, V=256):
    return np.random.default_rng(seed).integers(0, V, size=(B, S)).astype(np.int64)


# ---- 1. injected logits -------------------------------------------------------------------------------------------------------------------------------------
def injected(V, rng):
    normal = rng.standard_normal(V)
    normal = (normal * (30.0 / np.abs(normal).max())).astype(np.float32)
    equal = np.full(V, 1.25, np.float32)
    dup = rng.standard_normal(V).astype(np.float32)
    far = [3, V // 2, V - 2]                                   # duplicated maxima far apart ...
    dup[far] = 9.5
    if V > 1024:                                               # ... and duplicates that straddle a tile boundary (1024 entries per tile)
        dup[1022:1026] = 9.0
        dup[2047:2049] = 9.5
    else:
        dup[254:258] = 9.0                                     # one tile: a wave boundary instead
    holes = rng.standard_normal(V).astype(np.float32) * 4
    holes[rng.permutation(V)[: V // 10]] = -np.inf
    spike = np.zeros(V, np.float32)
    spike[V // 3] = 40.0
    return {"normal": normal, "equal": equal, "dup": dup, "holes": holes, "spike": spike}


@pytest.mark.parametrize("V", [320, 5003, 70001])
def test_injected_logits(hip, V):
    """one tile; several tiles with a ragged last one and V % 4 != 0; many tiles — top_n 0 / 1 / 5 / 20, greedy and sampled draws"""
    m = make(hip, 1, num_hidden_layers=1, vocab_size=V)
    vecs = injected(V, np.random.default_rng(V))
    worst, n = 0.0, 0
    for name, v in vecs.items():
        for top_n in (0, 1, 5, 20):
            for k in (0, 2):                                   # a greedy and a sampled produced token: the distribution is the model's either way
                m.set_logits(v)
                m.set_row_logprobs(0, top_n)
                tok = m.sample_row(0, MIX[k], SEEDS[k])
                n += 1
                rec = m.row_logprobs(0, 1)
                worst = max(worst, check_record(rec, 0, m.logits(rounded=False)[0], tok, top_n, what=f"V={V} {name} top_n={top_n} cfg{k}", greedy=k == 0))
                if name == "equal":
                    close(rec[0][0], -np.log(V), TOL)
                    np.testing.assert_array_equal(rec[1][0, :top_n], np.arange(top_n))
                if name == "spike" and k == 0:
                    assert tok == V // 3 and abs(rec[0][0]) < 1e-6
    print(f"injected V={V}: max |lp - ref| = {worst:.3e} over {n} records")
    with pytest.raises(TgxError) as ei:                        # the ring holds these n records and no more
        m.row_logprobs(0, n + 1)
    assert ei.value.status == ST_INVALID


# ---- 2. through the model -----------------------------------------------------------------------------------------------------------------------------------
# GPT-2: the fp32 family fixture of the GPU tests is gpt2_hd64 — gpt2_tiny has head_dim 32, which tgx_create refuses (64 and 128 are built; conftest.GPU_FAMILIES), it
# stays an oracle-only fixture.  Paged KV serves the 16-bit storage dtypes only (tgx_finalize refuses kv.budget_tokens on fp32 storage), so GPT-2's paged case runs bf16.
@pytest.mark.parametrize("fam,dtype,B,budget", [("llama_tiny", "bf16", 1, 0), ("llama_tiny", "bf16", 2, 0), ("llama_tiny", "bf16", 8, 0), ("llama_tiny", "bf16", 8, 2048),
                                                 ("gpt2_hd64", "fp32", 1, 0), ("gpt2_hd64", "fp32", 2, 0), ("gpt2_hd64", "fp32", 8, 0), ("gpt2_hd64", "bf16", 8, 2048)])
def test_through_the_model(hip, fam, dtype, B, budget):
    """GEMV step (1-2 rows), matrix-core step (8), paged; greedy and sampled rows with top_n differing per row and the last row off; then 20 steps in one call"""
    P = prompts(B, seed=B)
    top_of = lambda b: -1 if (b == B - 1 and B > 1) else (0, 3, 20, 1, 7)[b % 5]
    k_of = lambda b: b % len(MIX)
    m, t = make(hip, B, fam, dtype, budget), make(hip, B, fam, dtype, budget)
    for x, on in ((m, True), (t, False)):
        x.forward(P)
        for b in range(B):
            x.set_row_sampler(b, MIX[k_of(b)], SEEDS[k_of(b)])
            if on:
                x.set_row_logprobs(b, top_of(b))
    count = [0] * B
    worst = 0.0
    lg = m.logits(rounded=False)
    for b in range(B):
        tok, tok_t = m.sample_row(b, MIX[k_of(b)], SEEDS[k_of(b)]), t.sample_row(b, MIX[k_of(b)], SEEDS[k_of(b)])
        assert tok == tok_t
        if top_of(b) >= 0:
            count[b] += 1
            worst = max(worst, check_record(m.row_logprobs(b, 1), 0, lg[b], tok, top_of(b), what=f"first token row {b}", greedy=k_of(b) == 0))
    for step in range(6):                                      # one step per call: every step's logits can be read
        ids, new, fin = m.decode_rows(1)
        ids_t, _, _ = t.decode_rows(1)
        np.testing.assert_array_equal(ids, ids_t)
        lg = m.logits(rounded=False)
        for b in range(B):
            if top_of(b) < 0:
                continue
            count[b] += 1
            worst = max(worst, check_record(m.row_logprobs(b, 1), 0, lg[b], int(ids[0, b]), top_of(b), what=f"step {step} row {b}", greedy=k_of(b) == 0))
    ids, new, fin = m.decode_rows(20)                          # crosses the 16-step graph
    ids_t, _, _ = t.decode_rows(20)
    np.testing.assert_array_equal(ids, ids_t)
    lg = m.logits(rounded=False)
    np.testing.assert_array_equal(lg.view(np.uint32), t.logits(rounded=False).view(np.uint32))      # recording perturbs neither a greedy nor a sampled row
    for b in range(B):
        if top_of(b) < 0:
            with pytest.raises(TgxError) as ei:                # the "off" row's count stays 0
                m.row_logprobs(b, 1)
            assert ei.value.status == ST_STATE
            continue
        count[b] += 20
        rec = m.row_logprobs(b, 20)
        worst = max(worst, check_record(rec, 19, lg[b], int(ids[19, b]), top_of(b), what=f"last of 20 steps row {b}"))
        assert np.isfinite(rec[0]).all() and (rec[0] <= 0).all()
        m.row_logprobs(b, count[b])
        with pytest.raises(TgxError) as ei:
            m.row_logprobs(b, count[b] + 1)
        assert ei.value.status == ST_INVALID
    print(f"model {fam} {dtype} B={B} budget={budget}: max |lp - ref| = {worst:.3e}")


# ---- 3. against the oracle ----------------------------------------------------------------------------------------------------------------------------------
def test_against_the_oracle(hip, oracle_lib):
    """llama_tiny, 4 greedy rows, 12 steps: log_softmax moves by at most twice the sup-norm of the logit difference"""
    from oracle.oracle_ffi import OracleModel
    cfg, g = load_golden("llama_tiny")
    B = 4
    d = desc_from_hf_config(cfg, "bf16", max_batch=B)
    P = prompts(B, seed=3)
    m = Model(d, hip).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    o = OracleModel(d).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    m.forward(P); o.forward(P)
    for b in range(B):
        m.set_row_logprobs(b, 0)
        m.sample_row(b)
    o.sample(GREEDY)
    checked = 0
    for step in range(12):
        ids, _, _ = m.decode_rows(1)
        ids_o = o.decode(1, GREEDY)
        a, r = m.logits(rounded=False), o.logits(rounded=False)
        for b in range(B):
            if ids[0, b] != ids_o[0, b]:
                continue
            lp_ref = ref_logprobs(r[b])[0][int(ids[0, b])]
            bound = 2 * float(np.abs(a[b].astype(np.float64) - r[b]).max()) + TOL
            close(m.row_logprobs(b, 1)[0][0], lp_ref, bound, f"step {step} row {b}")
            checked += 1
        if not (ids == ids_o).all():
            break                                              # the sequences part ways: later steps compare different contexts
    assert checked >= B


# ---- 4. lifecycle -------------------------------------------------------------------------------------------------------------------------------------------
def status_of(fn):
    with pytest.raises(TgxError) as ei:
        fn()
    return ei.value.status


def test_lifecycle(hip):
    B = 4
    m = make(hip, B)
    P = prompts(3, seed=5)
    assert status_of(lambda: m.row_logprobs(0, 1)) == ST_STATE                   # nothing recorded, nothing allocated
    m.forward(P)
    for b in range(3):
        m.set_row_logprobs(b, 2)
        m.sample_row(b)
    # max_new 3 records exactly 3 more; a stop id records the stopping token; finished rows record nothing further
    free = make(hip, 1)
    free.forward(P[1:2]); free.sample_row(0)
    stop_tok = int(free.decode_rows(2)[0][1, 0])
    m.set_row_stop(0, max_new=3)
    m.set_row_stop(1, stop_ids=[stop_tok])
    new, lg1 = np.zeros(3, np.int64), None
    for done in range(1, 3):                                                      # one step per call up to row 1's stop: the stopping step's logits can be read
        ids, n1, fin = m.decode_rows(1)
        new += n1
        if fin[1]:
            assert int(ids[0, 1]) == stop_tok
            lg1 = m.logits(rounded=False)[1]
            break
    assert lg1 is not None
    check_record(m.row_logprobs(1, 1), 0, lg1, stop_tok, 2, what="the stopping token")
    ids, n1, fin = m.decode_rows(6 - done)
    new += n1
    assert new[0] == 3 and fin[0] == 2 and fin[1] == 1 and new[1] == done and new[2] == 6
    for b in range(3):
        n = 1 + int(new[b])
        assert len(m.row_logprobs(b, n)[0]) == n
        assert status_of(lambda: m.row_logprobs(b, n + 1)) == ST_INVALID
    ids2, new2, _ = m.decode_rows(2)                                              # rows 0 and 1 ride along finished
    assert new2[0] == 0 and new2[1] == 0 and new2[2] == 2
    assert status_of(lambda: m.row_logprobs(0, 5)) == ST_INVALID and len(m.row_logprobs(2, 9)[0]) == 9
    # a changed top_n takes effect in the next call, without a new graph
    m.set_row_logprobs(2, 5)
    ids3, _, _ = m.decode_rows(1)
    rec = m.row_logprobs(2, 2)
    assert rec[3].tolist() == [2, 5]
    check_record(rec, 1, m.logits(rounded=False)[2], int(ids3[0, 2]), 5)
    # a fork destination starts at 0 with its own setting untouched (off); the source's records are intact
    before = m.row_logprobs(2, 10)
    m.fork_row(2, [3])
    assert status_of(lambda: m.row_logprobs(3, 1)) == ST_STATE
    for a, b_ in zip(before, m.row_logprobs(2, 10)):
        np.testing.assert_array_equal(a, b_)
    m.decode_rows(1)
    assert status_of(lambda: m.row_logprobs(3, 1)) == ST_STATE and len(m.row_logprobs(2, 11)[0]) == 11
    # tgx_reset_row zeroes the count and the setting; a refilled row starts at 0
    m.reset_row(0)
    assert status_of(lambda: m.row_logprobs(0, 1)) == ST_STATE
    m.forward_row(0, P[0]); m.sample_row(0)
    m.decode_rows(1)
    assert status_of(lambda: m.row_logprobs(0, 1)) == ST_STATE                    # the setting went back to "off"
    m.set_row_logprobs(0, 0)
    m.decode_rows(2)
    assert len(m.row_logprobs(0, 2)[0]) == 2 and status_of(lambda: m.row_logprobs(0, 3)) == ST_INVALID
    m.reset_row(1); m.set_row_logprobs(1, 1)
    m.forward_row(1, P[1]); tok = m.sample_row(1)                                 # an admission INTO a row that records: its count restarts, its setting stays
    check_record(m.row_logprobs(1, 1), 0, m.logits(rounded=False)[1], tok, 1)
    assert status_of(lambda: m.row_logprobs(1, 2)) == ST_INVALID
    # tgx_extend_row and tgx_truncate_row keep the count
    m.extend_row(1, [5, 6, 7]); m.sample_row(1)
    assert len(m.row_logprobs(1, 2)[0]) == 2
    m.truncate_row(1, 10)
    assert len(m.row_logprobs(1, 2)[0]) == 2
    # the error statuses; the context stays usable
    for bad in (lambda: m.set_row_logprobs(-1, 0), lambda: m.set_row_logprobs(B, 0), lambda: m.set_row_logprobs(0, -2), lambda: m.set_row_logprobs(0, MAX_LOGPROBS + 1),
                lambda: m.row_logprobs(B, 1), lambda: m.row_logprobs(0, 0)):
        assert status_of(bad) == ST_INVALID
    m.extend_row(1, [8]); m.sample_row(1)
    m.decode_rows(1)
    m.reset_cache()
    assert status_of(lambda: m.row_logprobs(2, 1)) == ST_STATE
    m.forward(P); m.sample()
    m.decode_rows(2)
    assert status_of(lambda: m.row_logprobs(2, 1)) == ST_STATE                    # tgx_reset_cache restored "off"


def test_retired_row_records_nothing(hip):
    """a retired row rides along in the steps; switched on while retired it records nothing, and the setting takes effect with the admission"""
    m = make(hip, 2)
    P = prompts(2, seed=13)
    m.forward(P)
    m.set_row_logprobs(0, 1)
    m.sample_row(0); m.sample_row(1)
    m.reset_row(1)
    m.set_row_logprobs(1, 3)                                                     # on a retired row
    m.decode_rows(3)
    assert status_of(lambda: m.row_logprobs(1, 1)) == ST_STATE and len(m.row_logprobs(0, 4)[0]) == 4
    m.forward_row(1, P[1]); tok = m.sample_row(1)
    check_record(m.row_logprobs(1, 1), 0, m.logits(rounded=False)[1], tok, 3)
    ids, new, _ = m.decode_rows(2)
    rec = m.row_logprobs(1, 3)
    check_record(rec, 2, m.logits(rounded=False)[1], int(ids[1, 1]), 3)
    assert status_of(lambda: m.row_logprobs(1, 4)) == ST_INVALID
    m.reset_row(0)                                                               # retiring a recording row: off, count 0, and nothing more while it rides
    m.decode_rows(2)
    assert status_of(lambda: m.row_logprobs(0, 1)) == ST_STATE and len(m.row_logprobs(1, 5)[0]) == 5


def test_ring_keeps_the_last_256(hip):
    """300 tokens: n = 256 gives the records of tokens 44 .. 299 — those of a twin read in two halves — and n = 257 is TGX_ERR_INVALID"""
    P = prompts(1, seed=9)
    m, t = make(hip, 1, max_ctx=512), make(hip, 1, max_ctx=512)
    for x in (m, t):
        x.forward(P)
        x.set_row_logprobs(0, 4)
        x.sample_row(0)
    m.decode_rows(299)
    t.decode_rows(149)
    first = t.row_logprobs(0, 150)
    t.decode_rows(150)
    second = t.row_logprobs(0, 150)
    got = m.row_logprobs(0, LOGPROB_RING)
    for a, f, s in zip(got, first, second):
        np.testing.assert_array_equal(a, np.concatenate([f, s])[44:])
    assert status_of(lambda: m.row_logprobs(0, LOGPROB_RING + 1)) == ST_INVALID
    a, b = m.row_logprobs(0, 10), m.row_logprobs(0, 10)                           # reading does not consume
    np.testing.assert_array_equal(a[0], b[0])


# ---- 5. tgx_verify_row --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_draft,wrong_at", [(4, None), (15, None), (15, 6), (4, 0)])
def test_verify_row_records(hip, n_draft, wrong_at):
    """drafts from a twin's own greedy continuation: all, or a known prefix, accepted; one record per produced token, each from its position's logits"""
    P = prompts(1, seed=21)
    m, t = make(hip, 1), make(hip, 1)
    for x in (m, t):
        x.forward(P)
        x.set_row_logprobs(0, 2)
        x.sample_row(0)
    cont = t.decode_rows(n_draft + 1)[0][:, 0]
    lg_t = t.logits(rounded=False)[0]
    draft = cont[:n_draft].copy()
    if wrong_at is not None:
        draft[wrong_at] = (draft[wrong_at] + 1) % 256
    out, fin = m.verify_row(0, draft)
    want = n_draft + 1 if wrong_at is None else wrong_at + 1
    assert len(out) == want and fin == 0
    np.testing.assert_array_equal(out, cont[:want])
    rec = m.row_logprobs(0, want)
    assert status_of(lambda: m.row_logprobs(0, want + 2)) == ST_INVALID and len(m.row_logprobs(0, want + 1)[0]) == want + 1
    check_record(rec, want - 1, m.logits(rounded=False)[0], int(out[-1]), 2, what="the last record against the row's logits slot")
    twin = t.row_logprobs(0, n_draft + 1)
    bound = 2 * 1e-3 * float(np.abs(lg_t).max()) + TOL           # the GPU-against-GPU bound between kernel paths (tests/test_hip_verify_row.py)
    for i in range(want):
        close(rec[0][i], twin[0][i], bound, f"record {i}")
        if twin[2][i, 0] - twin[2][i, 1] > bound:
            assert rec[1][i, 0] == twin[1][i, 0]
    m.decode_rows(1)                                              # the row goes on recording from where the pass left it
    assert len(m.row_logprobs(0, want + 2)[0]) == want + 2
