"""tgx_splice_row (include/tgx.h): ranges cut out of the middle of a live row's cache — V rows move, K rows move and are re-rotated to the position they land on
(kernels/kv_splice.h), the block table and the position word follow (csrc/splice_plan.h).  2-layer, vocab-4096 models of the real geometries, contexts of 512.  Held to:
  1. the move: V rows and delta == 0 K rows bit for bit the source rows; rotated K entries against tests/splice_ref.py (fp64 rotation by the difference of the float32
     table angles) within one unit in the last place of the storage dtype at the entry's magnitude plus 2^-20 of the pair's norm — the four table entries and the fp32
     rotation each err by a few 2^-24 of the pair's norm, far below half a storage ulp at 16 bits, so the rounding differs by at most one step; the second term carries
     fp32 storage and the cosf difference between libraries.  (The families with unscaled frequencies; Llama-3's scaled ones are covered by 2.)
  2. layer 0 against a fresh prefill of the spliced token sequence (layer 0's K and V depend on token and position alone): V within check_kv's layer-0 form, K within
     that plus the double-rounding bound 1.25 u |pair|, u = 2^-8 (bf16), 2^-11 (fp16), 2^-23 (fp32) — the first rounding errs by at most sqrt(2) u/2 |pair| as a vector
     and survives the rotation, the second by at most u/2 of the entry.
  3. bookkeeping, bit for bit: splice + extend_row against a second context that prefills any new_len tokens, gets the spliced cache rows by write_kv and extends the
     same way — logits, every cache row and four forced decode steps (position word, host length, block table, the RoPE position of what follows).
  4. paged == unpaged bit for bit on every shape.
  5. paged accounting: kv.free_tokens after every shape; fork then splice with f inside a shared block takes exactly one fresh block and leaves the siblings alone; no free
     block is TGX_ERR_CONTEXT and changes nothing.
  6. a running batch: the rows not named stay bit-identical to a control across the splice and a joint decode_rows; a finished row is accepted and runs again.
  7. every refusal changes nothing (a call before tgx_finalize included); the no-logits state refuses sampling, stepping and forking until extend_row lifts it; a context that never splices allocates nothing."""
import copy

import numpy as np
import pytest

from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import GREEDY, Model, TgxError

import splice_ref

pytestmark = pytest.mark.gpu
BLK = 128
CTX = 512
# (past; kept ranges as (start, length)): overlap inside one block; delta 1 across the 128 boundary; a whole-block move; three deltas; no identity prefix (f = 0); a
# full row (the last table row read); tgx_truncate_row; a no-op
SHAPES = [(100, [(0, 10), (30, 70)]), (200, [(0, 5), (6, 194)]), (384, [(0, 128), (256, 128)]), (300, [(0, 4), (50, 10), (61, 129), (250, 50)]),
          (140, [(7, 133)]), (512, [(0, 4), (260, 252)]), (200, [(0, 77)]), (200, [(0, 200)])]
MODELS = [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16"), ("qwen3-1.7b", "bf16"), ("llama-3.2-1b", "fp32")]
FORCED = [17, 4001, 902, 33]
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -23}


def real(name, dtype, max_batch, max_ctx=CTX, budget=0):
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 2, 4096, max_ctx, max_batch
    if d.n_positions > 0:
        d.n_positions = max(d.n_positions, max_ctx)
    m = Model(d)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(1234, 0.02).finalize()


def kv_all(m, row, layers=2):
    return [m.read_kv(row, layer) for layer in range(layers)]


def same_kv(a, b, what=""):
    for (k0, v0), (k1, v1) in zip(a, b):
        np.testing.assert_array_equal(k0, k1, err_msg=str(what)); np.testing.assert_array_equal(v0, v1, err_msg=str(what))


def free(m):
    return m.get_option("kv.free_tokens")


def kept(ranges):
    return sum(n for _, n in ranges)


def storage_ulp(x, dtype):
    """one unit in the last place of the storage dtype at |x|"""
    a = np.abs(x)
    if dtype == "fp16":
        return np.spacing(a.astype(np.float16)).astype(np.float64)
    if dtype == "fp32":
        return np.spacing(a.astype(np.float32)).astype(np.float64)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 7)


def force(m, toks):
    V = m.desc.vocab
    onehot = np.full((len(toks), V), -1.0, np.float32); onehot[np.arange(len(toks)), toks] = 1.0
    m.set_logits(onehot)
    np.testing.assert_array_equal(m.sample(GREEDY), toks)
    return m.decode(1, GREEDY)[0].copy()


def run_steps(m):
    toks, logits = [int(m.sample_row(0, GREEDY))], []
    for t in FORCED:
        toks.append(int(force(m, np.array([t]))[0]))
        logits.append(m.logits(rounded=False)[0].copy())
    return toks, logits


def check_layer0(got, ref, dtype, what):
    """V by check_kv's layer-0 form (tests/test_hip_extend_row.py): one ulp of the entry plus 4e-6 of the largest; K by that plus 1.25 u |pair|"""
    ulp, u = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10, "fp32": 2.0 ** -23}[dtype], U[dtype]      # (check_kv's table; u for the double-rounding term alone)
    (gk, gv), (rk, rv) = got, ref
    assert gk.shape == rk.shape and gv.shape == rv.shape, what
    bad = np.abs(gv - rv) > ulp * np.abs(rv) + 4e-6 * np.abs(rv).max()
    assert not bad.any(), (what, "V", int(bad.sum()), float(np.abs(gv - rv).max()))
    bad = np.abs(gk - rk) > ulp * np.abs(rk) + 4e-6 * np.abs(rk).max() + 1.25 * u * splice_ref.pair_norm(rk)
    assert not bad.any(), (what, "K", int(bad.sum()), float(np.abs(gk - rk).max()))


@pytest.mark.parametrize("name,dtype", MODELS)
def test_the_move_layer0_and_paged_equals_unpaged(name, dtype):
    """checks 1, 2, 4 and the free count of 5 on every shape"""
    flat = real(name, dtype, 2)
    ctxs = [flat] + ([real(name, dtype, 2, budget=2 * CTX)] if dtype != "fp32" else [])
    table_ref = not flat.desc.rope_factor > 0
    ang = splice_ref.angles(flat.desc, CTX) if table_ref else None
    for past, ranges in SHAPES:
        seq = synth.synth_prompt(4096, past, 700 + past)
        src, new_len = splice_ref.source_positions(ranges), kept(ranges)
        runs = []
        for m in ctxs:
            what = (name, dtype, m is not flat, past, ranges)
            m.reset_cache(); m.forward_row(0, seq)
            before = kv_all(m, 0)
            assert m.splice_row(0, ranges) == new_len, what
            assert m.past_length_row(0) == new_len and m.past_length == new_len, what
            if m is not flat:
                assert free(m) == 2 * CTX - BLK * -(-new_len // BLK), what
            after = kv_all(m, 0)
            moved = src != np.arange(new_len)
            for (k0, v0), (k1, v1) in zip(before, after):
                np.testing.assert_array_equal(v1, v0[src], err_msg=str(what))
                np.testing.assert_array_equal(k1[~moved], k0[src][~moved], err_msg=str(what))
                if moved.any():
                    assert (k1[moved] != k0[src][moved]).any(), what
                if table_ref:
                    ref, _ = splice_ref.splice(k0, v0, ranges, ang)
                    err = np.abs(k1 - ref)
                    bound = storage_ulp(ref, dtype) + 2.0 ** -20 * splice_ref.pair_norm(ref)
                    print(what, "max err / bound", float((err / bound).max()))
                    assert (err <= bound).all(), (what, float((err / bound).max()))
            # layer 0 against a fresh prefill of the spliced tokens, in row 1
            m.forward_row(1, seq[src])
            check_layer0(after[0], m.read_kv(1, 0), dtype, what)
            runs.append(after)
        if len(runs) == 2:
            same_kv(runs[0], runs[1], (name, past, "paged vs unpaged"))
    for m in ctxs:
        m.close()


@pytest.mark.parametrize("name,dtype,paged", [("llama-3.2-1b", "bf16", 0), ("llama-3.2-1b", "bf16", 1), ("mistral-7b-v0.3", "fp16", 1), ("llama-3.2-1b", "fp32", 0)])
def test_bookkeeping_is_consistent_bit_for_bit(name, dtype, paged):
    """check 3: splice + extend_row in A; forward_row of any new_len tokens + write_kv of A's post-splice rows + the same extend_row in B"""
    A, B = real(name, dtype, 1, budget=CTX * paged), real(name, dtype, 1, budget=CTX * paged)
    ids = synth.synth_prompt(4096, 5, 77)
    for past, ranges in SHAPES:
        what = (name, dtype, paged, past, ranges)
        new_len = kept(ranges)
        A.reset_cache(); A.forward_row(0, synth.synth_prompt(4096, past, 700 + past))
        A.splice_row(0, ranges)
        rows = kv_all(A, 0)
        B.reset_cache(); B.forward_row(0, synth.synth_prompt(4096, new_len, 5))
        for layer, (k, v) in enumerate(rows):
            B.write_kv(0, layer, k, v)
        same_kv(kv_all(B, 0), rows, what)
        if new_len + len(ids) + len(FORCED) > CTX:
            continue
        for m in (A, B):
            m.extend_row(0, ids)
        assert A.past_length_row(0) == B.past_length_row(0) == new_len + len(ids), what
        np.testing.assert_array_equal(A.logits(rounded=False), B.logits(rounded=False), err_msg=str(what))
        same_kv(kv_all(A, 0), kv_all(B, 0), what)
        (ta, la), (tb, lb) = run_steps(A), run_steps(B)
        assert ta == tb, what
        for x, y in zip(la, lb):
            np.testing.assert_array_equal(x, y, err_msg=str(what))
        same_kv(kv_all(A, 0), kv_all(B, 0), what)
        if paged:
            assert free(A) == free(B), what
    A.close(); B.close()


def forked(budget_blocks=16):
    """paged: a 300-token prefix in row 0, forked into rows 1 and 2 (two full blocks shared, one tail block each)"""
    m = real("llama-3.2-1b", "bf16", 3, budget=budget_blocks * BLK)
    prefix = synth.synth_prompt(4096, 300, 81)
    m.forward_row(0, prefix); m.fork_row(0, [1, 2])
    return m, prefix


def test_fork_then_splice_copies_before_it_writes():
    """check 5: f = 150 lies inside shared block 1 — one fresh block, rows [128, 150) carried, the siblings' caches and their next step equal a control's; row 1 equals
    the same splice on an unpaged row; with an empty free list TGX_ERR_CONTEXT and nothing changes"""
    ranges = [(0, 150), (160, 140)]
    m, prefix = forked()
    ctrl, _ = forked()
    f0 = free(m)
    assert f0 == (16 - 5) * BLK
    assert m.splice_row(1, ranges) == 290
    assert free(m) == f0 - BLK                                # blocks: 0 shared, 1 fresh, 2 the row's own tail
    for r in (0, 2):
        same_kv(kv_all(m, r), kv_all(ctrl, r), r)
    solo = real("llama-3.2-1b", "bf16", 1)
    solo.forward_row(0, prefix); solo.splice_row(0, ranges)
    same_kv(kv_all(m, 1), kv_all(solo, 0), "row 1 against the unpaged splice")
    text = synth.synth_prompt(4096, 3, 9)
    m.extend_row(1, text); ctrl.extend_row(1, text)
    for x in (m, ctrl):
        x.sample(GREEDY)
    dm, dc = m.decode(1, GREEDY), ctrl.decode(1, GREEDY)
    np.testing.assert_array_equal(dm[:, [0, 2]], dc[:, [0, 2]])
    np.testing.assert_array_equal(m.logits(rounded=False)[[0, 2]], ctrl.logits(rounded=False)[[0, 2]])
    for r in (0, 2):
        same_kv(kv_all(m, r), kv_all(ctrl, r), r)
    m.reset_row(1)
    assert free(m) == f0 + BLK                                # row 1's blocks returned; the shared ones stay with rows 0 and 2
    m.close(); ctrl.close(); solo.close()
    # no free block: refused, nothing moves
    m, prefix = forked(budget_blocks=5)
    assert free(m) == 0
    before = [kv_all(m, r) for r in range(3)]
    with pytest.raises(TgxError) as ei:
        m.splice_row(1, ranges)
    assert ei.value.status == 8
    assert free(m) == 0 and [m.past_length_row(r) for r in range(3)] == [300] * 3
    for r in range(3):
        same_kv(before[r], kv_all(m, r), r)
    m.sample(GREEDY); m.decode(1, GREEDY)                     # not poisoned, every row still has its logits
    m.close()


@pytest.mark.parametrize("paged", [0, 1])
def test_splice_in_a_running_batch_leaves_the_other_rows_alone(paged):
    """check 6: three rows decoding, row 1 spliced and re-fed; rows 0 and 2 == a control bit for bit across the splice and a joint decode_rows; row 1, finished on
    max_new, is accepted and runs again"""
    budget = 6 * BLK if paged else 0
    gpu, ctrl = real("llama-3.2-1b", "bf16", 3, 256, budget), real("llama-3.2-1b", "bf16", 3, 256, budget)
    prompts = np.stack([synth.synth_prompt(4096, 150, 60 + r) for r in range(3)])
    for m in (gpu, ctrl):
        m.forward(prompts); m.sample(GREEDY); m.decode(1, GREEDY)
    gpu.set_row_stop(1, max_new=1)
    (ig, ng, fg), (ic, nc, fc) = gpu.decode_rows(1), ctrl.decode_rows(1)
    np.testing.assert_array_equal(ig, ic)
    assert fg[1] == 2 and fg[0] == fg[2] == 0
    others, p1 = [0, 2], gpu.past_length_row(1)
    assert p1 in (151, 152)
    n1 = 4 + p1 - 80
    assert gpu.splice_row(1, [(0, 4), (80, p1 - 80)]) == n1
    assert [gpu.past_length_row(r) for r in range(3)] == [152, n1, 152] and gpu.past_length == 152
    np.testing.assert_array_equal(gpu.logits(rounded=False)[others], ctrl.logits(rounded=False)[others])
    for r in others:
        same_kv(kv_all(gpu, r), kv_all(ctrl, r), r)
    with pytest.raises(TgxError) as ei:                       # row 1 holds no logits
        gpu.decode_rows(1)
    assert ei.value.status == 4
    gpu.extend_row(1, [int(ig[0, 1])]); gpu.sample_row(1, GREEDY)
    gpu.set_row_stop(1, max_new=0)
    (ig, ng, fg), (ic, nc, fc) = gpu.decode_rows(2), ctrl.decode_rows(2)
    np.testing.assert_array_equal(ig[:, others], ic[:, others])
    np.testing.assert_array_equal(gpu.logits(rounded=False)[others], ctrl.logits(rounded=False)[others])
    assert ng[1] == 2 and fg[1] == 0 and gpu.past_length_row(1) == n1 + 3      # the finished state was cleared: the row ran again
    for r in others:
        same_kv(kv_all(gpu, r), kv_all(ctrl, r), r)
    gpu.close(); ctrl.close()


@pytest.mark.parametrize("paged", [0, 1])
def test_refusals_change_nothing(paged):
    """check 7"""
    budget = 5 * BLK if paged else 0
    m, ctrl = real("llama-3.2-1b", "bf16", 5, budget=budget), real("llama-3.2-1b", "bf16", 5, budget=budget)
    P = lambda n, s: synth.synth_prompt(4096, n, s)
    for x in (m, ctrl):
        x.forward_rows([0, 1, 2, 3], [P(200, 1), P(100, 2), P(30, 3), P(10, 4)])
        for r in range(4):
            x.sample_row(r, GREEDY)
        x.reset_row(3)                                       # row 3: retired; row 4: beyond the batch
    allocs = m.get_option("mem.live_allocs")
    kv0 = [kv_all(m, r) for r in range(3)]

    def state(x):
        return x.get_option("kv.free_tokens"), [x.past_length_row(r) for r in range(5)], x.past_length

    def refused(status, fn):
        before = state(m)
        with pytest.raises(TgxError) as ei:
            fn()
        assert ei.value.status == status, str(ei.value)
        assert state(m) == before == state(ctrl)
        np.testing.assert_array_equal(m.logits(rounded=False), ctrl.logits(rounded=False))
        for r in range(3):
            same_kv(kv0[r], kv_all(m, r), r)

    refused(4, lambda: m.splice_row(3, [(0, 1)]))                        # retired row
    refused(4, lambda: m.splice_row(4, [(0, 1)]))                        # row >= batch
    refused(1, lambda: m.splice_row(5, [(0, 1)]))                        # outside [0, max_batch)
    refused(1, lambda: m.splice_row(-1, [(0, 1)]))
    refused(1, lambda: m.splice_row(0, np.zeros((0, 2))))                # n_keep 0
    refused(1, lambda: m.splice_row(0, [(i, 1) for i in range(0, 34, 2)]))      # n_keep 17
    refused(1, lambda: m.splice_row(0, [(0, 0)]))                        # empty
    refused(1, lambda: m.splice_row(0, [(10, 5), (3, 2)]))               # unsorted
    refused(1, lambda: m.splice_row(0, [(0, 10), (9, 5)]))               # overlapping
    refused(1, lambda: m.splice_row(0, [(0, 201)]))                      # outside [0, past)
    refused(1, lambda: m.splice_row(0, [(0, 4), (200, 1)]))
    refused(1, lambda: m.splice_row(0, [(-1, 5)]))
    import ctypes
    one = (ctypes.c_int64 * 1)(1)
    assert m.be.splice_row(m._ctx, 0, 1, None, one, None) == 1 and m.be.splice_row(m._ctx, 0, 1, one, None, None) == 1 and state(m) == state(ctrl)      # null pointers
    assert m.get_option("mem.live_allocs") == allocs                     # nothing was allocated by a context that never spliced
    assert m.splice_row(0, [(0, 200)]) == 200                            # the row as it is, logits and token in place: a no-op
    assert m.splice_row(0, [(0, 120), (120, 80)]) == 200                 # ... also in two touching pieces
    assert state(m) == state(ctrl) and m.get_option("mem.live_allocs") == allocs
    np.testing.assert_array_equal(m.decode(1, GREEDY), ctrl.decode(1, GREEDY))      # not poisoned, the same step
    np.testing.assert_array_equal(m.logits(rounded=False), ctrl.logits(rounded=False))
    # ---- the no-logits state
    assert m.splice_row(1, [(0, 4), (50, 51)]) == 55
    assert m.past_length_row(1) == 55 and m.past_length == 201
    for fn in (lambda: m.sample_row(1, GREEDY), lambda: m.sample(GREEDY), lambda: m.decode(1, GREEDY), lambda: m.decode_rows(1), lambda: m.fork_row(1, [3]),
               lambda: m.step_async(GREEDY)):
        with pytest.raises(TgxError) as ei:
            fn()
        assert ei.value.status == 4, str(ei.value)
    assert [m.past_length_row(r) for r in range(4)] == [201, 55, 31, 0]
    m.extend_row(1, P(3, 5)); m.sample_row(1, GREEDY)
    m.decode(1, GREEDY)
    assert [m.past_length_row(r) for r in range(3)] == [202, 59, 32]
    m.close(); ctrl.close()


def test_a_call_before_finalize_is_refused():
    d = copy.deepcopy(known_desc("llama-3.2-1b", "bf16"))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 2, 4096, CTX, 1
    m = Model(d)                                             # created, never finalized
    with pytest.raises(TgxError) as ei:
        m.splice_row(0, [(0, 1)])
    assert ei.value.status == 4, str(ei.value)
    m.close()


def test_gpt2_is_refused():
    m = real("gpt2", "bf16", 1)
    m.forward_row(0, synth.synth_prompt(4096, 100, 1))
    kv0 = kv_all(m, 0)
    with pytest.raises(TgxError) as ei:
        m.splice_row(0, [(0, 10), (30, 70)])
    assert ei.value.status == 2, str(ei.value)
    assert m.past_length_row(0) == 100
    same_kv(kv0, kv_all(m, 0))
    m.sample_row(0, GREEDY); m.decode(1, GREEDY)
    m.close()
