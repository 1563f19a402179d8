"""Row snapshots (include/tgx.h: tgx_row_snapshot_bytes / tgx_save_row / tgx_restore_row; csrc/row_snapshot.h, kernels/kv_pack.h): a live row saved to host memory and
restored into any row of any context of the same geometry.  Held to:
  * a saved, reset, dirtied and restored row continues BIT for bit like a control that never left the device (lengths, ids, logits, every cache row), prompts of
    5 / 128 / 200 / 300 tokens, slabs and paged, five geometries; greedy into another row, sampled into the same row;
  * the three states of a source (logits and token, logits only, no logits after tgx_truncate_row);
  * one format for both cache layouts: byte-identical blobs, the KV section as documented, blobs crossing between a paged and a slab context and into a second context;
  * staging groups of one layer; paged block accounting; refusals that change nothing; bystander rows and restated processor histories; device memory; the CPU oracle."""
import copy
import ctypes
import struct

import numpy as np
import pytest

from conftest import rel_err
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import GREEDY, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu

WARM = SamplerCfg(0.8, 0, 0.9, 0.0)
BLK = 128


# ---- the shapes and helpers of tests/test_hip_fork_row.py
def cut(name, dtype, max_batch, max_ctx, peaked=False):
    """the two-layer, vocabulary-4096 cut of a real geometry"""
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 2, 4096, max_ctx, max_batch
    if d.n_positions:
        d.n_positions = max(d.n_positions, max_ctx)
    if peaked:
        d.tied = False                    # the peaked checkpoint's loud rows live in an untied lm_head (tinygpt_amd/synth.py)
    return d


def real(name, dtype, max_batch, max_ctx, budget=0, peaked=False):
    m = Model(cut(name, dtype, max_batch, max_ctx, peaked))
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(1234, 0.02, peaked=peaked).finalize()


def prompt(n, seed):
    return synth.synth_prompt(4096, n, seed)


def free(m):
    return m.get_option("kv.free_tokens")


def assert_same_bits(a, b, rows, what):
    """logits and every layer's cache rows of `rows`, context a against context b"""
    np.testing.assert_array_equal(a.logits(rounded=False)[rows], b.logits(rounded=False)[rows], err_msg=str(what))
    for r in rows:
        assert a.past_length_row(r) == b.past_length_row(r), (what, r)
        for layer in range(2):
            for x, y in zip(a.read_kv(r, layer), b.read_kv(r, layer)):
                np.testing.assert_array_equal(x, y, err_msg=str(what + (r, layer)))


def refused(m, status, call, rows):
    """`call` is refused with `status` and leaves kv.free_tokens, every row's length and the longest length as they were"""
    def state():
        return free(m), [m.past_length_row(r) for r in range(rows)], m.past_length
    before = state()
    with pytest.raises(TgxError) as ei:
        call()
    assert ei.value.status == status, str(ei.value)
    assert state() == before


# prompt seeds of test_hip_fork_row.py::test_forked_row_against_the_cpu_oracle: with these the oracle's top-2 gap exceeds 2e-3 of its largest logit on 8 of the 8 steps
ORACLE_SEED = {"llama-3.2-1b": 8, "mistral-7b-v0.3": 8, "qwen3-1.7b": 8, "gpt2": 8}


_oracle_runs = {}      # (family, dtype, ...) -> oracle_steps' result: the paged and the slab case of a geometry share one oracle run


def oracle_steps(d, p, steps, peaked):
    """the CPU oracle alone on prompt p, free-running greedy: its logits before each of steps + 1 tokens, and the tokens"""
    key = (d.family, d.hidden, d.heads, d.compute_dtype, p.tobytes(), steps, peaked)
    if key not in _oracle_runs:
        _oracle_runs[key] = _oracle_steps(d, p, steps, peaked)
    return _oracle_runs[key]


def _oracle_steps(d, p, steps, peaked):
    from oracle.oracle_ffi import OracleModel
    ref = OracleModel(d)
    for name, bits in synth.synth_checkpoint(d, 1234, 0.02, peaked=peaked):
        ref.upload(name, bits)
    ref.finalize()
    ref.forward(p[None, :])
    logits, toks = [], []
    for step in range(steps + 1):
        logits.append(ref.logits(rounded=False)[0].copy())
        t = ref.sample(GREEDY)
        toks.append(int(t[0]))
        if step < steps:
            ref.forward(t[None, :])
    ref.close()
    return logits, toks


def clear_gap(l):
    top2 = np.partition(l, -2)[-2:]
    return (top2[1] - top2[0]) > 2e-3 * np.abs(l).max()


MODELS = [("llama-3.2-1b", "bf16", 0), ("llama-3.2-1b", "bf16", 1), ("mistral-7b-v0.3", "fp16", 0), ("mistral-7b-v0.3", "fp16", 1), ("qwen3-1.7b", "bf16", 0),
          ("qwen3-1.7b", "bf16", 1), ("gpt2", "bf16", 0), ("gpt2", "bf16", 1), ("gpt2", "fp32", 0)]
CTX = 512
HEADER = 128


def pair(name, dtype, paged, rows=2, ctx=CTX, blocks=8):
    budget = blocks * BLK if paged else 0
    return real(name, dtype, rows, ctx, budget), real(name, dtype, rows, ctx, budget)


def row_bits(m, row):
    """length, raw logits and every layer's cache rows of one row"""
    return [m.past_length_row(row), m.logits(rounded=False)[row]] + [x for layer in range(2) for x in m.read_kv(row, layer)]


def assert_rows_equal(a, ra, b, rb, what):
    for x, y in zip(row_bits(a, ra), row_bits(b, rb)):
        np.testing.assert_array_equal(x, y, err_msg=str(what))


def header(blob):
    """the header's fields by the byte offsets include/tgx.h documents"""
    magic, version, hbytes, total = struct.unpack_from("<8sIIQ", blob, 0)
    geom = struct.unpack_from("<9i", blob, 24)
    flags, past, s_off, s_bytes, kv_off, kv_bytes = struct.unpack_from("<IqQQQQ", blob, 60)
    return dict(magic=magic, version=version, header=hbytes, total=total, geom=geom, flags=flags, past=past, state_off=s_off, state_bytes=s_bytes, kv_off=kv_off,
                kv_bytes=kv_bytes, zeros=blob[104:128])


def start(m, row, p, cfg, seed, steps=7):
    """admission, sampler, first token, `steps` steps -> the ids produced"""
    m.forward_row(row, p); m.set_row_sampler(row, cfg, seed)
    first = m.sample_row(row, cfg, seed=seed)
    ids = m.decode_rows(steps)[0][:, row] if steps else np.zeros(0, np.int64)
    return [first] + [int(t) for t in ids]


def detour(m, row):
    """save `row`, retire it, dirty what it freed with another prompt, retire that -> the blob"""
    blob = m.save_row(row)
    m.reset_row(row)
    m.forward_row(row, prompt(150, 77)); m.reset_row(row)
    return blob


# ---- 1. round trip, bit for bit
@pytest.mark.parametrize("name,dtype,paged", MODELS)
def test_round_trip_bit_for_bit(name, dtype, paged):
    """context A: forward_row(0, p), sample_row, decode_rows(7), save_row(0), reset_row(0), another prompt through row 0 and reset again (the freed blocks / the slab are
    dirtied), restore_row, the sampler set again, decode_rows(40); context B: the same without the detour.  Greedy: A restores into row 1 (row == batch), B forks
    row 0 into row 1 and retires row 0 — row 1 against row 1.  T 0.8 / top-p 0.9, seed 101: A restores into row 0 itself (a draw hashes seed, position and ROW).
    Lengths, ids, raw logits and every layer's cache rows are equal as bits; 128 -> 175 crosses a block boundary"""
    A, B = pair(name, dtype, paged)
    for P in (5, 128, 200, 300):
        p = prompt(P, 500 + P)
        for cfg, seed, target in ((GREEDY, 0, 1), (WARM, 101, 0)):
            for m in (A, B):         # (retired rows ride along in the steps; tgx_reset_cache would leave empty rows in the batch, which no step accepts)
                m.reset_row(0); m.reset_row(1)
            ia, ib = start(A, 0, p, cfg, seed), start(B, 0, p, cfg, seed)
            assert ia == ib
            assert A.row_snapshot_bytes(0) == len(A.save_row(0))
            blob = detour(A, 0)
            A.restore_row(target, blob)
            if target == 1:
                B.fork_row(0, [1]); B.reset_row(0)
            assert A.past_length_row(target) == B.past_length_row(target) == P + 7
            assert_rows_equal(A, target, B, target, (P, target, "restored"))
            A.set_row_sampler(target, cfg, seed); B.set_row_sampler(target, cfg, seed)
            (ja, na, fa), (jb, nb, fb) = A.decode_rows(40), B.decode_rows(40)
            np.testing.assert_array_equal(ja[:, target], jb[:, target], err_msg=str((P, target)))
            assert na[target] == nb[target] == 40 and fa[target] == fb[target] == 0
            assert_rows_equal(A, target, B, target, (P, target, "decoded"))
    A.close(); B.close()


# ---- 2. the three states of a source
@pytest.mark.parametrize("paged", [0, 1])
def test_three_states(paged):
    """saved fresh from forward_row (logits, no token): sample_row after the restore gives the control's id, then its steps.  Saved after truncate_row(0, past - 3): the
    snapshot is smaller by 4 * (hidden + vocab) bytes plus alignment, sample_row / decode_rows / fork_row refuse with TGX_ERR_STATE until extend_row ran, and after
    extend_row with the three dropped tokens the row equals, bit for bit, a control extended without the detour.  (Mid-generation: the round trip above.)"""
    A, B = pair("llama-3.2-1b", "bf16", paged)
    d = A.desc
    p = prompt(200, 61)
    # logits, no token
    A.forward_row(0, p); B.forward_row(0, p)
    blob = A.save_row(0)
    h = header(blob)
    assert h["flags"] == 1 and h["past"] == 200 and struct.unpack_from("<II", blob, HEADER) == (200, 0)
    detour(A, 0); A.restore_row(0, blob)
    assert_rows_equal(A, 0, B, 0, "fresh")
    with pytest.raises(TgxError) as ei:      # no current token yet
        A.decode_rows(1)
    assert ei.value.status == 4
    assert A.sample_row(0, GREEDY) == B.sample_row(0, GREEDY)
    np.testing.assert_array_equal(A.decode_rows(12)[0], B.decode_rows(12)[0])
    assert_rows_equal(A, 0, B, 0, "fresh, decoded")
    # mid-generation: flags 3, the token word is the current token
    blob_mid = A.save_row(0)
    hm = header(blob_mid)
    assert hm["flags"] == 3 and hm["past"] == 212
    # no logits
    dropped = prompt(3, 62)
    for m in (A, B):
        m.extend_row(0, dropped); m.truncate_row(0, 212)
    blob = A.save_row(0)
    h = header(blob)
    assert h["flags"] == 0 and h["past"] == 212 and h["state_bytes"] == 8
    assert hm["state_bytes"] - h["state_bytes"] == 4 * (d.hidden + d.vocab)
    assert h["kv_bytes"] == hm["kv_bytes"] and h["kv_off"] == HEADER + 16 and hm["kv_off"] == (HEADER + hm["state_bytes"] + 15) // 16 * 16
    assert len(blob_mid) - len(blob) == hm["kv_off"] - h["kv_off"]
    detour(A, 0); A.restore_row(0, blob)
    assert A.past_length_row(0) == 212 and A.past_length == 212
    for call in (lambda: A.sample_row(0, GREEDY), lambda: A.decode_rows(1), lambda: A.decode(1, GREEDY), lambda: A.fork_row(0, [1])):
        with pytest.raises(TgxError) as ei:
            call()
        assert ei.value.status == 4, str(ei.value)
    for m in (A, B):
        m.extend_row(0, dropped)
    assert_rows_equal(A, 0, B, 0, "extended")
    assert A.sample_row(0, GREEDY) == B.sample_row(0, GREEDY)
    np.testing.assert_array_equal(A.decode_rows(8)[0], B.decode_rows(8)[0])
    assert_rows_equal(A, 0, B, 0, "extended, decoded")
    A.close(); B.close()


# ---- 3. one format, two layouts
def storage_bytes(x, dtype):
    """fp32 values that came out of the cache -> the bytes of the storage dtype (exact)"""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "fp32":
        return x.tobytes()
    if dtype == "fp16":
        return x.astype(np.float16).tobytes()
    return (x.view(np.uint32) >> 16).astype(np.uint16).tobytes()


@pytest.mark.parametrize("name,dtype", [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16")])
def test_one_format_two_layouts(name, dtype):
    """the same sequence saved on a paged and on a slab context: byte-identical blobs; the KV section is [layer][K, V][kv_head][past][head_dim] as assembled from read_kv;
    the paged blob restored into the slab context, the slab blob into the paged one, and a blob into a third context continue bit-identically to the control"""
    slab, paged, third, ctrl = real(name, dtype, 2, CTX), real(name, dtype, 2, CTX, 8 * BLK), real(name, dtype, 2, CTX, 8 * BLK), real(name, dtype, 2, CTX)
    p = prompt(300, 71)
    ids = [start(m, 0, p, GREEDY, 0, steps=5) for m in (slab, paged, ctrl)]
    assert ids[0] == ids[1] == ids[2]
    bs, bp = slab.save_row(0), paged.save_row(0)
    assert bs == bp
    h = header(bs)
    d = slab.desc
    assert h["magic"] == b"TGXSNAP\0" and h["version"] == 1 and h["header"] == HEADER and h["total"] == len(bs) and h["zeros"] == bytes(24)
    assert h["geom"] == (d.to_c().family, d.hidden, d.layers, d.heads, d.kv_heads, d.head_dim, d.vocab, d.to_c().compute_dtype, d.to_c().qk_norm)
    assert h["past"] == 305 and h["flags"] == 3 and h["state_off"] == HEADER and h["kv_off"] % 16 == 0
    esz = 2
    assert h["kv_bytes"] == 2 * 2 * d.kv_heads * 305 * d.head_dim * esz and h["kv_off"] + h["kv_bytes"] == len(bs)
    want = b""
    for layer in range(2):
        for x in slab.read_kv(0, layer):          # [T][kv_heads][hd] -> [kv_head][T][hd]
            want += storage_bytes(x.transpose(1, 0, 2), dtype)
    assert bs[h["kv_off"]:] == want
    state = np.frombuffer(bs, np.float32, d.hidden + d.vocab, HEADER + 8)
    np.testing.assert_array_equal(state[d.hidden:], slab.logits(rounded=False)[0])
    # crossing over, and into a context that never saw the sequence
    for m, blob in ((slab, bp), (paged, bs)):
        detour(m, 0); m.restore_row(0, blob)
    third.restore_row(0, bs)
    assert third.batch == 1 and third.past_length == 305
    want_ids = ctrl.decode_rows(30)[0][:, 0]
    for m in (slab, paged, third):
        np.testing.assert_array_equal(m.decode_rows(30)[0][:, 0], want_ids)
        assert_rows_equal(m, 0, ctrl, 0, "crossed")
    for m in (slab, paged, third, ctrl):
        m.close()


# ---- 4. staging groups
@pytest.mark.parametrize("paged", [0, 1])
def test_staging_one_layer_per_group(paged):
    """snapshot.stage_kib = 1 (one layer per group): the blob's bytes equal the default's, and a restore under it gives the default's bits"""
    A, B = pair("llama-3.2-1b", "bf16", paged)
    assert A.get_option("snapshot.stage_kib") == 65536
    A.set_option("snapshot.stage_kib", 1)
    p = prompt(300, 81)
    for m in (A, B):
        start(m, 0, p, GREEDY, 0, steps=3)
    ba, bb = A.save_row(0), B.save_row(0)
    assert ba == bb
    for m in (A, B):
        detour(m, 0); m.restore_row(1, ba); m.restore_row(0, ba)
    assert_rows_equal(A, 0, B, 0, "grouped"); assert_rows_equal(A, 1, B, 1, "grouped")
    assert_rows_equal(A, 0, A, 1, "two copies")
    np.testing.assert_array_equal(A.decode_rows(10)[0], B.decode_rows(10)[0])
    assert A.save_row(1) == B.save_row(0)
    A.close(); B.close()


# ---- 5. paged accounting
def test_paged_accounting():
    """kv.free_tokens is unchanged by a save and down by ceil(past / 128) * 128 after a restore; a restored sibling of a fork owns all its blocks and the other siblings
    decode on like a control that never saved; a restore that needs one block more than the pool can give is TGX_ERR_CONTEXT and changes nothing"""
    budget = 12 * BLK
    m, ctrl = real("llama-3.2-1b", "bf16", 4, CTX, budget), real("llama-3.2-1b", "bf16", 4, CTX, budget)
    p = prompt(300, 91)
    for x in (m, ctrl):
        x.forward_row(0, p); x.fork_row(0, [1, 2])
        for r in range(3):
            x.sample_row(r, GREEDY)
    assert free(m) == budget - 5 * BLK                   # two shared blocks, three tails
    blob = m.save_row(1)
    assert free(m) == budget - 5 * BLK
    m.reset_row(1); assert free(m) == budget - 4 * BLK
    m.restore_row(1, blob); assert free(m) == budget - 7 * BLK      # three blocks of its own
    m.reset_row(1); assert free(m) == budget - 4 * BLK              # ... all three come back
    m.restore_row(1, blob)
    (ia, _, _), (ib, _, _) = m.decode_rows(20), ctrl.decode_rows(20)
    np.testing.assert_array_equal(ia, ib)
    assert_same_bits(m, ctrl, range(3), ("siblings",))
    m.close(); ctrl.close()
    # exhaustion by exactly ONE block: 6 blocks; row 0 holds 3, row 1 holds 1 -> two free, and the new row 2 gives none back; a 3-block snapshot is one short
    budget = 6 * BLK
    m = real("llama-3.2-1b", "bf16", 3, CTX, budget)
    m.forward_row(0, p); m.sample_row(0, GREEDY)
    blob = m.save_row(0)
    m.forward_row(1, prompt(100, 92)); m.sample_row(1, GREEDY)
    assert free(m) == 2 * BLK and header(blob)["past"] == 300
    refused(m, 8, lambda: m.restore_row(2, blob), 3)
    assert m.batch == 2
    m.decode_rows(2)                                     # still decodes
    m.reset_row(1); assert free(m) == 3 * BLK
    m.restore_row(2, blob); assert free(m) == 0
    m.close()


# ---- 6. refusals change nothing
def patched(blob, off, fmt, value):
    b = bytearray(blob)
    struct.pack_into(fmt, b, off, value)
    return bytes(b)


def test_refusals_change_nothing():
    budget = 10 * BLK
    m, ctrl = real("llama-3.2-1b", "bf16", 4, CTX, budget), real("llama-3.2-1b", "bf16", 4, CTX, budget)
    for x in (m, ctrl):
        x.forward_rows([0, 1, 2], [prompt(200, 1), prompt(140, 2), prompt(20, 3)])
        for r in range(3):
            x.sample_row(r, GREEDY)
        x.reset_row(2)                                   # row 2 retired
        x.set_row_stop(1, max_new=2)
        assert x.decode_rows(2)[2][1] == 2               # row 1 finished
    blob = m.save_row(0)
    n = len(blob)

    def refused_and_decodes(status, call, what):
        """the refusal, then one step: ids, counts, finish reasons and row 0's raw logits equal the control's, which never made the call"""
        refused(m, status, call, 4)
        (ia, na, fa), (ib, nb, fb) = m.decode_rows(1), ctrl.decode_rows(1)
        np.testing.assert_array_equal(ia, ib, err_msg=str(what)); np.testing.assert_array_equal(na, nb); np.testing.assert_array_equal(fa, fb)
        np.testing.assert_array_equal(m.logits(rounded=False)[[0]], ctrl.logits(rounded=False)[[0]], err_msg=str(what))

    # ---- saves
    for status, row in ((4, 2), (4, 1), (4, 3), (1, 4), (1, -1)):        # retired, finished, >= batch, out of range
        for call in (lambda: m.save_row(row), lambda: m.row_snapshot_bytes(row)):
            refused_and_decodes(status, call, ("save", row))
    empty = real("llama-3.2-1b", "bf16", 2, CTX)
    refused(empty, 4, lambda: empty.save_row(0), 2)                        # an empty row
    buf = np.full(n, 0xAB, np.uint8)
    out = np.array([-7], np.int64)
    st = m.be.save_row(m._ctx, 0, buf.ctypes.data_as(ctypes.c_void_p), n - 1, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    assert st == 1 and (buf == 0xAB).all() and out[0] == -7
    assert m.be.save_row(m._ctx, 0, None, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == 1
    assert m.be.save_row(m._ctx, 0, buf.ctypes.data_as(ctypes.c_void_p), n, None) == 1 and (buf == 0xAB).all()
    # ---- restores into the retired row 2
    other_hd = real("mistral-7b-v0.3", "bf16", 1, CTX)
    other_hd.forward_row(0, prompt(200, 1))
    d2 = cut("llama-3.2-1b", "bf16", 1, CTX); d2.vocab = 2048
    other_v = Model(d2).load_synthetic(1234, 0.02).finalize()
    other_v.forward_row(0, synth.synth_prompt(2048, 200, 1))
    h = header(blob)
    bad = [(1, blob[:-1]), (1, blob[:HEADER]), (1, blob[:HEADER - 1]), (1, b""), (1, blob + b"\0"),
           (1, b"XGXSNAP\0" + blob[8:]), (1, patched(blob, 8, "<I", 2)),
           (1, other_hd.save_row(0)), (1, other_v.save_row(0)),
           (1, patched(blob, HEADER, "<I", h["past"] - 1)),          # the position word
           (1, patched(blob, HEADER + 4, "<I", 4096)),               # the token word == vocab
           (1, patched(blob, 60, "<I", 2)),                          # a token without logits
           (1, patched(blob, 64, "<q", h["past"] + 1)),              # past without the bytes for it
           (1, patched(blob, 88, "<Q", h["kv_off"] + 16))]
    other_hd.close(); other_v.close()
    for i, (status, b) in enumerate(bad):
        refused_and_decodes(status, lambda: m.restore_row(2, b), ("restore", i))
    small = real("llama-3.2-1b", "bf16", 1, 128)
    refused(small, 8, lambda: small.restore_row(0, blob), 1)            # past 202 > max_ctx 128
    small.close()
    refused_and_decodes(4, lambda: m.restore_row(0, blob), "a live target")
    refused_and_decodes(4, lambda: m.restore_row(1, blob), "a finished target")
    refused_and_decodes(1, lambda: m.restore_row(4, blob), "out of range")
    refused(empty, 1, lambda: empty.restore_row(1, blob), 2)            # a new row that is not `batch`
    empty.close()
    # ---- and a few steps on, still the control
    (ia, na, fa), (ib, nb, fb) = m.decode_rows(3), ctrl.decode_rows(3)
    np.testing.assert_array_equal(ia, ib); np.testing.assert_array_equal(na, nb); np.testing.assert_array_equal(fa, fb)
    np.testing.assert_array_equal(m.logits(rounded=False)[[0]], ctrl.logits(rounded=False)[[0]])
    m.restore_row(2, blob)                                              # and the blob itself was good
    assert m.past_length_row(2) == h["past"]
    m.close(); ctrl.close()


def test_restore_into_row_0_sets_ticket_0():
    """a snapshot with a current token restored into row 0: tgx_fetch_token(0) names that token, as after tgx_sample — not the one row 0 sampled in between"""
    m = real("llama-3.2-1b", "bf16", 2, CTX)
    ids = start(m, 0, prompt(40, 31), GREEDY, 0, steps=3)
    blob = m.save_row(0)
    assert struct.unpack_from("<I", blob, HEADER + 4)[0] == ids[-1] and m.fetch_token(0) == ids[-1]
    m.reset_row(0); m.forward_row(0, prompt(20, 32))
    other = (ids[-1] + 1) % 4096
    onehot = np.full((1, 4096), -1.0, np.float32); onehot[0, other] = 1.0
    m.set_logits(onehot)
    assert m.sample_row(0, GREEDY) == other and m.fetch_token(0) == other
    m.reset_row(0)
    m.restore_row(1, blob)
    assert m.fetch_token(0) == other                     # another row: ticket 0 stays
    m.reset_row(1)
    m.restore_row(0, blob)
    assert m.fetch_token(0) == ids[-1]
    assert int(m.decode_rows(1)[0][0, 0]) >= 0
    m.close()


# ---- 7. bystanders and processors
@pytest.mark.parametrize("paged", [0, 1])
def test_bystanders_keep_their_bits(paged):
    """rows 1 and 2 decode on either side of a save, reset and restore of row 0 (and while it is away): their ids, logits and cache rows equal those of a control whose
    row 0 never left.  (Row 2 is the longest row throughout, so both contexts step on the same attention form.)"""
    A, B = pair("llama-3.2-1b", "bf16", paged, rows=3, blocks=12)
    for m in (A, B):
        m.forward_rows([0, 1, 2], [prompt(150, 41), prompt(40, 42), prompt(260, 43)])
        for r in range(3):
            m.sample_row(r, GREEDY)
    np.testing.assert_array_equal(A.decode_rows(5)[0], B.decode_rows(5)[0])
    blob = detour(A, 0)
    np.testing.assert_array_equal(A.decode_rows(4)[0][:, 1:], B.decode_rows(4)[0][:, 1:])
    A.restore_row(0, blob)
    assert_same_bits(A, B, [1, 2], ("away",))
    np.testing.assert_array_equal(A.decode_rows(16)[0][:, 1:], B.decode_rows(16)[0][:, 1:])
    assert_same_bits(A, B, [1, 2], ("back",))
    assert A.past_length_row(0) == B.past_length_row(0) - 4
    A.close(); B.close()


def test_restated_processors():
    """a row with repetition 1.3 / frequency 0.5 on, saved and restored, with tgx_set_row_penalties and tgx_set_row_history restated from the ids the test holds, decodes
    20 steps equal to the control"""
    A, B = pair("llama-3.2-1b", "bf16", 1)
    p = prompt(100, 51)
    ids = []
    for m in (A, B):
        m.forward_row(0, p)
        m.set_row_penalties(0, repetition=1.3, frequency=0.5).set_row_history(0, prompt_ids=p)
        first = m.sample_row(0, GREEDY)
        ids.append([first] + [int(t) for t in m.decode_rows(9)[0][:, 0]])
    assert ids[0] == ids[1]
    blob = detour(A, 0)
    A.restore_row(0, blob)
    A.set_row_penalties(0, repetition=1.3, frequency=0.5).set_row_history(0, prompt_ids=p, produced_ids=ids[0][:-1])      # the current token is counted by the step that consumes it
    (ia, _, _), (ib, _, _) = A.decode_rows(20), B.decode_rows(20)
    np.testing.assert_array_equal(ia, ib)
    assert_rows_equal(A, 0, B, 0, "processors")
    A.close(); B.close()


# ---- 8. memory
def test_memory():
    """a context that only asked for a snapshot's size holds what one that never heard of snapshots holds; the first save / restore cycle allocates the staging buffer,
    the next nine allocate nothing"""
    def mem(m):
        return m.get_option("mem.live_allocs"), m.get_option("mem.live_kib")
    A, B = pair("llama-3.2-1b", "bf16", 1)
    p = prompt(300, 11)
    for m in (A, B):
        start(m, 0, p, GREEDY, 0, steps=2)
    assert A.row_snapshot_bytes(0) > 0
    assert mem(A) == mem(B)
    figures = []
    for cycle in range(10):
        blob = A.save_row(0); A.reset_row(0); A.restore_row(0, blob)
        figures.append(mem(A))
    assert figures[0] == figures[9]
    assert figures[0][0] == mem(B)[0] + 1                # the staging buffer, once
    np.testing.assert_array_equal(A.decode_rows(5)[0], B.decode_rows(5)[0])
    A.close(); B.close()


# ---- 9. against the CPU oracle
@pytest.mark.parametrize("paged", [0, 1])
@pytest.mark.parametrize("name,dtype", [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16"), ("qwen3-1.7b", "bf16"), ("gpt2", "bf16")])
def test_restored_row_against_the_cpu_oracle(name, dtype, paged, oracle_lib):
    """peaked checkpoint, the prompt seeds of test_hip_fork_row.py: a row restored from a snapshot, teacher-forced with the oracle's tokens over 8 steps, stays within the
    1e-3 that test holds its forked row to, against the oracle run alone on the same prompt, and picks its ids wherever its top-2 gap is clear"""
    STEPS, P = 8, 150
    peaked = name != "gpt2"
    d = cut(name, dtype, 1, 256, peaked=peaked)
    p = prompt(P, ORACLE_SEED[name])
    ref_logits, ref_toks = oracle_steps(cut(name, dtype, 1, 256, peaked=peaked), p, STEPS, peaked)
    m = Model(d)
    if paged:
        m.set_option("kv.budget_tokens", 4 * BLK)
    m.load_synthetic(1234, 0.02, peaked=peaked).finalize()
    m.forward_row(0, p)
    blob = detour(m, 0)
    m.restore_row(0, blob)
    compared = 0
    for step in range(STEPS + 1):
        lg = m.logits(rounded=False)
        err = rel_err(lg[0][None, :], ref_logits[step][None, :])
        print(name, dtype, paged, step, err)
        assert err < 1e-3, (step, err)
        if step > 0 and clear_gap(ref_logits[step]):
            compared += 1
            assert int(np.argmax(lg[0])) == ref_toks[step], step
        if step < STEPS:
            onehot = np.full((1, d.vocab), -1.0, np.float32); onehot[:, ref_toks[step]] = 1.0
            m.set_logits(onehot)
            assert list(m.sample(GREEDY)) == [ref_toks[step]]
            m.decode(1, GREEDY)
    assert compared >= 6, compared
    assert m.past_length_row(0) == P + STEPS
    m.close()
