"""The "HL" exponent-packed kernels (kernels/gemv_packed.h) at the BENCHMARK'S ROW GEOMETRY: a one-layer Llama descriptor at hidden 2048, intermediate 8192,
vocabulary 1024 — NX = 4 chunks per lane at KS = 1 (gate_up, lm_head: K = 2048) and at KS = 4 (down: K = 8192), no padding chunk, gate_up with several units
per wave.  tests/test_hip_packed.py covers the tiny families (padded quads), every escape value, the fallback and the oracle; here the packed launches of all
three classes (weights.packed_classes = 7) are held to the plain kernels (weights.packed = 0) BIT FOR BIT — ids and unrounded fp32 logits as uint32, graph on
and off — on the ordinary checkpoint, with escapes planted where the row-pair decode could go wrong, and with the repair branch never / once taken.

The checkpoint is synth_checkpoint(seed 7, std 0.02): no row of it has more than four out-of-window weights (python tools/packed_census.py --layers 1
--vocab 1024 --seed 7), so all three matrices ARE packed; seed 1234's down matrix has a row of five and would run the plain kernel."""
import copy

import numpy as np
import pytest

from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import GREEDY

pytestmark = pytest.mark.gpu
SEED, STD, STEPS, PROMPT = 7, 0.02, 4, 24
GATE, UP, DOWN, HEAD = ("model.layers.0.mlp.gate_proj.weight", "model.layers.0.mlp.up_proj.weight", "model.layers.0.mlp.down_proj.weight",
                        "model.embed_tokens.weight")      # (tied head)
MLP = (GATE, UP, DOWN, HEAD)


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def desc():
    d = copy.deepcopy(known_desc("llama-3.2-1b", "bf16"))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 1, 1024, 64, 1
    assert (d.hidden, d.inter, d.tied) == (2048, 8192, True)
    return d


@pytest.fixture(scope="module")
def checkpoint():
    """the tensors once per module: every context uploads (an edited copy of) these"""
    return [(name, np.array(bits, copy=True)) for name, bits in synth.synth_checkpoint(desc(), SEED, STD)]


def build(hip, checkpoint, packed, plant=None):
    from tinygpt_amd.ffi import Model
    m = Model(desc(), hip)
    m.set_option("weights.packed", packed)
    m.set_option("weights.packed_classes", 7)
    for name, bits in checkpoint:
        if plant and name in MLP:
            bits = bits.copy()
            plant(name, bits)
        m.upload(name, bits)
    m.finalize()
    return m


def run(m, graph):
    """prompt + STEPS greedy decode steps: the ids and the unrounded fp32 logits of every step"""
    m.set_option("graph", graph)
    m.reset_cache()
    m.forward(synth.synth_prompt(1024, PROMPT, SEED)[None, :])
    ids, logits = [m.sample(GREEDY).copy()], [m.logits(rounded=False).copy()]
    for _ in range(STEPS):
        ids.append(m.decode(1, GREEDY)[0].copy())
        logits.append(m.logits(rounded=False).copy())
    return np.stack(ids), np.stack(logits)


def check(hip, checkpoint, plant=None, max_row_esc=None):
    plain, packed = build(hip, checkpoint, 0, plant), build(hip, checkpoint, 1, plant)
    assert plain.get_option("weights.packed_matrices") == 0
    assert packed.get_option("weights.packed_matrices") == 3 and packed.get_option("weights.packed_fallbacks") == 0
    if max_row_esc is not None:
        assert packed.get_option("weights.packed_max_row_esc") == max_row_esc
    for graph in (1, 0):
        a, b = run(packed, graph), run(plain, graph)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))      # bit for bit (-0 / +0 included)
        assert np.isfinite(b[1]).all()
    plain.close(); packed.close()


def out_of_window(bits):
    e = ((bits >> 7) & 0xFF).astype(np.int32)
    emax = int(e[e < 255].max())
    d = (e >> 1) - max((emax >> 1) - 7, 0)
    return (d < 0) | (d > 7) | (e == 0) | (e == 255)


def clean_rows(bits, n):
    """the first n rows without an out-of-window weight of their own: a planted row then holds exactly what the test put there"""
    rows = np.nonzero(out_of_window(bits).sum(axis=1) == 0)[0][:n]
    assert rows.size == n
    return [int(r) for r in rows]


def test_bench_row_geometry_is_bit_identical(hip, checkpoint):
    check(hip, checkpoint)


# escape values: +0, -0, a subnormal, a weight 2^-40 under the matrix's largest (exponent field Emax - 40; Emax = 122 here)
V0, VN0, VSUB, VLOW = 0x0000, 0x8000, 0x0003, ((122 - 40) << 7) | 0x55


def plant_gate_only(name, bits):
    if name == GATE:
        r = clean_rows(bits, 2)
        bits[r[0], 5] = V0; bits[r[1], 2047] = VLOW
        bits[4096 + 77, [8, 1000, 1003]] = [VN0, VSUB, VLOW]       # (a row of the second half of the gate rows; with its own escapes, if it has any)


def plant_up_only(name, bits):
    if name == UP:
        r = clean_rows(bits, 2)
        bits[r[0], 0] = VSUB; bits[r[1], [511, 512, 1536, 2040]] = [V0, VN0, VLOW, VSUB]      # a full record, one entry per j


def plant_both_rows_same_chunk(name, bits):
    """unit u multiplies gate row u and up row u: the same chunk of both, at the same and at different elements"""
    if name in (GATE, UP):
        # rows clean in BOTH tensors are wanted: the two tensors are hashed independently, so take rows far down and check them
        for u, ks in ((4000, ([803], [803])), (4001, ([16, 17], [23])), (8191, ([2047], [2040]))):
            k = ks[0] if name == GATE else ks[1]
            bits[u, k] = VLOW if name == GATE else V0


def plant_down_kpart_edges(name, bits):
    """down runs KS = 4: K-part p holds chunks 256 p .. 256 p + 255, i.e. k in [2048 p, 2048 p + 2047]"""
    if name == DOWN:
        r = clean_rows(bits, 4)
        for p, row in enumerate(r):
            bits[row, [2048 * p, 2048 * p + 7, 2048 * p + 2040, 2048 * p + 2047]] = [V0, VLOW, VSUB, VN0]     # chunk 0 and the last chunk of K-part p


def plant_bf16_pairs(name, bits):
    """both weights of one bf16 pair (k = 2m, 2m + 1), in every class"""
    if name in (GATE, UP, DOWN, HEAD):
        r = clean_rows(bits, 1)[0]
        K = bits.shape[1]
        bits[r, [6, 7, K - 2, K - 1]] = [VLOW, V0, VN0, VSUB]


@pytest.mark.parametrize("plant", [plant_gate_only, plant_up_only, plant_both_rows_same_chunk, plant_down_kpart_edges, plant_bf16_pairs],
                         ids=lambda f: f.__name__[6:])
def test_planted_escapes_are_exact(plant, hip, checkpoint):
    by_name = dict(checkpoint)
    if plant is plant_both_rows_same_chunk:      # the planted rows must stay within the record together with what they already hold
        for u, n in ((4000, 1), (4001, 2), (8191, 1)):
            assert out_of_window(by_name[GATE][u:u + 1]).sum() + n <= 4 and out_of_window(by_name[UP][u:u + 1]).sum() + 1 <= 4
    assert out_of_window(by_name[GATE][4096 + 77:4096 + 78]).sum() + 3 <= 4
    check(hip, checkpoint, plant)


def into_window(bits):
    """every out-of-window weight of the tensor replaced by an in-window value of the same sign (exponent field Emax - 14, mantissa kept)"""
    esc = out_of_window(bits)
    e = (bits >> 7) & 0xFF
    emax = int(e[e < 255].max())
    bits[esc] = (bits[esc] & 0x807F) | ((emax - 14) << 7)


def plant_no_escape(name, bits):
    into_window(bits)


def plant_one_escape(name, bits):
    into_window(bits)
    if name != UP:       # one escape in one row of each launch matrix (gate and up are one matrix: the gate row holds it)
        bits[bits.shape[0] // 2 + 1, bits.shape[1] // 2 + 3] = V0


def test_repair_branch_never_taken(hip, checkpoint):
    check(hip, checkpoint, plant_no_escape, max_row_esc=0)


def test_repair_branch_taken_for_one_row(hip, checkpoint):
    check(hip, checkpoint, plant_one_escape, max_row_esc=1)
