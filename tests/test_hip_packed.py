"""Exponent-packed weights (option weights.packed, kernels/gemv_packed.h): the batch-1 gate_up / down / lm_head launches over the lossless 12-bit form must
compute what the plain kernels compute BIT FOR BIT — same weights, same per-lane order of multiply-adds, same reductions — for ordinary weights, for escapes
carried in the rows' records, and for a matrix that falls back to the plain kernel; and the packed context is held to the oracle like the plain one (1e-3)."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
from tinygpt_amd import synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY

pytestmark = pytest.mark.gpu
FAMILIES = ["llama_tiny", "qwen2_tiny"]
STEPS = 8


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def build(fam, hip, packed, plant=None):
    """a context of the family's synthetic checkpoint; plant(name, bits) may edit a tensor's bf16 patterns before upload"""
    from tinygpt_amd.ffi import Model
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(cfg, "bf16")
    m = Model(d, hip)
    m.set_option("weights.packed", packed)
    m.set_option("weights.packed_classes", 7)        # all three packed forms, whichever classes are adopted by default
    for name, bits in synth.synth_checkpoint(d, int(g["seed"]), float(g["std"])):
        bits = np.array(bits, copy=True)
        if plant:
            plant(name, bits)
        m.upload(name, bits)
    m.finalize()
    assert m.get_option("weights.packed") == packed
    if not packed:
        assert m.get_option("weights.packed_matrices") == 0
    return m, d, g


def run(m, g, graph):
    """prompt + STEPS greedy decode steps through tgx_decode: the ids and the unrounded fp32 logits of every step"""
    m.set_option("graph", graph)
    m.reset_cache()
    m.forward(g["prompt"])
    ids, logits = [m.sample(GREEDY).copy()], [m.logits(rounded=False).copy()]
    for _ in range(STEPS):
        ids.append(m.decode(1, GREEDY)[0].copy())
        logits.append(m.logits(rounded=False).copy())
    return np.stack(ids), np.stack(logits)


def assert_bit_identical(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))      # bit for bit (-0 / +0 and NaN payloads included)


def matrices(d):
    return 2 * d.layers + 1      # gate_up and down of every layer, the lm_head


@pytest.mark.parametrize("graph", [1, 0])
@pytest.mark.parametrize("fam", FAMILIES)
def test_packed_equals_plain_bit_for_bit(fam, graph, hip):
    plain, d, g = build(fam, hip, 0)
    packed, _, _ = build(fam, hip, 1)
    assert packed.get_option("weights.packed_matrices") == matrices(d) and packed.get_option("weights.packed_fallbacks") == 0
    assert_bit_identical(run(packed, g, graph), run(plain, g, graph))
    # (the tiny rows pad every lane's single chunk to a quad of planes, so the packed step streams MORE here; 12 bits per weight needs K % 2048 == 0)
    assert packed.bytes_per_token(16) != plain.bytes_per_token(16)


def emax(bits):
    e = (bits >> 7) & 0xFF
    return int(e[e < 255].max())


TARGETS = {"gate": "model.layers.0.mlp.gate_proj.weight", "down": "model.layers.1.mlp.down_proj.weight", "lm_head": "model.embed_tokens.weight"}     # (tied head)
# planted value -> bf16 pattern, given the tensor's largest exponent field
VALUES = {
    "+0": lambda em: 0x0000,
    "-0": lambda em: 0x8000,
    "subnormal": lambda em: 0x0003,
    "2^-40 below": lambda em: ((em - 40) << 7) | 0x55,
    "2^10 above": lambda em: 0x8000 | ((em + 10) << 7) | 0x2A,      # moves the window: the ordinary weights below it become the escapes
}


@pytest.mark.parametrize("count", [1, 4])
@pytest.mark.parametrize("value", list(VALUES))
def test_escapes_are_exact(value, count, hip):
    """the planted values in one row each of a gate, a down and the lm_head matrix: one per row, then four (the record's capacity), spread over the row's chunks
    and both halves of a bf16 pair.  '2^10 above' leaves ordinary weights below the moved window: rows of such a matrix may exceed the record and the matrix
    then runs plain — the result must be exact either way; every other value must be served from the records (no fallback)."""
    def plant(name, bits):
        for tgt in TARGETS.values():
            if name == tgt:
                row, K = 3, bits.shape[1]
                v = VALUES[value](emax(bits))
                for k in [K - 1, 0, K // 2 + 1, 10][:count]:
                    bits[row, k] = v
    plain, d, g = build("llama_tiny", hip, 0, plant)
    packed, _, _ = build("llama_tiny", hip, 1, plant)
    print(value, count, "packed", packed.get_option("weights.packed_matrices"), "fallbacks", packed.get_option("weights.packed_fallbacks"),
          "max escapes in a row", packed.get_option("weights.packed_max_row_esc"))
    if value != "2^10 above":
        assert packed.get_option("weights.packed_fallbacks") == 0 and packed.get_option("weights.packed_max_row_esc") >= count
    for graph in (1, 0):
        assert_bit_identical(run(packed, g, graph), run(plain, g, graph))


def test_a_row_beyond_the_record_sends_its_matrix_to_the_plain_kernel(hip):
    def plant(name, bits):
        if name == "model.layers.0.mlp.down_proj.weight":
            bits[5, [0, 9, 100, 257, bits.shape[1] - 1]] = 0x0000      # capacity + 1 out-of-window values in one row
    plain, d, g = build("llama_tiny", hip, 0, plant)
    packed, _, _ = build("llama_tiny", hip, 1, plant)
    assert packed.get_option("weights.packed_fallbacks") == 1
    assert packed.get_option("weights.packed_matrices") == matrices(d) - 1
    assert packed.get_option("weights.packed_max_row_esc") == 5
    for graph in (1, 0):
        assert_bit_identical(run(packed, g, graph), run(plain, g, graph))


@pytest.mark.parametrize("fam", FAMILIES)
def test_packed_context_against_the_oracle(fam, hip, oracle_lib):
    """the tiny-family parity comparison of tests/test_hip_parity.py on a context that runs the packed kernels, at the same bound"""
    from oracle.oracle_ffi import OracleModel
    gpu, d, g = build(fam, hip, 1)
    assert gpu.get_option("weights.packed_matrices") == matrices(d)
    ref = OracleModel(d).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    gpu.forward(g["prompt"]); ref.forward(g["prompt"])
    assert rel_err(gpu.logits(rounded=False), ref.logits(rounded=False)) < 1e-3
    np.testing.assert_array_equal(gpu.sample(GREEDY), ref.sample(GREEDY))
    n = g["ids_bf16"].shape[1] - 1
    for step in range(n):
        np.testing.assert_array_equal(gpu.decode(1, GREEDY), ref.decode(1, GREEDY))
        assert rel_err(gpu.logits(rounded=False), ref.logits(rounded=False)) < 1e-3, step
