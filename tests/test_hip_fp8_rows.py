"""Option weights.fp8_rows (include/tgx.h; kernels/skinny_fp8.h): skinny products of 3-64 activation rows over a matrix quantized by weights.fp8 stream its E4M3
codes on the matrix cores instead of the dequantized bf16 master.

The kernel is pinned to the panel / ring kernels' accumulation order and every dequantized weight is exactly a bf16, so nothing has a tolerance: context A
(weights.fp8 1, weights.fp8_rows 64, uploaded W) equals B (uploaded fp8_ref.dequantized(W), skinny.ksplit 0) BIT FOR BIT.  Geometry and plants: test_hip_fp8.py."""
import copy

import numpy as np
import pytest

import fp8_ref as R
import test_hip_fp8 as F
from conftest import load_golden
from tinygpt_amd import synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model, TgxError

pytestmark = pytest.mark.gpu
hip, checkpoint = F.hip, F.checkpoint


def bits_equal(xs, ys):
    for x, y in zip(xs, ys):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
        assert x.dtype != np.float32 or np.isfinite(x).all()


def pair(hip, checkpoint, max_batch, plant=None, vocab=None):
    W, DQ = checkpoint
    d = F.desc(max_batch)
    d.vocab = vocab or d.vocab
    a, b = Model(d, hip).set_option("weights.fp8", 1), Model(copy.deepcopy(d), hip)
    for name, bits in W:
        wa = wb = bits[:vocab] if vocab and name == F.HEAD else bits
        if name in F.MLP:
            if plant:
                wa = wa.copy()
                plant(name, wa)
            wb = R.dequantized(wa) if vocab else F.dequantized_after(wa, bits, DQ[name])
        a.upload(name, wa); b.upload(name, wb)
    a.finalize(); b.finalize()
    a.set_option("weights.fp8_rows", 64); b.set_option("skinny.ksplit", 0)
    return a, b


def run_rows(m, rows, graph, vocab=1024, steps=3):
    """forward_rows of prompts of different lengths, sample_row, then decode_rows steps: the logits after the prompts, the ids and the last step's logits"""
    m.set_option("graph", graph)
    m.reset_cache()
    m.forward_rows(range(rows), [synth.synth_prompt(vocab, 3 + (5 * i) % 11, 100 + i) for i in range(rows)])
    got = [m.logits(rounded=False).copy()]
    for r in range(rows):
        m.sample_row(r, GREEDY)
    ids, _, _ = m.decode_rows(steps)
    return got + [ids.copy(), m.logits(rounded=False).copy()]


def check_rows(a, b, rows, vocab=1024):
    for graph in (1, 0):
        bits_equal(run_rows(a, rows, graph, vocab), run_rows(b, rows, graph, vocab))
    assert a.get_option("weights.fp8_row_products") > 0 and b.get_option("weights.fp8_row_products") == 0
    a.close(); b.close()


@pytest.mark.parametrize("rows", [3, 16, 17, 33, 64])
def test_batched_steps_are_bit_identical(rows, hip, checkpoint):
    a, b = pair(hip, checkpoint, rows)
    check_rows(a, b, rows)


def plant_scales_apart_in_a_fragment(name, bits):
    """rows 32..47 (one 16-row fragment of down and the head; gate rows 16..23 with their up partners in the merged matrix): neighbours' scales 2^10 apart"""
    for r in range(32, 48):
        d = 5 if (r + (name == F.UP)) & 1 else -5
        assert ((bits[r] >> 7) & 0xFF).min() > 8
        bits[r] = (bits[r].astype(np.int32) + (d << 7)).astype(np.uint16)


def plant_run_edges(name, bits):
    """loud values in the first and last chunk of every 512-k run (the K-split ranges of down, 1024 k, begin and end on such edges), rows of two fragments"""
    loud = F.f2b([0.109375, -0.09375, 0.078125, -0.0625, 0.0546875, -0.046875, 0.0390625, -0.03125])
    for r in (50, 51, 77):
        for k in range(0, bits.shape[1], 512):
            bits[r, k:k + 8] = loud
            bits[r, k + 504:k + 512] = loud[::-1]


PLANTS = [F.plant_all_codes, F.plant_gate_up_scales_apart, plant_scales_apart_in_a_fragment, F.plant_all_zero_row, F.plant_negative_zero,
          F.plant_large_and_subnormal_codes, plant_run_edges, F.plant_last_rows]


@pytest.mark.parametrize("plant", PLANTS, ids=lambda f: f.__name__[6:])
def test_planted_weights_are_exact(plant, hip, checkpoint):
    a, b = pair(hip, checkpoint, 5, plant)
    check_rows(a, b, 5)


def test_vocabulary_that_is_no_multiple_of_64(hip, checkpoint):
    a, b = pair(hip, checkpoint, 5, vocab=129)      # 128 is the least the matrix-core step admits
    check_rows(a, b, 5, vocab=129)


@pytest.mark.parametrize("fam", ["llama_tiny", "qwen2_tiny", "mistral_tiny", "qwen3_tiny"])
def test_tiny_families_are_bit_identical(fam, hip):
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(cfg, "bf16")
    d.max_batch = 5
    a, b = Model(d, hip).set_option("weights.fp8", 1), Model(copy.deepcopy(d), hip)
    for name, bits in synth.synth_checkpoint(d, int(g["seed"]), float(g["std"])):
        a.upload(name, bits)
        b.upload(name, R.dequantized(bits) if F.is_quantized(name, 7, d.tied) and bits.ndim == 2 else bits)
    a.finalize(); b.finalize()
    a.set_option("weights.fp8_rows", 64); b.set_option("skinny.ksplit", 0)
    for graph in (1, 0):
        bits_equal(run_rows(a, 5, graph, d.vocab), run_rows(b, 5, graph, d.vocab))
    count = lambda: a.get_option("weights.fp8_row_products") + a.get_option("weights.fp8_row_fallbacks")
    n0 = count()
    a.decode_rows(1)                                   # eager: one step issues gate_up and down of every layer and the lm_head
    assert count() - n0 == 2 * d.layers + 1


def test_verify_and_extend_passes(hip, checkpoint):
    a, b = pair(hip, checkpoint, 2)
    out = []
    for m in (a, b):
        m.forward_rows([0], [synth.synth_prompt(1024, 12, 5)])
        vids, _ = m.verify_row(0, [m.sample_row(0, GREEDY), 5, 6])
        got = [vids.copy(), m.pass_logits().copy(), m.logits(rounded=False).copy()]
        m.extend_row(0, synth.synth_prompt(1024, 9, 6))
        out.append(got + [m.logits(rounded=False).copy()])
    bits_equal(*out)
    assert a.get_option("weights.fp8_row_products") > 0 and b.get_option("weights.fp8_row_products") == 0


def test_the_row_limit_and_its_values(hip, checkpoint):
    a, b = pair(hip, checkpoint, 17)
    a.set_option("weights.fp8_rows", 8)
    n = [a.get_option("weights.fp8_row_products")]
    for rows in (5, 17):
        run_rows(a, rows, 0, steps=1)
        n.append(a.get_option("weights.fp8_row_products"))
    assert n[1] > n[0] and n[2] == n[1]
    for bad in (1, 2, 65):
        with pytest.raises(TgxError) as e:
            a.set_option("weights.fp8_rows", bad)
        assert e.value.status == 1      # TGX_ERR_INVALID
    assert a.get_option("weights.fp8_rows") == 8
