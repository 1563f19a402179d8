"""Option weights.fp4_rows (include/tgx.h; kernels/skinny_fp4.h): skinny products of 3-64 activation rows over a matrix quantized by weights.fp4 stream its E2M1
codes and E8M0 block scales on the matrix cores instead of the dequantized bf16 master.

The kernel is pinned to the panel / ring kernels' accumulation order and every dequantized weight is exactly a bf16, so nothing has a tolerance: context A
(weights.fp4 1, weights.fp4_rows 64, uploaded W) equals B (option off, uploaded fp4_ref.dequantized(W), skinny.ksplit 0) BIT FOR BIT, ids and fp32 logits as
uint32, with graph 1 and graph 0.  Geometry, plants and helpers: test_hip_fp8.py, test_hip_fp4.py, test_hip_fp8_rows.py."""
import copy

import numpy as np
import pytest

import fp4_ref as R
import fp8_ref as R8
import test_hip_fp4 as F4
import test_hip_fp8 as F
import test_hip_fp8_rows as T8
from conftest import load_golden
from tinygpt_amd import synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model, TgxError

pytestmark = pytest.mark.gpu
hip, checkpoint = F4.hip, F4.checkpoint
PRODUCTS, FALLBACKS = "weights.fp4_row_products", "weights.fp4_row_fallbacks"


def pair(hip, checkpoint, max_batch, plant=None, vocab=None, opts=(), head=None):
    """A: weights.fp4 (+ opts), weights.fp4_rows 64.  B: an ordinary context on the dequantized tensors with skinny.ksplit 0"""
    if vocab:
        d = F.desc(max_batch)
        d.vocab = vocab
        a, b = Model(d, hip).set_option("weights.fp4", 1), Model(copy.deepcopy(d), hip)
        for name, bits in checkpoint[0]:
            w = bits[:vocab] if name == F.HEAD else bits
            a.upload(name, w); b.upload(name, R.dequantized(w) if name in F.MLP else w)
        a.finalize(); b.finalize()
    else:
        a, b = F4.pair(hip, checkpoint, plant, max_batch, F4.FP4 + opts, head)
    a.set_option("weights.fp4_rows", 64); b.set_option("skinny.ksplit", 0)
    return a, b


def check_rows(a, b, rows, vocab=1024):
    for graph in (1, 0):
        T8.bits_equal(T8.run_rows(a, rows, graph, vocab), T8.run_rows(b, rows, graph, vocab))
    assert a.get_option(PRODUCTS) > 0 and b.get_option(PRODUCTS) == 0
    a.close(); b.close()


@pytest.mark.parametrize("rows", [3, 16, 17, 33, 64])
def test_batched_steps_are_bit_identical(rows, hip, checkpoint):
    """gate_up and lm_head at K = 2048 (one whole quad per k-part); down at K = 8192 in split ranges of 1024 k, which begin and end inside a quad"""
    check_rows(*pair(hip, checkpoint, rows), rows)


PLANTS = [F4.plant_all_codes, F4.plant_block_scales_apart, F4.plant_zero_blocks_and_rows, F4.plant_clamped_block, F.plant_down_kpart_edges, F.plant_last_rows,
          T8.plant_run_edges]


@pytest.mark.parametrize("plant", PLANTS, ids=lambda f: f.__name__[6:])
def test_planted_weights_are_exact(plant, hip, checkpoint):
    """all_codes (every code at every element, neighbouring blocks at different scales) decides whether v_cvt_scalef32_pk_bf16_fp4 is exact"""
    check_rows(*pair(hip, checkpoint, 5, plant), 5)


def test_vocabulary_that_is_no_multiple_of_64(hip, checkpoint):
    check_rows(*pair(hip, checkpoint, 5, vocab=129), 5, vocab=129)      # 128 is the least the matrix-core step admits


@pytest.mark.parametrize("inter,streams", [(10240, True), (12288, True), (14336, True), (28672, False)])
def test_short_quads_and_fallbacks(inter, streams, hip):
    """down at NX = 5, 6, 7 (a whole quad and a short one of 1, 2, 3 slots) streams; at 28672 it is two ranges and falls back.  K = 192 .. 640: gate_up and
    lm_head fall back.  The model is the quantized one throughout"""
    cfg, g = load_golden("llama_tiny")
    d = desc_from_hf_config(dict(cfg, intermediate_size=inter), "bf16")
    d.max_batch = 5
    a, b = Model(d, hip).set_option("weights.fp4", 1), Model(copy.deepcopy(d), hip)
    for name, bits in synth.synth_checkpoint(d, int(g["seed"]), float(g["std"])):
        a.upload(name, bits)
        b.upload(name, R.dequantized(bits) if F.is_quantized(name, 7, d.tied) and bits.ndim == 2 else bits)
    a.finalize(); b.finalize()
    a.set_option("weights.fp4_rows", 64); b.set_option("skinny.ksplit", 0)
    for graph in (1, 0):
        T8.bits_equal(T8.run_rows(a, 5, graph, d.vocab), T8.run_rows(b, 5, graph, d.vocab))
    n0 = a.get_option(PRODUCTS), a.get_option(FALLBACKS)
    a.decode_rows(1)                                   # eager: one step issues gate_up and down of every layer and the lm_head
    n1 = a.get_option(PRODUCTS), a.get_option(FALLBACKS)
    assert n1[0] - n0[0] + n1[1] - n0[1] == 2 * d.layers + 1
    assert n1[0] - n0[0] == (d.layers if streams else 0)


def verify_and_extend(m):
    m.forward_rows([0], [synth.synth_prompt(1024, 12, 5)])
    vids, _ = m.verify_row(0, [m.sample_row(0, GREEDY), 5, 6])
    got = [vids.copy(), m.pass_logits().copy(), m.logits(rounded=False).copy()]
    m.extend_row(0, synth.synth_prompt(1024, 9, 6))
    return got + [m.logits(rounded=False).copy()]


def test_verify_and_extend_passes(hip, checkpoint):
    a, b = pair(hip, checkpoint, 2)
    T8.bits_equal(verify_and_extend(a), verify_and_extend(b))
    assert a.get_option(PRODUCTS) > 0 and b.get_option(PRODUCTS) == 0


def test_fp4_mlp_under_an_fp8_head_each_on_its_own_stream(hip, checkpoint):
    a, b = pair(hip, checkpoint, 5, opts=(("weights.fp4_classes", 3), ("weights.fp8", 1), ("weights.fp8_classes", 4)), head=R8.dequantized)
    a.set_option("weights.fp8_rows", 64)
    for graph in (1, 0):
        T8.bits_equal(T8.run_rows(a, 5, graph), T8.run_rows(b, 5, graph))
    assert a.get_option(PRODUCTS) > 0 and a.get_option("weights.fp8_row_products") > 0
    assert b.get_option(PRODUCTS) == 0 and b.get_option("weights.fp8_row_products") == 0


def test_the_row_limit_and_its_values(hip, checkpoint):
    a, _ = pair(hip, checkpoint, 17)
    a.set_option("weights.fp4_rows", 8)
    n = [a.get_option(PRODUCTS)]
    for rows in (5, 17):
        T8.run_rows(a, rows, 0, steps=1)
        n.append(a.get_option(PRODUCTS))
    assert n[1] > n[0] and n[2] == n[1]
    for bad in (1, 2, 65):
        with pytest.raises(TgxError) as e:
            a.set_option("weights.fp4_rows", bad)
        assert e.value.status == 1      # TGX_ERR_INVALID
    assert a.get_option("weights.fp4_rows") == 8
