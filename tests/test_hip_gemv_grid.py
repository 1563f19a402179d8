"""The grid of the batch-1 GEMV launches (csrc/gemv_grid.h; options <class>.bpc for the plain and <class>.packed_bpc for the exponent-packed kernels) does not
change a bit of the result: the one-layer descriptor of tests/test_hip_packed_hl.py (hidden 2048, intermediate 8192) with a vocabulary of 9001 — the lm_head has
4501 units, the last one without a second row — at 1..4 workgroups per CU.  On 256 CUs gate_up (2048 workgroups' worth of units) then takes 2-8 rounds, down
(1024) 1-4 with a ragged last round at 3 per CU, the lm_head (1126) 2-5 with a last workgroup whose slots run out of units.  The reference is the plain
kernels at the default grid (weights.packed = 0); ids and unrounded fp32 logits are compared bit for bit, graph on and off.  (CPU audit of the arithmetic:
tests/test_gemv_grid.py.)"""
import copy

import numpy as np
import pytest

from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import GREEDY

pytestmark = pytest.mark.gpu
SEED, STD, STEPS, PROMPT, VOCAB = 7, 0.02, 3, 24, 9001


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def desc():
    d = copy.deepcopy(known_desc("llama-3.2-1b", "bf16"))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 1, VOCAB, 64, 1
    assert (d.hidden, d.inter, d.tied) == (2048, 8192, True)
    return d


@pytest.fixture(scope="module")
def checkpoint():
    return [(name, np.array(bits, copy=True)) for name, bits in synth.synth_checkpoint(desc(), SEED, STD)]


def build(hip, checkpoint, packed, pre=()):
    from tinygpt_amd.ffi import Model
    m = Model(desc(), hip)
    m.set_option("weights.packed", packed)
    m.set_option("weights.packed_classes", 7)
    for k, v in pre:
        m.set_option(k, v)
    for name, bits in checkpoint:
        m.upload(name, bits)
    m.finalize()
    assert m.get_option("weights.packed_matrices") == (3 if packed else 0) and m.get_option("weights.packed_fallbacks") == 0
    return m


def run(m, graph):
    m.set_option("graph", graph)
    m.reset_cache()
    m.forward(synth.synth_prompt(VOCAB, PROMPT, SEED)[None, :])
    ids, logits = [m.sample(GREEDY).copy()], [m.logits(rounded=False).copy()]
    for _ in range(STEPS):
        ids.append(m.decode(1, GREEDY)[0].copy())
        logits.append(m.logits(rounded=False).copy())
    return np.stack(ids), np.stack(logits)


@pytest.fixture(scope="module")
def reference(hip, checkpoint):
    """the plain kernels at the default grid, computed once: (ids, logits) per graph setting"""
    m = build(hip, checkpoint, 0)
    ref = {graph: run(m, graph) for graph in (1, 0)}
    m.close()
    assert np.isfinite(ref[0][1]).all()
    for a, b in zip(ref[0], ref[1]):
        a.setflags(write=False); b.setflags(write=False)
    return ref


def assert_equal(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("wpc", [1, 2, 3, 4])
def test_packed_launches_at_every_grid(wpc, hip, checkpoint, reference):
    m = build(hip, checkpoint, 1, pre=[("lmhead.packed_bpc", wpc)])      # (sizes the argmax partials: before finalize)
    m.set_option("gateup.packed_bpc", wpc); m.set_option("down.packed_bpc", wpc)
    for graph in (1, 0):
        assert_equal(run(m, graph), reference[graph])
    m.close()


@pytest.mark.parametrize("wpc", [1, 3])
def test_plain_launches_at_other_grids(wpc, hip, checkpoint, reference):
    m = build(hip, checkpoint, 0, pre=[("lmhead.bpc", wpc)])
    for cls in ("qkv", "oproj", "gateup", "down"):
        m.set_option(cls + ".bpc", wpc)
    for graph in (1, 0):
        assert_equal(run(m, graph), reference[graph])
    m.close()
