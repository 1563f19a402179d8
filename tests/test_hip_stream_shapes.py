"""The FP8 and MXFP4 weight streams over their layout space (tests/stream_shapes.py): NX 1..8, ks 1 / 2 / 4 through the <class>.ks options, short and whole quads,
padded k-parts, split ranges that are whole runs or begin inside one, 3..64 rows in one, two and four activation blocks, two layers, a batch above 64 rows.

The method is the existing modules': context A (the form on, the case's <class>.ks options before finalize, weights.fp8_rows / weights.fp4_rows 64, uploaded W)
equals context B (form off, uploaded <form>_ref.dequantized(W), skinny.ksplit 0, everything else equal) BIT FOR BIT — ids and unrounded fp32 logits as uint32 —
with graph 1 and 0, on a batch-1 run, a 2-row step, and forward_rows + decode_rows at the case's row counts.  What keeps that from passing on fall-backs: the
counters after finalize and their deltas over one eager step must equal stream_shapes.predict_*, and tests/test_stream_shapes.py holds the predictions to the
reach list.  The row counters count per context, not per class: the pair (products, fallbacks) is compared with the sum over the predicted classes.

Three cases per form also run against the CPU oracle on the dequantized tensors at tests/test_hip_fuzz.py's bound for 16-bit storage (6e-3 at weight std 0.05).

Two cases set an option the issue's list does not name, on both contexts: prefill.splitk 0 (launch_skinny leaves a 512-row down unsplit only then: the stream
kernels' GEMM_RESIDUAL epilogue) and decode.step_rows 64 (by default a batch of 67 rows is ONE eight-block pass that no stream serves).

Measured on the MI355X (profiles/stream_shapes.txt): the whole module 3.51 s, its slowest case (fp8-h512) 0.35 s, tests/test_hip_fp4_rows.py in the same
session 2.11 s."""
import copy
import dataclasses
import functools

import numpy as np
import pytest

import fp4_ref as R4
import fp8_ref as R8
import stream_shapes as S
import test_hip_fp4 as F4
import test_hip_fp8 as F
import test_hip_fp8_rows as T8
from conftest import rel_err
from tinygpt_amd import synth
from tinygpt_amd.ffi import GREEDY, Model

pytestmark = pytest.mark.gpu
hip = F.hip
REF = {"fp8": R8, "fp4": R4}
GPU_CASES = [(form, c) for c in S.SHAPES for form in S.FORMS]      # shape-major: both forms of a shape share its tensors
PROMPT, STEPS = 24, 3


def head_name(case):
    return "model.embed_tokens.weight" if case.tied else "lm_head.weight"


def is_quantized(name, bits, case):
    return bits.ndim == 2 and F.is_quantized(name, 7, case.tied)


@functools.lru_cache(maxsize=2)
def tensors(case):
    return [(name, np.array(bits, copy=True)) for name, bits in synth.synth_checkpoint(case.desc(), S.SEED, S.STD)]


@functools.lru_cache(maxsize=4)
def dequantized(case, form):
    return {name: REF[form].dequantized(bits) for name, bits in tensors(case) if is_quantized(name, bits, case)}


def shape_of(case):
    """the fields that decide the tensors (cases that differ in options alone share them)"""
    return dataclasses.replace(case, name="", ks=(None, None, None), rows=(1,), plant=False, oracle=False, passes=False, opts=())


# ---- plants: the existing modules', at the case's K and K split -----------------------------------------------------------------------------------------
def plant(form, case, name, bits):
    """layer 0's gate / up / down and the head: every code at every element of every slot (test_hip_fp8.all_codes_rows / test_hip_fp4.all_codes_row) and
    neighbouring scales far apart (test_hip_fp8_rows.plant_scales_apart_in_a_fragment / test_hip_fp4.plant_block_scales_apart)"""
    cls = {F.GATE: "gateup", F.UP: "gateup", F.DOWN: "down", head_name(case): "lmhead"}.get(name)
    if cls is None:
        return
    K = bits.shape[1]
    e = {F.GATE: -12, F.UP: -15, F.DOWN: -13}.get(name, -11)
    if form == "fp8":
        lay = S.layout(form, cls, case)
        nchunk, nx, nh, per = R8.geometry(K, lay.ks)
        assert (nx, per) == (lay.nx, 64 * lay.nx)
        least = min(sum(1 for c in range(nchunk) if ((c % per) // 64) // 2 == h) for h in range(nh))      # chunks of a row in its emptiest plane
        F.all_codes_rows(bits, range(64, 64 + -(-254 // least)), lay.ks, e)
        T8.plant_scales_apart_in_a_fragment(name, bits)
    else:
        bits[64] = F4.all_codes_row(K, e); bits[65] = F4.all_codes_row(K, e + 3)
        F4.plant_block_scales_apart(name, bits)


def pair(hip, form, case, max_batch, twin=Model):
    """A and B of the module docstring (twin: Model, or the oracle's class)"""
    d = case.desc(max_batch)
    a, b = Model(d, hip), (Model(copy.deepcopy(d), hip) if twin is Model else twin(d))
    a.set_option(f"weights.{form}", 1)
    for m in (a, b) if twin is Model else (a,):
        for cls, ks in zip(S.CLASSES, case.ks):
            if ks:
                m.set_option(f"{cls}.ks", ks)
    base = shape_of(case)
    DQ = dequantized(base, form)
    for name, bits in tensors(base):
        wa = wb = bits
        if name in DQ:
            wb = DQ[name]
            if case.plant:
                wa = bits.copy()
                plant(form, case, name, wa)
                rows = np.nonzero((wa != bits).any(axis=1))[0]      # only the edited rows are worked out again
                wb = wb.copy()
                wb[rows] = REF[form].dequantized(wa[rows])
        a.upload(name, wa); b.upload(name, wb)
    a.finalize(); b.finalize()
    a.set_option(f"weights.{form}_rows", 64)
    if twin is Model:
        b.set_option("skinny.ksplit", 0)
        for m in (a, b):
            for key, value in case.opts:
                m.set_option(key, value)
    return a, b


def counters(m, form):
    return m.get_option(f"weights.{form}_row_products"), m.get_option(f"weights.{form}_row_fallbacks")


def run1(m, case, batch, graph, steps=STEPS):
    """a prompt of `batch` equal-length rows and greedy steps through tgx_forward / tgx_decode: batch 1 streams on the GEMV kernels, batch 2 must not stream"""
    m.set_option("graph", graph)
    m.reset_cache()
    m.forward(np.stack([synth.synth_prompt(case.vocab, PROMPT, S.SEED + r) for r in range(batch)]))
    ids, logits = [m.sample(GREEDY).copy()], [m.logits(rounded=False).copy()]
    for _ in range(steps):
        ids.append(m.decode(1, GREEDY)[0].copy())
        logits.append(m.logits(rounded=False).copy())
    return [np.stack(ids), np.stack(logits)]


def passes(m, case):
    """a verify pass of 3 positions and an extend pass of 16"""
    m.set_option("graph", 0)
    m.reset_cache()
    m.forward_rows([0], [synth.synth_prompt(case.vocab, 12, 5)])
    vids, _ = m.verify_row(0, [m.sample_row(0, GREEDY), 5, 6])
    got = [vids.copy(), m.pass_logits().copy(), m.logits(rounded=False)[:1].copy()]      # (row 0: the other rows' slots hold earlier runs' logits)
    m.extend_row(0, synth.synth_prompt(case.vocab, 16, 6))
    return got + [m.logits(rounded=False)[:1].copy()]


@pytest.mark.parametrize("form,case", GPU_CASES, ids=[S.case_id(fc) for fc in GPU_CASES])
def test_streams_are_bit_identical_and_counted(form, case, hip):
    a, b = pair(hip, form, case, max(2, max(case.rows)))
    told = "\n".join(S.step_table(form, case))
    # finalize: which matrices own a stream
    assert (a.get_option(f"weights.{form}_matrices"), a.get_option(f"weights.{form}_fallbacks")) == S.predict_finalize(form, case), told
    assert (b.get_option(f"weights.{form}_matrices"), b.get_option(f"weights.{form}_fallbacks")) == (0, 0)
    # batch 1: the GEMV stream kernels (and the prompt pass of 24 rows on the rows kernels).  One eager step moves no row counter
    for graph in (1, 0):
        T8.bits_equal(run1(a, case, 1, graph), run1(b, case, 1, graph))
    n0 = counters(a, form)
    a.decode(1, GREEDY)
    assert counters(a, form) == n0
    # two rows: launch_gemv's R = 2 form on the master — equal to B, and no row product either
    for graph in (1, 0):
        T8.bits_equal(run1(a, case, 2, graph, steps=1), run1(b, case, 2, graph, steps=1))
    n0 = counters(a, form)
    a.decode(1, GREEDY)
    assert counters(a, form) == n0
    # the rows kernels
    for rows in case.rows:
        for graph in (1, 0):
            T8.bits_equal(T8.run_rows(a, rows, graph, case.vocab, steps=2), T8.run_rows(b, rows, graph, case.vocab, steps=2))
        prods, want = S.predict_step(form, case, rows)
        n0 = counters(a, form)
        a.decode_rows(1)                                   # eager (graph 0 ran last): every product of one step is issued once
        n1 = counters(a, form)
        got = (n1[0] - n0[0], n1[1] - n0[1])
        assert got == want, f"rows {rows}: observed (products, fallbacks) {got}, predicted {want}\n" + "\n".join(p.geometry() for p in prods)
    if case.passes:
        n0 = counters(a, form)
        T8.bits_equal(passes(a, case), passes(b, case))
        assert counters(a, form)[0] > n0[0]
    assert counters(b, form) == (0, 0)
    a.close(); b.close()


# ---- against the CPU oracle -----------------------------------------------------------------------------------------------------------------------------
ORACLE_CASES = [(form, c, B) for c in S.SHAPES if c.oracle for form in S.FORMS for B in (1, 5)]


@pytest.mark.parametrize("form,case,B", ORACLE_CASES, ids=[f"{f}-{c.name}-b{B}" for f, c, B in ORACLE_CASES])
def test_quantized_context_against_the_oracle(form, case, B, hip, oracle_lib):
    """The differential above compares two kernels of this project; here A's logits, prompt + 3 teacher-forced steps, meet the CPU oracle uploaded the same
    dequantized tensors.  Bound: tests/test_hip_fuzz.py's for 16-bit storage at weight std 0.05 (the K / V rounding-flip floor of such models), no tighter"""
    from oracle.oracle_ffi import OracleModel
    gpu, ref = pair(hip, form, dataclasses.replace(case, plant=False), B, twin=OracleModel)
    prompt = np.stack([synth.synth_prompt(case.vocab, 7, 300 + b) for b in range(B)])
    gpu.forward(prompt); ref.forward(prompt)
    lg, lr = gpu.logits(rounded=False), ref.logits(rounded=False)
    print("prompt", rel_err(lg, lr))
    assert rel_err(lg, lr) < 6e-3
    tok = ref.sample(GREEDY); gpu.sample(GREEDY)
    for step in range(3):
        onehot = np.full((B, case.vocab), -1.0, np.float32); onehot[np.arange(B), tok] = 1.0
        gpu.set_logits(onehot); np.testing.assert_array_equal(gpu.sample(GREEDY), tok)      # the oracle's token, then the captured step
        gpu.decode(1, GREEDY)
        tr = ref.decode(1, GREEDY)[0]
        lg, lr = gpu.logits(rounded=False), ref.logits(rounded=False)
        print("step", step, rel_err(lg, lr))
        assert rel_err(lg, lr) < 6e-3, (step, rel_err(lg, lr))
        tok = tr
    assert counters(gpu, form)[0] > 0                      # (the prompt pass of 7 B rows, and the steps of five rows, ran on the rows kernels)
    gpu.close(); ref.close()
