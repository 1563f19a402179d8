"""Option weights.fp4 (include/tgx.h; kernels/gemv_fp4.h): tgx_finalize quantizes the gate_up / down / lm_head matrices to E2M1 codes with an E8M0 scale per
block of 32 k, overwrites the bf16 masters with the dequantized values, and the batch-1 launches stream the codes.

Every dq is exactly a bf16, so nothing has a tolerance: context A (weights.fp4 = 1, uploaded W) equals context B (option off, uploaded fp4_ref.dequantized(W))
BIT FOR BIT, ids and fp32 logits as uint32; the one tolerance is the CPU oracle's (tests/test_hip_parity.py's 1e-3).  Geometry and helpers: tests/test_hip_fp8.py."""
import numpy as np
import pytest

import fp4_ref as R
import fp8_ref as R8
from conftest import load_golden, rel_err
from test_hip_fp8 import (DOWN, GATE, HEAD, MLP, SEED, STD, UP, assert_bit_identical, desc, f2b, hip, is_quantized, plant_down_kpart_edges,      # noqa: F401
                          plant_last_rows, run, run_tiny)
from tinygpt_amd import synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model, TgxError

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = 1, 2, 4
FP4 = (("weights.fp4", 1),)


@pytest.fixture(scope="module")
def checkpoint():
    """the tensors once per module, and the dequantized form of the four quantized ones: every context uploads (an edited copy of) these"""
    W = [(name, np.array(bits, copy=True)) for name, bits in synth.synth_checkpoint(desc(), SEED, STD)]
    return W, {name: R.dequantized(bits) for name, bits in W if name in MLP}


def pair(hip, checkpoint, plant=None, max_batch=1, opts=FP4, head=None):
    """A: `opts` uploaded W.  B: no option, uploaded the dequantized tensors (the head's by `head` where a test quantizes it otherwise).  Else equal."""
    W, DQ = checkpoint
    a, b = Model(desc(max_batch), hip), Model(desc(max_batch), hip)
    for key, value in opts:
        a.set_option(key, value)
    for name, bits in W:
        wa = wb = bits
        if name in MLP:
            wb = DQ[name]
            if plant:
                wa = bits.copy()
                plant(name, wa)
                rows = np.nonzero((wa != bits).any(axis=1))[0]      # only the edited rows are worked out again
                wb = wb.copy()
                wb[rows] = R.dequantized(wa[rows])
            if name == HEAD and head:
                wb = head(wa)
        a.upload(name, wa); b.upload(name, wb)
    return a.finalize(), b.finalize()


def check(hip, checkpoint, plant=None, **kw):
    a, b = pair(hip, checkpoint, plant, **kw)
    for graph in (1, 0):
        assert_bit_identical(run(a, graph), run(b, graph))
    return a, b


def test_bench_row_geometry_is_bit_identical(hip, checkpoint):
    a, b = check(hip, checkpoint)
    assert (a.get_option("weights.fp4_matrices"), a.get_option("weights.fp4_fallbacks")) == (3, 0)
    assert (b.get_option("weights.fp4_matrices"), b.get_option("weights.fp4_fallbacks")) == (0, 0)
    for key in ("weights.fp4", "weights.fp4_classes"):
        with pytest.raises(TgxError) as e:
            a.set_option(key, 1)
        assert e.value.status == ERR_STATE

# ---- planted rows ----------------------------------------------------------------------------------------------------------------------------------
def all_codes_row(K, e0):
    """code (c + 3 t) mod 16 at element t of chunk c: every run of 64 chunks (one chunk slot j of the 64 lanes) shows all 16 codes at every t, every block of
    four chunks holds a +-6, which pins its exponent, and block b is at 2^(e0 - b % 5): neighbouring blocks, and the two rows of a unit, at different scales"""
    k = np.arange(K)
    return f2b(np.ldexp(R.code_value((k // 8 + 3 * (k % 8)) % 16), e0 - (k // 32) % 5))


def plant_all_codes(name, bits):
    K = bits.shape[1]
    if name == GATE: bits[40] = all_codes_row(K, -12); bits[41] = all_codes_row(K, -9)
    if name == UP: bits[40] = all_codes_row(K, -15)                   # (gate row 40's partner in unit 40)
    if name == DOWN: bits[1000] = all_codes_row(K, -13); bits[1001] = all_codes_row(K, -10)
    if name == HEAD: bits[500] = all_codes_row(K, -11); bits[501] = all_codes_row(K, -14)


def plant_block_scales_apart(name, bits):
    """every other block of a row louder by 2^20 (a power of two moves the exponent field: exact)"""
    odd = (np.arange(bits.shape[1]) // 32) % 2 == 1
    for r in (7, 8, bits.shape[0] // 2 + 7):
        bits[r, odd ^ (r % 2 == 0)] += 20 << 7


def plant_exact_ties(name, bits):
    """every midpoint of neighbouring grid values, both signs, under a 6 that pins each block's exponent"""
    mid = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5])
    row = f2b(np.ldexp(np.resize(np.concatenate([[6.0], mid, -mid]), bits.shape[1]), -14))
    bits[21] = row; bits[22] = np.roll(row, 3)


def plant_amax_at_the_exponent_switch(name, bits):
    """a block whose largest magnitude has mantissa exactly 1.5 and one with the next pattern above; the rest of both blocks 2^8 quieter than it was"""
    for r in (11, 12):
        assert ((bits[r, :64] >> 7) & 0xFF).min() > 8
        bits[r, :64] -= 8 << 7
        bits[r, 5] = 0x3BC0; bits[r, 32 + 5] = 0xBBC1                 # 1.5 * 2^-8 and -(1.5 + 2^-7) * 2^-8


def plant_zero_blocks_and_rows(name, bits):
    bits[17] = 0x0000; bits[18] = 0x8000
    bits[19, 32:64] = 0x0000; bits[19, 64:96] = 0x8000; bits[19, 100:104] = 0x8000


def plant_clamped_block(name, bits):
    """magnitudes around 2^-126 and bf16 subnormals: the block takes e = -125, its dq are 0 and 2^-126"""
    bits[25, 64:96] = np.resize(np.array([0x00C0, 0x0080, 0x8080, 0x0001, 0x807F, 0x0000, 0x8040, 0x00A0], np.uint16), 32)


PLANTS = [plant_all_codes, plant_block_scales_apart, plant_exact_ties, plant_amax_at_the_exponent_switch, plant_zero_blocks_and_rows, plant_clamped_block,
          plant_down_kpart_edges, plant_last_rows]


@pytest.mark.parametrize("plant", PLANTS, ids=lambda f: f.__name__[6:])
def test_planted_rows_are_exact(plant, hip, checkpoint):
    check(hip, checkpoint, plant)

# ---- the tiny families, fallbacks and refusals -----------------------------------------------------------------------------------------------------
def tiny_pair(fam, hip, dtype="bf16", inter=None, plant=None, opts=FP4, twin=Model):
    """A: `opts` uploaded W.  B (made by `twin`, an ordinary context or the oracle; None: no B): uploaded the dequantized tensors"""
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(dict(cfg, intermediate_size=inter) if inter else cfg, dtype)
    a, b = Model(d, hip), twin and (twin(d, hip) if twin is Model else twin(d))
    for key, value in opts:
        a.set_option(key, value)
    for name, bits in synth.synth_checkpoint(d, int(g["seed"]), float(g["std"])):
        bits = np.array(bits, copy=True)
        if plant:
            plant(name, bits)
        a.upload(name, bits)
        if twin:
            b.upload(name, R.dequantized(bits) if is_quantized(name, 7, d.tied) and bits.ndim == 2 else bits)
    return a, b, d, g


@pytest.mark.parametrize("fam,inter", [("llama_tiny", None), ("qwen2_tiny", None), ("mistral_tiny", None), ("qwen3_tiny", None), ("llama_tiny", 10240),
                                       ("llama_tiny", 12288), ("llama_tiny", 28672), ("llama_tiny", 16392)])
def test_tiny_families_are_bit_identical(fam, inter, hip):
    """K = 192 .. 640: one or two chunks per lane, padding lanes, an untied head (Mistral).  Intermediate 10240 / 12288: down at 5 / 6 chunks per lane (a whole
    quad and a short one).  28672, the 70B geometry: down runs as two launches over K ranges of 14336, 7 chunks per lane, each on its own stream.  16392: down's
    K is no multiple of 32 — no stream, but the model is the quantized one all the same"""
    a, b, d, g = tiny_pair(fam, hip, inter=inter)
    a.finalize(); b.finalize()
    fell = d.layers if inter == 16392 else 0
    assert (a.get_option("weights.fp4_matrices"), a.get_option("weights.fp4_fallbacks")) == (2 * d.layers + 1 - fell, fell)
    for graph in (1, 0):
        assert_bit_identical(run_tiny(a, g, graph, steps=3), run_tiny(b, g, graph, steps=3))


BOTH = FP4 + (("weights.fp8", 1), ("weights.fp8_classes", 6), ("weights.fp4_classes", 3))      # down selected twice
# gate_up by FP8, down by FP4: the scan of both forms' matrices runs before either overwrites a master, so the FP4 refusal below leaves the FP8 class untouched too
MIXED = FP4 + (("weights.fp8", 1), ("weights.fp8_classes", 1), ("weights.fp4_classes", 2))


@pytest.mark.parametrize("fam,dtype,opts,bad,status,names", [
    ("gpt2_hd64", "bf16", FP4, None, ERR_UNSUPPORTED, ["weights.fp4"]), ("llama_tiny", "fp16", FP4, None, ERR_UNSUPPORTED, ["weights.fp4"]),
    ("llama_tiny", "fp32", FP4, None, ERR_UNSUPPORTED, ["weights.fp4"]), ("llama_tiny", "bf16", BOTH, None, ERR_INVALID, ["weights.fp8", "weights.fp4"]),
    ("llama_tiny", "bf16", FP4, ("model.layers.1.mlp.up_proj.weight", 7, 0x7F80), ERR_UNSUPPORTED, ["model.layers.1.mlp.up_proj.weight"]),          # inf
    ("llama_tiny", "bf16", FP4, ("model.layers.0.mlp.down_proj.weight", 0, 0xFFC0), ERR_UNSUPPORTED, ["model.layers.0.mlp.down_proj.weight"]),      # NaN
    ("llama_tiny", "bf16", FP4, ("model.embed_tokens.weight", 255, 0x7180), ERR_UNSUPPORTED, ["model.embed_tokens.weight"]),                        # 2^100
    ("llama_tiny", "bf16", MIXED, ("model.layers.1.mlp.down_proj.weight", 3, 0x7F80), ERR_UNSUPPORTED, ["weights.fp4:", "model.layers.1.mlp.down_proj.weight"])])      # inf
def test_refusals(fam, dtype, opts, bad, status, names, hip):
    def plant(name, bits):
        if bad and name == bad[0]:
            bits[bad[1], 9] = bad[2]
    a, _, _, _ = tiny_pair(fam, hip, dtype=dtype, plant=plant, opts=opts, twin=None)
    with pytest.raises(TgxError) as e:
        a.finalize()
    assert e.value.status == status and all(n in str(e.value) for n in names)

# ---- one model on every path -----------------------------------------------------------------------------------------------------------------------
def test_fp4_mlp_with_an_fp8_head(hip, checkpoint):
    a, b = check(hip, checkpoint, opts=FP4 + (("weights.fp4_classes", 3), ("weights.fp8", 1), ("weights.fp8_classes", 4)), head=R8.dequantized)
    assert (a.get_option("weights.fp4_matrices"), a.get_option("weights.fp8_matrices"), a.get_option("weights.packed_matrices")) == (2, 1, 0)


def test_multi_row_paths_read_the_dequantized_master(hip, checkpoint):
    """tgx_forward_rows of two prompts, three tgx_decode_rows steps and one tgx_verify_row: none of them reads the codes, all of them compute A's model"""
    out = []
    for m in pair(hip, checkpoint, max_batch=4):
        m.forward_rows([0, 1], [synth.synth_prompt(1024, 24, 11), synth.synth_prompt(1024, 9, 12)])
        got = [m.logits(rounded=False).copy()]
        for r in (0, 1):
            m.sample_row(r, GREEDY)
        ids, _, _ = m.decode_rows(3)
        got += [ids.copy(), m.logits(rounded=False).copy()]
        vids, _ = m.verify_row(0, [int(ids[-1, 0]), 5, 6])
        out.append(got + [vids.copy(), m.pass_logits().copy(), m.logits(rounded=False).copy()])
    for x, y in zip(*out):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def test_bytes_per_token_is_the_layout_closed_form(hip, checkpoint):
    a, _ = pair(hip, checkpoint, opts=FP4 + (("weights.packed", 0),))
    c = Model(desc(), hip)
    c.set_option("weights.packed", 0)
    c.load_synthetic(SEED, STD).finalize()
    d = desc()
    H, I, V = d.hidden, d.inter, d.vocab
    saved = sum(2 * rows * K - rows * R.row_bytes(K, ks) for rows, K, ks in ((2 * I, H, 1), (H, I, 4), (V, H, 1)))
    for T in (0, 16):
        assert c.bytes_per_token(T) - a.bytes_per_token(T) == saved
    assert R.row_bytes(H, 1) * 32 == H * 17 and R.row_bytes(I, 4) * 32 == I * 17      # (no padding here: 4.25 bits per weight)


@pytest.mark.parametrize("fam", ["llama_tiny", "mistral_tiny"])
def test_quantized_context_against_the_oracle(fam, hip, oracle_lib):
    """A's teacher-forced logits against the CPU oracle uploaded the dequantized tensors, at tests/test_hip_parity.py's bound"""
    from oracle.oracle_ffi import OracleModel
    a, ref, d, g = tiny_pair(fam, hip, twin=OracleModel)
    a.finalize(); ref.finalize()
    ids = g["ids_bf16"]
    a.forward(g["prompt"]); ref.forward(g["prompt"])
    assert rel_err(a.logits(rounded=False), ref.logits(rounded=False)) < 1e-3
    for i in range(1, ids.shape[1]):
        a.forward(ids[:, i - 1:i]); ref.forward(ids[:, i - 1:i])
        assert rel_err(a.logits(rounded=False), ref.logits(rounded=False)) < 1e-3, f"step {i}"
