"""Option weights.fp8 (include/tgx.h; kernels/gemv_fp8.h): tgx_finalize quantizes the gate_up / down / lm_head matrices to E4M3 codes with a power-of-two scale
per row, overwrites the bf16 masters with the dequantized values, and the batch-1 launches stream the codes.

Every dequantized weight is exactly a bf16 value, so nothing here has a tolerance: context A (weights.fp8 = 1, uploaded W) must equal context B (weights.fp8 = 0,
uploaded fp8_ref.dequantized(W) for the quantized tensors) BIT FOR BIT — ids and unrounded fp32 logits as uint32 — on the batch-1 steps (the new kernel against
the plain / exponent-packed ones) and on every path that reads the master (prefill, batched steps, verify).  B's tensors come from tests/fp8_ref.py, the numpy
statement of the rule, so the device quantizer is held to it as well.  The one comparison with a tolerance is the CPU oracle's (tests/test_hip_parity.py's 1e-3).

Geometry as tests/test_hip_packed_hl.py: a one-layer Llama descriptor at hidden 2048, intermediate 8192, vocabulary 1024, tied head — NX = 4 chunks per lane at
KS = 1 (gate_up, lm_head) and at KS = 4 (down), two 16-byte loads per lane and row; the tiny families add padded pairs and K not a multiple of 512."""
import copy

import numpy as np
import pytest

import fp8_ref as R
from conftest import load_golden, rel_err
from tinygpt_amd import known_desc, synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model, TgxError

pytestmark = pytest.mark.gpu
SEED, STD, STEPS, PROMPT = 7, 0.02, 4, 24
GATE, UP, DOWN, HEAD = ("model.layers.0.mlp.gate_proj.weight", "model.layers.0.mlp.up_proj.weight", "model.layers.0.mlp.down_proj.weight",
                        "model.embed_tokens.weight")      # (tied head)
MLP = (GATE, UP, DOWN, HEAD)
ERR_UNSUPPORTED, ERR_STATE = 2, 4
FINITE = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], np.uint8)      # the 254 finite codes


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def desc(max_batch=1):
    d = copy.deepcopy(known_desc("llama-3.2-1b", "bf16"))
    d.layers, d.vocab, d.max_ctx, d.max_batch = 1, 1024, 64, max_batch
    assert (d.hidden, d.inter, d.tied) == (2048, 8192, True)
    return d


@pytest.fixture(scope="module")
def checkpoint():
    """the tensors once per module, and the dequantized form of the four quantized ones: every context uploads (an edited copy of) these"""
    W = [(name, np.array(bits, copy=True)) for name, bits in synth.synth_checkpoint(desc(), SEED, STD)]
    return W, {name: R.dequantized(bits) for name, bits in W if name in MLP}


def is_quantized(name, classes, tied=True):
    if "gate_proj" in name or "up_proj" in name:
        return bool(classes & 1)
    if "down_proj" in name:
        return bool(classes & 2)
    return bool(classes & 4) and name == ("model.embed_tokens.weight" if tied else "lm_head.weight")      # (a tied head IS the embedding table)


def dequantized_after(bits, base, base_dq):
    """fp8_ref.dequantized(bits) where bits is `base` with a few rows edited: only those rows are worked out again"""
    out = base_dq.copy()
    rows = np.nonzero((bits != base).any(axis=1))[0]
    if rows.size:
        out[rows] = R.dequantized(bits[rows])
    return out


def pair(hip, checkpoint, plant=None, max_batch=1, classes=7, packed=None):
    """A: weights.fp8 = 1 uploaded W.  B: weights.fp8 = 0 uploaded dequantized(W) for the tensors of the quantized classes.  Everything else equal."""
    W, DQ = checkpoint
    a, b = Model(desc(max_batch), hip), Model(desc(max_batch), hip)
    a.set_option("weights.fp8", 1); a.set_option("weights.fp8_classes", classes)
    if packed is not None:
        a.set_option("weights.packed", packed[0]); a.set_option("weights.packed_classes", packed[1])
    for name, bits in W:
        wa = wb = bits
        if name in MLP:
            if plant:
                wa = bits.copy()
                plant(name, wa)
            wb = dequantized_after(wa, bits, DQ[name]) if is_quantized(name, classes) else wa
        a.upload(name, wa); b.upload(name, wb)
    return a.finalize(), b.finalize()


def run(m, graph):
    """prompt + STEPS greedy decode steps: the ids and the unrounded fp32 logits of the prefill and of every step"""
    m.set_option("graph", graph)
    m.reset_cache()
    m.forward(synth.synth_prompt(1024, PROMPT, SEED)[None, :])
    ids, logits = [m.sample(GREEDY).copy()], [m.logits(rounded=False).copy()]
    for _ in range(STEPS):
        ids.append(m.decode(1, GREEDY)[0].copy())
        logits.append(m.logits(rounded=False).copy())
    return np.stack(ids), np.stack(logits)


def assert_bit_identical(x, y):
    np.testing.assert_array_equal(x[0], y[0])
    np.testing.assert_array_equal(x[1].view(np.uint32), y[1].view(np.uint32))      # bit for bit (-0 / +0 included)
    assert np.isfinite(y[1]).all()


def check(hip, checkpoint, plant=None):
    a, b = pair(hip, checkpoint, plant)
    assert (a.get_option("weights.fp8_matrices"), a.get_option("weights.fp8_fallbacks")) == (3, 0)
    assert (b.get_option("weights.fp8_matrices"), b.get_option("weights.fp8_fallbacks")) == (0, 0)
    for graph in (1, 0):
        assert_bit_identical(run(a, graph), run(b, graph))
    a.close(); b.close()


# ---- 1. the benchmark's row geometry --------------------------------------------------------------------------------------------------------------
def test_bench_row_geometry_is_bit_identical(hip, checkpoint):
    check(hip, checkpoint)


# ---- 2. planted rows ------------------------------------------------------------------------------------------------------------------------------
def f2b(v):
    return R.bf16_bits(np.asarray(v, np.float64))


def all_codes_rows(bits, rows, ks, e):
    """the 254 finite codes (as the weights code * 2^e, which quantize to themselves: 448 * 2^e among them pins the rows' exponent) over `rows` of a matrix
    whose launch splits K over `ks` waves, so that every element t = 0..7 of a chunk and both 16-byte loads h of a lane (chunk pairs j = 0, 1 and j = 2, 3 at
    NX = 4) see every code: within one h the n-th chunk holds code (n + 37 t) mod 254 at element t, and the rows together have at least 254 chunks per h"""
    K = bits.shape[1]
    nchunk, nx, nh, per = R.geometry(K, ks)
    count = [0] * nh
    seen = set()
    for r in rows:
        for c in range(nchunk):
            h = ((c % per) // 64) // 2
            for t in range(8):
                code = FINITE[(count[h] + 37 * t) % 254]
                bits[r, 8 * c + t] = f2b(np.ldexp(R.code_value(code), e))
                seen.add((int(code), t, h))
            count[h] += 1
    assert len(seen) == 254 * 8 * nh


def plant_all_codes(name, bits):
    if name == GATE: all_codes_rows(bits, (40, 41), 1, -12)
    if name == UP: all_codes_rows(bits, (40, 8190), 1, -15)           # (row 40 is gate row 40's partner in unit 40: another scale in the same 2-vector)
    if name == DOWN: all_codes_rows(bits, (1001,), 4, -13)
    if name == HEAD: all_codes_rows(bits, (500, 501), 1, -11)


def plant_gate_up_scales_apart(name, bits):
    """gate row u and up row u share a 2-vector FMA chain: their scales 2^10 apart, either way round (a power of two moves the exponent field: exact)"""
    for u, (dg, du) in ((0, (5, -5)), (1234, (-5, 5)), (8191, (6, -4))):
        d = dg if name == GATE else du if name == UP else 0
        if d:
            assert ((bits[u] >> 7) & 0xFF).min() > 8
            bits[u] = (bits[u].astype(np.int32) + (d << 7)).astype(np.uint16)


def plant_all_zero_row(name, bits):
    if name == GATE: bits[17] = 0x0000
    if name == UP: bits[18] = 0x0000; bits[19] = 0x8000
    if name == DOWN: bits[2] = 0x0000
    if name == HEAD: bits[3] = 0x0000


def plant_negative_zero(name, bits):
    K = bits.shape[1]
    bits[5, [0, 3, 7, 8, K // 2 + 5, K - 1]] = 0x8000
    bits[6, ::2] = 0x8000


def plant_large_and_subnormal_codes(name, bits):
    """one weight 2^16 above the largest of its row: every other weight falls into the subnormal code range (|w / 2^e| < 2^-6), most of them onto zero"""
    for r, k in ((9, 0), (10, bits.shape[1] - 1), (bits.shape[0] - 2, 1000)):
        big = int((bits[r] & 0x7FFF).max())
        bits[r, k] = ((big + (16 << 7)) & 0x7F80) | (0x8000 if r & 1 else 0)
        codes, _ = R.quantize(bits[r:r + 1])
        assert ((codes[0] & 0x78) == 0).sum() == bits.shape[1] - 1 and (codes[0] & 0x7F).astype(bool).sum() > 8      # subnormal codes, not all of them zero


def plant_exact_ties(name, bits):
    """the midpoint of every pair of neighbouring codes, both signs, under a pinned exponent: round-to-nearest-EVEN decides each"""
    v = R.code_value(np.arange(0, 0x7F))
    mid = (v[:-1] + v[1:]) / 2
    vals = np.concatenate([[448.0], mid, -mid])
    K = bits.shape[1]
    row = f2b(np.ldexp(np.resize(vals, K), -14))
    bits[21] = row
    bits[22] = np.roll(row, 3)


def plant_down_kpart_edges(name, bits):
    """down runs KS = 4: K-part p holds chunks 256 p .. 256 p + 255, i.e. k in [2048 p, 2048 p + 2047] — loud values in its first and last chunk"""
    if name == DOWN:
        loud = f2b([0.109375, -0.09375, 0.078125, -0.0625, 0.0546875, -0.046875, 0.0390625, -0.03125])
        for p, row in enumerate((30, 31, 32, 33)):
            bits[row, 2048 * p:2048 * p + 8] = loud
            bits[row, 2048 * p + 2040:2048 * p + 2048] = loud[::-1]
        for p in range(4):
            bits[34, 2048 * p:2048 * p + 8] = loud
            bits[34, 2048 * p + 2040:2048 * p + 2048] = loud[::-1]


def plant_last_rows(name, bits):
    """the last row of each matrix (of the gate half and of the up half of the merged one): louder by 2^3, a -0 and a zero at its ends"""
    r = bits.shape[0] - 1
    bits[r] = (bits[r].astype(np.int32) + (3 << 7)).astype(np.uint16)
    bits[r, 0] = 0x8000; bits[r, -1] = 0x0000


PLANTS = [plant_all_codes, plant_gate_up_scales_apart, plant_all_zero_row, plant_negative_zero, plant_large_and_subnormal_codes, plant_exact_ties,
          plant_down_kpart_edges, plant_last_rows]


@pytest.mark.parametrize("plant", PLANTS, ids=lambda f: f.__name__[6:])
def test_planted_rows_are_exact(plant, hip, checkpoint):
    check(hip, checkpoint, plant)


# ---- 3. the tiny families ---------------------------------------------------------------------------------------------------------------------------
def tiny_pair(fam, hip, dtype="bf16", inter=None, plant=None, fp8=1, twin=True):
    cfg, g = load_golden(fam)
    if inter:
        cfg = dict(cfg, intermediate_size=inter)
    d = desc_from_hf_config(cfg, dtype)
    a, b = Model(d, hip), Model(d, hip)
    a.set_option("weights.fp8", fp8)
    for name, bits in synth.synth_checkpoint(d, int(g["seed"]), float(g["std"])):
        bits = np.array(bits, copy=True)
        if plant:
            plant(name, bits)
        a.upload(name, bits)
        if twin:
            b.upload(name, R.dequantized(bits) if is_quantized(name, 7, d.tied) and bits.ndim == 2 else bits)
    return a, b, d, g


def run_tiny(m, g, graph, steps=6):
    m.set_option("graph", graph)
    m.reset_cache()
    m.forward(g["prompt"])
    ids, logits = [m.sample(GREEDY).copy()], [m.logits(rounded=False).copy()]
    for _ in range(steps):
        ids.append(m.decode(1, GREEDY)[0].copy())
        logits.append(m.logits(rounded=False).copy())
    return np.stack(ids), np.stack(logits)


@pytest.mark.parametrize("fam", ["llama_tiny", "qwen2_tiny", "mistral_tiny", "qwen3_tiny"])
def test_tiny_families_are_bit_identical(fam, hip):
    """K = 192 .. 640: one or two chunks per lane, lanes and whole chunk pairs that are padding, K no multiple of 512, an untied head (Mistral)"""
    a, b, d, g = tiny_pair(fam, hip)
    a.finalize(); b.finalize()
    assert (a.get_option("weights.fp8_matrices"), a.get_option("weights.fp8_fallbacks")) == (2 * d.layers + 1, 0)
    for graph in (1, 0):
        assert_bit_identical(run_tiny(a, g, graph), run_tiny(b, g, graph))


def test_a_shape_outside_the_layout_is_quantized_and_runs_plain(hip):
    """intermediate 16392: down's K needs 9 chunks per lane at KS = 4 — no stream, but the model is the quantized one all the same"""
    a, b, d, g = tiny_pair("llama_tiny", hip, inter=16392)
    a.finalize(); b.finalize()
    assert (a.get_option("weights.fp8_matrices"), a.get_option("weights.fp8_fallbacks")) == (d.layers + 1, d.layers)
    for graph in (1, 0):
        assert_bit_identical(run_tiny(a, g, graph, steps=3), run_tiny(b, g, graph, steps=3))


@pytest.mark.parametrize("fam,dtype", [("gpt2_hd64", "bf16"), ("llama_tiny", "fp16"), ("llama_tiny", "fp32")])
def test_other_dtypes_and_gpt2_are_refused(fam, dtype, hip):
    a, b, d, g = tiny_pair(fam, hip, dtype=dtype)
    with pytest.raises(TgxError) as e:
        a.finalize()
    assert e.value.status == ERR_UNSUPPORTED and "weights.fp8" in str(e.value)
    a2, _, _, _ = tiny_pair(fam, hip, dtype=dtype, fp8=0)
    a2.finalize()                                       # (the same uploads finalize without the option)


@pytest.mark.parametrize("tensor,row,bad", [("model.layers.1.mlp.up_proj.weight", 7, 0x7F80), ("model.layers.0.mlp.down_proj.weight", 0, 0xFFC0),
                                            ("model.embed_tokens.weight", 255, 0x7180)])
def test_a_refused_weight_names_its_tensor(tensor, row, bad, hip):
    """inf, NaN and 2^100"""
    def plant(name, bits):
        if name == tensor:
            bits[row, 9] = bad
    a, b, d, g = tiny_pair("llama_tiny", hip, plant=plant, twin=False)
    with pytest.raises(TgxError) as e:
        a.finalize()
    assert e.value.status == ERR_UNSUPPORTED and tensor in str(e.value)


# ---- 4. one model on every path ---------------------------------------------------------------------------------------------------------------------
def test_multi_row_paths_read_the_dequantized_master(hip, checkpoint):
    """tgx_forward_rows of two prompts, three tgx_decode_rows steps and one tgx_verify_row: none of them reads the codes, all of them compute A's model"""
    a, b = pair(hip, checkpoint, max_batch=4)
    prompts = [synth.synth_prompt(1024, 24, 11), synth.synth_prompt(1024, 9, 12)]
    out = []
    for m in (a, b):
        m.forward_rows([0, 1], prompts)
        got = [m.logits(rounded=False).copy()]
        for r in (0, 1):
            m.sample_row(r, GREEDY)
        ids, produced, fin = m.decode_rows(3)
        got += [ids.copy(), m.logits(rounded=False).copy()]
        draft = [int(ids[-1, 0]), 5, 6]
        vids, vfin = m.verify_row(0, draft)
        got += [vids.copy(), m.pass_logits().copy(), m.logits(rounded=False).copy()]
        out.append(got)
    for x, y in zip(*out):
        if x.dtype == np.float32:
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
        else:
            np.testing.assert_array_equal(x, y)


# ---- 5. against the oracle ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["llama_tiny", "mistral_tiny"])
def test_quantized_context_against_the_oracle(fam, hip, oracle_lib):
    """A's teacher-forced logits against the CPU oracle uploaded the dequantized tensors, at tests/test_hip_parity.py's bound"""
    from oracle.oracle_ffi import OracleModel
    a, _, d, g = tiny_pair(fam, hip)
    a.finalize()
    ref = OracleModel(d)
    for name, bits in synth.synth_checkpoint(d, int(g["seed"]), float(g["std"])):
        ref.upload(name, R.dequantized(bits) if is_quantized(name, 7, d.tied) and bits.ndim == 2 else bits)
    ref.finalize()
    ids = g["ids_bf16"]
    a.forward(g["prompt"]); ref.forward(g["prompt"])
    assert rel_err(a.logits(rounded=False), ref.logits(rounded=False)) < 1e-3
    for i in range(1, ids.shape[1]):
        a.forward(ids[:, i - 1:i]); ref.forward(ids[:, i - 1:i])
        assert rel_err(a.logits(rounded=False), ref.logits(rounded=False)) < 1e-3, f"step {i}"


# ---- 6. options and accounting ------------------------------------------------------------------------------------------------------------------------
def test_options_are_read_at_finalize(hip, checkpoint):
    a, b = pair(hip, checkpoint, packed=(1, 7))
    for key in ("weights.fp8", "weights.fp8_classes"):
        with pytest.raises(TgxError) as e:
            a.set_option(key, 1)
        assert e.value.status == ERR_STATE
    assert (a.get_option("weights.fp8"), a.get_option("weights.fp8_classes")) == (1, 7)
    assert a.get_option("weights.packed_matrices") == 0 and a.get_option("weights.fp8_matrices") == 3        # fp8 classes get no 12-bit copy
    assert (b.get_option("weights.fp8"), b.get_option("weights.fp8_classes")) == (0, 7)


def test_bytes_per_token_is_the_layout_closed_form(hip, checkpoint):
    a, b = pair(hip, checkpoint, packed=(0, 0))
    c = Model(desc(), hip)
    c.set_option("weights.packed", 0)
    c.load_synthetic(SEED, STD).finalize()
    d = desc()
    H, I, V = d.hidden, d.inter, d.vocab
    saved = 0
    for rows, K, ks in ((2 * I, H, 1), (H, I, 4), (V, H, 1)):
        saved += 2 * rows * K - rows * (R.row_bytes(K, ks) + 4)          # the code planes as laid out plus one 4-byte scale per row
    for T in (0, 16):
        assert c.bytes_per_token(T) - a.bytes_per_token(T) == saved
    assert R.row_bytes(H, 1) == H and R.row_bytes(I, 4) == I            # (no padding here: one byte per weight)


def test_a_class_mask_leaves_the_other_classes_alone(hip, checkpoint):
    """weights.fp8_classes = 1: gate_up alone is quantized; down and the head are the uploaded W (B is uploaded W for them)"""
    a, b = pair(hip, checkpoint, classes=1)
    assert (a.get_option("weights.fp8_matrices"), a.get_option("weights.fp8_fallbacks")) == (1, 0)
    for graph in (1, 0):
        assert_bit_identical(run(a, graph), run(b, graph))
    W, DQ = checkpoint
    assert (DQ[DOWN] != dict(W)[DOWN]).any()                            # (the comparison would notice a quantized down)
