"""Batched MFMA prefill (kernels/prefill.h) == the same prompt fed as single-position passes (the decode kernels,
which are parity-green against the oracle), and == the oracle directly on the fixtures.  Size-independent property at
real layer shapes: prefill(S) then decode == step-by-step, KV cache contents equal up to bf16 rounding flips."""
import copy

import numpy as np
import pytest

from conftest import GPU_FAMILIES, load_golden, rel_err
from tinygpt_amd import known_desc, synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model, product_backend

pytestmark = pytest.mark.gpu


def run(model, prompt, mfma, n_decode=4):
    model.reset_cache()
    model.set_option("prefill.mfma", int(mfma))
    model.forward(prompt)
    logits = model.logits(rounded=False).copy()
    first = model.sample(GREEDY).copy()
    rest = model.decode(n_decode, GREEDY).copy()
    kv = [model.read_kv(0, l) for l in range(model.desc.layers)]
    return logits, first, rest, kv


@pytest.mark.parametrize("fam", GPU_FAMILIES)
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_fixture_prefill_matches_steps_and_oracle(fam, dtype, oracle_lib):
    """Every family incl. GPT-2 (LayerNorm-split prologue, bias + gelu_new epilogue, learned positions) and every storage dtype: 16-bit
    storage runs the split-term bf16 / f16 MFMA GEMMs, fp32 storage the f32-input MFMA GEMMs (kernels/gemm_f32.h) with the decode
    attention kernel over the prompt rows."""
    from oracle.oracle_ffi import OracleModel
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(cfg, dtype)
    gpu = Model(d, product_backend()).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    ref = OracleModel(d).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    # a longer prompt than the golden one so that M is not a tile multiple and causal masking crosses a key tile
    prompt = synth.synth_prompt(d.vocab, min(d.max_ctx - 8, 97), 5)[None, :]
    l1, f1, r1, kv1 = run(gpu, prompt, mfma=True)
    l0, f0, r0, kv0 = run(gpu, prompt, mfma=False)
    ref.forward(prompt)
    lr = ref.logits(rounded=False)
    assert rel_err(l1, lr) < 1e-3 and rel_err(l0, lr) < 1e-3
    assert rel_err(l1, l0) < 1e-3          # same contract bound; the two schedules differ by bf16 KV rounding flips
    np.testing.assert_array_equal(f1, f0)
    np.testing.assert_array_equal(f1, ref.sample(GREEDY))
    np.testing.assert_array_equal(r1, r0)
    ulp = {"bf16": 8e-3, "fp16": 1e-3, "fp32": 1e-5}[dtype]
    for (k1, v1), (k0, v0) in zip(kv1, kv0):
        # cache entries of the two schedules: equal to within one storage ulp of the tensor's magnitude (the split
        # MFMA products are exact to ~2^-17 (bf16 x2) / 2^-22 (fp16 x2) of |x||w|, so near-zero elements may round differently)
        assert rel_err(k1, k0) < ulp and rel_err(v1, v0) < ulp
    if dtype == "fp32":                      # fp32 storage: both schedules sit on the oracle (and on HF fp32) to fp32 summation order
        assert rel_err(l1, lr) < 1e-4 and rel_err(l1, l0) < 1e-4


@pytest.mark.parametrize("name,S,dtype", [("llama-3.2-1b", 300, "bf16"), ("mistral-7b-v0.3", 130, "bf16"), ("qwen2.5-0.5b", 257, "bf16"),
                                          ("llama-3.2-1b", 300, "fp16"), ("mistral-7b-v0.3", 130, "fp16"),
                                          ("qwen2.5-3b", 200, "bf16"), ("qwen3-1.7b", 150, "bf16"),   # the README's other checkpoints: 8 query heads per kv head; q/k norm
                                          ("gpt2", 300, "bf16"), ("gpt2", 300, "fp16"), ("gpt2", 300, "fp32"),           # BASELINE configs[0]'s model
                                          ("llama-3.2-1b", 300, "fp32"), ("mistral-7b-v0.3", 130, "fp32"), ("qwen2.5-0.5b", 257, "fp32"), ("qwen3-1.7b", 90, "fp32"),
                                          # the long-prompt forms of round 5 at the shapes their A / B tests used (those compared new against old bit for bit through option
                                          # switches that are gone: VERDICT r5 item 6): gate_up on whole 128-byte lines, the QKV product on shared activation lines with RoPE /
                                          # cache append / q split in its epilogue (also with a QKV bias, ADVICE r5, and a ragged last row block), `down` as one slab
                                          ("llama-3.2-1b", 1024, "bf16"), ("llama-3.2-1b", 1900, "bf16"), ("llama-3.2-1b", 2048, "fp16"), ("mistral-7b-v0.3", 1100, "bf16"),
                                          ("llama-3.2-1b+qkv_bias", 1000, "bf16"), ("llama-3.2-1b", 2048, "bf16")])
def test_real_layer_shapes_prefill_equals_steps(name, S, dtype):
    """Real hidden/intermediate/head geometry (2 layers, 4096-entry vocabulary to keep the upload small): the batched matrix-core prefill against the same
    prompt through the decode kernels (other kernels, the same math)."""
    d = copy.deepcopy(known_desc(name.split("+")[0], dtype))
    d.layers, d.vocab, d.max_ctx = 2, 4096, max(512, S + 16)
    if name.endswith("+qkv_bias"):
        d.qkv_bias = True
    m = Model(d, product_backend()).load_synthetic(1234, 0.02).finalize()
    prompt = synth.synth_prompt(d.vocab, S, 77)[None, :]
    l1, f1, r1, kv1 = run(m, prompt, mfma=True, n_decode=3)
    l0, f0, r0, kv0 = run(m, prompt, mfma=False, n_decode=3)
    assert rel_err(l1, l0) < 1e-3, rel_err(l1, l0)
    np.testing.assert_array_equal(f1, f0)
    np.testing.assert_array_equal(r1, r0)
    ulp = {"bf16": 8e-3, "fp16": 1e-3, "fp32": 1e-5}[dtype]
    for (k1, v1), (k0, v0) in zip(kv1, kv0):
        assert rel_err(k1, k0) < ulp and rel_err(v1, v0) < ulp
    if dtype == "fp32":
        assert rel_err(l1, l0) < 1e-4


@pytest.mark.parametrize("fam,dtype", [("llama_tiny", "bf16"), ("qwen2_tiny", "bf16"), ("qwen3_tiny", "bf16"), ("mistral_tiny", "fp16")])
@pytest.mark.parametrize("nb,S", [(1, 33), (1, 48), (1, 64), (2, 29), (3, 21), (1, 65), (1, 100), (1, 128), (3, 40)])
def test_prompts_of_33_to_64_rows_on_the_skinny_kernels(fam, dtype, nb, S, oracle_lib):
    """Prompts whose rows (batch x length) number 33..64 run every product as a skinny MFMA GEMM with FOUR 16-row activation blocks, 65..128 rows with
    EIGHT (round 3, kernels/skinny.h MB = 4, kernels/skinny_dma.h MB = 4 / 8; option prefill.skinny_rows = 32 sends them back to the tiled split-K GEMMs;
    the fixtures' hidden sizes are below the 2048 limit of the eight-block form): against the oracle (<= 1e-3, first id where
    the gap is clear) and against the tiled path (<= 1e-3; K tails at hidden 192, QKV bias, q / k norm, head_dim 128, three-term QKV product in bf16)."""
    from oracle.oracle_ffi import OracleModel
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(cfg, dtype, max_batch=nb)
    d.max_ctx = 136
    gpu = Model(d, product_backend()).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    ref = OracleModel(d).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    ids = np.stack([synth.synth_prompt(d.vocab, S, 9 + b) for b in range(nb)])
    ref.forward(ids)
    lr = ref.logits(rounded=False)
    out = {}
    for rows in (128, 32):
        gpu.set_option("prefill.skinny_rows", rows)
        gpu.reset_cache(); gpu.forward(ids)
        lg = gpu.logits(rounded=False).copy()
        assert rel_err(lg, lr) < 1e-3, (rows, rel_err(lg, lr))
        first = gpu.sample(GREEDY).copy()
        out[rows] = (lg, first, gpu.decode(4, GREEDY).copy(), [gpu.read_kv(nb - 1, l) for l in range(d.layers)])
    top2 = np.sort(lr, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2e-3 * np.abs(lr).max()
    np.testing.assert_array_equal(out[128][1][clear], ref.sample(GREEDY)[clear])
    assert rel_err(out[128][0], out[32][0]) < 1e-3
    ulp = {"bf16": 8e-3, "fp16": 1e-3}[dtype]
    for (k1, v1), (k0, v0) in zip(out[128][3], out[32][3]):
        assert rel_err(k1, k0) < ulp and rel_err(v1, v0) < ulp


@pytest.mark.parametrize("name,S,dtype", [("llama-3.2-1b", 48, "bf16"), ("mistral-7b-v0.3", 40, "bf16"), ("qwen2.5-0.5b", 64, "bf16"), ("qwen3-1.7b", 57, "fp16")])
def test_real_layer_shapes_33_to_64_row_prompts_skinny_equals_tiled(name, S, dtype):
    """the same at real hidden / intermediate / head geometry (2 layers, 4096-entry vocabulary): the four-block skinny path against the tiled split-K path"""
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx = 2, 4096, 128
    m = Model(d, product_backend()).load_synthetic(1234, 0.02).finalize()
    prompt = synth.synth_prompt(d.vocab, S, 77)[None, :]
    res = {}
    m.set_option("prefill.skinny_hidden_max", 1 << 20)       # by default hidden > 2048 keeps 33-64-row prompts on the tiled path (faster there)
    for rows in (64, 32):
        m.set_option("prefill.skinny_rows", rows)
        res[rows] = run(m, prompt, mfma=True, n_decode=3)
    assert rel_err(res[64][0], res[32][0]) < 1e-3, rel_err(res[64][0], res[32][0])
    np.testing.assert_array_equal(res[64][1], res[32][1])
    np.testing.assert_array_equal(res[64][2], res[32][2])
    ulp = {"bf16": 8e-3, "fp16": 1e-3}[dtype]
    for (k1, v1), (k0, v0) in zip(res[64][3], res[32][3]):
        assert rel_err(k1, k0) < ulp and rel_err(v1, v0) < ulp


@pytest.mark.parametrize("name,S,dtype", [("llama-3.2-1b", 300, "bf16"), ("llama-3.2-1b", 1024, "bf16"), ("llama-3.2-1b", 700, "fp16"), ("mistral-7b-v0.3", 400, "bf16"), ("qwen2.5-0.5b", 600, "bf16")])
def test_n_hidden_products_as_k_slabs_on_the_eight_wave_kernel(name, S, dtype):
    """Round 4 (option prefill.splitk_8k, on by default): the o_proj / down products of a 129-1500-row prompt, whose 128 x 128 tiles number less than a chip, run as
    2-4 K slabs on the eight-wave LDS-DMA kernel (gemm_dma8k_kernel<.., GEMM_PARTIAL>; slabs summed in z order by the next row-wise kernel or the reducer).
    Against the same prompt without it (64-row register-staged slabs below 256 tiles, a half-empty chip above): the same products in another summation
    order — ONE layer (no cache row has a schedule-dependent input): logits within 2e-5, the same first token; and bit-identical on a second run."""
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx = 1, 4096, S + 16
    m = Model(d, product_backend()).load_synthetic(1234, 0.02).finalize()
    prompt = synth.synth_prompt(d.vocab, S, 78)[None, :]
    outs = []
    for on in (0, 1, 1):
        m.set_option("prefill.splitk_8k", on)
        m.reset_cache(); m.forward(prompt)
        outs.append((m.logits(rounded=False).copy(), m.sample(GREEDY).copy()))
    assert rel_err(outs[1][0], outs[0][0]) < 2e-5, rel_err(outs[1][0], outs[0][0])
    np.testing.assert_array_equal(outs[1][1], outs[0][1])
    np.testing.assert_array_equal(outs[1][0], outs[2][0])


@pytest.mark.parametrize("name,S", [("llama-3.2-1b", 1200), ("llama-3.2-1b", 1500), ("mistral-7b-v0.3", 600)])
def test_gate_up_on_128_tiles_where_the_256_tiling_is_ragged(name, S):
    """Round 4 (option prefill.wide_8k_eff, 76): a prompt whose 256 x 256 gate_up tiles would fill their last round of workgroups to less than 76 % (1152-1536 rows at
    intermediate 8192) takes the eight-wave 128 x 128 kernel instead — the kernel of the 129-384-row prompts on a larger grid.  Against the 256 x 256 tiling of the
    same prompt (option 0): the same products, the same siluMul epilogue, another tile shape: ONE layer, logits within 2e-5, same first token; the balanced QKV launch
    against K slabs (option prefill.qkv_nosplit) within 2e-4 (its results are rounded into this layer's cache)."""
    d = copy.deepcopy(known_desc(name, "bf16"))
    d.layers, d.vocab, d.max_ctx = 1, 4096, S + 16
    m = Model(d, product_backend()).load_synthetic(1234, 0.02).finalize()
    prompt = synth.synth_prompt(d.vocab, S, 79)[None, :]
    outs = []
    for eff, nosplit in ((0, 1), (76, 1), (76, 1), (76, 0)):
        m.set_option("prefill.wide_8k_eff", eff); m.set_option("prefill.qkv_nosplit", nosplit)
        m.reset_cache(); m.forward(prompt)
        outs.append((m.logits(rounded=False).copy(), m.sample(GREEDY).copy()))
    assert rel_err(outs[1][0], outs[0][0]) < 2e-5, rel_err(outs[1][0], outs[0][0])        # tile shape of gate_up only: no cache row changes
    np.testing.assert_array_equal(outs[1][1], outs[0][1])
    np.testing.assert_array_equal(outs[1][0], outs[2][0])
    # another schedule of the QKV product moves K / V entries across 16-bit rounding boundaries in THIS layer's cache: the two-layer bound of the form tests
    assert rel_err(outs[3][0], outs[1][0]) < 2e-4, rel_err(outs[3][0], outs[1][0])
    np.testing.assert_array_equal(outs[3][1], outs[1][1])


@pytest.mark.parametrize("name,S,dtype", [("llama-3.2-1b", 300, "bf16"), ("llama-3.2-1b", 777, "fp16"), ("qwen2.5-0.5b", 257, "bf16"),
                                          ("mistral-7b-v0.3", 300, "bf16"), ("llama-3.2-3b", 200, "fp16"), ("qwen3-1.7b", 333, "bf16")])
def test_prefill_attention_forms_agree(name, S, dtype):
    """Round 5: the two other schedules of the prompt attention — K / V tiles by LDS-DMA with the next tile's scores under the current softmax (head_dim 64,
    kernels/attn_prefill_dma.h: the same matrix instructions on the same operands in the same order -> BIT-identical) and the key split inside the workgroup
    (attn_prefill_kernel KP = 2: the odd tiles' online-softmax stream merged once at the end -> another fp32 summation order, 2e-5 on one layer) — forced on prompts
    that are ragged in the 128-query blocks and in the 64-key tiles.  The defaults take these forms only for long prompts / head_dim 128."""
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx = 1, 4096, S + 16
    m = Model(d, product_backend()).load_synthetic(1234, 0.02).finalize()
    prompt = synth.synth_prompt(d.vocab, S, 80)[None, :]
    outs = {}
    for form, (dma, ks) in {"plain": (0, 0), "dma": (2, 0), "ksplit": (0, 2), "plain2": (0, 0)}.items():
        m.set_option("prefill.attn_dma", dma); m.set_option("prefill.attn_ksplit", ks)
        m.reset_cache(); m.forward(prompt)
        outs[form] = (m.logits(rounded=False).copy(), m.sample(GREEDY).copy())
    np.testing.assert_array_equal(outs["plain"][0], outs["plain2"][0])
    if d.head_dim == 64:
        np.testing.assert_array_equal(outs["dma"][0], outs["plain"][0])
    assert rel_err(outs["ksplit"][0], outs["plain"][0]) < 2e-5, rel_err(outs["ksplit"][0], outs["plain"][0])
    np.testing.assert_array_equal(outs["ksplit"][1], outs["plain"][1])


@pytest.mark.parametrize("name,S,dtype", [("llama-3.2-1b", 1024, "bf16"), ("llama-3.2-1b", 1900, "bf16"), ("llama-3.2-1b", 2048, "fp16"), ("mistral-7b-v0.3", 1100, "bf16")])
def test_down_on_wide_tiles_matches_the_square_tiles(name, S, dtype):
    """Round 5: the K >> N product (`down`) of a prompt worth two chips of its workgroups (regime knob prefill.wide_n_min) runs on 128 x 256 tiles x 2 K slabs (kernels/gemm_dma.h
    gemm_dma8n_kernel: a third fewer operand lines per output; the slabs are summed in z order by the next norm launch) instead of one slab of 128 x 128 tiles — the same
    products in another fp32 summation order: TWO layers (the second layer's norm consumes the slabs), logits within 2e-5, the same first token; bit-identical on a rerun."""
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx = 2, 4096, S + 16
    m = Model(d, product_backend()).load_synthetic(1234, 0.02).finalize()
    prompt = synth.synth_prompt(d.vocab, S, 84)[None, :]
    outs = []
    for chips in (1 << 20, 1, 1):                     # never / from one chip's worth of workgroups on (the default: two)
        m.set_option("prefill.wide_n_min", chips)
        m.reset_cache(); m.forward(prompt)
        outs.append((m.logits(rounded=False).copy(), m.sample(GREEDY).copy()))
    assert rel_err(outs[1][0], outs[0][0]) < 2e-5, rel_err(outs[1][0], outs[0][0])
    np.testing.assert_array_equal(outs[1][1], outs[0][1])
    np.testing.assert_array_equal(outs[1][0], outs[2][0])




# the experiment knobs retired with their experiments (INTEGRATION.md "Which keys exist"): each is an unknown key now
RETIRED_KEYS = ["prefill.gemm_dma", "prefill.defer_min_rows", "prefill.terms_rows", "prefill.wide_8k_max", "prefill.skinny_hidden_max_wide",
                "attn.batch_la", "attn.batch_nw8", "attn.direct_g", "attn.fused_max", "attn.fused_nw4",
                "skinny.cfg", "skinny.cfg_mid", "skinny.wgs", "skinny.dma_nbw", "skinny.dma_rows", "skinny.dma_qkv", "skinny.terms_above", "skinny.gu_split"]


@pytest.fixture(scope="module")
def llama_tiny():
    cfg, g = load_golden("llama_tiny")
    return Model(desc_from_hf_config(cfg, "bf16"), product_backend()).load_synthetic(int(g["seed"]), float(g["std"])).finalize()


@pytest.mark.parametrize("key", RETIRED_KEYS)
def test_retired_option_is_an_unknown_key(llama_tiny, key):
    """tgx_set_option refuses a retired key like any unknown one (TGX_ERR_INVALID, "unknown option"), and tgx_get_option does not read it."""
    from tinygpt_amd.ffi import TgxError
    with pytest.raises(TgxError) as e:
        llama_tiny.set_option(key, 0)
    assert e.value.status == 1 and "unknown option" in str(e.value)      # TGX_ERR_INVALID
    with pytest.raises(TgxError) as e:
        llama_tiny.get_option(key)
    assert e.value.status == 1
