"""tgx_verify_row_sampled / tgx_read_pass_logits without a GPU: the header, ffi.ABI and the host backend's optional bindings name them; the engine with the CPU
oracle as backend (which exports neither) and GPTConfig::speculateSampled on keeps the old loop; the rule that picks the speculative path (host/spec_mode.h) in a
stand-alone program under the address and undefined-behaviour sanitizers; and the Python restatement of the draw that the GPU tests compute their expected ids
with (tests/verify_sampled_util.py) against OracleModel.sample, so that it is proven here before a GPU test trusts it."""
import ctypes
import os
import re
import subprocess
from ctypes import POINTER, c_float, c_int, c_int64, c_void_p

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from host_util import HostEngine, host_lib, write_model_dir
from tinygpt_amd import build
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import ABI, SamplerCfg
from verify_sampled_util import draw_from_probs, draw_uniform, expected_draw, top_p_band, walk


def test_header_and_ffi_declare_both_functions():
    src = open(os.path.join(ROOT, "include", "tgx.h")).read()
    assert re.search(r"TGX_API int tgx_verify_row_sampled\(tgx_ctx\* ctx, int row, const int64_t\* draft, int n_draft, int64_t\* out_ids[^;]*int32_t\* out_n, int32_t\* out_finish\);", src)
    assert re.search(r"TGX_API int tgx_read_pass_logits\(tgx_ctx\* ctx, float\* out[^;]*int cap_rows, int32_t\* out_rows\);", src)
    assert "#define TGX_ABI_VERSION 3" in src                              # additive
    assert ABI["verify_row_sampled"] == ABI["verify_row"]                  # the same signature
    assert ABI["read_pass_logits"][1][0] is c_void_p and len(ABI["read_pass_logits"][1]) == 4


def test_backend_binds_them_as_optional():
    src = open(os.path.join(ROOT, "tinygpt_amd", "host", "backend.h")).read()
    assert "TGXH_BIND(verify_row_sampled, false)" in src and "TGXH_BIND(read_pass_logits, false)" in src
    assert "(*verify_row_sampled)(tgx_ctx*, int, const int64_t*, int, int64_t*, int32_t*, int32_t*) = nullptr" in src


def spec_stats(e):
    buf = (c_int64 * 32)()
    n = e.lib.tgxe_spec_stats(e.h, buf, 32)
    return list(buf[:n])


def test_engine_on_a_backend_without_the_call_keeps_the_old_loop(oracle_lib, tmp_path):
    """the CPU oracle exports no tgx_verify_row_sampled: with speculate = 7 and speculateSampled on, a sampled run is the run of speculate = 0, and nothing is counted"""
    lib = host_lib(test_hooks=True)
    lib.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    lib.tgxe_set_speculate_sampled.argtypes = [c_void_p, c_int]
    lib.tgxe_spec_stats.restype = c_int
    lib.tgxe_spec_stats.argtypes = [c_void_p, POINTER(c_int64), c_int]
    cfg, g = load_golden("llama_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    e = HostEngine(lib, model_dir=str(tmp_path), backend_lib=oracle_lib.path, prefix="tgxo_", dtype=0, max_batch=4)
    assert e.prepare(), e.error()
    prompt = g["prompt"][0]
    runs = []
    for spec, sampled in ((0, 0), (7, 1)):
        lib.tgxe_set_speculate(e.h, spec)
        lib.tgxe_set_speculate_sampled(e.h, sampled)
        e.reconfigure(temperature=0.8, top_p=0.9, max_new=8)
        ids, new, fin = e.generate_sync([prompt])
        e.reconfigure(temperature=0.8, top_p=0.9, max_new=8)
        aids, anew, afin, seen = e.generate_async(prompt)
        runs.append((ids.tolist(), new, fin, aids.tolist(), anew, afin, seen))
    assert runs[0] == runs[1]
    assert spec_stats(e) == [0] * 21
    e.close()


def test_spec_mode_check_under_sanitizers():
    exe = build.build_spec_mode_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "spec_mode_check: ok" in r.stdout


CONFIGS = [SamplerCfg(1.5, 0, 1.0, 0.0), SamplerCfg(1.5, 40, 1.0, 0.0), SamplerCfg(1.5, 0, 0.9, 0.0), SamplerCfg(1.5, 40, 0.9, 0.0), SamplerCfg(1.5, 0, 1.0, 0.05),
           SamplerCfg(1.5, 40, 0.9, 0.05)]


def test_python_draw_equals_the_oracles(oracle_lib):
    """temperature only, top-k, top-p, top-k + top-p, min-p, all four — at several positions (the oracle's pastLength) and rows, three seeds, on the golden sampler
    logits: draw_uniform + filter_logits + draw_from_probs give OracleModel.sample's id, every time; the draws vary with position, row and seed"""
    from oracle.oracle_ffi import OracleModel
    vec = np.load(os.path.join(GOLDEN, "sampler", "golden.npz"))
    cfg, g = load_golden("llama_tiny")
    d = desc_from_hf_config(dict(cfg, vocab_size=512), "fp32", max_batch=3)        # fp32: the oracle's sampler sees the logits unrounded
    ref = OracleModel(d).load_synthetic(7, 0.05).finalize()
    rng = np.random.default_rng(3)
    rows = np.stack([vec["logits0"], vec["logits0"][::-1].copy(), (rng.standard_normal(512) * 2.5).astype(np.float32)])
    seen = set()
    for past in (1, 6, 19):
        ref.reset_cache()
        ref.forward(rng.integers(0, 512, (3, past)))
        assert ref.past_length == past
        for sc in CONFIGS:
            for seed in (0, 5, 2 ** 40 + 3):
                ref.be.set_logits(ref._ctx, np.ascontiguousarray(rows).ctypes.data_as(POINTER(c_float)), 3); ref.batch = 3
                got = ref.sample(sc, seed=seed)
                for r in range(3):
                    mine, p = expected_draw(sc, rows[r], seed, past, r)
                    assert mine == int(got[r]), (past, sc.temperature, sc.top_k, sc.top_p, sc.min_p, seed, r)
                    assert p[mine] > 0
                    seen.add((past, r, seed, mine))
    assert len({s[3] for s in seen}) >= 8
    ref.close()


def test_draw_helpers_edges():
    p = np.array([0.0, 0.25, 0.0, 0.5, 0.25], np.float32)
    assert draw_from_probs(p, 0.0) == 1 and draw_from_probs(p, 0.2499) == 1 and draw_from_probs(p, 0.25) == 3
    assert draw_from_probs(p, 0.75) == 4 and draw_from_probs(p, 0.9999999) == 4
    assert draw_from_probs(p, 1.0) == 4                                    # rounding left u at the total: the last kept entry
    assert 0.0 <= draw_uniform(1, 2, 3) < 1.0 and draw_uniform(1, 2, 3) != draw_uniform(1, 3, 3) != draw_uniform(1, 3, 2)
    assert walk([5, 6, 7], [5, 6]) == [5, 6, 7] and walk([5, 9, 7], [5, 6]) == [5, 9] and walk([4, 6, 7], [5, 6]) == [4]
    assert top_p_band(SamplerCfg(1.0, 0, 1.0, 0.0), np.zeros(8, np.float32)).size == 0
