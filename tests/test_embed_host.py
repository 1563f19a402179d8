"""Host-only checks of the embedding surface (no GPU): the numpy reference helper of tests/test_hip_embed_rows.py, tgx_cli's --embed flags, and the host engine's
clean refusal on a backend without tgx_embed_rows (the CPU oracle, through the test-hook builds)."""
import ctypes
import subprocess
from ctypes import POINTER, c_float, c_int, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from conftest import load_golden
from embed_ref import identity_head, pool_ref
from host_util import HostEngine, host_lib, write_model_dir
from tinygpt_amd import build, synth
from tinygpt_amd.desc import desc_from_hf_config


def test_pool_ref():
    h = np.array([[3.0, 4.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 2.0]])
    np.testing.assert_array_equal(pool_ref(h, "last", False), [0, 0, 2])
    np.testing.assert_array_equal(pool_ref(h, "first", False), [3, 4, 0])
    np.testing.assert_allclose(pool_ref(h, "mean", False), [4 / 3, 4 / 3, 2 / 3], rtol=1e-15)
    np.testing.assert_allclose(pool_ref(h, "first", True), [0.6, 0.8, 0], rtol=1e-15)
    np.testing.assert_array_equal(pool_ref(h, "first", True, dims=1), [1.0])                  # truncation comes BEFORE normalisation
    np.testing.assert_array_equal(pool_ref(h, "last", True, dims=2), [0, 0])                  # a zero vector stays zero
    v = pool_ref(np.random.default_rng(1).normal(size=(37, 64)), "mean", True, 16)
    assert v.shape == (16,) and abs(np.sqrt((v * v).sum()) - 1) < 1e-12


def test_identity_head_shows_the_hidden_row():
    cfg, g = load_golden("qwen3_tiny")
    d = desc_from_hf_config(cfg, "bf16")
    with pytest.raises(AssertionError):
        identity_head(d, {})                      # a tied description has no lm_head to replace
    d.tied = False
    t = identity_head(d, dict(synth.synth_checkpoint(d, int(g["seed"]), float(g["std"]))))
    W = synth.bf16_bits_to_f32(t["lm_head.weight"])
    assert W.shape == (d.vocab, d.hidden)
    np.testing.assert_array_equal(W[:d.hidden], np.eye(d.hidden, dtype=np.float32))
    assert (W[d.hidden:] == 0).all()


def run_cli(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=120)


def test_cli_embed_flags(tmp_path, oracle_lib):
    _, cli = build.build_host()
    assert "--embed" in run_cli(cli, "--help").stderr and "--embed-dims" in run_cli(cli, "--help").stderr
    for bad, msg in ((["--pool", "median"], "--pool: expected last, mean or first"), (["--embed-dims", "x"], "--embed-dims: expected a component count"),
                     (["--embed-dims", "-3"], "--embed-dims: expected a component count"), (["--embed", "--score"], "--embed does not combine"),
                     (["--embed", "--stream"], "--embed does not combine")):
        out = run_cli(cli, "--synthetic", "gpt2", *bad)
        assert out.returncode == 1 and msg in out.stderr, (bad, out.stderr)
    # the flags reach the engine: on a backend without tgx_embed_rows the call is refused by name, and nothing is printed
    cfg, g = load_golden("qwen2_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    _, tcli = build.build_host(test_hooks=True)
    out = run_cli(tcli, "--model", str(tmp_path), "--backend-lib", oracle_lib.path, "--backend-prefix", "tgxo_", "--embed", "--pool", "mean", "--embed-dims", "8",
                  "--no-normalize", "--prompt-ids", "5,6,7;1,2")
    assert out.returncode == 1 and "embed failed" in out.stderr and "lacks tgx_embed_rows" in out.stderr and out.stdout == "", (out.stdout, out.stderr)


def test_engine_embed_refuses_cleanly_without_the_call(tmp_path, oracle_lib):
    cfg, g = load_golden("qwen2_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    lib = host_lib(test_hooks=True)
    lib.tgxe_embed.argtypes = [c_void_p, c_int, POINTER(c_int32), POINTER(c_int32), c_int, c_int, c_int, POINTER(c_float), POINTER(c_int64)]
    e = HostEngine(lib, model_dir=str(tmp_path), backend_lib=oracle_lib.path, prefix="tgxo_", max_batch=2)
    assert e.prepare(), e.error()
    ids, lens = (c_int32 * 3)(5, 6, 7), (c_int32 * 1)(3)
    out = (c_float * cfg["hidden_size"])(*([7.5] * cfg["hidden_size"]))
    assert lib.tgxe_embed(e.h, 1, ids, lens, 0, 1, 0, out, None) == 1
    assert "lacks tgx_embed_rows" in e.error() and all(v == 7.5 for v in out)
    e.reconfigure(max_new=3)
    got, new, _ = e.generate_sync([[5, 6, 7]])     # the engine still generates
    assert new == 3 and got.shape == (1, 6)
    e.close()
