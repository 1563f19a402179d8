"""GPTConfig::weightsFp8 in the host engine (tinygpt_amd/host), without a GPU: the loader sets option weights.fp8 between tgx_create and tgx_finalize, and a
backend that cannot take it FAILS prepare() with a message that names the option — the CPU oracle bound through the test-hook build exports no tgx_set_option,
so it is that backend.  Without the flag the same engine prepares and generates as before.  (On the GPU: tests/test_hip_host_fp8.py.)"""
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from fp8_host_util import Fp8Engine
from host_util import HostEngine, host_lib, write_model_dir
from tinygpt_amd import build


@pytest.fixture(scope="module")
def lib():
    return host_lib(test_hooks=True)


def test_a_backend_without_set_option_fails_prepare_with_the_message(lib, oracle_lib, tmp_path):
    cfg, g = load_golden("llama_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    e = Fp8Engine(lib, 1, model_dir=str(tmp_path), backend_lib=oracle_lib.path, prefix="tgxo_")
    assert not e.prepare()
    assert "weights.fp8" in e.error() and "tgx_set_option" in e.error()
    e.close()
    # without the flag: as before, through the new entry point and the old one
    n = g["ids_bf16"].shape[1]
    for eng in (Fp8Engine(lib, 0, model_dir=str(tmp_path), backend_lib=oracle_lib.path, prefix="tgxo_"),
                HostEngine(lib, model_dir=str(tmp_path), backend_lib=oracle_lib.path, prefix="tgxo_", dtype=1)):
        assert eng.prepare(), eng.error()
        eng.reconfigure(max_new=n)
        ids, new, fin = eng.generate_sync([g["prompt"][0]])
        np.testing.assert_array_equal(ids[0, g["prompt"].shape[1]:], g["ids_bf16"][0])
        eng.close()


def test_the_synthetic_load_fails_the_same_way(lib, oracle_lib):
    e = Fp8Engine(lib, 1, synthetic="qwen2.5-0.5b", backend_lib=oracle_lib.path, prefix="tgxo_", max_batch=1)
    assert not e.prepare()
    assert "weights.fp8" in e.error() and "tgx_set_option" in e.error()
    e.close()


def test_cli_flag_fails_loudly_on_such_a_backend(oracle_lib, tmp_path):
    cfg, g = load_golden("llama_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    _, cli = build.build_host(test_hooks=True)
    base = [cli, "--model", str(tmp_path), "--backend-lib", oracle_lib.path, "--backend-prefix", "tgxo_", "--max-tokens", "4", "--temperature", "0", "--top-p", "1",
            "--prompt-ids", "5,6,7"]
    out = subprocess.run(base + ["--weights-fp8"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "weights.fp8" in out.stderr and "Output ids:" not in out.stdout
    out = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.count("Output ids:") == 1, out.stderr
    assert "--weights-fp8" in subprocess.run([cli, "--help"], capture_output=True, text=True).stderr
