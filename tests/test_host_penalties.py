"""SamplerConfig's penalties / logit bias on a backend without the per-row processor calls (the CPU oracle, bound through the test-hook build): a non-neutral
request FAILS the generate call with a message — never plain generation with the request dropped — and the neutral one runs as before (no GPU)."""
from ctypes import POINTER, c_float, c_int, c_int32, c_void_p

import numpy as np
import pytest

from conftest import load_golden
from host_util import HostEngine, host_lib, write_model_dir


@pytest.fixture(scope="module")
def lib():
    h = host_lib(test_hooks=True)
    h.tgxe_set_processors.argtypes = [c_void_p, c_float, c_float, c_float, POINTER(c_int32), POINTER(c_float), c_int]
    return h


def set_processors(lib, e, repetition=1.0, presence=0.0, frequency=0.0, bias=None):
    ids = np.asarray(list((bias or {}).keys()), np.int32)
    val = np.asarray(list((bias or {}).values()), np.float32)
    lib.tgxe_set_processors(e.h, repetition, presence, frequency, ids.ctypes.data_as(POINTER(c_int32)), val.ctypes.data_as(POINTER(c_float)), len(ids))


def test_non_neutral_request_fails_on_a_backend_without_the_calls(lib, oracle_lib, tmp_path):
    cfg, g = load_golden("llama_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    e = HostEngine(lib, model_dir=str(tmp_path), backend_lib=oracle_lib.path, prefix="tgxo_", dtype=0, max_batch=2)
    assert e.prepare(), e.error()
    prompt = [int(t) for t in g["prompt"][0]]
    e.reconfigure(max_new=6)
    plain, new, fin = e.generate_sync([prompt])
    assert new == 6
    for kw in (dict(repetition=1.3), dict(presence=0.5), dict(frequency=-0.25), dict(bias={7: float("-inf")})):
        set_processors(lib, e, **kw)
        e.reconfigure(max_new=6)                       # (the processors stay across a reconfigure)
        with pytest.raises(AssertionError, match="penalties / logit bias: the device shim lacks"):
            e.generate_sync([prompt])
        with pytest.raises(AssertionError, match="penalties / logit bias: the device shim lacks"):
            e.generate_async(prompt)
    set_processors(lib, e)                             # neutral: the existing loops, the same ids
    e.reconfigure(max_new=6)
    again, new, fin = e.generate_sync([prompt])
    np.testing.assert_array_equal(again, plain)
    e.reconfigure(max_new=6)
    one, _, _, _ = e.generate_async(prompt)
    np.testing.assert_array_equal(one, plain[0])
    e.close()


@pytest.mark.parametrize("arg", ["x:1", "5:abc", "5", ":1", "5:", "-3:1", "5:1,7"])
def test_cli_refuses_a_logit_bias_that_does_not_parse(arg):
    import subprocess
    from tinygpt_amd import build
    _, cli = build.build_host()
    out = subprocess.run([cli, "--synthetic", "llama-3.2-1b", "--logit-bias", arg], capture_output=True, text=True)
    assert out.returncode == 1 and "--logit-bias" in out.stderr
