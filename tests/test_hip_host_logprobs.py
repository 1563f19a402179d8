"""GPTConfig::logprobs of the host engine (tinygpt_amd/host/engine.h) and tgx_cli --logprobs: the engine steps through the per-row calls, drains the rows' record
rings and returns the ids it returns with logprobs off; its per-token log-probabilities are the ABI-level records of the same generation."""
import ctypes
import re
import subprocess
from ctypes import POINTER, c_float, c_int, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from conftest import load_golden
from host_util import HostEngine, host_lib, write_model_dir
from tinygpt_amd import build
from tinygpt_amd.ffi import GREEDY, Model, SamplerCfg, product_backend

pytestmark = pytest.mark.gpu

SEED, STD = 1234, 0.05
PROMPT = [5, 9, 17, 5, 9, 17, 5, 9, 17, 5, 9]      # (repeats: the prompt-lookup drafter has something to propose)


@pytest.fixture(scope="module")
def lib():
    h = host_lib()
    h.tgxe_set_logprobs.argtypes = [c_void_p, c_int]
    h.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    h.tgxe_last_logprobs.restype = c_int64
    h.tgxe_last_logprobs.argtypes = [c_void_p, POINTER(c_float), POINTER(c_int32), POINTER(c_float), c_int64, POINTER(c_int)]
    return h


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    cfg, _ = load_golden("llama_tiny")
    path = str(tmp_path_factory.mktemp("lp") / "llama_tiny")
    return path, write_model_dir(path, cfg, SEED, STD, eos=255)


def last_logprobs(lib, e, cap=4096):
    lp = np.empty(cap, np.float32)
    ids = np.empty(cap * 20, np.int32)
    tlp = np.empty(cap * 20, np.float32)
    k = c_int(0)
    n = lib.tgxe_last_logprobs(e.h, lp.ctypes.data_as(POINTER(c_float)), ids.ctypes.data_as(POINTER(c_int32)), tlp.ctypes.data_as(POINTER(c_float)), cap, ctypes.byref(k))
    return lp[:n], ids[:n * k.value].reshape(n, k.value), tlp[:n * k.value].reshape(n, k.value)


def abi_records(d, prompts, n_new, cfg, seed, top_n):
    """the same generation through the ABI: forward, sample_row, decode_rows, the rows' records"""
    B = len(prompts)
    d.max_batch = max(d.max_batch, B)
    m = Model(d, product_backend()).load_synthetic(SEED, STD).finalize()
    m.forward(np.asarray(prompts, np.int64))
    for b in range(B):
        m.set_row_sampler(b, cfg, seed)
        m.set_row_logprobs(b, top_n)
        m.sample_row(b, cfg, seed)
    top = float(np.abs(m.logits(rounded=False)).max())
    for _ in range(n_new - 1):                                  # (step by step: the largest |logit| of the generation bounds what kernel paths may differ by)
        m.decode_rows(1)
        top = max(top, float(np.abs(m.logits(rounded=False)).max()))
    return [m.row_logprobs(b, n_new) for b in range(B)], top


@pytest.mark.parametrize("sampler", [dict(), dict(temperature=0.8, top_p=0.9)])
def test_generate_sync_logprobs(lib, model_dir, sampler):
    path, d = model_dir
    prompts = [PROMPT, PROMPT[::-1]]
    n_new = 12
    e = HostEngine(lib, model_dir=path, max_batch=2)
    assert e.prepare(), e.error()
    e.reconfigure(max_new=n_new, **sampler)
    off, _, _ = e.generate_sync(prompts)
    assert len(last_logprobs(lib, e)[0]) == 0
    lib.tgxe_set_logprobs(e.h, 3)
    e.reconfigure(max_new=n_new, **sampler)
    on, new, _ = e.generate_sync(prompts)
    np.testing.assert_array_equal(on, off)                      # the ids it returns with logprobs off
    lp, ids, tlp = last_logprobs(lib, e)
    assert new == n_new and lp.shape == (2 * n_new,) and ids.shape == (2 * n_new, 3)
    cfg = SamplerCfg(sampler.get("temperature", 0.0), 0, sampler.get("top_p", 1.0), 0.0)
    recs, _ = abi_records(d, prompts, n_new, cfg, 0, 3)
    for b in range(2):
        np.testing.assert_array_equal(lp[b * n_new:(b + 1) * n_new], recs[b][0])
        np.testing.assert_array_equal(ids[b * n_new:(b + 1) * n_new], recs[b][1][:, :3])
        np.testing.assert_array_equal(tlp[b * n_new:(b + 1) * n_new], recs[b][2][:, :3])
    e.close()


def test_speculate_and_async_logprobs(lib, model_dir):
    """speculate = 4: the records come from tgx_verify_row's positions — the ids are the plain loop's, the log-probabilities agree with the step-by-step records
    inside the bound between kernel paths (tests/test_hip_logprobs.py)"""
    path, d = model_dir
    n_new = 24
    e = HostEngine(lib, model_dir=path, max_batch=1)
    assert e.prepare(), e.error()
    e.reconfigure(max_new=n_new)
    off, _, _ = e.generate_sync([PROMPT])
    lib.tgxe_set_logprobs(e.h, 3)
    lib.tgxe_set_speculate(e.h, 4)
    e.reconfigure(max_new=n_new)
    on, new, _ = e.generate_sync([PROMPT])
    np.testing.assert_array_equal(on, off)
    lp, ids, tlp = last_logprobs(lib, e)
    assert new == n_new and lp.shape == (n_new,)
    recs, top = abi_records(d, [PROMPT], n_new, GREEDY, 0, 3)
    rec = recs[0]
    np.testing.assert_allclose(lp, rec[0], rtol=0, atol=2 * 1e-3 * top + 2e-5)
    assert (lp <= 0).all()
    # generateAsync: the same tokens, one record per new token
    lib.tgxe_set_speculate(e.h, 0)
    e.reconfigure(max_new=n_new)
    toks, new_a, _, _ = e.generate_async(PROMPT)
    lp_a, _, _ = last_logprobs(lib, e)
    assert len(lp_a) == new_a
    np.testing.assert_array_equal(toks[len(PROMPT):], off[0, len(PROMPT):len(PROMPT) + new_a])
    np.testing.assert_array_equal(lp_a, rec[0][:new_a])
    e.close()


def test_unservable_request_fails(lib, model_dir):
    """more alternatives than TGX_MAX_LOGPROBS: the generate call fails with a message instead of generating without the lists"""
    path, _ = model_dir
    e = HostEngine(lib, model_dir=path, max_batch=1)
    assert e.prepare(), e.error()
    lib.tgxe_set_logprobs(e.h, 21)
    e.reconfigure(max_new=4)
    with pytest.raises(AssertionError, match="logprobs"):
        e.generate_sync([PROMPT])
    with pytest.raises(AssertionError, match="logprobs"):
        e.generate_async(PROMPT)
    lib.tgxe_set_logprobs(e.h, 20)
    e.reconfigure(max_new=4)
    out, new, _ = e.generate_sync([PROMPT])
    assert new == 4 and last_logprobs(lib, e)[1].shape == (4, 20)
    e.close()


def test_cli_prints_one_line_per_token(model_dir):
    path, _ = model_dir
    _, cli = build.build_host()
    out = subprocess.run([cli, "--model", path, "--prompt-ids", "5,9,17,5;7,7,7,7", "--max-tokens", "6", "--temperature", "0", "--top-p", "1", "--logprobs", "2"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("logprob row ")]
    assert len(lines) == 2 * 6
    for l in lines:
        m = re.match(r"logprob row (\d+) token (\d+) id (\d+): (-?[\d.]+) \| (\d+):(-?[\d.]+) (\d+):(-?[\d.]+)$", l)
        assert m, l
        assert float(m.group(4)) <= 0 and float(m.group(6)) >= float(m.group(8))
        if int(m.group(3)) == int(m.group(5)):                  # greedy: the produced token is the most likely one
            assert abs(float(m.group(4)) - float(m.group(6))) < 1e-6
    without = subprocess.run([cli, "--model", path, "--prompt-ids", "5,9,17,5;7,7,7,7", "--max-tokens", "6", "--temperature", "0", "--top-p", "1"], capture_output=True, text=True, timeout=120)
    assert "logprob row" not in without.stdout
    ids = lambda s: [l for l in s.splitlines() if l.startswith("Output ids:")]
    assert ids(out.stdout) == ids(without.stdout)
