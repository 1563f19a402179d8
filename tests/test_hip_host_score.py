"""GPTEngine::score of the host engine (tinygpt_amd/host/engine.h), its C view tgxe_score and tgx_cli --score: the values are tgx_score_row's bits (one prefill pass
on row 0 of a reset cache), the CLI prints them with %.9g — which round-trips a float — and a `ppl` line that is exp(-mean lp) of the printed values.  A device shim
without the symbol (the CPU oracle exports the ABI without tgx_score_row) fails the call with a message; that leg needs no GPU."""
import math
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_void_p

import numpy as np
import pytest

from conftest import load_golden
from host_util import HostEngine, host_lib, write_model_dir
from tinygpt_amd import build
from tinygpt_amd.ffi import MAX_LOGPROBS, Model, product_backend

SEED, STD = 1234, 0.05
IDS = [5, 9, 17, 5, 9, 200, 31, 5, 9, 17, 44, 3, 3, 250, 7, 9, 17, 5, 0, 12]


def bind(h):
    h.tgxe_score.restype = c_int
    h.tgxe_score.argtypes = [c_void_p, POINTER(c_int32), c_int, c_int, POINTER(c_float), POINTER(c_int32), POINTER(c_float)]
    return h


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    cfg, _ = load_golden("llama_tiny")
    path = str(tmp_path_factory.mktemp("score") / "llama_tiny")
    return path, write_model_dir(path, cfg, SEED, STD, eos=255)


def engine_score(lib, e, ids, top_n):
    n = len(ids) - 1
    a = np.asarray(ids, np.int32)
    lp, tid, tlp = np.empty(n, np.float32), np.empty((n, max(top_n, 1)), np.int32), np.empty((n, max(top_n, 1)), np.float32)
    rc = lib.tgxe_score(e.h, a.ctypes.data_as(POINTER(c_int32)), len(a), top_n, lp.ctypes.data_as(POINTER(c_float)), tid.ctypes.data_as(POINTER(c_int32)),
                        tlp.ctypes.data_as(POINTER(c_float)))
    return rc, lp, tid[:, :top_n], tlp[:, :top_n]


def abi_score(d, ids, top_n):
    m = Model(d, product_backend()).load_synthetic(SEED, STD).finalize()
    out = m.score_row(0, np.asarray(ids, np.int64), top_n)
    m.close()
    return out


@pytest.mark.gpu
def test_engine_score_returns_the_abi_calls_bits(model_dir):
    path, d = model_dir
    lib = bind(host_lib())
    e = HostEngine(lib, model_dir=path, max_batch=1)
    assert e.prepare(), e.error()
    e.reconfigure(max_new=4)
    e.generate_sync([IDS[:6]])                                   # the cache holds something else: score starts from a reset cache
    for top_n in (0, 3):
        rc, lp, tid, tlp = engine_score(lib, e, IDS, top_n)
        assert rc == 0, e.error()
        ref = abi_score(d, IDS, top_n)
        np.testing.assert_array_equal(lp, ref[0])
        np.testing.assert_array_equal(tid, ref[1][:, :top_n]); np.testing.assert_array_equal(tlp, ref[2][:, :top_n])
    assert engine_score(lib, e, IDS, MAX_LOGPROBS + 1)[0] == 1 and "alternatives" in e.error()
    out, new, _ = e.generate_sync([IDS[:6]])                     # the engine generates as before afterwards
    assert new == 4
    e.close()


@pytest.mark.gpu
def test_cli_score_prints_the_values_and_the_perplexity(model_dir):
    path, d = model_dir
    _, cli = build.build_host()
    prompts = [IDS, IDS[::-1][:7]]
    arg = ";".join(",".join(str(t) for t in p) for p in prompts)
    out = subprocess.run([cli, "--model", path, "--prompt-ids", arg, "--score", "--logprobs", "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "Output ids" not in out.stdout and "Generated" not in out.stdout      # it generates nothing
    lines = out.stdout.splitlines()
    at = 0
    for p in prompts:
        lp, tid, tlp = abi_score(d, p, 3)
        got = []
        for i in range(len(p) - 1):
            f = lines[at + i].split()
            assert len(f) == 3 + 3 and int(f[0]) == i + 1 and int(f[1]) == p[i + 1], lines[at + i]
            assert np.float32(f[2]) == lp[i], (f[2], lp[i])
            for k in range(3):
                a, b = f[3 + k].split(":")
                assert int(a) == tid[i, k] and np.float32(b) == tlp[i, k], lines[at + i]
            got.append(float(f[2]))
        at += len(p) - 1
        name, ppl = lines[at].split()
        assert name == "ppl"
        assert abs(float(ppl) - math.exp(-sum(float(np.float32(x)) for x in got) / len(got))) <= 1e-7 * float(ppl)
        at += 1
    assert at == len(lines)


@pytest.mark.gpu
def test_text_form_scores_the_tokenizers_ids(tmp_path):
    """GPTEngine::score(text) through tgxe_score_text: the ids are the tokenizer's, the values tgxe_score's of those ids; tgx_cli --score --prompt prints them.
    Without a tokenizer the text form fails with a message"""
    import os
    from ctypes import c_int64
    from conftest import GOLDEN
    from host_util import HostTokenizer
    tok_dir = os.path.join(GOLDEN, "tokenizer", "llama3_style")
    cfg, _ = load_golden("llama_tiny")
    write_model_dir(str(tmp_path), dict(cfg, vocab_size=1280), 77, 0.08)
    lib = bind(host_lib())
    lib.tgxe_score_text.restype = c_int
    lib.tgxe_score_text.argtypes = [c_void_p, c_char_p, c_int, POINTER(c_int32), c_int64, POINTER(c_int64), POINTER(c_float), POINTER(c_int32), POINTER(c_float)]
    text = "The capital of France is Paris, and the capital of Italy is Rome."
    tok = HostTokenizer(lib, tok_dir)
    want = tok.encode(text)
    tok.close()
    assert len(want) >= 8
    e = HostEngine(lib, model_dir=str(tmp_path), tokenizer_dir=tok_dir, max_batch=1)
    assert e.prepare(), e.error()
    ids, n = np.zeros(256, np.int32), c_int64(0)
    lp, tid, tlp = np.empty(255, np.float32), np.empty(255 * 2, np.int32), np.empty(255 * 2, np.float32)
    rc = lib.tgxe_score_text(e.h, text.encode(), 2, ids.ctypes.data_as(POINTER(c_int32)), 256, n, lp.ctypes.data_as(POINTER(c_float)),
                             tid.ctypes.data_as(POINTER(c_int32)), tlp.ctypes.data_as(POINTER(c_float)))
    assert rc == 0, e.error()
    assert ids[:n.value].tolist() == want
    rc, lp2, tid2, tlp2 = engine_score(lib, e, want, 2)
    assert rc == 0
    k = len(want) - 1
    np.testing.assert_array_equal(lp[:k], lp2)
    np.testing.assert_array_equal(tid[:2 * k].reshape(k, 2), tid2); np.testing.assert_array_equal(tlp[:2 * k].reshape(k, 2), tlp2)
    e.close()
    _, cli = build.build_host()
    out = subprocess.run([cli, "--model", str(tmp_path), "--tokenizer", tok_dir, "--prompt", text, "--score"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == k + 1 and lines[-1].startswith("ppl ")
    for i in range(k):
        f = lines[i].split()
        assert len(f) == 3 and int(f[0]) == i + 1 and int(f[1]) == want[i + 1] and np.float32(f[2]) == lp2[i], lines[i]
    bare = HostEngine(lib, model_dir=str(tmp_path), max_batch=1)              # no tokenizer beside the model
    assert bare.prepare(), bare.error()
    assert lib.tgxe_score_text(bare.h, text.encode(), 0, None, 0, None, None, None, None) == 1 and "tokenizer" in bare.error()
    bare.close()


def test_a_shim_without_the_symbol_fails_with_a_message(oracle_lib, tmp_path):
    """the CPU oracle exports the ABI without tgx_score_row: bound through the test-hook build's backend table, score fails cleanly and the engine still generates"""
    lib = bind(host_lib(test_hooks=True))
    cfg, g = load_golden("llama_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    e = HostEngine(lib, model_dir=str(tmp_path), backend_lib=oracle_lib.path, prefix="tgxo_", dtype=0, max_batch=1)
    assert e.prepare(), e.error()
    rc, _, _, _ = engine_score(lib, e, IDS, 0)
    assert rc == 1 and "tgx_score_row" in e.error()
    e.reconfigure(max_new=3)
    _, new, _ = e.generate_sync([IDS[:5]])
    assert new == 3
    e.close()
