"""Greedy speculative decoding without a GPU: the prompt-lookup drafter (tinygpt_amd/host/spec_draft.h) through the host library's C view, the same drafter in a
stand-alone program under the address and undefined-behaviour sanitizers (tests/spec_draft_check.cpp), and the engine's rule that GPTConfig::speculate changes
nothing where it does not apply (a backend without tgx_verify_row — the CPU oracle — or a sampler configuration that is not greedy)."""
import ctypes
import subprocess
from ctypes import POINTER, c_int, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from conftest import load_golden
from host_util import HostEngine, host_lib, write_model_dir
from tinygpt_amd import build


@pytest.fixture(scope="module")
def lib():
    lib = host_lib(test_hooks=True)
    lib.tgxh_ngram_draft.restype = c_int
    lib.tgxh_ngram_draft.argtypes = [POINTER(c_int32), c_int, c_int, POINTER(c_int32)]
    lib.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    lib.tgxe_spec_stats.restype = c_int
    lib.tgxe_spec_stats.argtypes = [c_void_p, POINTER(c_int64), c_int]
    return lib


def draft(lib, seq, max_draft):
    ids = np.ascontiguousarray(np.asarray(seq, np.int32))
    out = (c_int32 * 16)()
    ptr = ids.ctypes.data_as(POINTER(c_int32)) if len(ids) else None
    n = lib.tgxh_ngram_draft(ptr, len(ids), max_draft, out)
    assert 0 <= n <= max(0, min(max_draft, 15))
    return list(out[:n])


def spec_stats(e):
    buf = (c_int64 * 32)()
    n = e.lib.tgxe_spec_stats(e.h, buf, 32)
    assert n == 4 + 17
    return list(buf[:n])


CASES = [
    ("no match -> empty", [1, 2, 3, 4, 5], 7, []),
    ("a sequence of length 1", [5], 7, []),
    ("an empty sequence", [], 7, []),
    # the suffix [1, 2, 3] occurs at 0 (followed by 9, 8); its last token alone also occurs later, at 6 (followed by 6): the longer match decides
    ("longest suffix wins over a shorter, more recent one", [1, 2, 3, 9, 8, 7, 3, 6, 1, 2, 3], 2, [9, 8]),
    ("most recent occurrence wins", [4, 5, 10, 4, 5, 20, 4, 5], 1, [20]),
    ("clipped by max_draft", [1, 2, 3, 4, 5, 6, 7, 1, 2, 3], 3, [4, 5, 6]),
    ("clipped by the end of the sequence", [1, 2, 3, 4, 1, 2, 3], 15, [4, 1, 2, 3]),
    # the only occurrence of every suffix is the suffix itself, which ends at the sequence end: nothing follows it
    ("a match that ends at the sequence end proposes nothing", [1, 2, 3], 7, []),
    ("an earlier occurrence may overlap the suffix", [7, 7, 7, 7], 5, [7]),
    ("max_draft 0", [1, 2, 1, 2], 0, []),
]


@pytest.mark.parametrize("what,seq,max_draft,want", CASES, ids=[c[0] for c in CASES])
def test_ngram_draft(lib, what, seq, max_draft, want):
    assert draft(lib, seq, max_draft) == want, what


def test_ngram_draft_against_definition(lib):
    """random sequences over small alphabets (many repeats) against the definition spelled out: every suffix length from 3 down, every earlier start from the latest"""
    def naive(seq, md):
        n = len(seq)
        for k in (3, 2, 1):
            for s in range(n - k - 1, -1, -1):
                if seq[s:s + k] == seq[n - k:]:
                    return seq[s + k:s + k + md]
        return []
    rng = np.random.default_rng(7)
    for _ in range(500):
        seq = rng.integers(0, int(rng.integers(2, 6)), size=int(rng.integers(0, 40))).tolist()
        md = int(rng.integers(1, 16))
        assert draft(lib, seq, md) == naive(seq, md), (seq, md)


def test_spec_draft_check_under_sanitizers():
    exe = build.build_spec_draft_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "spec_draft_check: ok" in r.stdout


def make_engine(lib, oracle_lib, tmp_path, eos=None):
    cfg, g = load_golden("llama_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]), eos=eos)
    e = HostEngine(lib, model_dir=str(tmp_path), backend_lib=oracle_lib.path, prefix="tgxo_", dtype=0, max_batch=4)
    assert e.prepare(), e.error()
    return e, g


def test_speculate_without_verify_row_keeps_the_old_loop(lib, oracle_lib, tmp_path):
    """the CPU oracle exports no tgx_verify_row: with speculate = 7 generateSync and generateAsync produce the golden ids and callbacks, and nothing was drafted"""
    e, g = make_engine(lib, oracle_lib, tmp_path, eos=[2, 999])
    gold, prompt = g["ids_fp32"][0], g["prompt"][0]
    n = len(gold)
    lib.tgxe_set_speculate(e.h, 7)
    e.reconfigure(max_new=n)
    ids, new, fin = e.generate_sync([prompt])
    assert new == n and fin == "length"
    np.testing.assert_array_equal(ids[0, len(prompt):], gold)
    e.reconfigure(max_new=n)
    ids, new, fin, seen = e.generate_async(prompt)
    assert fin == "length" and seen == list(gold[:n - 1]) and new == n
    np.testing.assert_array_equal(ids[len(prompt):], gold)
    stop = int(gold[5])
    k = list(gold).index(stop)
    e.reconfigure(max_new=n, extra_stop=[stop])
    ids, new, fin, seen = e.generate_async(prompt)
    assert fin == "stop" and seen == list(gold[:k])
    assert spec_stats(e) == [0] * 21
    e.close()


def test_speculate_with_a_sampling_configuration_keeps_the_old_loop(lib, oracle_lib, tmp_path):
    """speculate applies to greedy generation only: a sampled run is the same run with and without it"""
    e, g = make_engine(lib, oracle_lib, tmp_path)
    prompt = g["prompt"][0]
    runs = []
    for spec in (0, 7):
        lib.tgxe_set_speculate(e.h, spec)
        e.reconfigure(temperature=0.8, top_p=0.9, max_new=8)
        ids, new, fin = e.generate_sync([prompt])
        e.reconfigure(temperature=0.8, top_p=0.9, max_new=8)
        aids, anew, afin, seen = e.generate_async(prompt)
        runs.append((ids.tolist(), new, fin, aids.tolist(), anew, afin, seen))
    assert runs[0] == runs[1]
    assert spec_stats(e) == [0] * 21
    e.close()
