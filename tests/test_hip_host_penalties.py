"""SamplerConfig's penalties and logit bias in the host engine (tinygpt_amd/host/engine.h): the engine steps through the per-row calls, seeds every row's history
from the prompt it admitted (left padding not counted), and its ids are the argmax of the float32 restatement (tests/logit_proc_ref.py) over the model's raw
logits — checked against the ffi model on the same synthetic checkpoint.  With the neutral defaults the existing loop's ids come back, before and after."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_int32, c_void_p

import numpy as np
import pytest

from conftest import load_golden
from host_util import HostEngine, host_lib, write_model_dir
from logit_proc_ref import argmax_lowest, count, history, process_np
from tinygpt_amd.ffi import GREEDY, Model, product_backend

pytestmark = pytest.mark.gpu

SEED, STD = 1234, 0.05
PROMPTS = [[5, 9, 17, 5, 9, 17, 5, 9, 17, 5, 9], [200, 31, 8, 77, 31, 8]]      # unequal lengths: the second is left-padded with id 0
N_NEW = 14


@pytest.fixture(scope="module")
def lib():
    h = host_lib()
    h.tgxe_set_processors.argtypes = [c_void_p, c_float, c_float, c_float, POINTER(c_int32), POINTER(c_float), c_int]
    return h


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    cfg, _ = load_golden("llama_tiny")
    path = str(tmp_path_factory.mktemp("pen") / "llama_tiny")
    return path, write_model_dir(path, cfg, SEED, STD, eos=255)


def set_processors(lib, e, repetition=1.0, presence=0.0, frequency=0.0, bias=None):
    ids = np.asarray(list((bias or {}).keys()), np.int32)
    val = np.asarray(list((bias or {}).values()), np.float32)
    lib.tgxe_set_processors(e.h, repetition, presence, frequency, ids.ctypes.data_as(POINTER(c_int32)), val.ctypes.data_as(POINTER(c_float)), len(ids))


def padded(prompts, pad=0):
    S = max(len(p) for p in prompts)
    return np.asarray([[pad] * (S - len(p)) + list(p) for p in prompts], np.int64)


def test_engine_ids_follow_the_restatement(lib, model_dir):
    path, d = model_dir
    e = HostEngine(lib, model_dir=path, max_batch=2)
    assert e.prepare(), e.error()
    e.reconfigure(max_new=N_NEW)
    plain, new, _ = e.generate_sync(PROMPTS)
    S = plain.shape[1] - N_NEW
    # the existing loop: forward, sample, decode on the ffi model
    d.max_batch = max(d.max_batch, 2)
    m = Model(d, product_backend()).load_synthetic(SEED, STD).finalize()
    m.forward(padded(PROMPTS))
    first = m.sample(GREEDY)
    np.testing.assert_array_equal(plain[:, S:], np.concatenate([first[None], m.decode(N_NEW - 1)]).T)
    # repetition 1.3 and row 0's first plain token banned
    ban = int(plain[0, S])
    rep, bias = 1.3, {ban: float("-inf"), 3: 0.5}
    set_processors(lib, e, repetition=rep, bias=bias)
    e.reconfigure(max_new=N_NEW)
    got, new, fin = e.generate_sync(PROMPTS)
    assert new == N_NEW and fin == "length" and ban not in got[:, S:]
    np.testing.assert_array_equal(got[:, :S], plain[:, :S])
    m.reset_cache()
    m.forward(padded(PROMPTS))
    words = [history(m.desc.vocab, prompt_ids=p) for p in PROMPTS]          # the prompts as supplied: no pad token
    raw = m.logits(rounded=False)
    for b in range(2):
        assert int(got[b, S]) == argmax_lowest(process_np(raw[b], words[b], rep, 0.0, 0.0, bias)), b
        m.set_row_penalties(b, rep).set_row_logit_bias(b, bias).set_row_history(b, prompt_ids=PROMPTS[b])
        assert m.sample_row(b, GREEDY) == int(got[b, S])
        m.set_row_sampler(b, GREEDY)
    for i in range(1, N_NEW):
        for b in range(2):
            count(words[b], got[b, S + i - 1])
        ids, _, _ = m.decode_rows(1)
        raw = m.logits(rounded=False)
        for b in range(2):
            assert int(got[b, S + i]) == int(ids[0, b]) == argmax_lowest(process_np(raw[b], words[b], rep, 0.0, 0.0, bias)), (i, b)
    # one streamed sequence under the same settings: the ids of the one-prompt generateSync
    e.reconfigure(max_new=N_NEW)
    solo, _, _ = e.generate_sync([PROMPTS[0]])
    assert ban not in solo[0, len(PROMPTS[0]):]
    e.reconfigure(max_new=N_NEW)
    one, new, _, seen = e.generate_async(PROMPTS[0])
    np.testing.assert_array_equal(one, solo[0])
    # neutral again: the rows were switched back, the existing loop's ids return
    set_processors(lib, e)
    e.reconfigure(max_new=N_NEW)
    again, _, _ = e.generate_sync(PROMPTS)
    np.testing.assert_array_equal(again, plain)
    e.close()
