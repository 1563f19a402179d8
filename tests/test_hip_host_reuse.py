"""GPTConfig::reusePrefix of the host engine (tinygpt_amd/host/engine.h): generateAsync keeps row 0's KV cache between calls and prefills only what follows the
longest prefix the new prompt shares with it (tgx_truncate_row + tgx_extend_row).  Three turns of a conversation on two engines, the switch on and off: the ids and
finish reasons are equal, and tgxe_last_reused shows that the reuse path ran (peaked synthetic checkpoint: no greedy choice sits on a near-tie)."""
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest

from conftest import load_golden
from host_util import HostEngine, host_lib, write_model_dir

pytestmark = pytest.mark.gpu


def test_three_turns_with_and_without_prefix_reuse(tmp_path):
    cfg, g = load_golden("mistral_tiny")                         # an untied lm_head (where the peaked checkpoint's loud rows live) and a context of 128: room for three turns
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]), peaked=True)
    lib = host_lib()
    lib.tgxe_set_reuse_prefix.argtypes = [c_void_p, c_int]
    lib.tgxe_set_reuse_prefix.restype = None
    lib.tgxe_last_reused.argtypes = [c_void_p]
    lib.tgxe_last_reused.restype = c_int64
    engines = []
    for on in (1, 0):
        e = HostEngine(lib, model_dir=str(tmp_path), device="mi355x", dtype=1, max_batch=1)
        assert e.prepare(), e.error()
        lib.tgxe_set_reuse_prefix(e.h, on)
        engines.append(e)
    V = int(cfg["vocab_size"])
    rng = np.random.default_rng(21)
    prompt1 = rng.integers(3, V, 40).astype(np.int32)
    outs = {}

    def turn(name, prompt):
        res = []
        for e in engines:
            e.reconfigure(max_new=12)
            ids, new, fin, seen = e.generate_async(prompt)
            res.append((ids.copy(), new, fin, seen, int(lib.tgxe_last_reused(e.h))))
        (i1, n1, f1, s1, r1), (i0, n0, f0, s0, r0) = res
        np.testing.assert_array_equal(i1, i0, err_msg=name)
        assert (n1, f1, s1) == (n0, f0, s0), name
        assert r0 == 0, name                                      # the switch off: nothing is ever served from the cache
        outs[name] = i1
        return r1

    assert turn("turn 1", prompt1) == 0
    new1 = outs["turn 1"][len(prompt1):]
    prompt2 = np.concatenate([prompt1, new1, rng.integers(3, V, 20).astype(np.int32)])
    r2 = turn("turn 2", prompt2)
    assert r2 > 0 and r2 >= len(prompt2) - 20 - 1, r2             # everything but the last generated token (never fed back) and the new text
    prompt3 = prompt2.copy(); prompt3[30] = (prompt3[30] + 1) % V
    assert turn("turn 3", prompt3) == 30
    # generateSync takes the reset path and the next generateAsync starts from nothing
    for e in engines:
        e.reconfigure(max_new=3)
        e.generate_sync([prompt1], pad=0)
    assert turn("turn 4", prompt1) == 0
    for e in engines:
        e.close()
