"""GPTConfig::contextShift of the host engine (tinygpt_amd/host/engine.h): generation past the context.  A row whose next step would exceed contextSize() keeps its
first shiftKeep positions, drops half of the rest, slides the tail down (include/tgx.h tgx_splice_row), is fed its current token again and goes on.  A synthetic
2-layer model with a context of 256 generates 700 tokens greedily; the ids must equal a Python driver that makes the same splice / extend / sample / decode calls
through tinygpt_amd/ffi.py, the produced count stops exactly at maxNewTokens, and with the switch off the run ends at the context as before.  (Peaked synthetic
checkpoint: the winners are its loud lm_head rows, and the EOS id of the fixture is none of them, so no run ends early.)
generateSync left-pads its prompts to one length, so the rows of a call hold the same number of positions at every step and fill up together: the two-row case
runs the per-row branches of the engine's loop in lock-step only — one row shifting while another does not, and the room taken over rows of different length, are
states generateSync cannot reach without a regex that ends a row early, and are not run here.  A shiftKeep that leaves nothing to discard fails with a message."""
import copy
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest

from conftest import load_golden
from host_util import HostEngine, host_lib, write_model_dir
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, Model

pytestmark = pytest.mark.gpu
CTX, KEEP, RING_HALF = 256, 4, 128


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    cfg, g = load_golden("mistral_tiny")
    cfg = copy.deepcopy(cfg); cfg["max_position_embeddings"] = CTX
    path = str(tmp_path_factory.mktemp("shift_model"))
    write_model_dir(path, cfg, int(g["seed"]), float(g["std"]), peaked=True, eos=5)      # (id 2 is one of this seed's loud rows; 5 is not)
    lib = host_lib()
    lib.tgxe_set_context_shift.argtypes = [c_void_p, c_int, c_int]
    lib.tgxe_set_context_shift.restype = None
    lib.tgxe_last_shifts.argtypes = [c_void_p]
    lib.tgxe_last_shifts.restype = c_int64
    return cfg, g, path, lib


def driver_model(cfg, g, batch):
    d = desc_from_hf_config(cfg, "bf16", max_batch=batch)
    assert d.max_ctx == CTX
    return Model(d).load_synthetic(int(g["seed"]), float(g["std"]), peaked=True).finalize()


def shift(m, row, cur):
    """the engine's rule: n_keep = min(shiftKeep, past - 1), n_discard = (past - n_keep) / 2; the current token fed again; the next one sampled"""
    past = m.past_length_row(row)
    n_keep = min(KEEP, past - 1); n_discard = (past - n_keep) // 2
    ranges = ([(0, n_keep)] if n_keep else []) + [(n_keep + n_discard, past - n_keep - n_discard)]
    assert m.splice_row(row, ranges) == past - n_discard
    m.extend_row(row, [cur])
    return int(m.sample_row(row, GREEDY))


def test_generate_async_past_the_context(setup):
    cfg, g, path, lib = setup
    V, S, NEW = int(cfg["vocab_size"]), 40, 700
    prompt = np.random.default_rng(4).integers(6, V, S).astype(np.int32)
    eng = HostEngine(lib, model_dir=path, device="mi355x", dtype=1, max_batch=1)
    assert eng.prepare(), eng.error()
    assert lib.tgxe_context_size(eng.h) == CTX
    eos = eng.eos_ids()
    assert eos == [5]
    # the switch off: the run ends at the context, as before
    eng.reconfigure(max_new=NEW)
    ids0, new0, _, _ = eng.generate_async(prompt)
    assert new0 < NEW and len(ids0) <= CTX + 2 and lib.tgxe_last_shifts(eng.h) == 0
    lib.tgxe_set_context_shift(eng.h, 1, KEEP)
    eng.reconfigure(max_new=NEW)                                  # (resets the cache, as before every request)
    ids, new, fin, seen = eng.generate_async(prompt)
    shifts = int(lib.tgxe_last_shifts(eng.h))
    eng.close()
    assert new == NEW and len(ids) == S + NEW and fin == "length", (new, fin)
    assert seen == list(ids[S:-1])                                # every token but the last is reported
    np.testing.assert_array_equal(ids[:CTX - 8], ids0[:CTX - 8])  # up to the context the two runs are the same run
    # ---- the driver
    m = driver_model(cfg, g, 1)
    m.forward(prompt[None, :].astype(np.int64))
    m.set_row_sampler(0, GREEDY, 0)
    seq = [int(t) for t in prompt] + [int(m.sample_row(0, GREEDY))]
    m.set_row_stop(0, NEW - 1, eos)
    n_shifts, finished = 0, False
    while len(seq) - S < NEW and not finished:
        if m.past_length_row(0) >= CTX:
            seq.append(shift(m, 0, seq[-1])); n_shifts += 1
            rem = S + NEW - len(seq)
            if rem <= 0:
                finished = True
            else:
                m.set_row_stop(0, rem, eos)
        else:
            out, made, f = m.decode_rows(1)
            seq += [int(t) for t in out[:made[0], 0]]
            finished = f[0] != 0
    m.close()
    assert n_shifts == shifts >= 3, (n_shifts, shifts)
    np.testing.assert_array_equal(ids, np.asarray(seq, np.int32))


def test_a_keep_that_leaves_nothing_to_discard_fails_with_a_message(setup):
    cfg, g, path, lib = setup
    prompt = np.random.default_rng(4).integers(6, int(cfg["vocab_size"]), 40).astype(np.int32)
    eng = HostEngine(lib, model_dir=path, device="mi355x", dtype=1, max_batch=1)
    assert eng.prepare(), eng.error()
    lib.tgxe_set_context_shift(eng.h, 1, CTX)
    eng.reconfigure(max_new=300)
    ids, new, fin, seen = eng.generate_async(prompt)          # ends where the first shift would have been
    assert new < 300 and len(ids) <= CTX + 2 and lib.tgxe_last_shifts(eng.h) == 0
    assert "shiftKeep" in eng.error(), eng.error()
    eng.close()


def test_generate_sync_two_rows_past_the_context(setup):
    cfg, g, path, lib = setup
    V, NEW = int(cfg["vocab_size"]), 300
    rng = np.random.default_rng(6)
    prompts = [rng.integers(6, V, 40).astype(np.int32), rng.integers(6, V, 25).astype(np.int32)]
    eng = HostEngine(lib, model_dir=path, device="mi355x", dtype=1, max_batch=2)
    assert eng.prepare(), eng.error()
    lib.tgxe_set_context_shift(eng.h, 1, KEEP)
    eng.reconfigure(max_new=NEW)
    ids, new, fin = eng.generate_sync(prompts, pad=0)
    shifts = int(lib.tgxe_last_shifts(eng.h))
    eng.close()
    S = 40
    assert ids.shape == (2, S + NEW) and new == NEW and fin == "length"
    # ---- the driver: the rows with their length on the device, never more steps per call than the fullest row has room for
    B, n_more = 2, NEW - 1
    padded = np.zeros((B, S), np.int64)
    for b, p in enumerate(prompts):
        padded[b, S - len(p):] = p
    np.testing.assert_array_equal(ids[:, :S], padded)
    m = driver_model(cfg, g, B)
    m.forward(padded)
    cur, got, over, n_shifts = [], [[] for _ in range(B)], [False] * B, 0
    for b in range(B):
        m.set_row_sampler(b, GREEDY, 0)
        cur.append(int(m.sample_row(b, GREEDY)))

    def restate(b):
        rem = n_more - len(got[b])
        if rem <= 0:
            over[b] = True; m.reset_row(b)
        else:
            m.set_row_stop(b, rem)

    for b in range(B):
        restate(b)
    first = list(cur)
    while not all(over):
        room = RING_HALF
        for b in range(B):
            if over[b]:
                continue
            if m.past_length_row(b) >= CTX:
                cur[b] = shift(m, b, cur[b]); got[b].append(cur[b]); n_shifts += 1
                restate(b)
                if over[b]:
                    continue
            room = min(room, CTX - m.past_length_row(b), n_more - len(got[b]))
        if all(over):
            break
        out, made, f = m.decode_rows(max(1, room))
        for b in range(B):
            if over[b]:
                continue
            got[b] += [int(t) for t in out[:made[b], b]]
            cur[b] = got[b][-1]
            over[b] = f[b] != 0
    m.close()
    assert n_shifts == shifts >= 2, (n_shifts, shifts)
    for b in range(B):
        np.testing.assert_array_equal(ids[b, S:], np.asarray([first[b]] + got[b], np.int32), err_msg=str(b))
