"""The row fuzzer without a GPU: tests/row_model.py's driver on OracleDevice (the row calls answered from the model of include/tgx.h plus one CPU oracle per row), for
the seeds and arms tests/test_hip_row_fuzz.py runs on the device.  It checks the model against itself, the two conditions on the inputs that the GPU bounds rest on
(the oracle against its reordered twin), that the seed set still reaches every state the fuzzer is there for, and the block figures of two scripted GPU tests on
the model alone."""
import os

import numpy as np
import pytest

import row_model as rm
from row_model import BLK, CONTEXT, OK, RowModel

SEEDS = list(range(int(os.environ.get("TGX_FUZZ_SEEDS_ROWS", "8"))))
N_OPS = 40
BOUND = {"f32_slab": 1e-4, "h16_slab": 1e-2, "h16_paged": 1e-2}
FLOOR = {"f32_slab": 1e-5, "h16_slab": 1e-2 / 3, "h16_paged": 1e-2 / 3}      # the oracle against its reordered twin: what the inputs must stay below
_done = {}


def dry_run(seed, arm, device_cls=rm.OracleDevice):
    k = rm.case(seed, arm)
    dev = device_cls(k["fam"], k["dtype"], k["max_batch"], k["max_ctx"], k["budget"])
    aux_budget = 0 if k["budget"] else (0 if arm == "f32_slab" else 4 * BLK)      # the second context has the other cache layout (fp32 storage has no paged cache)
    aux = device_cls(k["fam"], k["dtype"], 3, k["max_ctx"], aux_budget)
    model = RowModel(k["max_batch"], k["max_ctx"], dev.desc.vocab, k["budget"])
    aux_model = RowModel(3, k["max_ctx"], dev.desc.vocab, aux_budget)
    return rm.run_sequence(dev, model, k["rng"], N_OPS, fam=k["fam"], dtype=k["dtype"], bound=BOUND[arm], aux=(aux, aux_model), tag=f"seed {seed} {arm} {k['fam']} {k['dtype']}")


def stats_of(seed, arm):
    if (seed, arm) not in _done:
        _done[(seed, arm)] = dry_run(seed, arm)
    return _done[(seed, arm)]


@pytest.mark.parametrize("arm", rm.ARMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_the_driver_runs_clean_on_the_oracle_device(seed, arm, oracle_lib):
    s = stats_of(seed, arm)
    print(f"row_fuzz dry seed {seed} {arm}: {s.line()}")
    assert s.floor < FLOOR[arm], f"the oracle is {s.floor:.3e} from its reordered twin on this sequence: pick another seed or shorter rows, the bound stays"
    assert s.greedy and s.compared >= 0.7 * s.greedy, f"only {s.compared} of {s.greedy} greedy ids had a clear top-2 gap"


def test_the_seed_set_reaches_what_the_fuzzer_is_for(oracle_lib):
    if len(SEEDS) < 8:
        return      # the coverage conditions are stated for the 8 default seeds
    acc, ref, classes, cov = {}, {}, {}, {}
    for seed in SEEDS:
        for arm in rm.ARMS:
            s = stats_of(seed, arm)
            for src, dst in ((s.accepted, acc), (s.refused, ref), (s.classes, classes), (s.cov, cov)):
                for k, v in src.items():
                    dst[k] = dst.get(k, 0) + v
    print("accepted", acc, "\nrefused", ref, "\nclasses", classes, "\ncoverage", cov)
    for kind in rm.Driver.KINDS:
        assert acc.get(kind, 0) >= 1, f"{kind} was never accepted"
        assert ref.get(kind, 0) >= 1, f"{kind} was never refused"
    for cls in ["forward_row:target_live", "sample_row:truncated", "fork_row:truncated", "decode_rows:truncated", "extend_row:extend_retired", "verify_row:no_token",
                "verify_row:sampled_row", "save_row:save_finished", "restore_row:target_live", "forward_row:new_row_not_batch", "extend_row:max_ctx"]:
        assert classes.get(cls, 0) >= 1, f"the refusal class {cls} never occurred"
    assert any(k.endswith(":pool") for k in classes), "the pool was never exhausted"
    for what in ["fork_no_tail", "fork_tail", "cow_truncation", "decode_rows_crosses_block", "verify_crosses_block", "restore_other_row", "restore_cross_layout",
                 "finished_then_extended", "finished_row_surplus_block"]:
        assert cov.get(what, 0) >= 1, f"no sequence reached: {what}"


def prompt(n):
    return list(range(n))


def test_fork_block_accounting_on_the_model_alone():
    """the figures of tests/test_hip_fork_row.py::test_block_accounting"""
    budget = 16 * BLK
    m = RowModel(4, 512, 1000, budget)
    free = m.free_tokens

    def go(kind, *a, out=None):
        st, why = m.status(kind, *a)
        if st == OK:
            m.apply(kind, *a, out=out)
        return st
    assert free() == budget
    assert go("forward_row", 0, prompt(300)) == OK and free() == budget - 3 * BLK
    assert go("fork_row", 0, [1, 2, 3]) == OK and free() == budget - 6 * BLK
    assert go("reset_row", 0) == OK and free() == budget - 5 * BLK
    assert go("reset_row", 2) == OK and free() == budget - 4 * BLK
    assert go("reset_row", 1) == OK and free() == budget - 3 * BLK
    assert go("reset_row", 3) == OK and free() == budget
    assert go("forward_row", 0, prompt(256)) == OK and free() == budget - 2 * BLK
    assert go("fork_row", 0, [1, 2, 3]) == OK and free() == budget - 2 * BLK
    for r in range(4):
        assert go("sample_row", r, out=7) == OK
    assert go("decode", 1, out=np.full((1, 4), 7)) == OK and free() == budget - 6 * BLK      # every row writes position 256 into a block of its own
    for r in range(4):
        go("reset_row", r)
    assert free() == budget
    budget = 10 * BLK
    m = RowModel(4, 512, 1000, budget)
    for r in range(3):
        assert go("forward_row", r, prompt(380)) == OK
    assert go("forward_row", 3, prompt(380)) == CONTEXT
    m = RowModel(4, 512, 1000, budget)
    assert go("forward_row", 0, prompt(380)) == OK and go("fork_row", 0, [1, 2, 3]) == OK
    assert m.free_tokens() == budget - 6 * BLK
    for r in range(4):
        go("sample_row", r, out=7)
    assert go("decode", 8, out=np.full((8, 4), 7)) == OK                                       # 380 -> 388: a fourth block per row
    assert m.free_tokens() == 0 and [m.past_length_row(r) for r in range(4)] == [388] * 4


def test_snapshot_block_accounting_on_the_model_alone():
    """the figures of tests/test_hip_row_snapshot.py::test_paged_accounting"""
    budget = 12 * BLK
    m = RowModel(4, 1024, 1000, budget)

    def go(kind, *a, out=None):
        st, why = m.status(kind, *a)
        return (st, m.apply(kind, *a, out=out)) if st == OK else (st, None)
    go("forward_row", 0, prompt(300)); go("fork_row", 0, [1, 2])
    for r in range(3):
        go("sample_row", r, out=5)
    assert m.free_tokens() == budget - 5 * BLK                     # two shared blocks, three tails
    st, blob = go("save_row", 1)
    assert st == OK and m.free_tokens() == budget - 5 * BLK
    go("reset_row", 1); assert m.free_tokens() == budget - 4 * BLK
    assert go("restore_row", 1, blob)[0] == OK and m.free_tokens() == budget - 7 * BLK      # three blocks of its own
    go("reset_row", 1); assert m.free_tokens() == budget - 4 * BLK                           # ... all three come back
    budget = 6 * BLK
    m = RowModel(3, 1024, 1000, budget)
    go("forward_row", 0, prompt(300)); go("sample_row", 0, out=5)
    st, blob = go("save_row", 0)
    go("forward_row", 1, prompt(100)); go("sample_row", 1, out=5)
    assert m.free_tokens() == 2 * BLK and len(blob.tokens) == 300
    assert go("restore_row", 2, blob)[0] == CONTEXT and m.batch == 2 and m.free_tokens() == 2 * BLK
    ids = np.full((2, 2), 9)
    assert go("decode_rows", 2, out=(ids, np.array([2, 2]), np.array([0, 0])))[0] == OK        # still decodes
    go("reset_row", 1); assert m.free_tokens() == 3 * BLK
    assert go("restore_row", 2, blob)[0] == OK and m.free_tokens() == 0
