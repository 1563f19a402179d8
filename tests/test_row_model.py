"""The row fuzzer without a GPU: tests/row_model.py's driver on OracleDevice (the row calls answered from the model of include/tgx.h plus one CPU oracle per row), for
the seeds and arms tests/test_hip_row_fuzz.py runs on the device.  It checks the model against itself, the two conditions on the inputs that the GPU bounds rest on
(the oracle against its reordered twin), that the seed set still reaches every state the fuzzer is there for — the later row calls of the _x arms included —, and the block figures of four scripted GPU
tests on the model alone."""
import os

import numpy as np
import pytest

import row_model as rm
from row_model import BLK, CONTEXT, OK, RowModel

SEEDS = list(range(int(os.environ.get("TGX_FUZZ_SEEDS_ROWS", "8"))))
N_OPS = 40
BOUND = {"f32_slab": 1e-4, "h16_slab": 1e-2, "h16_paged": 1e-2}
FLOOR = {"f32_slab": 1e-5, "h16_slab": 1e-2 / 3, "h16_paged": 1e-2 / 3}      # the oracle against its reordered twin: what the inputs must stay below
for _arm in rm.ARMS:                                                          # an _x arm: its base arm's bound and floor
    BOUND[_arm], FLOOR[_arm] = BOUND[rm.base_arm(_arm)], FLOOR[rm.base_arm(_arm)]
X_ARMS = [a for a in rm.ARMS if a.endswith("_x")]
_done = {}


def dry_run(seed, arm, device_cls=rm.OracleDevice):
    k = rm.case(seed, arm)
    dev = device_cls(k["fam"], k["dtype"], k["max_batch"], k["max_ctx"], k["budget"])
    aux_budget = 0 if k["budget"] else (0 if k["dtype"] == "fp32" else 4 * BLK)      # the second context has the other cache layout (fp32 storage has no paged cache)
    aux = device_cls(k["fam"], k["dtype"], 3, k["max_ctx"], aux_budget)
    gpt2 = dev.desc.family == "gpt2"
    model = RowModel(k["max_batch"], k["max_ctx"], dev.desc.vocab, k["budget"], gpt2=gpt2)
    aux_model = RowModel(3, k["max_ctx"], dev.desc.vocab, aux_budget, gpt2=gpt2)
    return rm.run_sequence(dev, model, k["rng"], N_OPS, fam=k["fam"], dtype=k["dtype"], bound=BOUND[arm], aux=(aux, aux_model), tag=f"seed {seed} {arm} {k['fam']} {k['dtype']}",
                           extended=k["extended"])


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
    def gather(arms):
        acc, ref, classes, cov = {}, {}, {}, {}
        for seed in SEEDS:
            for arm in arms:
                s = stats_of(seed, arm)
                for src, dst in ((s.accepted, acc), (s.refused, ref), (s.classes, classes), (s.cov, cov)):
                    for k, v in src.items():
                        dst[k] = dst.get(k, 0) + v
        print(arms, "\naccepted", acc, "\nrefused", ref, "\nclasses", classes, "\ncoverage", cov)
        return acc, ref, classes, cov
    acc, ref, classes, cov = gather([a for a in rm.ARMS if a not in X_ARMS])
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
    # ---- the later row calls, over the 8 seeds of the _x arms
    acc, ref, classes, cov = gather(X_ARMS)
    for kind in rm.Driver.KINDS_X:
        assert acc.get(kind, 0) >= 3, f"{kind} was accepted {acc.get(kind, 0)} times"
        assert ref.get(kind, 0) >= 1, f"{kind} was never refused"
    for cls in ["splice_row:gpt2", "splice_row:bad_range", "splice_row:pool", "verify_rows:row_twice", "verify_rows:no_token", "verify_rows:positions",
                "advance_rows:gap", "advance_rows:step_no_logits", "advance_rows:pool", "advance_rows:neg_len", "beam_advance:parent_is_spare", "beam_advance:finished_source", "beam_advance:pool"]:
        assert classes.get(cls, 0) >= 1, f"the refusal class {cls} never occurred"
    assert any(k.endswith(":pool") for k in classes), "the pool was never exhausted"
    for what in ["splice_cow_block", "splice_shared_prefix_kept", "splice_then_fork", "splice_then_restore_cross_layout", "truncate_spliced_row", "verify_rows_all_zero_drafts",
                 "verify_rows_rejects_tail_block", "advance_feed_more_then_feed", "advance_admits_new_row", "advance_over_finished_row", "beam_childless_source_retired",
                 "beam_copied_child_tail_block", "beam_on_already_forked_rows", "beam_new_row_spare",
                 # the splice forms and row states the draws must include, and both kinds of row that hold nothing
                 "splice_noop", "splice_truncation_form", "splice_lead_inside_block", "splice_lead_on_block_edge", "splice_ranges_touch", "splice_on_token_row",
                 "splice_on_logits_only_row", "splice_on_no_logits_row", "splice_on_finished_row", "splice_refused_retired_row", "splice_refused_row_beyond_batch"]:
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


def test_splice_block_accounting_on_the_model_alone():
    """the figures of tests/test_hip_splice_row.py::test_fork_then_splice_copies_before_it_writes"""
    ranges = [(0, 150), (160, 140)]

    def forked(blocks):
        m = RowModel(3, 512, 4096, blocks * BLK)
        m.apply("forward_row", 0, prompt(300)); m.apply("fork_row", 0, [1, 2])
        return m
    m = forked(16)
    f0 = m.free_tokens()
    assert f0 == (16 - 5) * BLK
    assert m.status("splice_row", 1, ranges)[0] == OK
    m.apply("splice_row", 1, ranges, out=290)
    assert m.free_tokens() == f0 - BLK and m.past_length_row(1) == 290      # blocks: 0 shared, 1 fresh, 2 the row's own tail
    assert m.pool.shared(m.rows[1].blocks[0]) and not m.pool.shared(m.rows[1].blocks[1]) and m.rows[0].blocks[:2] == m.rows[2].blocks[:2]
    assert not m.rows[1].has_logits and m.rows[1].tokens == prompt(150) + list(range(160, 300))
    m.apply("reset_row", 1)
    assert m.free_tokens() == f0 + BLK
    m = forked(5)                                                           # no free block: refused, although the row's own tail block would have covered it
    assert m.free_tokens() == 0 and m.status("splice_row", 1, ranges) == (CONTEXT, "pool")


def test_beam_block_accounting_on_the_model_alone():
    """the paged figures of tests/test_hip_beam.py::test_advance_placement_cache_and_blocks at P = 200 (a tail behind a shared block), and the shortfall of
    its test_refusals_change_nothing"""
    budget, P, G = 24 * BLK, 200, [1, 2, 3, 4]
    m = RowModel(6, 512, 4096, budget)

    def advance(rows, parent, tokens, want):
        assert m.status("beam_advance", rows, parent, tokens)[0] == OK
        assert m.apply("beam_advance", rows, parent, tokens, out=want)[0] == want

    def step(n_rows):
        ids = np.full((1, n_rows), 7)
        live = [r for r in range(n_rows) if m.rows[r].state == rm.LIVE]
        m.apply("decode_rows", 1, out=(np.where(np.isin(np.arange(n_rows), live), ids, -1), np.isin(np.arange(n_rows), live).astype(int), np.zeros(n_rows, int)))
    m.apply("forward_rows", [0, 1], [prompt(40), prompt(P)]); m.apply("sample_row", 0, out=7)
    f = budget - 3 * BLK
    assert m.free_tokens() == f
    advance(G, [0, 0, 0, 0], [11, 12, 13, 14], [1, 2, 3, 4]); f -= 3 * BLK
    assert m.free_tokens() == f
    step(5); assert m.free_tokens() == f
    advance(G, [0, 1, 2, 3], [21, 22, 23, 24], [1, 2, 3, 4]); assert m.free_tokens() == f
    step(5)
    advance(G, [2, 0, 2, 1], [31, 32, 33, 34], [3, 1, 4, 2]); assert m.free_tokens() == f      # row 4's private tail block went back and came again
    advance(G, [1, 1, 1, 1], [41, 42, 43, 44], [2, 1, 3, 4]); assert m.free_tokens() == f
    step(5)
    advance(G, [2, 0], [51, 52], [3, 1]); f += 2 * BLK
    assert m.free_tokens() == f and [m.rows[r].state for r in (2, 4)] == [rm.RETIRED] * 2
    step(5)
    advance(G, [0, 0, 2], [61, 62, 63], [1, 2, 3])
    step(5)
    assert [m.past_length_row(r) for r in range(5)] == [45, P + 5, P + 5, P + 5, 0]
    # two tail blocks, one free: refused; one tail block: what fits, fits
    m = RowModel(6, 768, 4096, 7 * BLK)
    m.apply("forward_rows", [0, 1, 2, 3], [prompt(300), prompt(200), prompt(5), prompt(20)])
    m.apply("reset_row", 2); m.apply("reset_row", 1)
    m.apply("forward_row", 1, prompt(200))
    assert m.free_tokens() == BLK
    assert m.status("beam_advance", [0, 2, 4], [0, 0, 0], [1, 1, 1]) == (CONTEXT, "pool")
    advance([0, 2, 4], [0, 0], [1, 1], [0, 2])
    assert m.free_tokens() == 0 and m.batch == 4
