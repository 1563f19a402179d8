"""The whole row API of include/tgx.h fuzzed with random call sequences (tests/row_model.py's driver): every operation is predicted by the host-only model of the
header, run on the device, and checked — status, lengths, kv.free_tokens, counts, bystanders and copies exactly; the logits against one batch-1 CPU oracle per row.

  fp32 storage, slab cache     the raw logits of every row that holds logits within rel_err < 1e-4 of its oracle's after every operation (tests/test_hip_fuzz.py's
                               bound for fp32 storage, where no 16-bit rounding can flip): the arm that catches subtly wrong arithmetic or indexing.  Its inputs keep
                               the oracle within 1e-5 of its reordered twin (asserted in tests/test_row_model.py, where it can be measured without a GPU).
  bf16 / fp16, slab and paged  default options, the matrix-core routes.  1e-2 against the oracle as a sanity bound (a flipped cache entry stays flipped for the rest of
                               a sequence: tests/test_hip_rows.py), greedy ids equal wherever the oracle's top-2 gap exceeds 4e-3 of its largest logit; the oracle-to-
                               twin floor is tracked per row and printed with a failure, and stays below a third of the bound in the CPU dry run.
A failing assertion prints the seed, the index of the operation and the whole operation log.

The arms whose name ends in _x have their base arm's dtype, layout and bound, a random stream of their own, and draw the later row calls as well — tgx_splice_row,
tgx_verify_rows, tgx_advance_rows, tgx_beam_select, tgx_beam_advance — with about half of the weight (Driver.WEIGHTS_X); the old arms draw what they drew before.
In the 16-bit _x arms the form each accepted tgx_verify_rows / tgx_advance_rows took is tallied (verify.last_form, advance.last_form): over the 8 seeds each arm must
have seen the joint pass of either call; with fp32 storage every call runs row by row (and some call of either kind was accepted).  The arm's last seed holds
the tally, where the session ran all 8 seeds of the arm.
Measured on an MI355X, median `wall` of a case over the 8 seeds: f32_slab 0.27 s, h16_slab 0.30 s, h16_paged 0.33 s; f32_slab_x 0.39 s, h16_slab_x 0.32 s,
h16_paged_x 0.25 s (largest case 0.69 s) — inside twice the old arms' medians."""
import os

import numpy as np
import pytest

import row_model as rm
from row_model import BLK, RowModel
from tinygpt_amd.ffi import Model

pytestmark = pytest.mark.gpu

SEEDS = list(range(int(os.environ.get("TGX_FUZZ_SEEDS_ROWS", "8"))))
N_OPS = 40
BOUND = {"f32_slab": 1e-4, "h16_slab": 1e-2, "h16_paged": 1e-2}
for _arm in rm.ARMS:                                                          # an _x arm: its base arm's bound
    BOUND[_arm] = BOUND[rm.base_arm(_arm)]
_forms = {}      # arm -> {seed: {(call, last_form): accepted calls}}


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def device(hip, fam, dtype, max_batch, max_ctx, budget):
    d, seed, std = rm.make_desc(fam, dtype, max_batch, max_ctx)
    m = Model(d, hip)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(seed, std).finalize()


@pytest.mark.parametrize("arm", rm.ARMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_random_call_sequences_against_the_model_of_the_header(seed, arm, hip, oracle_lib):
    from test_hip_logprobs import TOL
    k = rm.case(seed, arm)
    dev = device(hip, k["fam"], k["dtype"], k["max_batch"], k["max_ctx"], k["budget"])
    aux_budget = 0 if k["budget"] else (0 if k["dtype"] == "fp32" else 4 * BLK)      # the second context has the other cache layout (paged KV refuses fp32 storage)
    aux = device(hip, k["fam"], k["dtype"], 3, k["max_ctx"], aux_budget)
    gpt2 = dev.desc.family == "gpt2"
    model = RowModel(k["max_batch"], k["max_ctx"], dev.desc.vocab, k["budget"], gpt2=gpt2)
    aux_model = RowModel(3, k["max_ctx"], dev.desc.vocab, aux_budget, gpt2=gpt2)
    try:
        s = rm.run_sequence(dev, model, k["rng"], N_OPS, fam=k["fam"], dtype=k["dtype"], bound=BOUND[arm], lp_tol=TOL, aux=(aux, aux_model),
                            tag=f"seed {seed} {arm} {k['fam']} {k['dtype']}", extended=k["extended"])
    finally:
        dev.close(); aux.close()
    _forms.setdefault(arm, {})[seed] = dict(s.forms)
    print(f"row_fuzz gpu seed {seed} {arm} {k['fam']} {k['dtype']}: {s.line()} forms(call, last_form) {sorted(s.forms.items())}")
    assert s.greedy and 2 * s.compared >= s.greedy, f"only {s.compared} of the {s.greedy} greedy ids produced were compared with the oracle's"
    if arm == "f32_slab_x":                                         # fp32 storage runs row by row (include/tgx.h, Forms)
        assert all(form == 2 for _, form in s.forms), f"fp32 storage took another form than row by row: {s.forms}"
    # the arm's last seed closes its tally: stated for the 8 default seeds, so it is held only where this session ran all of them (a selection with -k states nothing)
    if k["extended"] and len(SEEDS) >= 8 and seed == SEEDS[-1] and set(_forms[arm]) == set(SEEDS):
        total = {}
        for forms in _forms[arm].values():
            for key, n in forms.items():
                total[key] = total.get(key, 0) + n
        print(f"row_fuzz gpu {arm} forms over the {len(SEEDS)} seeds: {sorted(total.items())}")
        for call in ("verify", "advance"):
            want = 2 if arm == "f32_slab_x" else 1                  # 16-bit storage: the joint pass at least once; fp32: row by row, and at least once at all
            assert total.get((call, want), 0) >= 1, f"{arm}: {call}.last_form was never {want} over the {len(SEEDS)} seeds: {total}"
