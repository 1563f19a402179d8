"""The whole row API of include/tgx.h fuzzed with random call sequences (tests/row_model.py's driver): every operation is predicted by the host-only model of the
header, run on the device, and checked — status, lengths, kv.free_tokens, counts, bystanders and copies exactly; the logits against one batch-1 CPU oracle per row.

  fp32 storage, slab cache     the raw logits of every row that holds logits within rel_err < 1e-4 of its oracle's after every operation (tests/test_hip_fuzz.py's
                               bound for fp32 storage, where no 16-bit rounding can flip): the arm that catches subtly wrong arithmetic or indexing.  Its inputs keep
                               the oracle within 1e-5 of its reordered twin (asserted in tests/test_row_model.py, where it can be measured without a GPU).
  bf16 / fp16, slab and paged  default options, the matrix-core routes.  1e-2 against the oracle as a sanity bound (a flipped cache entry stays flipped for the rest of
                               a sequence: tests/test_hip_rows.py), greedy ids equal wherever the oracle's top-2 gap exceeds 4e-3 of its largest logit; the oracle-to-
                               twin floor is tracked per row and printed with a failure, and stays below a third of the bound in the CPU dry run.
A failing assertion prints the seed, the index of the operation and the whole operation log."""
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
    aux_budget = 0 if k["budget"] else (0 if arm == "f32_slab" else 4 * BLK)      # the second context has the other cache layout (paged KV refuses fp32 storage)
    aux = device(hip, k["fam"], k["dtype"], 3, k["max_ctx"], aux_budget)
    model = RowModel(k["max_batch"], k["max_ctx"], dev.desc.vocab, k["budget"])
    aux_model = RowModel(3, k["max_ctx"], dev.desc.vocab, aux_budget)
    try:
        s = rm.run_sequence(dev, model, k["rng"], N_OPS, fam=k["fam"], dtype=k["dtype"], bound=BOUND[arm], lp_tol=TOL, aux=(aux, aux_model),
                            tag=f"seed {seed} {arm} {k['fam']} {k['dtype']}")
    finally:
        dev.close(); aux.close()
    print(f"row_fuzz gpu seed {seed} {arm} {k['fam']} {k['dtype']}: {s.line()}")
    assert s.greedy and 2 * s.compared >= s.greedy, f"only {s.compared} of the {s.greedy} greedy ids produced were compared with the oracle's"
