"""tests/stream_shapes.py held to its own reach list, on the CPU: the condition that keeps tests/test_hip_stream_shapes.py from passing by falling back
everywhere.  Every feature of the list names the case that reaches it; the cases stay inside the stated weight budget; the references' stream sizes agree with
the transcribed layout; and every dequantized weight of every case is exactly a bf16 value, which is what makes bit-identity meaningful."""
import numpy as np
import pytest

import fp4_ref as R4
import fp8_ref as R8
import stream_shapes as S
from tinygpt_amd import synth

REF = {"fp8": R8, "fp4": R4}


def test_every_feature_is_reached_and_names_its_case():
    reached = {}
    for form, case in S.CASES:
        for f in sorted(S.features(form, case)):
            reached.setdefault(f, f"{form}-{case.name}")
    missing = [f for f in S.reach_list() if f not in reached]
    for f in S.reach_list():
        print(f"{f:40s} {reached.get(f, '-- NOT REACHED --')}")
    assert not missing, missing


def test_every_listed_row_count_runs_somewhere():
    for form in S.FORMS:
        ran = {m for f, c in S.CASES if f == form for rows in c.rows for m in S.step_passes(c, rows)}
        assert set(S.M_VALUES) <= ran


def test_the_split_geometry_does_not_depend_on_the_cu_count():
    """cfg picks 128-row groups only where they alone oversubscribe the chip: no product here is that wide on a device of 128 CUs or more"""
    for _, case in S.CASES:
        for cls in S.CLASSES:
            N, K = S.dims(cls, case)
            assert {S.skinny_cfg(N, cus) for cus in (128, 256, 304)} == {0}, (case.name, cls)
            assert len({S.skinny_split(5, N, K, cls == "down", cus) for cus in (128, 256, 304)}) == 1


def test_the_cases_stay_inside_the_weight_budget():
    for case in S.SHAPES:
        assert case.weight_bytes() <= S.BUDGET_BYTES, (case.name, case.weight_bytes())
        assert max(case.rows) <= 67 and case.desc().max_ctx <= 128 and case.layers <= 2


def test_row_bytes_agree_with_the_references():
    for form, case in S.CASES:
        for cls in S.CLASSES:
            lay = S.layout(form, cls, case)
            assert lay.stream, (form, case.name, cls)      # every matrix of the table owns a stream
            assert lay.row_bytes == REF[form].row_bytes(lay.K, lay.ks), lay.geometry()
            if form == "fp8":
                assert R8.covered(lay.K, lay.ks) and R8.geometry(lay.K, lay.ks)[1] == lay.nx


def test_the_predictions_of_the_existing_modules_geometry():
    """hidden 2048 / intermediate 8192 / vocabulary 1024 (tests/test_hip_fp8_rows.py): all three stream, down in 16 ranges of 512 k"""
    case = S.Case("bench", 2048, 8192, 1024, heads=32, kv_heads=8)
    for form in S.FORMS:
        prods, delta = S.predict_step(form, case, 5)
        assert delta == (3, 0) and [(p.lay.nx, p.lay.ks) for p in prods] == [(4, 1), (4, 4), (4, 1)]
        assert (prods[1].nsplit, prods[1].k_per, prods[1].epi) == (8, 1024, "PARTIAL")
        assert S.predict_finalize(form, case) == (3, 0)
    # a 2-row step: no row counter moves, and launch_gemv's R = 2 rule moves gate_up at NX = 4 to two waves per row pair — the stream is not its layout
    assert S.gemv_launch_ks(2048, 1, 2, "gateup") == 2 and S.gemv_launch_ks(2048, 1, 1, "gateup") == 1
    assert not S.gemv_streams(S.layout("fp8", "gateup", case), "gateup", case, 2)


def quantized(name, case):
    return any(k in name for k in ("gate_proj", "up_proj", "down_proj")) or name == ("model.embed_tokens.weight" if case.tied else "lm_head.weight")


@pytest.mark.parametrize("case", S.SHAPES, ids=lambda c: c.name)
def test_dequantized_weights_are_exactly_bf16(case):
    """dq = code * 2^e recomputed in float64 from the codes and exponents equals the uint16 pattern `dequantized` returns, for both forms, on the case's own
    tensors (whole rows — the K axis is what the layouts depend on — of up to 48 rows spread over each matrix)"""
    for name, bits in synth.synth_checkpoint(case.desc(), S.SEED, S.STD):
        if not quantized(name, case):
            continue
        rows = bits[::max(1, bits.shape[0] // 48)]
        codes, e = R8.quantize(rows)
        np.testing.assert_array_equal(R8.bf16_value(R8.dequantized(rows)), np.ldexp(R8.code_value(codes), e[:, None]))
        codes, sb = R4.quantize(rows)
        ek = np.repeat(sb.astype(np.int64) - 127, R4.BLOCK, axis=1)[:, :rows.shape[1]]
        dq = R4.dequantized(rows)
        np.testing.assert_array_equal(R8.bf16_value(dq), np.ldexp(R4.code_value(codes), ek))
        assert np.isfinite(R8.bf16_value(dq)).all() and (dq != rows).any()
