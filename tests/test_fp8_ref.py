"""Option weights.fp8: the quantization rule and the stream layout as tests/fp8_ref.py states them, held to torch's CPU cast to float8_e4m3fn and to the
bounds the rule promises.  No GPU: tests/test_hip_fp8.py holds the device quantizer and kernels/gemv_fp8.h to fp8_ref bit for bit."""
import numpy as np
import pytest
import torch

import fp8_ref as R

FINITE = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], np.uint8)      # the 254 finite codes
POS = np.arange(0, 0x7F, dtype=np.uint8)                                          # +0 .. 448 in value order


def bits_of(v):
    return R.bf16_bits(np.asarray(v, np.float64))


def pinned_row(values, e):
    """a row whose first weight, 448 * 2^e, pins the row exponent to e; the others are values * 2^e (which must be bf16 values)"""
    return bits_of(np.ldexp(np.concatenate([[448.0], np.asarray(values, np.float64)]), e))[None, :]


def ties():
    """the midpoint of every pair of neighbouring codes, both signs: 5 significant bits at the most, so each is a bf16"""
    v = R.code_value(POS)
    mid = (v[:-1] + v[1:]) / 2
    return np.concatenate([mid, -mid])


def random_rows(seed, n=64, k=256):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((n, k)) * 0.02 * np.exp2(rng.integers(-12, 12, (n, 1)))).astype(np.float32)
    W[rng.random((n, k)) < 0.05] *= 2.0 ** -9            # a tail deep in the subnormal code range
    u = W.view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)      # RNE to bf16


def cases():
    sub = np.arange(-40, 41) * 2.0 ** -12                 # the subnormal range and below it, in steps of an eighth of the codes' step
    out = {
        "random": random_rows(1),
        "random_wide": random_rows(2, n=32, k=2048),
        "ties_e0": pinned_row(ties(), 0),
        "ties_e-20": pinned_row(ties(), -20),
        "ties_e_min": pinned_row(ties(), R.E_MIN),
        "subnormal_range": pinned_row(sub, -7),
        "signed_zeros": np.array([[0x0000, 0x8000, 0x3C00, 0x8000, 0x0000, 0xBC00, 0x0000, 0x8000]], np.uint16),
        "all_zero_row": np.array([[0x0000] * 8, [0x8000] * 8, [0x0000, 0x8000] * 4], np.uint16),
        "m_0.875": bits_of([[0.875 * 2.0 ** -3, 0.09375, -0.01171875, 2.0 ** -12, 0, 0, 0, 0]]),
        "m_above_0.875": bits_of([[0.87890625 * 2.0 ** -3, 0.09375, -0.01171875, 2.0 ** -12, 0, 0, 0, 0]]),      # 0.875 + 2^-8: the next bf16
        "bf16_subnormal_row": np.array([[0x007F, 0x0001, 0x8040, 0x0000, 0x0020, 0x0010, 0x0008, 0x0003]], np.uint16),
        "clamped_row": bits_of(np.ldexp([[1.0, 0.5, 0.515625, -0.25, 1.75, 0.0078125, 0.01171875, 0.001953125]], -120)),
        "largest_allowed": bits_of(np.ldexp([[1.75, 1.0, -1.5, 2.0 ** -100, 0, 0, 0, 0]], 99)),
    }
    return out


CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_codes_equal_torch_cast_of_exact_quotients(name):
    W = CASES[name]
    codes, e = R.quantize(W)
    q = np.ldexp(R.bf16_value(W), -e[:, None])
    q32 = q.astype(np.float32)
    exact = q32.astype(np.float64) == q                  # (a quotient below fp32's range is far below half the smallest code: both sides give the signed zero)
    assert exact.all() or (np.abs(q[~exact]) < 2.0 ** -100).all()
    want = torch.from_numpy(q32).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    np.testing.assert_array_equal(codes, want)
    assert ((codes & 0x7F) != 0x7F).all()
    np.testing.assert_array_equal(codes >> 7, W >> 15)   # the sign is kept, -0 included


def test_row_exponent_is_the_smallest_that_fits():
    for W in CASES.values():
        e = R.row_exponents(W)
        amax = np.abs(R.bf16_value(W)).max(axis=1)
        live = amax > 0
        assert (amax <= 448 * np.exp2(e.astype(np.float64))).all()
        free = live & (e > R.E_MIN)
        assert (amax[free] > 448 * np.exp2(e[free] - 1.0)).all()
        assert (e[~live] == 0).all() and (e >= R.E_MIN).all()
    m, x = np.frexp(0.875 * 2.0 ** -3)
    assert m == 0.875 and R.row_exponents(CASES["m_0.875"])[0] == x - 9 and R.row_exponents(CASES["m_above_0.875"])[0] == x - 8
    assert R.row_exponents(CASES["ties_e_min"])[0] == R.E_MIN and R.row_exponents(CASES["clamped_row"])[0] == R.E_MIN


@pytest.mark.parametrize("name", sorted(CASES))
def test_dq_is_bf16_within_the_bounds_and_idempotent(name):
    W = CASES[name]
    codes, e = R.quantize(W)
    D = R.dequantize(codes, e)                            # (bf16_bits asserts the round trip through bf16)
    expo = (D >> 7) & 0xFF
    assert (((D & 0x7FFF) == 0) | ((expo > 0) & (expo < 255))).all()      # a zero or a NORMAL bf16
    w, dq = R.bf16_value(W), R.bf16_value(D)
    scale = np.exp2(e.astype(np.float64))[:, None]
    big = np.abs(w / scale) >= 2.0 ** -6
    assert (np.abs(dq - w)[big] <= (np.abs(w) / 16)[big]).all()
    assert (np.abs(dq - w)[~big] <= np.broadcast_to(scale * 2.0 ** -10, w.shape)[~big]).all()
    np.testing.assert_array_equal(R.dequantized(D), D)    # dq(q(dq(W))) == dq(W), also where the row exponent moves
    np.testing.assert_array_equal(R.dequantized(W), D)


def test_every_finite_code_survives():
    for e in (R.E_MIN, -30, 0, 17, 91):
        W = R.dequantize(FINITE[None, :], np.array([e]))
        codes, e2 = R.quantize(W)
        assert e2[0] == e
        np.testing.assert_array_equal(codes[0], FINITE)


def test_refused_weights():
    for bad in (0x7F80, 0xFF80, 0x7FC0, 0x7180, 0xF180):      # inf, -inf, NaN, 2^100 (exponent field 227), its negative
        W = np.array([[0x3C00] * 8, [0x3C00] * 7 + [bad]], np.uint16)
        with pytest.raises(ValueError):
            R.row_exponents(W)
    R.row_exponents(np.array([[0x717F] * 8], np.uint16))      # the largest bf16 below 2^100 is allowed


def test_integer_restatement_agrees_for_every_bf16_pattern():
    """the device quantizer (kernels/gemv_fp8.h) decides a code by integer arithmetic on the pattern: held here to the value arithmetic, exhaustively"""
    pats = np.arange(0x10000, dtype=np.int64)
    pats = pats[((pats >> 7) & 0xFF) < 227].astype(np.uint16)
    val = R.bf16_value(pats)
    for e in list(range(R.E_MIN, R.E_MIN + 12)) + list(range(-60, 93, 7)) + [92]:
        ok = np.abs(val) <= 448 * 2.0 ** e
        want = R.round_to_codes(np.ldexp(val[ok], -e))
        got = R.code_int(pats[ok], e)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(R.dq_bits_int(got, e), R.bf16_bits(np.ldexp(R.code_value(got), e)))
    for W in CASES.values():
        np.testing.assert_array_equal(R.row_exponents_int(W), R.row_exponents(W))
    rows = R.dequantize(np.tile(POS[1:, None], (1, 8)), np.zeros(126, np.int64))      # amax = every positive code value
    np.testing.assert_array_equal(R.row_exponents_int(rows), R.row_exponents(rows))


@pytest.mark.parametrize("K,ks", [(2048, 1), (8192, 4), (64, 1), (520, 1), (1288, 2), (4088, 1), (8, 1), (3072, 4)])
def test_layout_inverts(K, ks):
    rng = np.random.default_rng(K + ks)
    codes = rng.integers(1, 256, (3, K), dtype=np.uint8)        # no zero: padding is told from data
    P = R.to_planes(codes, ks)
    nchunk, nx, nh, per = R.geometry(K, ks)
    assert P.nbytes == 3 * R.row_bytes(K, ks) and P.shape[2] == nh
    assert np.count_nonzero(P) == codes.size                    # every code once, everything else padding 0
    np.testing.assert_array_equal(R.from_planes(P, K, ks), codes)
    # lane l of k-part p, chunk j: the 8 bytes at ((p * NH + j // 2) * 64 + l) * 16 + 8 * (j & 1) of the row are k = 8 (p * per + l + 64 j) ..
    flat = P.reshape(3, -1)
    for p, j, l in ((0, 0, 0), (ks - 1, 0, 5), (0, nx - 1, 63), (ks - 1, nx - 1, 1)):
        c = min(p * per, nchunk) + l + 64 * j
        if c < min(min(p * per, nchunk) + per, nchunk):
            off = ((p * nh + j // 2) * 64 + l) * 16 + 8 * (j & 1)
            np.testing.assert_array_equal(flat[:, off:off + 8], codes[:, 8 * c:8 * c + 8])


def test_layout_coverage():
    assert R.covered(2048, 1) and R.covered(8192, 4) and R.covered(16384, 4) and not R.covered(16392, 4) and not R.covered(2052, 1)
    assert R.row_bytes(2048, 1) == 2048 and R.row_bytes(8192, 4) == 8192      # no padding at the benchmark's shapes: one byte per weight
