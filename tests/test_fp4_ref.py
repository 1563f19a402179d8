"""Option weights.fp4: the rule as tests/fp4_ref.py states it, held to an independent float64 statement — the nearest grid value by brute force, the issue's
tie table, the exponent from the definition.  No GPU: tests/test_hip_fp4.py holds the device quantizer and kernels/gemv_fp4.h to fp4_ref bit for bit."""
import numpy as np

import fp4_ref as R
from fp8_ref import bf16_bits, bf16_value

GRID = [0, 0.5, 1, 1.5, 2, 3, 4, 6]
TIES = {0.25: 0, 0.75: 1, 1.25: 1, 1.75: 2, 2.5: 2, 3.5: 4, 5: 4}      # midpoint -> the grid value whose code has low bit 0


def brute(bits):
    """dq of one block (float64 values), from the definition"""
    w = bf16_value(bits)
    amax = np.abs(w).max()
    e = 0
    if amax:
        x = int(np.floor(np.log2(amax)))
        e = max(x - 2 if amax / 2.0 ** x <= 1.5 else x - 1, -125)
    out = []
    for v in w:
        q = abs(v) / 2.0 ** e
        g = TIES[q] if q in TIES else min(GRID, key=lambda t: abs(t - q))
        out.append(np.copysign(g * 2.0 ** e, v))
    return np.array(out)


def test_dequantized_is_the_rule():
    e = -9
    octaves = np.arange(((e - 10 + 127) << 7), ((e + 3 + 127) << 7), dtype=np.uint16)      # every magnitude pattern of 2^(e-10) .. 2^(e+3) ...
    octaves = octaves[bf16_value(octaves) <= 6 * 2.0 ** e]                                 # ... that a block pinned to e can hold
    body = np.concatenate([octaves, octaves | 0x8000, [0x0000, 0x8000]])
    body = np.resize(body, (-(-body.size // 31), 31))
    pinned = np.concatenate([np.full((body.shape[0], 1), bf16_bits(6 * 2.0 ** e)), body], axis=1)
    blocks = [row for row in pinned] + [
        bf16_bits(np.ldexp([1.5, 0.1875, -0.5625, 0.9375, 1.3125, 0.4375, -1.25, 0.0625], -8)),      # amax mantissa exactly 1.5: e = x - 2
        bf16_bits(np.ldexp([1.5078125, 0.1875, -0.5625, 0.9375, 1.3125, 0.4375, -1.25, 0.0625], -8)),      # the next pattern: e = x - 1
        np.array([0x00C0, 0x0080, 0x8080, 0x0001, 0x807F, 0x0000, 0x0100, 0x0140], np.uint16),      # around 2^-126: the clamp at e = -125
        np.array([0x007F, 0x8001, 0x0040], np.uint16),      # bf16 subnormals only
        np.array([0x0000, 0x8000, 0x0000], np.uint16),      # zeros
    ]
    for blk in blocks:
        got = R.dequantized(blk[None, :])[0]
        np.testing.assert_array_equal(bf16_value(got), brute(blk))
        np.testing.assert_array_equal(got >> 15, blk >> 15)      # -0 stays -0
    W = np.concatenate([blocks[0], np.tile(blocks[-3], 4), blocks[-5]])[None, :]      # one row of three blocks at different scales, the last one short
    codes, sb = R.quantize(W)
    assert sb.shape == (1, 3) and sb[0, 0] == e + 127
    np.testing.assert_array_equal(np.ldexp(R.code_value(codes[0]), np.repeat(sb[0].astype(int) - 127, 32)[:W.shape[1]]), bf16_value(R.dequantized(W)[0]))
