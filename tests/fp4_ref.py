"""Option weights.fp4 as numpy: the written specification of the quantization rule (include/tgx.h) and of the 4-bit stream's size
(tinygpt_amd/csrc/kernels/gemv_fp4.h).  No GPU.  tests/test_fp4_ref.py holds it to a brute-force float64 statement; the GPU tests upload dequantized(W) to an
ordinary context and hold the quantized context to it bit for bit.

  rule      per output row, per block of 32 consecutive k (the last may be shorter): amax = max |w| = m * 2^x, m in [1, 2); e = x - 2 if m <= 1.5 else x - 1,
            clamped to >= -125; an all-zero block takes 0.  code = sign | the E2M1 magnitude nearest the exact quotient |w| / 2^e on {0, .5, 1, 1.5, 2, 3, 4, 6},
            ties to the code with low bit 0; scale byte = e + 127; dq = code * 2^e, always exactly a bf16.  A non-finite weight or |w| >= 2^100 is refused.
  stream    a chunk slot (8 codes = 4 bytes of each of 64 lanes, one scale byte of each of 16 lane groups) is 272 bytes: row_bytes = ks * NX * 272

Everything works on bf16 bit patterns (uint16) and float64 values: every bf16, every quotient by a power of two and every dq is exact in float64."""
import numpy as np

from fp8_ref import bf16_bits, bf16_value

E_MIN, BLOCK = -125, 32
GRID = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6])


def block_exponents(W):
    """W: uint16 [N][K] -> e of every block (int64 [N][ceil(K / 32)]); ValueError where the rule refuses the matrix"""
    N, K = W.shape
    nb = -(-K // BLOCK)
    mag = np.zeros((N, nb * BLOCK), np.uint16)
    mag[:, :K] = W & 0x7FFF
    amax = bf16_value(mag.reshape(N, nb, BLOCK).max(axis=2))      # (magnitudes order as their patterns do; a NaN pattern is the largest)
    if not np.isfinite(amax).all() or (amax >= 2.0 ** 100).any():
        raise ValueError("non-finite weight or |w| >= 2^100")
    m, x = np.frexp(amax)                                         # amax = m * 2^x, m in [0.5, 1): the rule's m is twice that, its x one less
    e = np.maximum(np.where(m <= 0.75, x - 3, x - 2), E_MIN).astype(np.int64)
    e[amax == 0] = 0
    return e


def round_to_codes(q):
    """exact quotients q (float64, |q| <= 6) -> uint8 codes; the sign of q, -0 included, is kept"""
    a = np.abs(q)
    assert (a <= 6).all()
    step = np.where(a < 2, 0.5, np.where(a < 4, 1.0, 2.0))
    v = np.rint(a / step) * step                                  # half-to-even on the count of steps, whose parity is the code's
    return (np.searchsorted(GRID, v) | np.where(np.signbit(q), 8, 0)).astype(np.uint8)


def code_value(code):
    c = np.asarray(code, np.int64)
    return np.where(c & 8, -GRID[c & 7], GRID[c & 7])


def _apply(W, which):
    """(codes, dq patterns)[which] of W and the block exponents: the rule applied once per (exponent, pattern) instead of once per weight"""
    W = np.asarray(W, np.uint16)
    e = block_exponents(W)
    ek = np.repeat(e, BLOCK, axis=1)[:, :W.shape[1]]
    out = np.zeros(W.shape, (np.uint8, np.uint16)[which])
    pats = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    val = bf16_value(pats)
    for ev in np.unique(e):
        ok = np.isfinite(val) & (np.abs(np.where(np.isfinite(val), val, 0.0)) <= 6 * 2.0 ** int(ev))
        table = np.zeros(0x10000, out.dtype)
        codes = round_to_codes(np.ldexp(val[ok], -int(ev)))
        table[ok] = codes if which == 0 else bf16_bits(np.ldexp(code_value(codes), int(ev)))
        sel = ek == ev
        out[sel] = table[W[sel]]
    return out, e


def quantize(W):
    """W: uint16 [N][K] -> (codes uint8 [N][K], scale bytes uint8 [N][ceil(K / 32)])"""
    codes, e = _apply(W, 0)
    return codes, (e + 127).astype(np.uint8)


def dequantized(W):
    """the bf16 master that tgx_finalize leaves with weights.fp4 = 1: what an ordinary context must be uploaded to compute the same model"""
    W = np.asarray(W, np.uint16)
    return _apply(W.reshape(-1, W.shape[-1]), 1)[0].reshape(W.shape)


def row_bytes(K, ks):
    nx = (K // 8 + ks * 64 - 1) // (ks * 64)
    return ks * nx * 272
