"""Option weights.fp8 as numpy: the written specification of the quantization rule (include/tgx.h) and of the 8-bit stream layout
(tinygpt_amd/csrc/kernels/gemv_fp8.h).  No GPU.  tests/test_fp8_ref.py holds it to torch's float8_e4m3fn cast; the GPU tests upload dequantized(W) to an
ordinary context and hold the quantized context to it bit for bit.

  rule      per output row r: amax = max |w| = m * 2^x, m in [0.5, 1) (frexp); e_r = x - 9 if m <= 0.875 else x - 8 (the smallest e with amax <= 448 * 2^e),
            clamped to >= -117; an all-zero row takes 0.  code = RNE of the exact quotient w / 2^e_r onto the OCP e4m3fn grid (subnormals of step 2^-9, sign
            kept, 0x7f / 0xff never produced); dq = code * 2^e_r, always exactly a bf16.  A non-finite weight or |w| >= 2^100 is refused.
  chunk     the 8 codes of 8 consecutive k, 8 bytes in k order
  planes    lane l of k-part p owns chunks p * per + l + 64 j (per = 64 NX, NX = ceil(K / 8 / (64 ks))); pairs h = j // 2 of chunks in one [64 lanes][16 bytes]
            plane: chunk 2h then chunk 2h + 1.  Row r, k-part p, plane h at byte r * row_bytes + (p * NH + h) * 1024, NH = ceil(NX / 2).  Padding: code 0.
  scales    [N] fp32 2^e_r

Everything here works on bf16 bit patterns (uint16) and float64 values: every bf16, every quotient by a power of two and every dq is exact in float64."""
import numpy as np

E_MIN = -117
REFUSE = 2.0 ** 100


def bf16_value(bits):
    with np.errstate(invalid="ignore"):      # (a signalling NaN pattern is quieted on the way to float64: nobody reads its payload)
        return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_bits(v):
    """float64 values that ARE bf16 values -> their patterns (asserts that nothing is rounded)"""
    f = np.asarray(v, np.float64).astype(np.float32)
    assert (f.astype(np.float64) == v).all()
    u = f.view(np.uint32)
    assert ((u & 0xFFFF) == 0).all()
    return (u >> 16).astype(np.uint16)


def row_exponents(W):
    """W: uint16 [N][K].  e_r of every row (int64 [N]); ValueError where the rule refuses the matrix"""
    amax = np.abs(bf16_value((np.asarray(W, np.uint16) & 0x7FFF).max(axis=1)))      # (magnitudes order as their patterns do; a NaN pattern is the largest)
    if not np.isfinite(amax).all() or (amax >= REFUSE).any():
        raise ValueError("non-finite weight or |w| >= 2^100")
    m, x = np.frexp(amax)
    e = np.where(m <= 0.875, x - 9, x - 8).astype(np.int64)
    e = np.maximum(e, E_MIN)
    e[amax == 0] = 0
    return e


def code_value(code):
    """the value of an e4m3fn code (float64); 0x7f / 0xff are NaN and never asked for"""
    c = np.asarray(code, np.int64)
    ef, mm = (c >> 3) & 15, c & 7
    mag = np.where(ef == 0, mm * 2.0 ** -9, np.ldexp(1.0 + mm / 8.0, ef - 7))
    return np.where(c & 0x80, -mag, mag)


def round_to_codes(q):
    """RNE of exact quotients q (float64, |q| <= 448) onto the e4m3fn grid -> uint8 codes; the sign of q, -0 included, is kept"""
    q = np.asarray(q, np.float64)
    a = np.abs(q)
    assert (a <= 448).all()
    _, x = np.frexp(a)                                        # a = m * 2^x, m in [0.5, 1): floor(log2 a) = x - 1
    step = np.ldexp(1.0, np.maximum(x - 1 - 3, -9))           # four significant bits, never finer than the subnormal step
    v = np.rint(a / step) * step                              # (a / step is exact: a power-of-two divisor; rint is half-to-even)
    _, xv = np.frexp(v)
    E = xv - 1
    code = np.where(v < 2.0 ** -6, np.rint(v * 512.0), ((E + 7) << 3) + np.rint((np.ldexp(v, -E) - 1.0) * 8.0)).astype(np.int64)
    code = np.where(v == 0, 0, code)
    return (code | np.where(np.signbit(q), 0x80, 0)).astype(np.uint8)


def _tables(e):
    """(code, dq pattern) of every bf16 pattern a row of exponent e can hold, indexed by pattern — the rule applied once per pattern instead of once per weight"""
    pats = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    val = bf16_value(pats)
    ok = np.isfinite(val) & (np.abs(np.where(np.isfinite(val), val, 0.0)) <= 448 * 2.0 ** int(e))
    codes, dq = np.zeros(0x10000, np.uint8), np.zeros(0x10000, np.uint16)
    codes[ok] = round_to_codes(np.ldexp(val[ok], -int(e)))
    dq[ok] = bf16_bits(np.ldexp(code_value(codes[ok]), int(e)))
    return codes, dq


def _apply(W, which):
    W = np.asarray(W, np.uint16)
    e = row_exponents(W)
    out = np.zeros(W.shape, (np.uint8, np.uint16)[which])
    for ev in np.unique(e):
        rows = e == ev
        out[rows] = _tables(ev)[which][W[rows]]
    return out, e


def quantize(W):
    """W: uint16 [N][K] -> (codes uint8 [N][K], e int64 [N])"""
    return _apply(W, 0)


def dequantize(codes, e):
    """code * 2^e as bf16 patterns [N][K]"""
    return bf16_bits(np.ldexp(code_value(codes), np.asarray(e)[:, None]))


def dequantized(W):
    """the bf16 master that tgx_finalize leaves with weights.fp8 = 1: what an ordinary context must be uploaded to compute the same model"""
    W = np.asarray(W, np.uint16)
    return _apply(W.reshape(-1, W.shape[-1]), 1)[0].reshape(W.shape)


# ---- the device quantizer's arithmetic (kernels/gemv_fp8.h fp8_row_exp / fp8_code / fp8_dq_bits), integer for integer -------------------------------
def row_exponents_int(W):
    amax = (np.asarray(W, np.uint16) & 0x7FFF).max(axis=1).astype(np.int64)
    Ef, M = amax >> 7, amax & 0x7F
    e = np.maximum(np.where(M <= 0x60, Ef - 126 - 9, Ef - 126 - 8), E_MIN)
    e = np.where(Ef == 0, E_MIN, e)
    return np.where(amax == 0, 0, e)


def code_int(bits, e):
    bits = np.asarray(bits, np.int64)
    e = np.asarray(e, np.int64)
    s, Ef, M = (bits >> 8) & 0x80, (bits >> 7) & 0xFF, bits & 0x7F
    sig = np.where(Ef != 0, 0x80 | M, M)
    t9 = np.where(Ef != 0, Ef, 1) - 134 - e + 9
    msb = np.floor(np.log2(np.maximum(sig, 1))).astype(np.int64)
    g = np.maximum(msb + t9 - 3, 0)
    sh = g - t9
    shc = np.clip(sh, 1, 9)
    q, rem, half = sig >> shc, sig & ((1 << shc) - 1), 1 << (shc - 1)
    r_round = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    r = np.where(sh <= 0, sig << np.clip(-sh, 0, 8), np.where(sh > 9, 0, r_round))
    return np.where(sig == 0, s, s | ((g << 3) + r)).astype(np.uint8)


def dq_bits_int(code, e):
    code = np.asarray(code, np.int64)
    e = np.asarray(e, np.int64)
    s, ef, mm = (code & 0x80) << 8, (code >> 3) & 15, code & 7
    r = np.where(ef != 0, 8 + mm, mm)
    g = np.where(ef != 0, ef - 1, 0)
    mb = np.floor(np.log2(np.maximum(r, 1))).astype(np.int64)
    out = s | ((mb + g - 9 + e + 127) << 7) | ((r << (7 - mb)) & 0x7F)
    return np.where(r == 0, s, out).astype(np.uint16)


# ---- the stream layout -------------------------------------------------------------------------------------------------------------------------------
def geometry(K, ks):
    """(chunks per row, NX, NH, chunks per k-part)"""
    nchunk = K // 8
    nx = (nchunk + ks * 64 - 1) // (ks * 64)
    return nchunk, nx, (nx + 1) // 2, 64 * nx


def row_bytes(K, ks):
    return ks * geometry(K, ks)[2] * 1024


def covered(K, ks):
    """the layout serves K % 8 == 0 at up to 8 chunks per lane"""
    return K % 8 == 0 and geometry(K, ks)[1] <= 8


def to_planes(codes, ks):
    """codes uint8 [N][K] -> planes uint8 [N][ks][NH][64][16] (padding 0)"""
    N, K = codes.shape
    assert covered(K, ks)
    nchunk, nx, nh, per = geometry(K, ks)
    ch = codes.reshape(N, nchunk, 8)
    P = np.zeros((N, ks, nh, 64, 16), np.uint8)
    for p in range(ks):
        c_begin = min(p * per, nchunk); c_end = min(c_begin + per, nchunk)
        for j in range(nx):
            for l in range(64):
                c = c_begin + l + 64 * j
                if c < c_end:
                    P[:, p, j // 2, l, 8 * (j & 1):8 * (j & 1) + 8] = ch[:, c]
    return P


def from_planes(P, K, ks):
    """the inverse of to_planes: what lane l of k-part p reads as chunk j, put back at its k"""
    N = P.shape[0]
    nchunk, nx, nh, per = geometry(K, ks)
    assert P.shape == (N, ks, nh, 64, 16)
    ch = np.zeros((N, nchunk, 8), np.uint8)
    for p in range(ks):
        c_begin = min(p * per, nchunk); c_end = min(c_begin + per, nchunk)
        for j in range(nx):
            for l in range(64):
                c = c_begin + l + 64 * j
                if c < c_end:
                    ch[:, c] = P[:, p, j // 2, l, 8 * (j & 1):8 * (j & 1) + 8]
    return ch.reshape(N, K)
