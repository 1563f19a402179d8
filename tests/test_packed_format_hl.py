"""The "HL" exponent-packed weight format (tinygpt_amd/csrc/kernels/gemv_packed.h) as a numpy reference packer / unpacker: the written
specification of the LIVE layout.  (tests/test_packed_format.py specifies the S/C layout this one replaced; it keeps passing as arithmetic but no kernel
reads that layout any more.)  No GPU: the device packer and kernels are held to bit identity with the plain kernels in tests/test_hip_packed.py and
tests/test_hip_packed_hl.py.

  window    E0h = max((Emax >> 1) - 7, 0), Emax = largest exponent field below 255 of the matrix.  In band: exponent field in [2 E0h, 2 E0h + 15], not 0, not 255
  chunk     8 consecutive k -> L0, L1 (the low bytes e0 << 7 | mantissa of w0..w3 / w4..w7 in k order) and Nb (nibble of w[t] at bit 8t, of w[4 + t] at 8t + 4);
            nibble = sign << 3 | ((exponent field >> 1) - E0h); an out-of-band weight is written as nibble 0, L 0 (no in-band flag) and listed in the record
  decode    t = Nb & 0x0f0f0f0f (w0..w3) or (Nb >> 4) & 0x0f0f0f0f (w4..w7); H4 = (((t << 4) + t) & 0x87878787) + E0h * 0x01010101;
            weight t as fp32 bits = H4.byte[t] << 24 | L.byte[t] << 16
  record    per row 4 entries k << 16 | bits, unused 0xffffffff; a row with more than 4 escapes -> the matrix is not packed
  planes    lane l of k-part p owns chunks p * per + l + 64 j; quads of 4 chunks in three [64 lanes][4 dwords] planes (L of chunks 0-1, L of chunks 2-3, Nb of 0-3)
"""
import numpy as np
import pytest

ESC = 4
M32 = 0xFFFFFFFF


def geometry(K, ks):
    nchunk = K // 8
    nx = (nchunk + ks * 64 - 1) // (ks * 64)
    return nchunk, nx, (nx + 3) // 4, 64 * nx


def window_base(W):
    e = (W >> 7) & 0xFF
    finite = e[e < 255]
    emax = int(finite.max()) if finite.size else 0
    return max((emax >> 1) - 7, 0)


def in_band(W, E0h):
    e = ((W >> 7) & 0xFF).astype(np.int64)
    d = (e >> 1) - E0h
    return (d >= 0) & (d <= 7) & (e != 0) & (e != 255)


def high4(t, E0h):
    """the kernel's arithmetic on a whole dword of four nibbles (one per byte); uint64 holds the intermediate, the result is taken mod 2^32 as the VALU does"""
    t = np.asarray(t, np.uint64)
    return (((((t << np.uint64(4)) + t) & np.uint64(M32)) & np.uint64(0x87878787)) + np.uint64(E0h * 0x01010101)) & np.uint64(M32)


def pack(W, ks):
    """W: uint16 [N][K] bf16 patterns.  Returns None (fallback: the matrix stays plain) or (planes uint32 [N][ks][NQ][3][64][4], records uint32 [N][4], E0h)."""
    N, K = W.shape
    assert K % 8 == 0 and K <= 32768
    E0h = window_base(W)
    band = in_band(W, E0h)
    rec = np.full((N, ESC), M32, np.uint32)
    for r in range(N):
        ks_ = np.nonzero(~band[r])[0]
        if ks_.size > ESC:
            return None
        rec[r, :ks_.size] = (ks_.astype(np.uint32) << 16) | W[r, ks_]
    lo = np.where(band, W & 0xFF, 0).astype(np.uint32)
    nib = np.where(band, ((W >> 12) & 8) | (((W >> 8) & 0x7F).astype(np.int64) - E0h), 0).astype(np.uint32)
    nchunk, nx, nq, per = geometry(K, ks)
    lc, nc = lo.reshape(N, nchunk, 8), nib.reshape(N, nchunk, 8)
    L0 = lc[..., 0] | (lc[..., 1] << 8) | (lc[..., 2] << 16) | (lc[..., 3] << 24)
    L1 = lc[..., 4] | (lc[..., 5] << 8) | (lc[..., 6] << 16) | (lc[..., 7] << 24)
    Nb = np.zeros((N, nchunk), np.uint32)
    for t in range(4):
        Nb |= (nc[..., t] << (8 * t)) | (nc[..., 4 + t] << (8 * t + 4))
    P = np.zeros((N, ks, nq, 3, 64, 4), np.uint32)          # padding: all zero
    lanes = np.arange(64)
    for p in range(ks):
        c_begin = min(p * per, nchunk); c_end = min(c_begin + per, nchunk)
        for j in range(nx):
            c = c_begin + lanes + 64 * j
            ok = c < c_end
            q, jj = divmod(j, 4)
            P[:, p, q, jj >> 1, lanes[ok], (jj & 1) * 2] = L0[:, c[ok]]
            P[:, p, q, jj >> 1, lanes[ok], (jj & 1) * 2 + 1] = L1[:, c[ok]]
            P[:, p, q, 2, lanes[ok], jj] = Nb[:, c[ok]]
    return P, rec, E0h


def unpack(P, rec, E0h, K, ks):
    """What a lane of the kernel computes: per chunk the two H4 dwords, the byte selection into fp32 bit patterns, then the repair from the row's record
    (which the kernel runs only for a row whose record is non-empty).  Returns the bf16 patterns (the fp32 patterns' upper halves; the lower are zero)."""
    N = P.shape[0]
    nchunk, nx, nq, per = geometry(K, ks)
    F = np.zeros((N, nchunk, 8), np.uint32)
    lanes = np.arange(64)
    for p in range(ks):
        c_begin = min(p * per, nchunk); c_end = min(c_begin + per, nchunk)
        for j in range(nx):
            c = c_begin + lanes + 64 * j
            ok = c < c_end
            q, jj = divmod(j, 4)
            L = [P[:, p, q, jj >> 1, lanes[ok], (jj & 1) * 2], P[:, p, q, jj >> 1, lanes[ok], (jj & 1) * 2 + 1]]
            Nb = P[:, p, q, 2, lanes[ok], jj]
            H = [high4(Nb & 0x0F0F0F0F, E0h), high4((Nb >> 4) & 0x0F0F0F0F, E0h)]
            for t in range(8):
                h, b = t >> 2, 8 * (t & 3)
                F[:, c[ok], t] = ((((H[h] >> np.uint64(b)) & np.uint64(0xFF)) << np.uint64(24)) | (((L[h] >> b) & 0xFF).astype(np.uint64) << np.uint64(16))).astype(np.uint32)
    F = F.reshape(N, K)
    for r in range(N):
        if rec[r, 0] != M32:               # records fill from entry 0
            for en in rec[r]:
                if en != M32:
                    F[r, int(en) >> 16] = (int(en) & 0xFFFF) << 16
    assert not (F & 0xFFFF).any()
    return (F >> 16).astype(np.uint16)


def roundtrip(W, ks):
    got = pack(W, ks)
    return W.copy() if got is None else unpack(*got, W.shape[1], ks)       # fallback: the bf16 original is what the plain kernel reads


def all_patterns_matrix():
    """every one of the 65 536 bf16 patterns in one [N][8] matrix, at most four out-of-band values per row (Emax = 254: E0h = 120, the band is 240..254)"""
    allp = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    e = (allp >> 7) & 0xFF
    inw = (e >= 240) & (e <= 254)
    win, out = allp[inw], allp[~inw]
    assert win.size == 15 * 256 and out.size % 4 == 0
    N = out.size // 4
    W = np.empty((N, 8), np.uint16)
    W[:, [0, 3, 5, 6]] = out.reshape(N, 4)
    W[:, [1, 2, 4, 7]] = np.resize(win, N * 4).reshape(N, 4)
    return W


def test_every_bf16_pattern_round_trips_through_codes_and_escape_records():
    W = all_patterns_matrix()
    assert np.unique(W).size == 65536
    got = pack(W, 1)
    assert got is not None and got[2] == 120
    assert (got[1] != M32).sum() == 65536 - 15 * 256            # every out-of-band pattern sits in a record
    np.testing.assert_array_equal(unpack(*got, 8, 1), W)


def test_escapes_are_written_in_band_as_zero_nibble_and_zero_low_byte():
    W = all_patterns_matrix()
    P, rec, E0h = pack(W, 1)
    # NX = 1 at K = 8: lane 0 holds the row's only chunk, quad 0
    for shift in (0, 24):
        assert not ((P[:, 0, 0, 0, 0, 0] >> shift) & 0xFF).any()       # L0 bytes of w0, w3
        assert not ((P[:, 0, 0, 2, 0, 0] >> shift) & 0x0F).any()       # their nibbles
    assert not ((P[:, 0, 0, 0, 0, 1] >> 8) & 0xFFFF).any()             # L1 bytes of w5, w6
    assert not ((P[:, 0, 0, 2, 0, 0] >> 12) & 0x0F).any() and not ((P[:, 0, 0, 2, 0, 0] >> 20) & 0x0F).any()


def test_dword_high_byte_arithmetic_equals_the_per_byte_definition():
    """H4 on whole dwords against sign << 7 | (d + E0h) per byte, for all 16 nibbles in every byte position and every legal E0h (Emax <= 254)"""
    nibs = np.arange(16, dtype=np.uint64)
    a, b, c, d = np.meshgrid(nibs, nibs[::5], nibs[::3], nibs, indexing="ij")      # every nibble in bytes 0 and 3, a spread in bytes 1 and 2 ...
    t1 = (a | (b << np.uint64(8)) | (c << np.uint64(16)) | (d << np.uint64(24))).ravel()
    a, b, c, d = np.meshgrid(nibs[::5], nibs, nibs, nibs[::3], indexing="ij")      # ... and the other way round
    t2 = (a | (b << np.uint64(8)) | (c << np.uint64(16)) | (d << np.uint64(24))).ravel()
    t = np.concatenate([t1, t2])
    for E0h in range(0, 121):
        got = high4(t, E0h)
        for byte in range(4):
            n = (t >> np.uint64(8 * byte)) & np.uint64(15)
            want = ((n >> np.uint64(3)) << np.uint64(7)) | ((n & np.uint64(7)) + np.uint64(E0h))
            assert (want <= 0xFF).all()
            np.testing.assert_array_equal((got >> np.uint64(8 * byte)) & np.uint64(0xFF), want)


def test_a_row_with_five_escapes_is_reported_as_overflow():
    W = all_patterns_matrix()
    W[7, 1] = 0x0000                     # a fifth out-of-band value in row 7
    assert pack(W, 1) is None
    np.testing.assert_array_equal(roundtrip(W, 1), W)


@pytest.mark.parametrize("K,ks", [(64, 1), (1536, 2), (2048, 1), (8192, 4)])
def test_layouts_with_k_splits_quads_and_padding(K, ks):
    rng = np.random.default_rng(K + ks)
    N = 6
    x = (rng.uniform(-0.0346, 0.0346, (N, K)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    for r, (k, bits) in enumerate([(0, 0x0000), (K - 1, 0x8000), (K // 2, 0x0001), (3, 0x7F80), (K - 8, 0xFFC1)]):
        x[r, k] = bits                   # +0, -0, a subnormal, inf, a NaN: one per row (row 5 keeps only what the draw gave it)
    got = pack(x, ks)
    assert got is not None
    P, rec, E0h = got
    nchunk, nx, nq, per = geometry(K, ks)
    assert P[0].nbytes == ks * nq * 3072
    if nchunk % (64 * 4 * ks) == 0:
        assert P[0].nbytes == K * 3 // 2          # no padding: 12 bits per weight
    else:
        assert nchunk < ks * nq * 4 * 64          # (64 / ks 1 and 1536 / ks 2: padding chunks exist)
    np.testing.assert_array_equal(unpack(P, rec, E0h, K, ks), x)


def binades_in_band(emax):
    W = np.zeros((1, 8), np.uint16)
    W[0, :] = emax << 7
    E0h = window_base(W)
    e = np.arange(1, 255)
    band = in_band((e << 7).astype(np.uint16), E0h)
    assert band[e == emax].all()
    lo, hi = e[band].min(), e[band].max()
    assert band.sum() == hi - lo + 1              # one contiguous range
    return int((e[band] <= emax).sum()), lo, hi


def test_even_emax_covers_15_binades_and_odd_emax_16():
    for emax in range(16, 255):
        n, lo, hi = binades_in_band(emax)
        assert n == (16 if emax & 1 else 15), emax
        assert lo == 2 * ((emax >> 1) - 7)
    # the benchmark checkpoint's Emax = 122: exponent fields 108..122, the same fifteen as the S/C format's window E0 + 1 .. E0 + 15 = 108..122
    assert binades_in_band(122) == (15, 108, 123)
    # small Emax: the window starts at exponent field 0, which itself (zeros, subnormals) stays an escape
    assert binades_in_band(9) == (9, 1, 15)
