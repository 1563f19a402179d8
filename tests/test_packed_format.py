"""The exponent-packed weight format (tinygpt_amd/csrc/kernels/gemv_packed.h) as a numpy reference packer / unpacker: the written
specification of the layout.  No GPU: the device packer and kernels are held to bit identity with the plain kernels in tests/test_hip_packed.py.

  code      c = exponent field - E0, E0 = max(Emax - 15, 0), Emax = largest exponent field below 255 of the matrix; c outside 1..15 -> 0 (escape)
  chunk     8 consecutive k -> S0, S1 (bytes sign << 7 | mantissa in the order w0 w2 w1 w3 / w4 w6 w5 w7) and C (code of w[2t] at bit 4t, of w[2t+1] at 4t + 16)
  record    per row 4 entries k << 16 | bits, unused 0xffffffff; a row with more than 4 escapes -> the matrix is not packed
  planes    lane l of k-part p owns chunks p * per + l + 64 j; quads of 4 chunks in three [64 lanes][4 dwords] planes (S of chunks 0-1, S of chunks 2-3, C of 0-3)
"""
import numpy as np
import pytest

ESC = 4


def geometry(K, ks):
    nchunk = K // 8
    nx = (nchunk + ks * 64 - 1) // (ks * 64)
    return nchunk, nx, (nx + 3) // 4, 64 * nx


def pack(W, ks):
    """W: uint16 [N][K] bf16 patterns.  Returns None (fallback: the matrix stays plain) or (planes uint32 [N][ks][NQ][3][64][4], records uint32 [N][4], E0)."""
    N, K = W.shape
    assert K % 8 == 0 and K <= 32768
    e = (W >> 7) & 0xFF
    finite = e[e < 255]
    E0 = max(int(finite.max()) - 15 if finite.size else 0, 0)
    code = e.astype(np.int64) - E0
    code[(code < 1) | (code > 15)] = 0
    rec = np.full((N, ESC), 0xFFFFFFFF, np.uint32)
    for r in range(N):
        ks_ = np.nonzero(code[r] == 0)[0]
        if ks_.size > ESC:
            return None
        rec[r, :ks_.size] = (ks_.astype(np.uint32) << 16) | W[r, ks_]
    b = (((W >> 8) & 0x80) | (W & 0x7F)).astype(np.uint32)
    nchunk, nx, nq, per = geometry(K, ks)
    bc, cc = b.reshape(N, nchunk, 8), code.reshape(N, nchunk, 8).astype(np.uint32)
    S0 = bc[..., 0] | (bc[..., 2] << 8) | (bc[..., 1] << 16) | (bc[..., 3] << 24)
    S1 = bc[..., 4] | (bc[..., 6] << 8) | (bc[..., 5] << 16) | (bc[..., 7] << 24)
    C = np.zeros((N, nchunk), np.uint32)
    for t in range(4):
        C |= (cc[..., 2 * t] << (4 * t)) | (cc[..., 2 * t + 1] << (4 * t + 16))
    P = np.zeros((N, ks, nq, 3, 64, 4), np.uint32)
    P[:, :, :, 2] = 0x11111111          # padding: S = 0, every code 1
    lanes = np.arange(64)
    for p in range(ks):
        c_begin = min(p * per, nchunk); c_end = min(c_begin + per, nchunk)
        for j in range(nx):
            c = c_begin + lanes + 64 * j
            ok = c < c_end
            q, jj = divmod(j, 4)
            P[:, p, q, jj >> 1, lanes[ok], (jj & 1) * 2] = S0[:, c[ok]]
            P[:, p, q, jj >> 1, lanes[ok], (jj & 1) * 2 + 1] = S1[:, c[ok]]
            P[:, p, q, 2, lanes[ok], jj] = C[:, c[ok]]
    return P, rec, E0


def unpack(P, rec, E0, K, ks):
    """What a lane of the kernel rebuilds: four dwords per chunk from (S0, S1, C, base), then the repair from the row's record."""
    N = P.shape[0]
    nchunk, nx, nq, per = geometry(K, ks)
    base2 = np.uint32((E0 << 7) | (E0 << 23))
    out = np.zeros((N, nchunk, 4), np.uint32)
    lanes = np.arange(64)
    for p in range(ks):
        c_begin = min(p * per, nchunk); c_end = min(c_begin + per, nchunk)
        for j in range(nx):
            c = c_begin + lanes + 64 * j
            ok = c < c_end
            q, jj = divmod(j, 4)
            S = [P[:, p, q, jj >> 1, lanes[ok], (jj & 1) * 2], P[:, p, q, jj >> 1, lanes[ok], (jj & 1) * 2 + 1]]
            C = P[:, p, q, 2, lanes[ok], jj]
            for dd in range(4):
                s = S[dd >> 1]
                v = ((s & 0x007F007F) | ((s << 8) & 0x80008000)) if dd % 2 == 0 else (((s >> 8) & 0x007F007F) | (s & 0x80008000))
                out[:, c[ok], dd] = v + ((((C >> (4 * dd)) & 0x000F000F) << 7) + base2)
    W = np.zeros((N, nchunk, 8), np.uint16)
    W[..., 0::2] = (out & 0xFFFF).astype(np.uint16)
    W[..., 1::2] = (out >> 16).astype(np.uint16)
    W = W.reshape(N, K)
    for r in range(N):                     # the repair (the kernel enters it only for chunks whose C has a zero nibble: every escape has one)
        for en in rec[r]:
            if en != 0xFFFFFFFF:
                W[r, int(en) >> 16] = int(en) & 0xFFFF
    return W


def roundtrip(W, ks):
    got = pack(W, ks)
    return W.copy() if got is None else unpack(*got, W.shape[1], ks)       # fallback: the bf16 original is what the plain kernel reads


def all_patterns_matrix():
    """every one of the 65 536 bf16 patterns in one [N][8] matrix, at most four out-of-window values per row (Emax = 254: the window is 239 + 1..15)"""
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
    assert got is not None and got[2] == 239
    assert (got[1] != 0xFFFFFFFF).sum() == 65536 - 15 * 256            # every out-of-window pattern sits in a record
    np.testing.assert_array_equal(unpack(*got, 8, 1), W)


def test_a_row_with_five_escapes_sends_the_matrix_to_the_fallback():
    W = all_patterns_matrix()
    W[7, 1] = 0x0000                     # a fifth out-of-window value in row 7
    assert pack(W, 1) is None
    np.testing.assert_array_equal(roundtrip(W, 1), W)


@pytest.mark.parametrize("K,ks", [(8, 1), (256, 1), (2048, 1), (1032, 2), (8192, 4), (320, 2), (4096, 1)])
def test_layouts_with_k_splits_quads_and_padding(K, ks):
    rng = np.random.default_rng(K + ks)
    N = 6
    x = (rng.uniform(-0.0346, 0.0346, (N, K)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    for r, (k, bits) in enumerate([(0, 0x0000), (K - 1, 0x8000), (K // 2, 0x0001), (3, 0x7F80), (K - 8, 0xFFC1)]):
        x[r, k] = bits                   # +0, -0, a subnormal, inf, a NaN: one per row (row 5 keeps only what the draw gave it)
    got = pack(x, ks)
    assert got is not None
    P, rec, E0 = got
    nchunk, nx, nq, per = geometry(K, ks)
    assert P[0].nbytes == ks * nq * 3072
    if nchunk % (64 * 4 * ks) == 0:
        assert P[0].nbytes == K * 3 // 2          # no padding: 12 bits per weight
    np.testing.assert_array_equal(unpack(P, rec, E0, K, ks), x)
