"""The escape records of the "HL" exponent-packed format PER (ROW, K-PART) (tinygpt_amd/csrc/kernels/gemv_packed.h): the written
specification of the record layout, as a numpy packer / unpacker over the planes of tests/test_packed_format_hl.py (which this file imports: the planes, the
window and the decode arithmetic are unchanged).  No GPU: the device packer and kernels are held to bit identity with the plain kernels in
tests/test_hip_packed_kpart.py.

  record    rec[row][p], p = 0..ks-1: 4 entries k << 16 | bits (k the ROW's k), unused 0xffffffff, filled from entry 0 in k order, of the escapes whose chunk
            k // 8 lies in K-part p's range [c_begin(p), c_end(p)) = [min(p * per, nchunk), min(p * per + per, nchunk)), per = 64 * NX
  overflow  more than 4 escapes in one (row, K-part) -> the matrix is not packed.  A row may hold 4 * ks escapes.
  repair    the wave of K-part p reads rec[row][p] only
  ks = 1    one record per row: the layout of test_packed_format_hl.pack()
"""
import numpy as np
import pytest

from test_packed_format_hl import ESC, M32, geometry, in_band, pack as pack_hl, unpack as unpack_hl, window_base

CASES = [(2048, 1), (8192, 4), (8200, 4), (512, 1)]


def part_ranges(K, ks):
    nchunk, nx, nq, per = geometry(K, ks)
    return [(min(p * per, nchunk), min(min(p * per, nchunk) + per, nchunk)) for p in range(ks)]


def pack(W, ks):
    """W: uint16 [N][K].  Returns None (fallback) or (planes as test_packed_format_hl.pack lays them out, records uint32 [N][ks][4], E0h)."""
    N, K = W.shape
    E0h = window_base(W)
    band = in_band(W, E0h)
    rec = np.full((N, ks, ESC), M32, np.uint32)
    for r in range(N):
        esc = np.nonzero(~band[r])[0]
        for p, (cb, ce) in enumerate(part_ranges(K, ks)):
            mine = esc[(esc // 8 >= cb) & (esc // 8 < ce)]
            if mine.size > ESC:
                return None
            rec[r, p, :mine.size] = (mine.astype(np.uint32) << 16) | W[r, mine]
    # The planes do not depend on the records.  An escape is written as nibble 0, low byte 0, which is what the in-band pattern (2 E0h) << 7 (sign 0, exponent
    # field 2 E0h, mantissa 0) packs to: the per-row packer gives the planes from a copy with that pattern in every escape's place (E0h > 0 in the cases here;
    # the copy keeps W[0, 0], hence Emax and the window).
    assert E0h > 0 and band[0, 0]
    planes = pack_hl(np.where(band, W, np.uint16((2 * E0h) << 7)), ks)
    assert planes is not None and planes[2] == E0h and (planes[1] == M32).all()
    return planes[0], rec, E0h


def unpack(P, rec, E0h, K, ks):
    """the planes decoded as every lane does, then, K-part by K-part, the repair the wave of that part runs: from ITS record, over ITS chunks only"""
    N = P.shape[0]
    F = unpack_hl(P, np.full((N, ESC), M32, np.uint32), E0h, K, ks)         # no repair
    for r in range(N):
        for p, (cb, ce) in enumerate(part_ranges(K, ks)):
            if rec[r, p, 0] != M32:                   # records fill from entry 0
                for en in rec[r, p]:
                    if en != M32 and cb <= (int(en) >> 19) < ce:          # an entry outside the wave's chunks never meets a lane of it
                        F[r, int(en) >> 16] = int(en) & 0xFFFF
    return F


def weights(N, K, seed):
    rng = np.random.default_rng(seed)
    x = (rng.uniform(0.004, 0.0346, (N, K)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)        # three binades: no escape of the draw's own
    x[rng.random((N, K)) < 0.5] |= 0x8000
    x[0, 0] = 0x3D0E                                   # pins Emax = 122 (the benchmark checkpoint's): E0h = 54
    return x


PLANTED = [0x0000, 0x8000, 0x0001, 0x007F, 0x7F80, 0xFF80, 0xFFC1, ((122 - 40) << 7) | 0x55, 0x8000 | ((122 - 16) << 7) | 0x2A]      # +-0, subnormals, +-inf, NaN, below the window


@pytest.mark.parametrize("K,ks", CASES)
def test_every_planted_pattern_round_trips(K, ks):
    N = len(PLANTED) + 2
    W = weights(N, K, K + ks)
    assert window_base(W) == 54 and in_band(W, 54).all()
    ranges = part_ranges(K, ks)
    for r, bits in enumerate(PLANTED):
        for p, (cb, ce) in enumerate(ranges):
            if ce > cb:                                # (8200 / ks 4: per = 320 chunks, the fourth part holds 65; 512 / ks 1: one part)
                ks_ = sorted({8 * cb + (r % 8), 8 * ce - 1 - (r % 8)} - {0})
                W[r, ks_] = bits
    got = pack(W, ks)
    assert got is not None
    P, rec, E0h = got
    assert rec.shape == (N, ks, ESC)
    np.testing.assert_array_equal(unpack(P, rec, E0h, K, ks), W)
    # every entry sits in the record of the part that owns its chunk
    for r in range(N):
        for p, (cb, ce) in enumerate(ranges):
            for en in rec[r, p][rec[r, p] != M32]:
                assert cb <= (int(en) >> 19) < ce


def test_four_escapes_in_each_of_four_k_parts_pack():
    K, ks = 8192, 4
    W = weights(3, K, 1)
    for p in range(4):
        W[1, [2048 * p, 2048 * p + 9, 2048 * p + 1000, 2048 * p + 2047]] = [0x0000, 0x8000, 0x0003, 0x0000]
    got = pack(W, ks)
    assert got is not None                             # 16 escapes in the row
    P, rec, E0h = got
    assert (rec[1] != M32).all() and (rec[0] == M32).all() and (rec[2] == M32).all()
    assert pack_hl(W, ks) is None                      # (the per-row record of four could not hold them)
    np.testing.assert_array_equal(unpack(P, rec, E0h, K, ks), W)


def test_five_escapes_in_one_k_part_do_not_pack():
    K, ks = 8192, 4
    W = weights(3, K, 2)
    W[2, [4096, 4100, 5000, 6000, 6143]] = 0x0000
    assert pack(W, ks) is None
    W[2, 6143] = 0x3C00; W[2, 6144] = 0x0000           # the fifth moved over the boundary into K-part 3: 4 + 1
    got = pack(W, ks)
    assert got is not None
    assert (got[1][2, 2] != M32).sum() == 4 and (got[1][2, 3] != M32).sum() == 1
    np.testing.assert_array_equal(unpack(*got, K, ks), W)


def test_boundary_escapes_land_in_the_part_that_owns_the_chunk():
    K, ks = 8192, 4
    W = weights(2, K, 3)
    W[1, [2047, 2048, 4095, 4096]] = [0x0001, 0x0002, 0x0003, 0x0004]
    P, rec, E0h = pack(W, ks)
    want = np.full((ks, ESC), M32, np.uint32)
    want[0, 0] = (2047 << 16) | 1                      # chunk 255: the last of part 0
    want[1, 0] = (2048 << 16) | 2; want[1, 1] = (4095 << 16) | 3       # chunks 256 and 511: part 1, in k order
    want[2, 0] = (4096 << 16) | 4                      # chunk 512: the first of part 2
    np.testing.assert_array_equal(rec[1], want)
    np.testing.assert_array_equal(unpack(P, rec, E0h, K, ks), W)


@pytest.mark.parametrize("K", [2048, 512])
def test_at_ks_1_the_records_are_the_per_row_records(K):
    W = weights(6, K, K)
    W[1, [0, K - 1]] = [0x0000, 0x8000]; W[3, [7, 8, K // 2, K - 8]] = [0x0001, 0x7F80, 0xFFC1, 0x0000]
    P, rec, E0h = pack(W, 1)
    P0, rec0, E0h0 = pack_hl(W, 1)
    assert E0h == E0h0
    np.testing.assert_array_equal(rec[:, 0, :], rec0)
    np.testing.assert_array_equal(P, P0)
    np.testing.assert_array_equal(unpack(P, rec, E0h, K, 1), unpack_hl(P0, rec0, E0h0, K, 1))
