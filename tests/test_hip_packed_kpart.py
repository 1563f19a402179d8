"""Escape records per (row, K-part) (kernels/gemv_packed.h; the layout's specification is tests/test_packed_format_kpart.py) in the K-split packed launch:
the descriptor of tests/test_hip_packed_hl.py — one layer, hidden 2048, intermediate 8192, vocabulary 1024, weights.packed_classes = 7 — whose down launch runs
KS = 4: wave p of a workgroup owns k in [2048 p, 2048 p + 2047] and reads the record of its own K-part only.  Everything is held to weights.packed = 0 BIT FOR
BIT: ids, and the unrounded fp32 logits as uint32, graph on and off."""
import numpy as np
import pytest

from tinygpt_amd import synth
from test_hip_packed_hl import DOWN, STD, V0, VLOW, VN0, VSUB, build, clean_rows, desc, out_of_window, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def tensors(seed):
    return [(name, np.array(bits, copy=True)) for name, bits in synth.synth_checkpoint(desc(), seed, STD)]


@pytest.fixture(scope="module")
def checkpoint():
    return tensors(7)          # (test_hip_packed_hl.py's: no row beyond four escapes)


def per_part(bits):
    """escapes per (row, K-part) of a down matrix [2048][8192] at KS = 4"""
    return out_of_window(bits).reshape(bits.shape[0], 4, 2048).sum(axis=2)


def check(hip, checkpoint, plant=None, matrices=3, fallbacks=0, max_row_esc=None):
    plain, packed = build(hip, checkpoint, 0, plant), build(hip, checkpoint, 1, plant)
    assert plain.get_option("weights.packed_matrices") == 0
    assert packed.get_option("weights.packed_matrices") == matrices and packed.get_option("weights.packed_fallbacks") == fallbacks
    if max_row_esc is not None:
        assert packed.get_option("weights.packed_max_row_esc") == max_row_esc
    for graph in (1, 0):
        a, b = run(packed, graph), run(plain, graph)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        assert np.isfinite(b[1]).all()
    plain.close(); packed.close()


def test_a_row_of_five_escapes_packs_when_no_k_part_holds_more_than_four(hip):
    """seed 1234 (the benchmark's): layer 0's down matrix has a row of five escapes, at most 2 in one K-part — it ran the plain kernel under per-row records"""
    ck = tensors(1234)
    down = dict(ck)[DOWN]
    assert out_of_window(down).sum(axis=1).max() == 5 and per_part(down).max() == 2
    check(hip, ck, max_row_esc=5)


def test_four_escapes_in_every_k_part_of_one_row(hip, checkpoint):
    """16 escapes in one row: every wave's record full, entries at the first and the last chunk of each K-part"""
    vals = [V0, VLOW, VSUB, VN0]
    planted = {}

    def plant(name, bits):
        if name == DOWN:
            row = clean_rows(bits, 1)[0]
            for p in range(4):
                bits[row, [2048 * p, 2048 * p + 7, 2048 * p + 2040, 2048 * p + 2047]] = vals[p:] + vals[:p]
            planted["per_part"] = per_part(bits)[row].tolist()
    check(hip, checkpoint, plant, max_row_esc=16)
    assert planted["per_part"] == [4, 4, 4, 4]


def test_five_escapes_in_one_k_part_fall_back(hip, checkpoint):
    def plant(name, bits):
        if name == DOWN:
            row = clean_rows(bits, 1)[0]
            bits[row, [4096, 4100, 5000, 6000, 6143]] = [V0, VN0, VSUB, VLOW, V0]          # all in K-part 2
    check(hip, checkpoint, plant, matrices=2, fallbacks=1, max_row_esc=5)


def test_escapes_in_the_last_k_part_only(hip, checkpoint):
    """every escape of the down matrix moved into the window, then one row with escapes in K-part 3 alone: the records of parts 0..2 are empty in EVERY row, so
    the waves of those parts never take the repair branch; a wave of part 3 takes it for that row"""
    def plant(name, bits):
        if name == DOWN:
            esc = out_of_window(bits)
            e = (bits >> 7) & 0xFF
            emax = int(e[e < 255].max())
            bits[esc] = (bits[esc] & 0x807F) | ((emax - 14) << 7)
            bits[1001, [6144, 7000, 8191]] = [VSUB, V0, VLOW]
            assert per_part(bits).sum(axis=0).tolist() == [0, 0, 0, 3]
    check(hip, checkpoint, plant)
