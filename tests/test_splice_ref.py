"""tests/splice_ref.py, the numpy reference of tgx_splice_row's move, checked against itself without a GPU: two splices in a row equal the one combined splice —
the angle differences add up, table(d) - table(m) + table(m) - table(s) = table(d) - table(s) — within 2^-20 of the pair's norm (the reference rounds nothing to a
storage dtype, so the storage ulp of the GPU test's bound does not enter); V rows and delta == 0 K rows are copies."""
import numpy as np

from tinygpt_amd import known_desc

import splice_ref


def compose(first, second):
    """the ranges, in the original row's positions, that splicing by `first` and then by `second` keeps"""
    src = splice_ref.source_positions(first)[splice_ref.source_positions(second)]
    out = []
    for s in src:
        if out and out[-1][0] + out[-1][1] == s:
            out[-1][1] += 1
        else:
            out.append([int(s), 1])
    return [tuple(r) for r in out]


def test_two_splices_equal_the_combined_splice():
    rng = np.random.default_rng(3)
    for name in ("mistral-7b-v0.3", "qwen3-1.7b"):
        d = known_desc(name, "bf16")
        T = 512
        ang = splice_ref.angles(d, T)
        k = rng.standard_normal((T, 2, d.head_dim)).astype(np.float32)
        v = rng.standard_normal((T, 2, d.head_dim)).astype(np.float32)
        first = [(0, 4), (50, 10), (61, 129), (250, 262)]
        second = [(0, 2), (3, 100), (143, 200), (400, 5)]
        k1, v1 = splice_ref.splice(k, v, first, ang)
        k2, v2 = splice_ref.splice(k1, v1, second, ang)
        both = compose(first, second)
        assert sum(n for _, n in both) == len(k2) == 307
        kc, vc = splice_ref.splice(k, v, both, ang)
        np.testing.assert_array_equal(v2, vc)
        np.testing.assert_array_equal(vc, v[splice_ref.source_positions(both)])
        assert (np.abs(k2 - kc) <= 2.0 ** -20 * splice_ref.pair_norm(kc)).all()
        np.testing.assert_array_equal(kc[:2], k[:2])                 # delta == 0: copies
        assert np.abs(kc[2:] - k[splice_ref.source_positions(both)][2:]).max() > 0.1      # ... and the rest is rotated
        # a rotation keeps every pair's norm
        np.testing.assert_allclose(splice_ref.pair_norm(kc), splice_ref.pair_norm(k[splice_ref.source_positions(both)]), rtol=1e-12)


def test_angles_are_the_table_angles():
    """position 0 is angle 0, the first frequency is 1, and the angles are float32 products of float32 factors"""
    d = known_desc("mistral-7b-v0.3", "fp16")
    inv, ang = splice_ref.inv_freq(d), splice_ref.angles(d, 300)
    assert inv.dtype == np.float32 and ang.dtype == np.float32 and inv[0] == 1.0 and (ang[0] == 0).all()
    assert (ang[:, 0] == np.arange(300)).all() and (np.diff(inv) < 0).all()
    assert ang[299, 5] == np.float32(inv[5] * np.float32(299))
