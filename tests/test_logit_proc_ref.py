"""The numpy restatement of the logit processors (tests/logit_proc_ref.py) on hand-worked vectors: every expected value below is written out as the float32
operations of the header's formula, one rounding each (no GPU)."""
import numpy as np

from logit_proc_ref import COUNT_MASK, PROMPT_BIT, count, history, process_np

f32 = np.float32


def test_history_words():
    w = history(8, prompt_ids=[1, 1, 5], produced_ids=[5, 5, 2])
    assert w[1] == PROMPT_BIT and w[5] == (PROMPT_BIT | np.uint32(2)) and w[2] == 1 and w[0] == 0
    w[3] = COUNT_MASK
    count(w, 3)
    assert w[3] == COUNT_MASK                    # the count saturates below the prompt bit
    count(w, 1)
    assert w[1] == (PROMPT_BIT | np.uint32(1))


def test_repetition_positive_and_negative():
    """HF's rule under repetition 1.3: a positive logit is divided, a negative one multiplied; an id the row never saw is untouched; the prompt bit alone is enough"""
    L = np.array([2.0, -2.0, 2.0, -2.0, 0.0], np.float32)
    w = history(5, prompt_ids=[0, 1], produced_ids=[4])
    out = process_np(L, w, repetition=1.3)
    assert out.dtype == np.float32
    assert out[0] == f32(2.0) / f32(1.3) and out[1] == f32(-2.0) * f32(1.3)
    assert out[2] == f32(2.0) and out[3] == f32(-2.0)
    assert out[4] == f32(0.0) * f32(1.3)         # 0 is not > 0: multiplied
    assert out[0].tobytes() == np.float32(1.5384615659713745).tobytes()      # 2 / 1.3f rounded to fp32


def test_frequency_and_presence_counts():
    """n = 0, 1 and 3 under frequency 0.5 / presence 0.25; a prompt-only id pays neither"""
    L = np.full(4, 1.0, np.float32)
    w = history(4, prompt_ids=[3], produced_ids=[1, 2, 2, 2])
    out = process_np(L, w, presence=0.25, frequency=0.5)
    np.testing.assert_array_equal(out, np.array([1.0, 1.0 - 0.5 - 0.25, 1.0 - 1.5 - 0.25, 1.0], np.float32))
    # two roundings, not one fused: v - fl(f * n), in float32
    L = np.array([0.1], np.float32)
    out = process_np(L, history(1, produced_ids=[0] * 3), frequency=0.1)
    assert out[0] == f32(f32(0.1) - f32(f32(0.1) * f32(3.0)))


def test_order_of_the_three_steps():
    L = np.array([3.0], np.float32)
    out = process_np(L, history(1, produced_ids=[0, 0]), repetition=1.3, presence=0.5, frequency=0.25, bias={0: 1.5})
    want = f32(f32(f32(f32(3.0) / f32(1.3)) - f32(f32(0.25) * f32(2.0))) - f32(0.5)) + f32(1.5)
    assert out[0] == f32(want)


def test_bias_and_ban():
    L = np.array([0.5, -1.0, 2.0], np.float32)
    out = process_np(L, None, bias={0: -0.75, 2: -np.inf})
    assert out[0] == f32(-0.25) and out[1] == f32(-1.0) and out[2] == -np.inf
    out = process_np(L, None, bias=[(1, 4.0)])
    assert out[1] == f32(3.0)


def test_neutral_is_the_identity():
    rng = np.random.default_rng(0)
    L = (rng.standard_normal(300) * 3).astype(np.float32)
    L[7] = -np.inf
    w = history(300, prompt_ids=[1, 2, 3], produced_ids=[3, 4, 7])
    assert process_np(L, w).tobytes() == L.tobytes()
