"""Device memory of a context (tinygpt_amd/csrc/dev_mem.h; tgx_get_option "mem.live_allocs" / "mem.live_kib"): a workspace that grows replaces its buffers instead of
adding to them, whatever path took it to its size — the figures of a grown context are those of a context that went straight there, with option act.round16 (its
all-zero term buffer is allocated and released with the workspace) and without; a row extension on the split attention form allocates its partials once; logits do
not depend on which buffers hold the workspace; contexts are created and destroyed in a loop.  Nothing here reads device-wide free memory.  The leak proof is the
CPU check (tests/test_dev_mem.py): these tests see the record, not the allocator."""
import numpy as np
import pytest

from conftest import load_golden
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import Model

pytestmark = pytest.mark.gpu
IDS = np.random.default_rng(7).integers(3, 256, size=64)      # llama_tiny: vocab 256, context 256


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def make(hip, round16=0):
    cfg, g = load_golden("llama_tiny")
    m = Model(desc_from_hf_config(cfg, "bf16", max_batch=2), hip).load_synthetic(int(g["seed"]), float(g["std"])).finalize()
    if round16:
        m.set_option("act.round16", 1)
    return m


def mem(m):
    return m.get_option("mem.live_allocs"), m.get_option("mem.live_kib")


def straight(hip, n, round16=0):
    """a fresh context that forwards n tokens at once -> (figures after finalize, figures after the forward, logits)"""
    m = make(hip, round16)
    at_finalize = mem(m)
    m.forward(IDS[:n])
    out = at_finalize, mem(m), m.logits(rounded=False).copy()
    m.close()
    return out


@pytest.fixture(scope="module")
def straight40(hip):
    return straight(hip, 40)


def grown(hip, round16=0):
    """8 tokens, reset, 40 tokens: the workspace grows from 8 rows to 40"""
    m = make(hip, round16)
    m.forward(IDS[:8])
    small = mem(m)
    m.reset_cache()
    m.forward(IDS[:40])
    return m, small


def test_growth_replaces(hip, straight40):
    at_finalize, at40, _ = straight40
    m, small = grown(hip)
    print("finalize", at_finalize, "8 tokens", small, "grown to 40", mem(m), "straight to 40", at40)
    assert at_finalize[0] > 0 and at40[0] > at_finalize[0] and at40[1] > at_finalize[1]      # the prompt allocated its workspace
    assert at_finalize[0] < small[0] <= at40[0] and small[1] < at40[1]                       # ... a smaller one for 8 rows
    assert mem(m) == at40
    m.close()


def test_growth_replaces_with_round16_and_its_zero_term_goes_with_the_option(hip, straight40):
    _, at40_r16, _ = straight(hip, 40, round16=1)
    m, _ = grown(hip, round16=1)
    print("act.round16: grown to 40", mem(m), "straight to 40", at40_r16, "without the option", straight40[1])
    assert mem(m) == at40_r16
    assert at40_r16[0] == straight40[1][0] + 1 and at40_r16[1] > straight40[1][1]      # one buffer more than without the option: ws_zero
    m.set_option("act.round16", 0)
    m.reset_cache()
    m.forward(IDS[:48])      # grows past the workspace's 40 rows: ws_zero is released and not allocated again
    _, at48, _ = straight(hip, 48)
    print("option off, grown to 48", mem(m), "never had the option, straight to 48", at48)
    assert mem(m) == at48
    m.close()


def test_second_extension_on_the_split_attention_allocates_nothing(hip):
    m = make(hip)
    m.set_option("extend.attn_splits", 4)
    m.forward(IDS[:40])
    before = mem(m)
    m.extend_row(0, IDS[40:48])
    first = mem(m)
    if first == before:
        pytest.skip("tgx_extend_row of 8 tokens after 40 allocated nothing: the fixture's pass did not size the split attention's partials (ensure_extend_ws)")
    m.extend_row(0, IDS[48:56])
    print("40 tokens", before, "first extension", first, "second extension", mem(m))
    assert first[0] == before[0] + 1      # the partials, and nothing else
    assert mem(m) == first
    m.close()


def test_logits_do_not_depend_on_growth(hip, straight40):
    m, _ = grown(hip)
    np.testing.assert_array_equal(m.logits(rounded=False), straight40[2])
    m.close()


def test_create_forward_destroy_in_a_loop(hip):
    """eight contexts one after the other, act.round16 on in rounds 1, 2, 5, 6: a double free in tgx_destroy's order would end the process here"""
    logits = []
    for i in range(8):
        m = make(hip, round16=i % 4 in (1, 2))
        m.forward(IDS[:40])
        logits.append(m.logits(rounded=False).copy())
        m.close()
    np.testing.assert_array_equal(logits[7], logits[0])
    np.testing.assert_array_equal(logits[6], logits[1])
