"""Shared-prefix decode attention (option attn.shared_prefix; kernels/attn_prefix.h, csrc/prefix_groups.h) on planted caches against the CPU oracle, as
tests/test_hip_attn_keyrange.py (tests/kv_plant.py: every key at a tile / block edge is loud; one lost boundary key moves the oracle's logits by >= 1.6e-2); every
case proves the path was taken by attn.last_prefix_groups.  Bounds: that file's for the form this one replaces (batch-mfma): 1e-4 on the Llama-3.2-1B and Qwen2.5-0.5B
cuts, 1e-3 on the Mistral-7B cut (its floor is the step's own appended row rounding to bf16, not the attention).
Measured on an MI355X (rel_err maxima; printed at the module's end): every key once — Llama 9.7e-06, Mistral 8.0e-05, Qwen 5.8e-06; nested — 7.2e-06, 7.5e-05, 4.8e-06."""
import numpy as np
import pytest

import kv_plant as kp
from conftest import rel_err
from tinygpt_amd import synth
from tinygpt_amd.ffi import GREEDY, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu
TOL = {"llama-3.2-1b": 1e-4, "mistral-7b-v0.3": 1e-3, "qwen2.5-0.5b": 1e-4}
CUTS = list(TOL)
CTX, ROWS, WARM = 768, 10, SamplerCfg(0.8, 0, 0.9, 0.0)
PROMPT, EXT = synth.synth_prompt(4096, 513, 4321), synth.synth_prompt(4096, 140, 4242)
TOKS = [1717, 5, 4000, 911, 2048, 3333, 64, 127, 2999, 1]      # row r steps on TOKS[r]: a column mix-up between rows shows
_ctx, _ref, _base, _step_ref, MEASURED = {}, {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_everything():
    yield
    for k in sorted(MEASURED):
        print("measured max GPU-vs-oracle  %-40s %.2e" % (k, MEASURED[k]))
    for m in list(_ctx.values()) + list(_ref.values()):
        m.close()


def gpu(name, tag="plant", paged=True, peaked=False, option=128):      # one context per (model, tag); option None: attn.shared_prefix never touched
    if (name, tag) not in _ctx:
        d = kp.cut_desc(name, "bf16", CTX, ROWS)
        d.tied = d.tied and not peaked        # the peaked checkpoint's loud rows live in an untied lm_head (tinygpt_amd/synth.py)
        m = Model(d).set_option("kv.budget_tokens", ROWS * CTX if paged else 0)
        m.load_synthetic(1234, 0.02, peaked=peaked).finalize().set_option("decode.mfma_min_batch", 2)      # the batched route from 2 rows on
        if option is not None:
            m.set_option("attn.shared_prefix", option)
        _ctx[(name, tag)] = m
    return _ctx[(name, tag)]


def write_planted(m, name, row, L):      # the planted rows of PROMPT[:L] (from ONE GPU prefill of PROMPT: a causal model's rows [0, L) do not depend on later tokens)
    for layer, (k, v) in enumerate(_base[name]):
        m.write_kv(row, layer, *kp.plant(k, v, L))


def step_ref(name, L):      # -> (the oracle, its logits after one step on each of TOKS over the planted cache of length L): computed once, shared by every shape
    from oracle.oracle_ffi import OracleModel
    if name not in _ref:
        m = gpu(name)
        m.reset_cache(); m.forward_row(0, PROMPT)
        _base[name] = [m.read_kv(0, layer) for layer in range(m.desc.layers)]
        _ref[name] = OracleModel(kp.cut_desc(name, "bf16", CTX, 1)).load_synthetic(1234, 0.02).finalize()
    r = _ref[name]
    if (name, L) not in _step_ref:
        write_planted(r, name, 0, L)
        out = []
        for t in TOKS:
            r.set_past(L); r.forward(np.array([[t]]))
            out.append(r.logits(rounded=False)[0].copy())
        _step_ref[(name, L)] = np.stack(out)
    return r, _step_ref[(name, L)]


def admit(m, name, row, L, fork_into=()):
    m.forward_row(row, PROMPT[:L])
    write_planted(m, name, row, L)            # BEFORE the fork: tgx_write_kv refuses shared blocks
    if len(fork_into):
        m.fork_row(row, fork_into)


def step_all(m, n, groups):      # rows 0 .. n - 1 step once, row r on TOKS[r] -> their logits
    m.set_logits(kp.onehot(TOKS[:n], m.desc.vocab))
    np.testing.assert_array_equal(m.sample(GREEDY), TOKS[:n])
    m.decode_rows(1)
    assert m.get_option("attn.last_prefix_groups") == groups
    return m.logits(rounded=False).copy()


@pytest.mark.parametrize("L", [129, 191, 256, 257, 385, 513])     # 1 .. 4 shared blocks; tails of 1 / 63 / 0 / 1 / 1 / 1 keys + the step's own
@pytest.mark.parametrize("name", CUTS)
def test_every_row_sees_every_key_once(name, L):
    """2 rows; a full group (8 rows, 4 on the Qwen cut); a full group + 1; two groups from two admissions + a bystander; the source row reset and refilled after the fork"""
    m, want, errs = gpu(name), step_ref(name, L)[1], {}
    cap = 32 // (m.desc.heads // m.desc.kv_heads)
    for sid, n, groups in (("two", 2, 1), ("full", cap, 1), ("full+1", cap + 1, 1), ("two-prompts", 5, 2), ("refilled", 4, 1)):
        m.reset_cache()
        if sid == "two-prompts":              # the same content in three sets of blocks: groups {0, 3} and {1, 4}, row 2 the bystander
            admit(m, name, 0, L); admit(m, name, 1, L); admit(m, name, 2, L); m.fork_row(0, [3]); m.fork_row(1, [4])
        else:
            admit(m, name, 0, L, range(1, n))
        if sid == "refilled":                 # the group's first member is row 1 now; row 0 holds blocks of its own
            m.reset_row(0); admit(m, name, 0, L)
        lg = step_all(m, n, groups)
        errs[sid] = max(rel_err(lg[r:r + 1], want[r:r + 1]) for r in range(n))
    print(name, L, " ".join("%s:%.1e" % kv for kv in errs.items()))
    MEASURED["every key once  " + name] = max(MEASURED.get("every key once  " + name, 0.0), max(errs.values()))
    assert max(errs.values()) < TOL[name], errs


@pytest.mark.parametrize("name", CUTS)
def test_unequal_tails_and_nested_sharing(name):
    """fork at 256 into rows 1-2, row 1 extended by 70 + 70, row 2 by 1, row 1 forked into row 3: rows 1 and 3 share 3 blocks, all four 2 -> one group of four over 2"""
    m, (r, ref0) = gpu(name), step_ref(name, 256)
    want = {0: ref0[0]}
    m.reset_cache(); admit(m, name, 0, 256, [1, 2])
    m.extend_row(1, EXT[:70]); m.extend_row(2, EXT[:1]); m.extend_row(1, EXT[70:]); m.fork_row(1, [3])
    lg = step_all(m, 4, 1)
    write_planted(r, name, 0, 256)
    for i in range(len(EXT)):                 # the oracle walks EXT from the planted prefix; a step on each row's token from where that row stands
        r.set_past(256 + i); r.forward(EXT[None, i:i + 1])
        for row in {0: [2], len(EXT) - 1: [1, 3]}.get(i, []):
            r.set_past(257 + i); r.forward(np.array([[TOKS[row]]]))
            want[row] = r.logits(rounded=False)[0].copy()
    MEASURED["nested  " + name] = err = max(rel_err(lg[row:row + 1], want[row][None, :]) for row in range(4))
    assert err < TOL[name]


def free_run(m):
    """200 tokens forked into 4 rows, rows 1, 3 at T 0.8 / top-p 0.9; 40 steps twice (-> 240 -> 280: the second call's multi-step graphs cross 256) -> [ids, logits, cache rows ...], groups"""
    m.reset_cache()
    m.forward_row(0, PROMPT[:200]); m.fork_row(0, [1, 2, 3])
    for r in range(4):
        m.set_row_sampler(r, WARM if r % 2 else GREEDY, 100 + r)
    first = [m.sample_row(r, WARM if r % 2 else GREEDY, seed=100 + r) for r in range(4)]
    ids = np.concatenate([[first], m.decode_rows(40)[0], m.decode_rows(40)[0]])
    return [ids, m.logits(rounded=False).copy()] + [x for r in range(4) for layer in range(m.desc.layers) for x in m.read_kv(r, layer)], m.get_option("attn.last_prefix_groups")


@pytest.mark.parametrize("name", CUTS)
def test_free_running_and_off_is_off(name):
    """peaked checkpoint.  On: the ids of option 0, two contexts bit for bit.  Off: 128 and back to 0, and an unpaged context at 128, give the bits of one that never touched it; 64 is refused"""
    def same_bits(x, y):
        assert len(x) == len(y) and all(np.array_equal(a, b) for a, b in zip(x, y))
    (a, ga), (b, gb), (off, goff) = (free_run(gpu(name, tag, peaked=True, option=o)) for tag, o in (("on-a", 128), ("on-b", 128), ("never", None)))
    assert (ga, gb, goff) == (1, 1, 0)
    np.testing.assert_array_equal(a[0], off[0])
    same_bits(a, b)
    m = gpu(name, "on-a")
    with pytest.raises(TgxError):
        m.set_option("attn.shared_prefix", 64)
    back, gback = free_run(m.set_option("attn.shared_prefix", 0))
    assert gback == 0
    same_bits(back, off)
    (f1, g1), (f0, _) = (free_run(gpu(name, tag, paged=False, peaked=True, option=o)) for tag, o in (("flat-on", 128), ("flat-never", None)))
    assert g1 == 0
    same_bits(f1, f0)
