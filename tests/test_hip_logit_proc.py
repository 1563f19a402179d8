"""Per-row logit processors on the device (include/tgx.h: tgx_set_row_penalties / tgx_set_row_logit_bias / tgx_set_row_history; kernels/logit_proc.h).  Held to:
  * the kernel against the float32 numpy restatement (tests/logit_proc_ref.py), model-free: sampling the processed logits == sampling the restatement's, ids and
    probability vectors bit for bit, on one tile, on a vocabulary that is no multiple of 4 and on one with a partial last tile;
  * greedy rows of tgx_decode_rows: every produced id is the argmax of the restatement over the step's raw logits and the test's own history, on the GEMV step and
    the matrix-core step, unpaged and paged, one step per call and across the 16-step graph;
  * sampled rows: the probability vector of every step is the one a scratch context gives for the restatement's logits; a banned id is never produced;
  * neighbours and neutrality, device-side stops, the lifecycle calls, and the refusals the header names."""
import numpy as np
import pytest

from conftest import load_golden
from logit_proc_ref import argmax_lowest, count, history, process_np
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, MAX_LOGIT_BIAS, Model, SamplerCfg, TgxError

pytestmark = pytest.mark.gpu

ST_INVALID, ST_UNSUPPORTED, ST_STATE = 1, 2, 4
NINF = float("-inf")
MIX = [GREEDY, SamplerCfg(0.8, 0, 0.9, 0.0), SamplerCfg(1.0, 50, 1.0, 0.0), SamplerCfg(0.7, 0, 1.0, 0.05), SamplerCfg(0.9, 40, 0.95, 0.05)]
SEEDS = [11, 22, 33, 44, 55]
# per-row processor settings: everything off, only a bias, each penalty alone and together, a negative frequency, a repetition below 1, a long bias list.
# "ban_top": the id the row's raw first-step argmax names is banned as well (so that the ban changes what the row does)
SPECS = [
    dict(),
    dict(bias={3: 2.5, 77: -1.0}, ban_top=True),
    dict(repetition=1.3, ban_top=True),
    dict(presence=0.4, frequency=0.3),
    dict(repetition=1.15, presence=0.2, frequency=0.1, bias={0: 1.0, 255: NINF}),
    dict(frequency=-0.2),
    dict(repetition=0.8),
    dict(repetition=1.5, presence=0.1, frequency=0.05, bias={i: 0.01 * (i % 7) - 0.02 for i in range(100, 140)}, ban_top=True),
]


@pytest.fixture(scope="module")
def hip():
    from tinygpt_amd.ffi import product_backend
    return product_backend()


def make(hip, B, budget=0, max_ctx=256, **over):
    cfg, g = load_golden("llama_tiny")
    cfg = dict(cfg, **over)
    d = desc_from_hf_config(cfg, "bf16", max_batch=B)
    d.max_ctx = max_ctx
    m = Model(d, hip)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    return m.load_synthetic(int(g["seed"]), float(g["std"])).finalize()


def prompts(B, S=9, seed=0, V=256):
    return np.random.default_rng(seed).integers(0, V, size=(B, S)).astype(np.int64)


def is_on(spec):
    return bool(spec.get("bias")) or spec.get("repetition", 1.0) != 1.0 or spec.get("presence", 0.0) != 0.0 or spec.get("frequency", 0.0) != 0.0


def apply_spec(m, b, spec):
    m.set_row_penalties(b, spec.get("repetition", 1.0), spec.get("presence", 0.0), spec.get("frequency", 0.0))
    m.set_row_logit_bias(b, spec.get("bias"))


def proc(spec, raw, words):
    """what the row's step draws from: the restatement for a row with a processor on, the raw logits otherwise"""
    if not is_on(spec):
        return raw
    return process_np(raw, words, spec.get("repetition", 1.0), spec.get("presence", 0.0), spec.get("frequency", 0.0), spec.get("bias"))


class Rows:
    """a batch started the way a server starts requests: prefill, every row's processors and history (seeded from its prompt), its first token through
    tgx_sample_row (processed, not counted) and its sampler settings — with the test's own mirror of every row's history"""

    def __init__(self, hip, B, P, spec_of, cfg_of=lambda b: 0, processors=True, **kw):
        self.m = m = make(hip, B, **kw)
        self.B, self.V = B, m.desc.vocab
        m.forward(P)
        raw = m.logits(rounded=False)
        self.raw0 = raw
        self.spec, self.k, self.words, self.cur = [], [], [], []
        for b in range(B):
            spec = dict(spec_of(b)) if processors else {}
            if spec.pop("ban_top", False):
                spec["bias"] = {**(spec.get("bias") or {}), argmax_lowest(raw[b]): NINF}
            self.spec.append(spec)
            self.k.append(cfg_of(b))
            self.words.append(history(self.V, prompt_ids=P[b]))
            if processors:
                apply_spec(m, b, spec)
                m.set_row_history(b, prompt_ids=P[b])
        for b in range(B):
            k = self.k[b]
            self.cur.append(m.sample_row(b, MIX[k], SEEDS[k]))
            m.set_row_sampler(b, MIX[k], SEEDS[k])

    def banned(self, b):
        return [i for i, v in (self.spec[b].get("bias") or {}).items() if v == NINF]

    def count_current(self):
        """the counting step of the next tgx_decode_rows step, on the mirror"""
        for b in range(self.B):
            if is_on(self.spec[b]):
                count(self.words[b], self.cur[b])

    def processed(self, b, raw_b):
        return proc(self.spec[b], raw_b, self.words[b])


# ---- 1. the kernel against the restatement, model-free -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [256, 2503, 3080])
def test_kernel_matches_restatement(hip, V):
    """one tile; no multiple of 4 (entry by entry, the second row unaligned); a multiple of 4 with a partial last tile.  set_logits(L) + processors + sample_row
    == processors off + set_logits(process_np(L)) + sample_row: the same id and the same probability bits, and a banned id has probability exactly 0"""
    m = make(hip, 2, vocab_size=V, hidden_size=64, intermediate_size=64, num_attention_heads=1, num_key_value_heads=1, num_hidden_layers=1)
    rng = np.random.default_rng(V)
    peaked = (rng.standard_normal((2, V)) * 2.5).astype(np.float32)
    flat = (rng.standard_normal((2, V)) * 0.05).astype(np.float32)
    tied = (np.round(peaked * 2) / 2).astype(np.float32)
    holes = peaked.copy()
    holes[:, rng.choice(V, 12, replace=False)] = NINF
    edge = [i for i in (0, 1023, 1024, V - 1) if i < V]
    others = [int(i) for i in rng.choice(np.setdiff1d(np.arange(V), edge), 40, replace=False)]
    # row 0: the edge ids carry the prompt bit and counts 0 .. 3, a dozen others counts 1 .. 3; row 1: other ids, and a bias list longer than the workgroup
    hist = [dict(prompt=edge + others[:6], produced=[t for n, t in enumerate(edge) for _ in range(n % 4)] + [t for n, t in enumerate(others[6:18]) for _ in range(1 + n % 3)]),
            dict(prompt=others[20:30], produced=edge * 3 + others[30:40])]
    long_bias = {int(i): float(0.03 * (n % 11) - 0.1) for n, i in enumerate(rng.choice(V, min(V, 300), replace=False))}
    specs = [dict(repetition=1.3, presence=0.4, frequency=0.3,
                  bias={**{i: 1.25 + 0.5 * n for n, i in enumerate(edge)}, others[0]: NINF, others[7]: NINF, others[19]: -2.0, int(np.argmax(peaked[0])): NINF}),
             dict(repetition=0.9, presence=-0.1, frequency=0.2, bias={**long_bias, edge[-1]: NINF})]
    assert len(specs[1]["bias"]) > 256 or V == 256
    words = [history(V, h["prompt"], h["produced"]) for h in hist]
    cfgs = [GREEDY, SamplerCfg(0.8, 0, 0.9, 0.0), SamplerCfg(1.0, 50, 1.0, 0.0), SamplerCfg(0.9, 40, 0.95, 0.05)]
    for L in (peaked, flat, tied, holes):
        want = np.stack([proc(specs[b], L[b], words[b]) for b in range(2)])
        for b in range(2):
            assert all(want[b][i] == NINF for i, v in specs[b]["bias"].items() if v == NINF)
        for k, cfg in enumerate(cfgs):
            got = []
            m.set_logits(L)
            for b in range(2):
                apply_spec(m, b, specs[b])
                m.set_row_history(b, hist[b]["prompt"], hist[b]["produced"])
            for b in range(2):
                t = m.sample_row(b, cfg, 5 + k)
                got.append((t, None if cfg.greedy else m.probs()[b].copy()))
            for b in range(2):
                apply_spec(m, b, {})
            m.set_logits(want)
            for b in range(2):
                t = m.sample_row(b, cfg, 5 + k)
                assert t == got[b][0], (V, k, b)
                if cfg.greedy:
                    assert t == argmax_lowest(want[b])
                    continue
                p = m.probs()[b]
                assert p.tobytes() == got[b][1].tobytes(), (V, k, b)
                assert p[t] > 0
                for i, v in specs[b]["bias"].items():
                    if v == NINF:
                        assert got[b][1][i] == 0.0


# ---- 2. greedy rows in tgx_decode_rows, exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [0, 1024])
@pytest.mark.parametrize("B", [2, 8])
def test_greedy_rows_follow_the_restatement(hip, B, budget):
    P = prompts(B, seed=B)
    spec_of = lambda b: SPECS[b % len(SPECS)]
    r = Rows(hip, B, P, spec_of, budget=budget)
    m = r.m
    for b in range(B):
        assert r.cur[b] == argmax_lowest(r.processed(b, r.raw0[b])), b
        assert r.cur[b] not in r.banned(b)
    assert any(r.banned(b) for b in range(B))
    first = list(r.cur)
    single = []
    for step in range(24):
        r.count_current()
        ids, new, fin = m.decode_rows(1)
        assert (new == 1).all() and not fin.any()
        raw = m.logits(rounded=False)
        for b in range(B):
            assert int(ids[0, b]) == argmax_lowest(r.processed(b, raw[b])), (step, b)
            r.cur[b] = int(ids[0, b])
        single.append(ids[0].copy())
    single = np.stack(single)
    assert any((single[:, b] != single[:, 0]).any() for b in range(B))
    # a fresh identical context, one call of 24 steps (a 16-step graph, then single steps): the same ids
    r2 = Rows(hip, B, P, spec_of, budget=budget)
    assert r2.cur == first
    ids, new, fin = r2.m.decode_rows(24)
    assert (new == 24).all()
    np.testing.assert_array_equal(ids, single)


# ---- 3. sampled rows in tgx_decode_rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 8])
def test_sampled_rows_draw_from_the_processed_logits(hip, B):
    P = prompts(B, seed=10 + B)
    r = Rows(hip, B, P, lambda b: SPECS[(b + 1) % len(SPECS)], cfg_of=lambda b: (b + 1) % len(MIX))
    m = r.m
    scratch = make(hip, 1)
    assert any(r.banned(b) and not MIX[r.k[b]].greedy for b in range(B))
    for step in range(40):
        r.count_current()
        ids, new, fin = m.decode_rows(1)
        raw, pm = m.logits(rounded=False), m.probs()
        for b in range(B):
            t, cfg = int(ids[0, b]), MIX[r.k[b]]
            assert t not in r.banned(b), (step, b)
            if cfg.greedy:
                assert not pm[b].any()
                assert t == argmax_lowest(r.processed(b, raw[b]))
            else:
                scratch.set_logits(r.processed(b, raw[b])[None])
                scratch.sample(cfg, SEEDS[r.k[b]])
                assert scratch.probs()[0].tobytes() == pm[b].tobytes(), (step, b)
                assert pm[b][t] > 0
                assert all(pm[b][i] == 0.0 for i in r.banned(b))
            r.cur[b] = t


# ---- 4. neighbours and neutrality ----------------------------------------------------------------------------------------------------------------------------
def test_neighbours_and_neutral_settings(hip):
    B = 8
    P = prompts(B, seed=4)
    on_rows = {1: dict(bias={5: -1e-3}), 4: SPECS[4], 6: SPECS[7]}
    spec_of = lambda b: on_rows.get(b, {})
    cfg_of = lambda b: 0 if b == 1 else b % len(MIX)
    r = Rows(hip, B, P, spec_of, cfg_of)
    tw = Rows(hip, B, P, spec_of, cfg_of, processors=False)          # nothing was ever set
    neutral = make(hip, B)                                            # neutral values on every row of a fresh context
    neutral.forward(P)
    allocs = neutral.get_option("mem.live_allocs")
    for b in range(B):
        neutral.set_row_penalties(b, 1.0, 0.0, 0.0).set_row_logit_bias(b, None).set_row_history(b)
    assert neutral.get_option("mem.live_allocs") == allocs
    for b in range(B):
        assert neutral.sample_row(b, MIX[cfg_of(b)], SEEDS[cfg_of(b)]) == tw.cur[b]
        neutral.set_row_sampler(b, MIX[cfg_of(b)], SEEDS[cfg_of(b)])
    raw_same = 0
    diverged = False
    for n in (1, 1, 1, 1, 20):
        ids, _, _ = r.m.decode_rows(n)
        it, _, _ = tw.m.decode_rows(n)
        jn, _, _ = neutral.decode_rows(n)
        lm, lt, ln = r.m.logits(rounded=False), tw.m.logits(rounded=False), neutral.logits(rounded=False)
        pm, pt, pn = r.m.probs(), tw.m.probs(), neutral.probs()
        np.testing.assert_array_equal(jn, it)
        assert ln.tobytes() == lt.tobytes() and pn.tobytes() == pt.tobytes()
        for b in range(B):
            if b in on_rows:
                continue
            np.testing.assert_array_equal(ids[:, b], it[:, b])
            assert lm[b].tobytes() == lt[b].tobytes() and pm[b].tobytes() == pt[b].tobytes(), b
        # tgx_read_logits after a processed step: the MODEL's logits — the twin's, while the row's ids have not diverged
        diverged = diverged or r.cur[1] != tw.cur[1] or (ids[:, 1] != it[:, 1]).any()
        if not diverged:
            assert lm[1].tobytes() == lt[1].tobytes()
            raw_same += 1
    assert raw_same >= 3
    assert neutral.get_option("mem.live_allocs") == tw.m.get_option("mem.live_allocs") < r.m.get_option("mem.live_allocs")


# ---- 5. stops ------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_banned_stop_id_never_stops_the_row(hip):
    B = 2
    P = prompts(B, seed=5)
    probe = Rows(hip, B, P, lambda b: {}, processors=False)
    t_star = int(probe.m.decode_rows(1)[0][0, 0])                     # the twin's first greedy token
    tw = Rows(hip, B, P, lambda b: {}, processors=False)
    tw.m.set_row_stop(0, 10, [t_star])
    ids, new, fin = tw.m.decode_rows(10)
    ids_tw = ids.copy()
    assert new[0] == 1 and fin[0] == 1 and ids[0, 0] == t_star and new[1] == 10 and fin[1] == 0
    r = Rows(hip, B, P, lambda b: dict(bias={t_star: NINF}) if b == 0 else {})
    r.m.set_row_stop(0, 10, [t_star])
    ids, new, fin = r.m.decode_rows(10)
    assert new[0] == 10 and fin[0] == 2 and t_star not in ids[:, 0]
    np.testing.assert_array_equal(ids[:, 1], ids_tw[:, 1])      # the neighbour: untouched
    assert new[1] == 10 and fin[1] == 0


# ---- 6. lifecycle --------------------------------------------------------------------------------------------------------------------------------------------
def greedy_steps(r, n, rows=None):
    """n single greedy steps of r, every listed row checked against the restatement; -> the ids"""
    out = []
    for _ in range(n):
        r.count_current()
        ids, _, _ = r.m.decode_rows(1)
        raw = r.m.logits(rounded=False)
        for b in (range(r.B) if rows is None else rows):
            assert int(ids[0, b]) == argmax_lowest(r.processed(b, raw[b])), b
        r.cur = [int(t) for t in ids[0]]
        out.append(ids[0].copy())
    return np.stack(out)


def test_reset_row_clears_settings_and_history(hip):
    B = 2
    P = prompts(B, seed=6)
    r = Rows(hip, B, P, lambda b: SPECS[7])
    greedy_steps(r, 5)
    r.m.reset_row(0)
    r.m.forward_row(0, P[0])
    t0 = r.m.sample_row(0, GREEDY)
    fresh = Rows(hip, B, P, lambda b: {}, processors=False)
    assert t0 == fresh.cur[0]
    # row 0 refilled: settings neutral, history empty — it decodes like the fresh context's; row 1 keeps its processors
    r.spec[0], r.words[0], r.cur[0] = {}, history(r.V), t0
    got = greedy_steps(r, 6)
    np.testing.assert_array_equal(got[:, 0], fresh.m.decode_rows(6)[0][:, 0])
    # ... and switched on again it counts from an empty history
    r.spec[0] = dict(repetition=1.4, frequency=0.5)
    apply_spec(r.m, 0, r.spec[0])
    greedy_steps(r, 4)


def test_a_retired_row_neither_counts_nor_processes(hip):
    """settings and history stated for a RETIRED row (ahead of its admission, the order the log-probability setting supports as well): the row rides along in the
    other row's steps and publishes tokens, which must not be counted into the history the caller just stated.  After the admission it equals, bit for bit, a
    context whose row was given the same settings and history after the admission — under pure temperature sampling every id's probability is in the vector, so
    one stray count anywhere shows"""
    B = 2
    P = prompts(B, seed=15)
    spec = dict(repetition=1.4, presence=0.3, frequency=0.6, bias={9: 0.5, 30: NINF})
    cfg, seed = SamplerCfg(1.0, 0, 1.0, 0.0), 7

    def begin():
        m = make(hip, B)
        m.forward(P)
        for b in range(B):
            m.sample_row(b, GREEDY)
        m.decode_rows(3)
        m.reset_row(1)
        return m

    def state(m):
        apply_spec(m, 1, spec)
        m.set_row_history(1, prompt_ids=P[1])
        m.set_row_sampler(1, cfg, seed)

    m, fresh = begin(), begin()
    state(m)                                     # row 1 is retired: kept on the host, "off" on the device
    ride, _, _ = m.decode_rows(5)
    ride_f, _, _ = fresh.decode_rows(5)
    np.testing.assert_array_equal(ride[:, 0], ride_f[:, 0])
    assert (ride[:, 1] == -1).all()
    m.forward_row(1, P[1])                       # the settings travel with the admission
    fresh.forward_row(1, P[1])
    state(fresh)
    assert m.sample_row(1, cfg, seed) == fresh.sample_row(1, cfg, seed)
    assert m.probs()[1].tobytes() == fresh.probs()[1].tobytes()
    assert m.probs()[1][30] == 0.0 and m.probs()[1].any()
    for step in range(6):
        a, _, _ = m.decode_rows(1)
        b, _, _ = fresh.decode_rows(1)
        np.testing.assert_array_equal(a, b)
        assert m.probs()[1].tobytes() == fresh.probs()[1].tobytes(), step
        assert m.logits(rounded=False).tobytes() == fresh.logits(rounded=False).tobytes()


def test_fork_copies_the_history(hip):
    P = prompts(1, seed=8)
    spec = dict(repetition=1.5, presence=0.3, frequency=0.4, bias={9: 0.5})
    m = make(hip, 3)
    m.forward_row(0, P[0])
    apply_spec(m, 0, spec)
    m.set_row_history(0, prompt_ids=P[0])
    words = history(m.desc.vocab, prompt_ids=P[0])
    cur = m.sample_row(0, GREEDY)
    for _ in range(6):
        count(words, cur)
        cur = int(m.decode_rows(1)[0][0, 0])
    m.fork_row(0, [1, 2])
    apply_spec(m, 1, spec)                      # row 1: the source's settings, and the history the fork copied; row 2: its settings stay neutral
    for step in range(8):
        count(words, cur)                       # rows 0 and 1: the same sequence, the same words
        ids, _, _ = m.decode_rows(1)
        raw = m.logits(rounded=False)
        for b in (0, 1):
            assert int(ids[0, b]) == argmax_lowest(proc(spec, raw[b], words)), (step, b)
        assert int(ids[0, 2]) == argmax_lowest(raw[2])
        cur = int(ids[0, 0])


def test_truncate_and_extend_keep_the_words(hip):
    B = 2
    P = prompts(B, seed=9)
    r = Rows(hip, B, P, lambda b: dict(repetition=1.6, frequency=0.6, presence=0.2))
    got = greedy_steps(r, 6)
    m = r.m
    n = m.past_length_row(0)
    m.truncate_row(0, n - 2)
    m.extend_row(0, got[-3:-1, 0])               # the two positions back: the tokens those steps consumed
    raw = m.logits(rounded=False)[0]
    t = m.sample_row(0, GREEDY)                  # no counting step; the words still hold everything the row counted
    assert t == argmax_lowest(r.processed(0, raw))


def test_a_changed_penalty_takes_effect_in_the_next_call(hip):
    B = 8
    P = prompts(B, seed=12)
    r = Rows(hip, B, P, lambda b: dict(repetition=1.1))
    r.count_current()
    ids, _, _ = r.m.decode_rows(20)              # captures the multi-step graph and the single step
    for s in range(20):                          # the mirror follows: each step counted the token the one before produced
        if s:
            for b in range(B):
                count(r.words[b], int(ids[s - 1, b]))
    r.cur = [int(t) for t in ids[-1]]
    greedy_steps(r, 2)
    for b in range(B):
        r.spec[b] = dict(repetition=1.0 + 0.1 * b, presence=0.05 * b, frequency=0.5, bias={b: 3.0})
        apply_spec(r.m, b, r.spec[b])
    greedy_steps(r, 3)                           # replayed graphs, new values


def test_logprobs_of_a_biased_row_are_the_models(hip):
    B = 2
    P = prompts(B, seed=13)
    m, tw = make(hip, B), make(hip, B)
    for x in (m, tw):
        x.forward(P)
        x.set_row_logprobs(0, 5)
    raw = m.logits(rounded=False)[0]
    top = argmax_lowest(raw)
    m.set_row_logit_bias(0, {top: NINF, (top + 1) % 256: 1.0})
    a, b = m.sample_row(0, GREEDY), tw.sample_row(0, GREEDY)
    assert b == top and a != top
    la, lb = m.row_logprobs(0, 1), tw.row_logprobs(0, 1)
    np.testing.assert_array_equal(la[1], lb[1])
    assert la[2].tobytes() == lb[2].tobytes() and la[1][0][0] == top
    m.set_row_sampler(0, GREEDY).set_row_sampler(1, GREEDY)
    m.sample_row(1, GREEDY)
    m.decode_rows(3)
    lp, ids, lps, _ = m.row_logprobs(0, 3)
    raw = m.logits(rounded=False)[0]             # the last step's raw logits: its record ranks them, not the processed ones
    order = np.lexsort((np.arange(raw.size), -raw.astype(np.float64)))[:5]
    np.testing.assert_array_equal(ids[-1][:5], order)


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    B = 2
    P = prompts(B, seed=14)
    cfg, g = load_golden("llama_tiny")
    early = Model(desc_from_hf_config(cfg, "bf16", max_batch=1), hip)
    for call in (lambda: early.set_row_penalties(0, 1.2), lambda: early.set_row_logit_bias(0, {1: 1.0}), lambda: early.set_row_history(0, [1])):
        with pytest.raises(TgxError) as e:
            call()
        assert e.value.status == ST_STATE
    early.close()
    r = Rows(hip, B, P, lambda b: dict(repetition=1.2, bias={7: 0.5}) if b == 0 else {})
    m = r.m
    V = r.V
    nan, inf = float("nan"), float("inf")
    bad = [
        lambda: m.set_row_penalties(-1, 1.2), lambda: m.set_row_penalties(B, 1.2),
        lambda: m.set_row_penalties(0, 0.0), lambda: m.set_row_penalties(0, -1.0), lambda: m.set_row_penalties(0, nan), lambda: m.set_row_penalties(0, inf),
        lambda: m.set_row_penalties(0, 1.0, nan, 0.0), lambda: m.set_row_penalties(0, 1.0, 0.0, inf), lambda: m.set_row_penalties(0, 1.0, -inf, 0.0),
        lambda: m.set_row_logit_bias(B, {1: 1.0}), lambda: m.set_row_logit_bias(-1, {1: 1.0}),
        lambda: m.set_row_logit_bias(0, [(i % V, 0.1) for i in range(MAX_LOGIT_BIAS + 1)]),
        lambda: m.set_row_logit_bias(0, {V: 1.0}), lambda: m.set_row_logit_bias(0, {-1: 1.0}),
        lambda: m.set_row_logit_bias(0, [(3, 1.0), (4, 1.0), (3, 2.0)]),
        lambda: m.set_row_logit_bias(0, {3: nan}), lambda: m.set_row_logit_bias(0, {3: inf}),
        lambda: m.set_row_logit_bias(0, {i: NINF for i in range(V)}),
        lambda: m.set_row_history(B, [1]), lambda: m.set_row_history(0, [V]), lambda: m.set_row_history(0, [1], [-1]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(TgxError) as e:
            call()
        assert e.value.status == ST_INVALID, i
    with pytest.raises(TgxError) as e:           # a null cfg
        m._check(m.be.set_row_penalties(m._ctx, 0, None))
    assert e.value.status == ST_INVALID
    with pytest.raises(TgxError) as e:           # n out of range, seen by the C interface
        m._check(m.be.set_row_logit_bias(m._ctx, 0, -1, None, None))
    assert e.value.status == ST_INVALID
    m.set_row_logit_bias(1, {i: NINF for i in range(V - 1)})      # legal: fewer than V bans
    m.set_row_logit_bias(1, None)
    # tgx_verify_row on a processed row: refused, nothing changes
    n0 = m.past_length_row(0)
    with pytest.raises(TgxError) as e:
        m.verify_row(0, [1, 2, 3])
    assert e.value.status == ST_UNSUPPORTED and m.past_length_row(0) == n0
    out, fin = m.verify_row(1, [1, 2, 3])        # the unprocessed neighbour verifies
    assert 1 <= len(out) <= 4
    r.cur[1] = int(out[-1])
    # nothing above changed row 0's settings or poisoned the context: it still follows the restatement
    greedy_steps(r, 3, rows=[0])
