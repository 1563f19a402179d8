"""tgx_verify_tree (include/tgx.h): a token TREE of guesses verified in one pass — pass position p in cache slot past + p, rotated for past + depth(p), attending
the history and its own branch; the walk and the compaction of the accepted branch on the device.  The row must stand as after out_n steps of tgx_decode_rows, up
to the order of the fp32 sums, with the project's numbers (tests/test_hip_verify_row.py): GPU against GPU rel_err < 1e-3, equal greedy ids where the CPU oracle's
top-2 gap clears BAND, cache rows by check_kv.  Held to:
  * every node sees its branch and nothing else: each node's row of tgx_read_pass_logits against the last row of a tgx_verify_row chain pass over its root path
    on a fork of the row (1e-3).  So that a missing mask (or a rotation by slot instead of depth) cannot pass, the CPU oracle's logits for the nodes in index order
    as ONE linear sequence differ from its logits for the node's root path by at least 4e-3 at every compared node that is not on the first branch — asserted
    from the oracle alone, no node skipped; node tokens are drawn from seed TOKEN_SEED, for which that holds;
  * equals stepping, greedy: trees around a control context's own greedy ids, the right branch at sibling rank 0 / 1 / last, the first wrong token at depth 0, 1,
    the middle, the last level (the leaf alone) and nowhere, every tree at every past; ids, out_n, length, kv.free_tokens, logits, every live cache row (a K row at the wrong rotation or in the wrong slot fails check_kv
    grossly), then 4 forced steps; prompt seeds whose oracle top-2 gap clears BAND (test_hip_verify_row.SEEDS and NEW_SEEDS, found the same way on the CPU);
  * equals stepping, sampled: tests/test_hip_verify_sampled.py's scheme — the draws restated from the pass's own logits with the key of each node's DEPTH, the walk
    in Python, the logits slot bit for bit, tgx_sample_row returns the last id again;
  * a chain-shaped tree is tgx_verify_row_sampled bit for bit; the compaction moves bits (the same tree renumbered so that the accepted path is in place);
  * lifecycle: determinism, stop id and max_new, kv.free_tokens, an exhausted budget, a forked source, the other rows of a batch, every refusal, which refusal
    wins, the TGX_ERR_UNSUPPORTED cases.
Pasts: 5; 58 (the new keys straddle a 64-key tile); 120 (they straddle a 128-token block; new length exactly 128); 700 (the key-split attention form: automatic
at head_dim 64, option extend.attn_splits at head_dim 128).
Reduced for the few-seconds budget of a case, and only there: the branch test compares every node of all five trees at past 5 and of two trees at each other past
(MASK_CASES: the oracle feeds every node on a CPU — 7 s per tree for the Mistral cut at past 700 — and every node costs a fork and a chain pass); the sampled test
runs two sampler configurations.  Everything else runs the three models, paged and unpaged, at the four pasts."""
import ctypes
from ctypes import c_int32, c_int64

import numpy as np
import pytest

from conftest import rel_err
from test_hip_verify_row import BAND, BLK, CTX, FORCED, K, SEEDS, V, check_kv, check_row, cut, force, gpu_model, kv_all, oracle_run, start
from tinygpt_amd import synth
from tinygpt_amd.ffi import GREEDY, SamplerCfg, TgxError
from verify_sampled_util import expected_draw, top_p_band

pytestmark = pytest.mark.gpu
MODELS = [("llama-3.2-1b", "bf16"), ("qwen3-1.7b", "bf16"), ("mistral-7b-v0.3", "fp16")]
PASTS = (5, 58, 120, 700)
# prompt seeds of the pasts test_hip_verify_row.SEEDS does not hold, found as that table was: the first seed whose K + 1 free-running oracle steps all clear BAND
NEW_SEEDS = {
    ("llama-3.2-1b", "bf16", 58): 1, ("llama-3.2-1b", "bf16", 120): 1,
    ("qwen3-1.7b", "bf16", 58): 1, ("qwen3-1.7b", "bf16", 120): 1, ("qwen3-1.7b", "bf16", 700): 1,
    ("mistral-7b-v0.3", "fp16", 58): 1, ("mistral-7b-v0.3", "fp16", 120): 2, ("mistral-7b-v0.3", "fp16", 700): 1,
}
TOKEN_SEED = 1
MASK_BOUND = 1e-3          # that file's GPU-against-GPU bound


def prompt_seed(name, dtype, past):
    return SEEDS.get((name, dtype, past), NEW_SEEDS.get((name, dtype, past)))


# ---- the trees: parent[i] of node i (-1: a child of the row's current token)
def caterpillar(n=15):
    """a chain with one extra leaf per level: spine nodes 0, 2, 4, .., the leaf of each level right behind its spine node"""
    return [-1 if i < 2 else 2 * ((i // 2) - 1) for i in range(n)]


TREES = {
    "two": [-1, -1],                                            # M = 3
    "star": [-1] * 15,
    "caterpillar": caterpillar(),
    "interleaved": [-1, -1] + list(range(13)),                  # two branches interleaved in index order: an accepted path is non-contiguous, its moves overlap
    "binary": [-1, -1] + [(i - 2) // 2 for i in range(2, 14)],  # 14 nodes
}


def shape(parent):
    """per pass position: depth, parent position, root path (positions, root first)"""
    M = len(parent) + 1
    par = [-1] + [p + 1 for p in parent]
    depth, path = [0] * M, [[0]] + [None] * (M - 1)
    for q in range(1, M):
        depth[q] = depth[par[q]] + 1
        path[q] = path[par[q]] + [q]
    return depth, par, path


def children(par, q):
    return [c for c in range(q + 1, len(par)) if par[c] == q]


def branch(parent, rank):
    """the root-to-leaf path (positions below the root) through the child of rank min(rank, last) at every level"""
    _, par, _ = shape(parent)
    out, q = [], 0
    while children(par, q):
        ch = children(par, q)
        q = ch[min(rank, len(ch) - 1)]
        out.append(q)
    return out


def tree_tokens(parent, right, n_right, c_ids):
    """node tokens: the first n_right nodes of the branch `right` carry the control's ids (the node at depth d: c_ids[d], the token produced at depth d - 1), the
    rest of that branch and every other node a token the model will not choose there, distinct among siblings"""
    depth, par, _ = shape(parent)
    tok = [None] * len(par)
    for q in range(1, len(par)):
        d = depth[q]
        good = q in right[:n_right]
        rank = children(par, par[q]).index(q)
        tok[q] = c_ids[d] if good else (c_ids[d] + 1 + rank) % V
    return tok[1:]


def py_walk(parent, tokens, chosen):
    """the walk: chosen(position) = the token the row's settings choose at that position -> (produced ids, the positions that produced them)"""
    _, par, _ = shape(parent)
    ids, path, q = [], [], 0
    while True:
        g = int(chosen(q))
        ids.append(g); path.append(q)
        nxt = [c for c in children(par, q) if int(tokens[c - 1]) == g]
        assert len(nxt) <= 1
        if not nxt:
            return ids, path
        q = nxt[0]


def set_splits(m, name, past, on=True):
    """past 700 runs the key-split attention form: automatic at head_dim 64 (past + M > 512), by option at head_dim 128 (its automatic threshold is 1024)"""
    if past == 700 and name != "llama-3.2-1b":
        m.set_option("extend.attn_splits", 4 if on else -1)


# ---- every node sees its branch and nothing else -------------------------------------------------------------------------------------------------------------
MASK_CASES = {5: ("two", "star", "caterpillar", "interleaved", "binary"), 58: ("interleaved", "binary"), 120: ("caterpillar", "star"), 700: ("interleaved", "two")}
_oracle_mask = {}


def node_tokens(n, past, tree):
    rng = np.random.default_rng([TOKEN_SEED, past, sorted(TREES).index(tree)])
    return [int(t) for t in rng.choice(V, size=n, replace=False)]


def oracle_mask_gaps(name, dtype, past, tree):
    """from the CPU oracle alone: per pass position q >= 1, rel_err between its logits with the nodes fed in index order as one linear sequence and its logits
    with its root path fed (both behind the prompt and t0); computed once per case.  The root paths share prefixes: a depth-first walk that sets the oracle's
    length back to past + depth feeds every node once"""
    key = (name, dtype, past, tree)
    if key not in _oracle_mask:
        from oracle.oracle_ffi import OracleModel
        d, peaked = cut(name, dtype)
        ref = OracleModel(d).load_synthetic(1234, 0.02, peaked=peaked).finalize()
        prompt = synth.synth_prompt(V, past, prompt_seed(name, dtype, past))
        ref.forward(prompt[None, :])
        t0 = int(ref.sample(GREEDY)[0])
        parent = TREES[tree]
        toks = [t0] + node_tokens(len(parent), past, tree)
        depth, par, _ = shape(parent)

        def feed(t):
            ref.forward(np.array([[t]], dtype=np.int64))
            return ref.logits(rounded=False)[0].copy()
        ref.set_past(past)
        linear = [feed(t) for t in toks]
        by_path = [None] * len(toks)

        def dfs(q):
            ref.set_past(past + depth[q])                   # the cache holds q's ancestors in the slots below
            by_path[q] = feed(toks[q])
            for c in children(par, q):
                dfs(c)
        dfs(0)
        ref.close()
        _oracle_mask[key] = [rel_err(linear[q][None, :], by_path[q][None, :]) for q in range(len(toks))]
    return _oracle_mask[key]


@pytest.mark.parametrize("past", PASTS)
@pytest.mark.parametrize("name,dtype,paged", [(n, d, p) for n, d in MODELS for p in (0, 1)])
def test_every_node_sees_its_branch_and_nothing_else(name, dtype, paged, past, oracle_lib):
    budget = 4 * CTX if paged else 0
    m = gpu_model(name, dtype, 2, budget)
    set_splits(m, name, past)
    prompt = synth.synth_prompt(V, past, prompt_seed(name, dtype, past))
    for tree in MASK_CASES[past]:
        parent = TREES[tree]
        depth, par, paths = shape(parent)
        first_branch = [q for q in range(len(par)) if paths[q] == list(range(q + 1))]      # its linear prefix IS its root path
        gaps = oracle_mask_gaps(name, dtype, past, tree)
        for q in range(1, len(par)):
            if q not in first_branch:
                assert gaps[q] >= 4 * MASK_BOUND, (name, dtype, past, tree, q, gaps[q])     # the oracle's own logits: a missing mask moves this node's logits
        tokens = node_tokens(len(parent), past, tree)
        start(m, prompt)
        m.verify_tree(0, tokens, parent)
        L = m.pass_logits()
        assert L.shape[0] == len(parent) + 1
        for q in range(1, len(par)):                        # no node skipped
            start(m, prompt)
            m.fork_row(0, [1])
            m.verify_row(1, [tokens[p - 1] for p in paths[q][1:]])
            C = m.pass_logits()
            assert C.shape[0] == depth[q] + 1
            e = rel_err(L[q][None, :], C[-1][None, :])
            assert e < MASK_BOUND, (name, dtype, paged, past, tree, q, e)
            if q == 1:
                assert rel_err(L[0][None, :], C[0][None, :]) < MASK_BOUND
    m.close()


# ---- equals stepping, greedy ---------------------------------------------------------------------------------------------------------------------------------
# (tree, sibling rank of the right branch, depth of the first wrong token: 0, 1, "mid", "last" = the branch's leaf alone is wrong — the walk reaches the deepest
# internal node and the child search misses on a leaf —, None = nowhere)
STEP_CASES = [(t, r, w) for t in ("caterpillar", "interleaved", "binary") for r, w in ((0, None), (1, 0), (1, 1), (2, "mid"), (2, None), (0, "mid"), (0, "last"), (1, "last"))] + \
             [("two", 0, None), ("two", 1, None), ("two", 1, 0), ("two", 1, "last"), ("star", 0, None), ("star", 14, None), ("star", 7, 0), ("star", 3, "last")]


@pytest.mark.parametrize("past", PASTS)
@pytest.mark.parametrize("name,dtype,paged", [(n, d, p) for n, d in MODELS for p in (0, 1)])
def test_tree_equals_stepping_greedy(name, dtype, paged, past, oracle_lib):
    budget = 2 * CTX if paged else 0
    gpu, ctrl = gpu_model(name, dtype, 1, budget), gpu_model(name, dtype, 1, budget)
    set_splits(gpu, name, past)
    seed = prompt_seed(name, dtype, past)
    prompt = synth.synth_prompt(V, past, seed)
    o_ids, o_gaps = oracle_run(name, dtype, past, seed)
    assert min(o_gaps) >= BAND, (name, dtype, past, seed, min(o_gaps))      # the oracle's own logits: no id comparison below is skipped
    c_ids = [start(ctrl, prompt)] + [int(t) for t in ctrl.decode_rows(K)[0][:, 0]]
    assert c_ids == o_ids, (name, dtype, past)
    todo = list(STEP_CASES)
    if past == 120:
        todo.append(("caterpillar", 0, 7))                  # 8 tokens: the new length is exactly 128
    for tree, rank, wrong in todo:
        what = (name, dtype, paged, past, tree, rank, wrong)
        parent = TREES[tree]
        right = branch(parent, rank)
        n_right = {None: len(right), "mid": len(right) // 2, "last": len(right) - 1}.get(wrong, wrong)
        tokens = tree_tokens(parent, right, n_right, c_ids)
        want_ids, want_path = py_walk(parent, tokens, lambda q, _d=shape(parent)[0]: c_ids[_d[q] + 1])
        want = len(want_ids)
        assert want == n_right + 1 and want_path[1:] == right[:n_right], what
        assert start(gpu, prompt) == c_ids[0], what
        ids, fin = gpu.verify_tree(0, tokens, parent)
        assert list(ids) == want_ids == c_ids[1:1 + want] and fin == 0, (what, list(ids), want_ids)
        assert gpu.past_length_row(0) == past + want == gpu.past_length, what
        if paged:
            assert gpu.get_option("kv.free_tokens") == budget - -(-(past + want) // BLK) * BLK, what
        assert start(ctrl, prompt) == c_ids[0]
        ctrl.decode_rows(want)
        lg, lc = gpu.logits(rounded=False)[0].copy(), ctrl.logits(rounded=False)[0].copy()
        assert rel_err(lg[None, :], lc[None, :]) < 1e-3, (what, rel_err(lg[None, :], lc[None, :]))
        assert int(np.argmax(lg)) == int(np.argmax(lc)) == c_ids[want], what      # never skipped: the oracle's gap is >= BAND
        check_kv(kv_all(gpu, 0), kv_all(ctrl, 0), dtype, what)
        for t in FORCED:
            tg, tc = force(gpu, np.array([t])), force(ctrl, np.array([t]))
            check_row(gpu.logits(rounded=False)[0], tg[0], ctrl.logits(rounded=False)[0], tc[0])
        assert gpu.past_length_row(0) == past + want + len(FORCED), what
    gpu.close(); ctrl.close()


# ---- equals stepping, sampled --------------------------------------------------------------------------------------------------------------------------------
def sampled_cfgs():
    T = 100.0                  # the peaked cuts' logits reach several hundred: draws leave the argmax (tests/test_hip_verify_sampled.py)
    return {"top-p": SamplerCfg(T, 0, 0.9, 0.0), "all": SamplerCfg(T, 40, 0.9, 0.05)}


@pytest.mark.parametrize("name,dtype,paged", [(n, d, p) for n, d in MODELS for p in (0, 1)])
def test_tree_equals_stepping_sampled(name, dtype, paged, oracle_lib):
    """context A steps under the row's sampler; context B (same kernels, same first token) verifies a tree whose siblings include A's draw at every depth of one
    branch.  What B must return is computed from B's own pass logits with the key of each position's DEPTH; nothing is skipped"""
    budget = 3 * CTX if paged else 0
    A, B = gpu_model(name, dtype, 3, budget), gpu_model(name, dtype, 3, budget)
    row, seed = 2, 977
    draws_n, off_argmax, band, deep = 0, 0, 0, 0
    for cname, cfg in sampled_cfgs().items():
        for past in PASTS:
            set_splits(B, name, past)
            prompts = [synth.synth_prompt(V, past if r == row else 5, 31 + r) for r in range(3)]
            firsts = []
            for m in (A, B):
                m.reset_cache()
                for r, p in enumerate(prompts):
                    m.forward_row(r, p)
                for r in range(3):
                    if r != row:
                        m.sample_row(r, GREEDY)
                m.set_row_sampler(row, cfg, seed)
                firsts.append(int(m.sample_row(row, cfg, seed)))
            assert firsts[0] == firsts[1]
            c_ids = [firsts[0]] + [int(t) for t in A.decode_rows(K)[0][:, row]]
            for tree, rank in (("interleaved", 1), ("binary", 2), ("caterpillar", 0), ("star", 9)):
                what = (name, dtype, paged, cname, past, tree, rank)
                parent = TREES[tree]
                depth, par, _ = shape(parent)
                right = branch(parent, rank)
                tokens = tree_tokens(parent, right, len(right), c_ids)
                B.reset_cache()
                for r, p in enumerate(prompts):
                    B.forward_row(r, p)
                for r in range(3):
                    if r != row:
                        B.sample_row(r, GREEDY)
                B.set_row_sampler(row, cfg, seed)
                assert int(B.sample_row(row, cfg, seed)) == c_ids[0], what
                ids, fin = B.verify_tree(row, tokens, parent)
                L = B.pass_logits()
                assert L.shape[0] == len(parent) + 1
                drawn = {}

                def chosen(q):
                    s, _ = expected_draw(cfg, L[q], seed, past + depth[q] + 1, row)
                    drawn[q] = s
                    return s
                want_ids, want_path = py_walk(parent, tokens, chosen)
                for q, s in drawn.items():
                    draws_n += 1
                    off_argmax += int(s != int(np.argmax(L[q])))
                    band += int(s in top_p_band(cfg, L[q]))
                assert list(ids) == want_ids and fin == 0, (what, list(ids), want_ids)
                assert B.past_length_row(row) == past + len(want_ids), what
                np.testing.assert_array_equal(B.logits(rounded=False)[row], L[want_path[-1]], err_msg=str(what))
                assert int(B.sample_row(row, cfg, seed)) == want_ids[-1], what
                deep += int(len(want_ids) >= 3)
            set_splits(B, name, past, on=False)
    assert off_argmax >= 0.25 * draws_n, (off_argmax, draws_n)      # an argmax in place of the draw would not pass
    assert deep >= 8, deep                                           # the walks went down the trees (the two paths differ by summation order alone)
    assert band == 0, band
    A.close(); B.close()


def test_sampled_tree_leaves_the_row_like_a_control():
    """the row afterwards: logits and cache rows against a control that took the accepted inputs by tgx_extend_row, four forced steps, no tgx_read_probs vector"""
    name, dtype = "llama-3.2-1b", "bf16"
    gpu, ctrl = gpu_model(name, dtype), gpu_model(name, dtype)
    cfg, seed, past = sampled_cfgs()["top-p"], 5, 58
    prompt = synth.synth_prompt(V, past, 3)

    def begin(m):
        m.reset_cache(); m.forward_row(0, prompt); m.set_row_sampler(0, cfg, seed)
        return int(m.sample_row(0, cfg, seed))
    t0 = begin(gpu)
    c_ids = [t0] + [int(t) for t in gpu.decode_rows(8)[0][:, 0]]
    for tree, rank in (("interleaved", 1), ("binary", 1)):
        parent = TREES[tree]
        right = branch(parent, rank)
        tokens = tree_tokens(parent, right, len(right), c_ids)
        assert begin(gpu) == t0
        ids, fin = gpu.verify_tree(0, tokens, parent)
        assert len(ids) >= 2, (tree, ids)
        with pytest.raises(TgxError) as ei:                 # the pass's scratch is not the row's: no vector until its next sampled step
            gpu.probs()
        assert ei.value.status == 4
        ctrl.reset_cache(); ctrl.forward_row(0, prompt)
        ctrl.extend_row(0, [t0] + [int(t) for t in ids[:-1]])
        assert gpu.past_length_row(0) == ctrl.past_length_row(0) == past + len(ids)
        lg, lc = gpu.logits(rounded=False)[0], ctrl.logits(rounded=False)[0]
        assert rel_err(lg[None, :], lc[None, :]) < 1e-3
        check_kv(kv_all(gpu, 0), kv_all(ctrl, 0), dtype, tree)
        gpu.set_row_sampler(0, GREEDY, 0)
        for t in FORCED:
            tg, tc = force(gpu, np.array([t])), force(ctrl, np.array([t]))
            check_row(gpu.logits(rounded=False)[0], tg[0], ctrl.logits(rounded=False)[0], tc[0])
    gpu.close(); ctrl.close()


# ---- a chain-shaped tree, the compaction ---------------------------------------------------------------------------------------------------------------------
def wrong_at(ids, j):
    d = list(ids)
    if j is not None:
        d[j] = (d[j] + 1) % V
    return d


@pytest.mark.parametrize("sampled", [0, 1])
@pytest.mark.parametrize("name,dtype,paged", [(n, d, p) for n, d in MODELS for p in (0, 1)])
def test_a_chain_shaped_tree_is_verify_row_sampled(name, dtype, paged, sampled):
    """ids, logits slot, pass logits, every cache row, kv.free_tokens: bit for bit, on the route the chain takes (by steps at 2 positions, skinny above)"""
    budget = 2 * CTX if paged else 0
    a, b = gpu_model(name, dtype, 1, budget), gpu_model(name, dtype, 1, budget)
    cfg, seed = (SamplerCfg(100.0, 0, 0.9, 0.0), 7) if sampled else (GREEDY, 0)
    for past, n, j in ((5, 1, None), (5, 3, 1), (58, 7, 3), (120, 7, None), (700, 15, 9)):
        set_splits(a, name, past); set_splits(b, name, past)
        prompt = synth.synth_prompt(V, past, 77)

        def begin(m):
            m.reset_cache(); m.forward_row(0, prompt); m.set_row_sampler(0, cfg, seed)
            return int(m.sample_row(0, cfg, seed))
        begin(a)
        draft = wrong_at([int(t) for t in a.decode_rows(n)[0][:, 0]], j)
        outs = []
        for m, call in ((a, lambda: a.verify_row_sampled(0, draft)), (b, lambda: b.verify_tree(0, draft, list(range(-1, n - 1))))):
            begin(m)
            ids, fin = call()
            outs.append((list(ids), fin, m.logits(rounded=False)[0].copy(), kv_all(m, 0), m.get_option("kv.free_tokens") if paged else 0, m.pass_logits()))
        x, y = outs
        assert x[0] == y[0] and x[1] == y[1] and x[4] == y[4], (past, n, j, x[0], y[0])
        np.testing.assert_array_equal(x[2], y[2]); np.testing.assert_array_equal(x[5], y[5])
        for (k1, v1), (k2, v2) in zip(x[3], y[3]):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    a.close(); b.close()


@pytest.mark.parametrize("name,dtype,paged", [(n, d, p) for n, d in MODELS for p in (0, 1)])
def test_compaction_moves_bits(name, dtype, paged):
    """the same tree with its nodes renumbered so that the accepted path is already in place (the right branch first, as a chain): layer 0's K / V rows of a node
    depend on its token and its depth alone, so the moved rows are bit-identical to the rows written in place; deeper layers see the new keys in another order of
    summation and match within check_kv"""
    budget = 2 * CTX if paged else 0
    m = gpu_model(name, dtype, 1, budget)
    for past in PASTS:
        set_splits(m, name, past)
        prompt = synth.synth_prompt(V, past, prompt_seed(name, dtype, past))
        c_ids = [start(m, prompt)] + [int(t) for t in m.decode_rows(K)[0][:, 0]]
        for tree, rank in (("interleaved", 1), ("binary", 2), ("caterpillar", 0)):
            parent = TREES[tree]
            right = branch(parent, rank)
            tokens = tree_tokens(parent, right, len(right), c_ids)
            order = [q - 1 for q in right] + [i for i in range(len(parent)) if i + 1 not in right]      # old node index of new node k: the right branch first
            new_of = {old: k for k, old in enumerate(order)}
            parent2 = [-1 if parent[old] < 0 else new_of[parent[old]] for old in order]
            tokens2 = [tokens[old] for old in order]
            assert all(p < k for k, p in enumerate(parent2)) and parent2[:len(right)] == list(range(-1, len(right) - 1))
            runs = []
            for tk, pr in ((tokens, parent), (tokens2, parent2)):
                assert start(m, prompt) == c_ids[0]
                ids, fin = m.verify_tree(0, tk, pr)
                runs.append((list(ids), kv_all(m, 0), m.logits(rounded=False)[0].copy()))
            (i1, kv1, l1), (i2, kv2, l2) = runs
            what = (name, dtype, paged, past, tree)
            assert i1 == i2 == c_ids[1:len(right) + 2], (what, i1, i2)
            assert kv1[0][0].shape[0] == past + len(i1)
            np.testing.assert_array_equal(kv1[0][0], kv2[0][0], err_msg=str(what)); np.testing.assert_array_equal(kv1[0][1], kv2[0][1], err_msg=str(what))
            check_kv(kv1, kv2, dtype, what)
            assert rel_err(l1[None, :], l2[None, :]) < 1e-3, what
    m.close()


# ---- lifecycle -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("llama-3.2-1b", "bf16"), ("mistral-7b-v0.3", "fp16")])
def test_tree_is_deterministic_and_paged_equals_unpaged(name, dtype):
    flat, paged = gpu_model(name, dtype), gpu_model(name, dtype, 1, 2 * CTX)
    for past, tree, rank in ((5, "two", 1), (120, "interleaved", 1), (600, "binary", 2)):
        prompt = synth.synth_prompt(V, past, 77)
        parent = TREES[tree]
        runs = []
        for m in (flat, paged):
            c_ids = [start(m, prompt)] + [int(t) for t in m.decode_rows(K)[0][:, 0]]
            right = branch(parent, rank)
            tokens = tree_tokens(parent, right, len(right), c_ids)
            two = []
            for _ in range(2):
                start(m, prompt)
                ids, fin = m.verify_tree(0, tokens, parent)
                two.append((list(ids), fin, m.logits(rounded=False)[0].copy(), kv_all(m, 0), m.pass_logits(), int(m.decode_rows(1)[0][0, 0]), m.logits(rounded=False)[0].copy()))
            runs.append(two[0])
            for a, b in ((two[0], two[1]), ):
                assert a[0] == b[0] and a[1] == b[1] and a[5] == b[5]
                for i in (2, 4, 6):
                    np.testing.assert_array_equal(a[i], b[i])
                for (k1, v1), (k2, v2) in zip(a[3], b[3]):
                    np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
        a, b = runs
        assert a[0] == b[0] and a[5] == b[5], (name, past, "paged vs unpaged")
        for i in (2, 4, 6):
            np.testing.assert_array_equal(a[i], b[i])
        for (k1, v1), (k2, v2) in zip(a[3], b[3]):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    flat.close(); paged.close()


def right_tree(m, prompt, tree="interleaved", rank=1, n_steps=K):
    """(t0, the control ids, tokens of `tree` with its rank-th branch all right) from a throw-away run of m itself"""
    t0 = start(m, prompt)
    c_ids = [t0] + [int(t) for t in m.decode_rows(n_steps)[0][:, 0]]
    parent = TREES[tree]
    right = branch(parent, rank)
    return t0, c_ids, tree_tokens(parent, right, len(right), c_ids), parent


def test_stop_conditions_end_the_walk_on_the_device():
    m = gpu_model("llama-3.2-1b", "bf16", 1, 2 * CTX)
    prompt = synth.synth_prompt(V, 40, 3)
    t0, c_ids, tokens, parent = right_tree(m, prompt)
    steps = c_ids[1:]
    assert steps[2] not in steps[:2]
    assert start(m, prompt) == t0
    m.set_row_stop(0, 0, [steps[2]])                        # a stop id at produced index 2 of a branch that is right all the way down
    ids, fin = m.verify_tree(0, tokens, parent)
    assert list(ids) == steps[:3] and fin == 1 and m.past_length_row(0) == 43
    assert m.get_option("kv.free_tokens") == 2 * CTX - BLK
    with pytest.raises(TgxError) as ei:                     # finished: as after tgx_decode_rows
        m.verify_tree(0, tokens, parent)
    assert ei.value.status == 4
    assert start(m, prompt) == t0
    m.set_row_stop(0, 2, [])                                # max_new = 2
    ids, fin = m.verify_tree(0, tokens, parent)
    assert list(ids) == steps[:2] and fin == 2 and m.past_length_row(0) == 42
    assert start(m, prompt) == t0
    m.set_row_stop(0, 0, [steps[0]])                        # the token of the root position itself
    ids, fin = m.verify_tree(0, tokens, parent)
    assert list(ids) == steps[:1] and fin == 1 and m.past_length_row(0) == 41
    m.close()


def test_paged_free_tokens_follow_the_new_length():
    budget = 4 * BLK
    m = gpu_model("llama-3.2-1b", "bf16", 1, budget)
    prompt = synth.synth_prompt(V, 250, 9)                  # two blocks; a pass of 16 positions from 250 needs a third
    t0, c_ids, tokens, parent = right_tree(m, prompt)
    right = branch(parent, 1)
    assert start(m, prompt) == t0 and m.get_option("kv.free_tokens") == budget - 2 * BLK
    ids, fin = m.verify_tree(0, tree_tokens(parent, right, 2, c_ids), parent)      # 3 tokens: length 253 -> the third block goes back
    assert list(ids) == c_ids[1:4] and m.get_option("kv.free_tokens") == budget - 2 * BLK
    assert start(m, prompt) == t0
    ids, fin = m.verify_tree(0, tokens, parent)                                    # 8 tokens: length 258 -> three blocks
    assert list(ids) == c_ids[1:9] and m.past_length_row(0) == 258 and m.get_option("kv.free_tokens") == budget - 3 * BLK
    m.close()


def test_budget_exhausted_is_refused_and_changes_nothing():
    budget = 3 * BLK
    gpu = gpu_model("llama-3.2-1b", "bf16", 2, budget)
    start(gpu, synth.synth_prompt(V, 250, 9))
    gpu.fork_row(0, [1])                                    # 1 shared + 2 tails = 3 blocks: nothing free
    assert gpu.get_option("kv.free_tokens") == 0
    l0, kv0 = gpu.logits(rounded=False).copy(), [kv_all(gpu, r) for r in (0, 1)]
    with pytest.raises(TgxError) as ei:
        gpu.verify_tree(1, [1, 2, 3, 4, 5, 6, 7], [-1, -1, 0, 1, 2, 3, 4])      # 250 + 8 = 258: a third block for the row
    assert ei.value.status == 8
    assert gpu.get_option("kv.free_tokens") == 0 and gpu.past_length_row(1) == 250 and gpu.past_length_row(0) == 250
    np.testing.assert_array_equal(gpu.logits(rounded=False), l0)
    for r in (0, 1):
        for (k1, v1), (k2, v2) in zip(kv_all(gpu, r), kv0[r]):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    ids, fin = gpu.verify_tree(1, [1, 2, 3, 4, 5], [-1, -1, 0, 1, 2])           # 250 + 6 = 256 fits the row's own tail block
    assert len(ids) >= 1 and gpu.get_option("kv.free_tokens") == 0
    gpu.close()


def test_tree_on_a_forked_copy_leaves_the_source_alone():
    budget = 4 * BLK
    gpu, ctrl = gpu_model("llama-3.2-1b", "bf16", 2, budget), gpu_model("llama-3.2-1b", "bf16", 2, budget)
    prompt = synth.synth_prompt(V, 250, 9)
    t0, c_ids, tokens, parent = right_tree(ctrl, prompt)
    for m in (gpu, ctrl):
        start(m, prompt)
        m.fork_row(0, [1])                                  # one full block shared, a tail block each: 3 blocks, 1 free
    right = branch(parent, 1)
    ids, fin = gpu.verify_tree(1, tree_tokens(parent, right, 1, c_ids), parent)      # 266 positions: the free block is taken, and goes back at length 252
    assert list(ids) == c_ids[1:3] and gpu.past_length_row(1) == 252 and gpu.past_length_row(0) == 250
    assert gpu.get_option("kv.free_tokens") == budget - 3 * BLK
    np.testing.assert_array_equal(gpu.logits(rounded=False)[0], ctrl.logits(rounded=False)[0])
    for (k1, v1), (k2, v2) in zip(kv_all(gpu, 0), kv_all(ctrl, 0)):
        np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    k, v = gpu.read_kv(0, 0)
    with pytest.raises(TgxError) as ei:                     # the full block is still shared
        gpu.write_kv(0, 0, k[:BLK], v[:BLK])
    assert ei.value.status == 4
    og, oc = gpu.decode_rows(1)[0], ctrl.decode_rows(1)[0]
    assert og[0, 0] == oc[0, 0]
    np.testing.assert_array_equal(gpu.logits(rounded=False)[0], ctrl.logits(rounded=False)[0])
    gpu.close(); ctrl.close()


@pytest.mark.parametrize("paged", [0, 1])
def test_tree_in_a_running_batch_leaves_the_other_rows_alone(paged):
    budget = 6 * BLK if paged else 0
    gpu, ctrl = gpu_model("llama-3.2-1b", "bf16", 3, budget), gpu_model("llama-3.2-1b", "bf16", 3, budget)
    prompts = np.stack([synth.synth_prompt(V, 50, 60 + r) for r in range(3)])
    for m in (gpu, ctrl):
        m.forward(prompts); m.sample(GREEDY); m.decode(2, GREEDY)
    look = [int(t) for t in ctrl.decode_rows(4)[0][:, 1]]   # row 1's next ids, from a throw-away run of the control
    ctrl.reset_cache(); ctrl.forward(prompts); ctrl.sample(GREEDY); ctrl.decode(2, GREEDY)
    parent = TREES["binary"]
    right = branch(parent, 1)
    ids, fin = gpu.verify_tree(1, tree_tokens(parent, right, 2, [None] + look), parent)
    assert list(ids) == look[:3] and fin == 0
    assert [gpu.past_length_row(r) for r in range(3)] == [52, 55, 52]
    lg, lc = gpu.logits(rounded=False), ctrl.logits(rounded=False)
    for r in (0, 2):
        np.testing.assert_array_equal(lg[r], lc[r])
        for (k1, v1), (k2, v2) in zip(kv_all(gpu, r), kv_all(ctrl, r)):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(v1, v2)
    og, oc = gpu.decode_rows(2)[0], ctrl.decode_rows(2)[0]
    np.testing.assert_array_equal(og[:, [0, 2]], oc[:, [0, 2]])
    lg, lc = gpu.logits(rounded=False), ctrl.logits(rounded=False)
    for r in (0, 2):
        np.testing.assert_array_equal(lg[r], lc[r])
    gpu.close(); ctrl.close()


def test_every_refusal_changes_nothing():
    budget = 4 * BLK
    gpu, ctrl = gpu_model("llama-3.2-1b", "bf16", 4, budget), gpu_model("llama-3.2-1b", "bf16", 4, budget)
    prompts = np.stack([synth.synth_prompt(V, 30, 11 + r) for r in range(3)])
    for m in (gpu, ctrl):
        m.forward(prompts); m.sample(GREEDY)
        m.reset_row(2)                                      # row 2 retired; row 3 never used

    def state():
        return ([gpu.past_length_row(r) for r in range(4)], gpu.get_option("kv.free_tokens"), gpu.logits(rounded=False).copy())

    def refused(status, row, tokens, parent, prepare=None):
        if prepare:
            prepare()
        s0 = state()
        with pytest.raises(TgxError) as ei:
            gpu.verify_tree(row, tokens, parent)
        assert ei.value.status == status, (status, row, tokens, parent, str(ei.value))
        s1 = state()
        assert s0[0] == s1[0] and s0[1] == s1[1]
        np.testing.assert_array_equal(s0[2], s1[2])

    refused(1, -1, [1, 2], [-1, -1]); refused(1, 4, [1, 2], [-1, -1])     # row outside [0, max_batch)
    refused(1, 0, [], []); refused(1, 0, list(range(16)), [-1] * 16)      # n_nodes outside [1, 15]
    refused(1, 0, [1, V], [-1, -1]); refused(1, 0, [-1, 2], [-1, -1])     # a token id out of range
    refused(1, 0, [1, 2, 3], [-1, 1, 0]); refused(1, 0, [1, 2, 3], [-1, -1, 2]); refused(1, 0, [1, 2], [-2, -1]); refused(1, 0, [1, 2], [0, -1])      # parent[i] outside [-1, i)
    refused(1, 0, [5, 5], [-1, -1]); refused(1, 0, [5, 6, 7, 7], [-1, -1, 0, 0])      # two children of one parent with the same token
    n, f = c_int32(), c_int32()
    out = (c_int64 * 16)()
    t = (c_int64 * 2)(1, 2)
    p = (c_int32 * 2)(-1, -1)
    be, ctx = gpu.be, gpu._ctx
    assert be.verify_tree(ctx, 0, None, p, 2, out, ctypes.byref(n), ctypes.byref(f)) == 1      # null pointers
    assert be.verify_tree(ctx, 0, t, None, 2, out, ctypes.byref(n), ctypes.byref(f)) == 1
    assert be.verify_tree(ctx, 0, t, p, 2, None, ctypes.byref(n), ctypes.byref(f)) == 1
    assert be.verify_tree(ctx, 0, t, p, 2, out, None, ctypes.byref(f)) == 1
    assert be.verify_tree(ctx, 0, t, p, 2, out, ctypes.byref(n), None) == 1
    refused(4, 2, [1, 2], [-1, -1]); refused(4, 3, [1, 2], [-1, -1])      # a retired row, an empty one
    # the state is the control's: a decode step on both gives the same bits
    np.testing.assert_array_equal(gpu.decode_rows(1)[0], ctrl.decode_rows(1)[0])
    np.testing.assert_array_equal(gpu.logits(rounded=False), ctrl.logits(rounded=False))
    # a finished row; a row fresh from tgx_extend_row (no current token); a truncated row (no logits)
    gpu.set_row_stop(0, 1, [])
    _, new, fin = gpu.decode_rows(1)
    assert fin[0] == 2
    refused(4, 0, [1, 2], [-1, -1])
    gpu.extend_row(1, [5, 6])
    refused(4, 1, [1, 2], [-1, -1])
    gpu.sample_row(1, GREEDY)
    gpu.truncate_row(1, 10)
    refused(4, 1, [1, 2], [-1, -1])
    gpu.close(); ctrl.close()
    # the context size
    m = gpu_model("llama-3.2-1b", "bf16", 1)
    start(m, synth.synth_prompt(V, CTX - 4, 5))
    l0 = m.logits(rounded=False).copy()
    with pytest.raises(TgxError) as ei:
        m.verify_tree(0, [1, 2, 3, 4], [-1, -1, 0, 1])      # past + 5 > max_ctx
    assert ei.value.status == 8 and m.past_length_row(0) == CTX - 4
    np.testing.assert_array_equal(m.logits(rounded=False), l0)
    ids, fin = m.verify_tree(0, [1, 2, 3], [-1, -1, 0])     # past + 4 == max_ctx fits
    assert len(ids) >= 1
    m.close()


def test_which_refusal_wins():
    """calls that break two rules: argument checks first, then the row's state in tgx_verify_row_sampled's order, then the tree's shape, what a tree that is no
    chain cannot have, the route, the room"""
    m = gpu_model("llama-3.2-1b", "bf16", 2, 3 * BLK)
    m.forward_row(0, synth.synth_prompt(V, 250, 5)); m.forward_row(1, synth.synth_prompt(V, 31, 12))
    for r in (0, 1):
        m.sample_row(r, GREEDY)

    def no(status, text, row, tokens, parent):
        s0 = ([m.past_length_row(r) for r in range(2)], m.get_option("kv.free_tokens"))
        with pytest.raises(TgxError) as ei:
            m.verify_tree(row, tokens, parent)
        assert ei.value.status == status and text in str(ei.value), (status, text, str(ei.value))
        assert s0 == ([m.past_length_row(r) for r in range(2)], m.get_option("kv.free_tokens")), (row, tokens)

    no(1, "row 5 out of range", 5, [V, 2], [3, 3])                         # the row before the ids before the shape
    no(1, "token id out of range", 1, [V, 2], [3, 3])                      # an id before a parent
    m.set_row_stop(1, 1, [])
    assert m.decode_rows(1)[2][1] == 2
    no(4, "row 1 finished", 1, [7, 7], [-1, -1])                           # the row's state before the tree's shape
    m.extend_row(1, [3]); m.sample_row(1, GREEDY); m.set_row_stop(1, 0, [])
    m.set_row_penalties(1, repetition=1.3)
    no(2, "tgx_verify_tree: row 1 has a logit processor on", 1, [7, 7], [-1, -1])      # ... a processor as well
    m.set_row_penalties(1)
    m.set_row_logprobs(1, 0)
    no(1, "carries the token of an earlier child", 1, [7, 7], [-1, -1])   # the shape before the log-probability records
    no(2, "records log-probabilities", 1, [7, 8], [-1, -1])
    m.set_row_logprobs(1, -1)
    m.set_option("prefill.mfma", 0)
    no(2, "needs the skinny matrix-core pass", 0, [7, 8, 9, 10, 11, 12, 13], [-1, -1, 0, 1, 2, 3, 4])      # the route before the room (250 + 8 needs a block that is not free)
    m.set_option("prefill.mfma", 1)
    no(8, "KV budget exhausted", 0, [7, 8, 9, 10, 11, 12, 13], [-1, -1, 0, 1, 2, 3, 4])
    m.close()


def test_unsupported_cases():
    """a tree that is no chain: TGX_ERR_UNSUPPORTED and nothing changes; the same row then takes a chain-shaped tree (tgx_verify_row_sampled's pass)"""
    tree = ([7, 8, 9], [-1, -1, 0])
    chain = ([7, 8, 9], [-1, 0, 1])

    def refused(m, row=0):
        s0 = (m.past_length_row(row), m.logits(rounded=False).copy())
        with pytest.raises(TgxError) as ei:
            m.verify_tree(row, *tree)
        assert ei.value.status == 2, str(ei.value)
        assert m.past_length_row(row) == s0[0]
        np.testing.assert_array_equal(m.logits(rounded=False), s0[1])

    prompt = synth.synth_prompt(V, 20, 4)
    for name, dtype in (("llama-3.2-1b", "fp32"), ("gpt2", "bf16")):       # fp32 storage, GPT-2: no skinny route
        m = gpu_model(name, dtype)
        start(m, prompt)
        refused(m)
        assert len(m.verify_tree(0, *chain)[0]) >= 1
        m.close()
    m = gpu_model("llama-3.2-1b", "bf16")
    start(m, prompt)
    for opt in ("prefill.mfma", "prefill.skinny"):
        m.set_option(opt, 0)
        refused(m)
        m.set_option(opt, 1)
    m.set_option("prefill.min_rows", 64)                                   # a speed threshold for chains: it does not bind a tree
    ids, fin = m.verify_tree(0, *tree)
    assert len(ids) >= 1 and m.past_length_row(0) == 20 + len(ids)
    m.set_option("prefill.min_rows", 4)
    start(m, prompt)
    m.set_row_penalties(0, repetition=1.2)                                 # a logit processor
    refused(m)
    m.set_row_penalties(0)
    table = np.zeros((1, V), np.uint16)                                    # an automaton that allows everything is still a processor
    aid = m.automaton_create(table)
    m.set_row_automaton(0, aid)
    refused(m)
    m.set_row_automaton(0, -1)
    m.set_row_logprobs(0, 0)                                               # log-probability records: a tree refuses, a chain records
    refused(m)
    assert len(m.verify_tree(0, *chain)[0]) >= 1
    m.close()
    m = gpu_model("llama-3.2-1b", "bf16", 1, 2 * BLK, max_ctx=1025 * BLK)  # more than 1024 blocks per row
    start(m, synth.synth_prompt(V, 3, 4))
    refused(m)
    assert m.get_option("kv.free_tokens") == BLK
    m.close()
