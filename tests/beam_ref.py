"""The reference of tgx_beam_select (include/tgx.h) in numpy float64, and the generator of tests/test_hip_beam.py's injected cases.  No GPU, no library: the cases
and the assertion on their gaps can be produced and checked on a CPU (python tests/beam_ref.py prints every case's smallest gap).

key(i, t) = float64(float32 score_i) + (float64(v_i[t]) - lse_i), lse_i the float64 log-sum-exp of the fp32 vector; the joint order is key descending, array index i
ascending, rank within the row (value descending, index ascending) ascending; -inf keys are no candidates.  The result is the prefix that ends at the k-th
candidate whose token is no end id, cut at 32 entries."""
import numpy as np

MAX_CAND = 32


def log_softmax64(v):
    v = np.asarray(v, np.float64)
    m = v.max()
    if not np.isfinite(m):
        return np.full(v.shape, -np.inf)
    with np.errstate(divide="ignore"):
        return v - (m + np.log(np.exp(v - m).sum()))


_rows = {}      # id(vector) -> (vector, its log_softmax, its first entries): the cases share a handful of vectors


def row_ref(v, depth=48):
    if id(v) not in _rows or _rows[id(v)][0] is not v:
        _rows[id(v)] = (v, log_softmax64(v), np.argsort(-np.asarray(v, np.float64), kind="stable")[:depth])
    return _rows[id(v)][1:]


def joint_order(vecs, scores):
    """the first 48 entries of every row (more than any row can bring into a prefix of 32), merged in the joint order -> list of (key, i, rank, token, lp)"""
    out = []
    for i, v in enumerate(vecs):
        lp, order = row_ref(v)
        for rank, t in enumerate(order):
            key = float(np.float64(np.float32(scores[i])) + lp[t])
            if key > -np.inf:
                out.append((key, i, rank, int(t), float(lp[t])))
    out.sort(key=lambda c: (-c[0], c[1], c[2]))
    return out


def select(vecs, scores, k, end_ids=()):
    """-> (prefix, rest): the candidates tgx_beam_select returns and the ones behind them"""
    cands = joint_order(vecs, scores)
    ends = set(int(e) for e in end_ids)
    n, live = 0, 0
    while n < len(cands) and n < MAX_CAND and live < k:
        live += cands[n][3] not in ends
        n += 1
    return cands[:n], cands[n:]


def tied_by_construction(a, b, vecs, scores):
    """candidates a, b carry the same key because they are the same numbers: equal scores, identical rows (or one row), equal logits"""
    (_, ia, _, ta, _), (_, ib, _, tb, _) = a, b
    return (np.float32(scores[ia]) == np.float32(scores[ib]) and (ia == ib or np.array_equal(vecs[ia], vecs[ib])) and vecs[ia][ta] == vecs[ib][tb])


def min_gap(vecs, scores, k, end_ids=()):
    """the smallest key difference between adjacent candidates of the returned prefix and its first follower that are not tied by construction (inf: none)"""
    prefix, rest = select(vecs, scores, k, end_ids)
    seq = prefix + rest[:1]
    gap = np.inf
    for a, b in zip(seq, seq[1:]):
        if not tied_by_construction(a, b, vecs, scores):
            gap = min(gap, a[0] - b[0])
    return gap


# ---- the injected cases ---------------------------------------------------------------------------------------------------------------------------------
def injected(V, rng):
    """the five vectors of tests/test_hip_logprobs.py::injected"""
    from test_hip_logprobs import injected as inj
    return inj(V, rng)


ORDER = ["normal", "dup", "holes", "spike", "equal", "normal", "dup", "holes"]      # the rows of a mixed group, in array order
SEED = {320: 3, 5003: 1, 70001: 1}      # generator seeds per vocabulary, chosen on the reference alone so that every case below clears GAP with room (python
                                        # tests/beam_ref.py: 8.8e-3, 6.5e-3, 5.4e-3; V = 320 read 9.5e-4 with seed 1 and 1.2e-3 with seed 2)
GAP = 1e-3
_drawn = {}


def rows_of(V, n, kind):
    """n rows of vocabulary V.  'mixed': the injected vectors in ORDER (the second round from a second draw); 'twins': rows that are identical in pairs — exact
    ties with identical scores"""
    if V not in _drawn:
        _drawn[V] = (injected(V, np.random.default_rng(SEED[V])), injected(V, np.random.default_rng(SEED[V] + 1000)))
    a, b = _drawn[V]
    if kind == "mixed":
        return [(a if i < 5 else b)[ORDER[i]] for i in range(n)]
    base = [a["normal"], a["dup"], b["holes"], a["equal"]]
    return [base[(i // 2) % 4] for i in range(n)]


def scores_of(n, kind, pattern, rng):
    """'near0': within a few units below 0; 'deep': the same offsets around -1e4 (an ulp of the fp32 score is ~1e-3 there); 'wide': 0 down to -1e4.  Twins share
    their score.  Offsets are multiples of 1/64: exact in fp32 at either depth"""
    off = -np.round(rng.uniform(0, 6, n) * 64) / 64
    if kind == "twins":
        off = off[(np.arange(n) // 2)]
    if pattern == "near0":
        s = off
    elif pattern == "deep":
        s = -1e4 + off
    else:
        s = np.linspace(0.0, -1e4, n) if n > 1 else np.array([-1e4])
        if kind == "twins":
            s = s[(np.arange(n) // 2) * 2]
    return s.astype(np.float32)


def end_ids_of(vecs, scores, k, n_end):
    """0: none; 1: the token at the head of the joint order (a hypothesis that ends at once); 8: every second token of the k = 8 prefix, so end-id candidates
    interleave with the others"""
    if n_end == 0:
        return []
    head = [c[3] for c in joint_order(vecs, scores)]
    if n_end == 1:
        return head[:1]
    out = []
    for t in head[::2]:
        if t not in out:
            out.append(t)
        if len(out) == n_end:
            break
    return out


def cases(V):
    """every injected case of vocabulary V: (n, kind, pattern, vecs, scores, k, end_ids)"""
    out = []
    for n in (1, 3, 8):
        for kind in ("mixed", "twins"):
            if kind == "twins" and n == 1:
                continue
            vecs = rows_of(V, n, kind)
            for pi, pattern in enumerate(("near0", "deep", "wide")):
                scores = scores_of(n, kind, pattern, np.random.default_rng(SEED[V] * 100 + n * 10 + pi))
                for k in (1, 4, 8):
                    for n_end in (0, 1, 8):
                        out.append((n, kind, pattern, vecs, scores, k, end_ids_of(vecs, scores, k, n_end)))
    return out


if __name__ == "__main__":
    for V in SEED:
        worst = min(min_gap(vecs, scores, k, ends) for (_, _, _, vecs, scores, k, ends) in cases(V))
        print(f"V={V} seed={SEED[V]}: {len(cases(V))} cases, smallest gap {worst:.3e} ({'ok' if worst >= GAP else 'TOO SMALL'})")
