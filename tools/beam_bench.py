#!/usr/bin/env python3
"""beam_bench.py — the cost of a beam-search step through tgx_beam_select / tgx_beam_advance (include/tgx.h), per cell of K beams x context x cache form:
  (a) tgx_decode_rows(1) alone on K rows: the floor;
  (b) the full beam step: (a) + tgx_beam_select + tgx_beam_advance, the K best candidates taken (so the step copies what a real search copies);
  (c) the emulation the two calls replace, on the PARENT commit's library (--parent-lib, a build without them): tgx_read_logits of the batch, the ranking on the host
      (numpy: log-softmax and the K best entries per row, merged), tgx_fork_row of each parent into freshly retired rows, a one-token tgx_extend_row per child,
      tgx_reset_row of the old rows — 2K rows.
(a) and (b) alternate inside every repetition on ONE context; (c) runs on its own context of the other library.  Every form is warmed up first; each figure is the
median of --reps repetitions with their min .. max beside it — the run-to-run spread a difference has to exceed — each timed from a synchronised device to the
call's own synchronise.

    python tools/beam_bench.py --parent-lib PATH [--model llama-3.2-1b] [--dtype bf16] [--reps 12] [--beams 4,8] [--contexts 256,2048] [--forms slabs,paged] [--out profiles/beam_search.txt]

The lines are printed and appended to --out."""
import argparse, dataclasses, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import ABI, Backend, GREEDY, Model, product_backend

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama-3.2-1b")
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--beams", default="4,8")
ap.add_argument("--contexts", default="256,2048")
ap.add_argument("--forms", default="slabs,paged")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_search.txt"))
args = ap.parse_args()

beams = [int(v) for v in args.beams.split(",")]
contexts = [int(v) for v in args.contexts.split(",")]
B, ctx = 2 * max(beams), max(contexts) + 128
desc = dataclasses.replace(known_desc(args.model, args.dtype), max_batch=B, max_ctx=ctx)
BLK = 128
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def context(backend, paged):
    m = Model(desc, backend)
    if paged:
        m.set_option("kv.budget_tokens", B * ((ctx + BLK - 1) // BLK) * BLK)
    return m.load_synthetic(1234, 0.02).finalize()


def timed(m, call):
    m.synchronize()
    t0 = time.perf_counter()
    call()
    m.synchronize()
    return (time.perf_counter() - t0) * 1e3


def seat(m, K, T):
    """K live rows 0 .. K - 1 of T positions, each with a current token"""
    m.reset_cache()
    m.forward_row(0, synth.synth_prompt(desc.vocab, T, 77))
    if K > 1:
        m.fork_row(0, list(range(1, K)))
    for r in range(K):
        m.sample_row(r, GREEDY)


class Beams:
    """(a) and (b) on the library under test"""

    def __init__(self, m, K, T):
        self.m, self.K, self.rows, self.scores = m, K, list(range(K)), np.zeros(K, np.float32)
        seat(m, K, T)

    def floor(self):
        return timed(self.m, lambda: self.m.decode_rows(1))

    def step(self):
        def run():
            self.m.decode_rows(1)
            beam, tok, score, _ = self.m.beam_select(self.rows, self.scores, self.K)
            self.copies = self.K - len(set(beam[:self.K].tolist()))
            self.rows = self.m.beam_advance(self.rows, beam[:self.K], tok[:self.K]).tolist()
            self.scores = score[:self.K].copy()
        return timed(self.m, run)


class Emulation:
    """(c): the same step with the calls the parent commit has, in 2K rows"""

    def __init__(self, m, K, T):
        self.m, self.K, self.rows, self.spare, self.scores = m, K, list(range(K)), list(range(K, 2 * K)), np.zeros(K, np.float64)
        seat(m, 2 * K, T)
        for r in self.spare:    # the batch holds 2K rows from the start: fork destinations must be retired rows of the batch
            m.reset_row(r)
        for r in range(K):      # the state the loop keeps: rows that hold logits (a one-token extension leaves them)
            m.extend_row(r, [int(r + 1)])

    def step(self):
        def run():
            m, K = self.m, self.K
            lg = m.logits(rounded=False)[self.rows].astype(np.float64)
            mx = lg.max(axis=1, keepdims=True)
            lp = lg - (mx + np.log(np.exp(lg - mx).sum(axis=1, keepdims=True)))
            top = np.argpartition(-lp, K, axis=1)[:, :K]
            cand = sorted(((self.scores[i] + lp[i, t], i, int(t)) for i in range(K) for t in top[i]), key=lambda c: (-c[0], c[1]))[:K]
            by_parent = {}
            for j, (_, i, _) in enumerate(cand):
                by_parent.setdefault(i, []).append(self.spare[j])
            for i, dst in by_parent.items():
                m.fork_row(self.rows[i], dst)
            for j, (_, _, t) in enumerate(cand):
                m.extend_row(self.spare[j], [t])
            for r in self.rows:
                m.reset_row(r)
            self.rows, self.spare = self.spare, self.rows
            self.scores = np.array([c[0] for c in cand])
        return timed(self.m, run)


cell = lambda v: f"{np.median(v):7.3f} [{min(v):7.3f} .. {max(v):7.3f}]"
say(f"# tools/beam_bench.py --model {args.model} --dtype {args.dtype} --reps {args.reps} --beams {args.beams} --contexts {args.contexts} --forms {args.forms}"
    f"{' --parent-lib <parent build>' if args.parent_lib else ''}   (ms per step: median [min .. max])")
results = {}
for form in args.forms.split(","):
    paged = form == "paged"
    m = context(product_backend(), paged)
    for K in beams:
        for T in contexts:
            run = Beams(m, K, T)
            for _ in range(3):
                run.floor(); run.step()
            a, b, copies = [], [], []
            for _ in range(args.reps):
                a.append(run.floor()); b.append(run.step()); copies.append(run.copies)
            results[(form, K, T)] = (a, b, copies)
    m.close()
    if args.parent_lib:
        old = context(Backend(args.parent_lib, "tgx_", required=[n for n in ABI if n not in ("beam_select", "beam_advance")]), paged)
        for K in beams:
            for T in contexts:
                run = Emulation(old, K, T)
                for _ in range(3):
                    run.step()
                results[(form, K, T)] += ([run.step() for _ in range(args.reps)],)
        old.close()
for (form, K, T), r in results.items():
    a, b, copies = r[:3]
    line = (f"{desc.name} {args.dtype} {form:5s} K = {K} context {T:4d}: (a) tgx_decode_rows(1) {cell(a)}   (b) beam step {cell(b)}   (b) - (a) {np.median(b) - np.median(a):+.3f}"
            f"   rows copied per step {np.mean(copies):.1f}")
    if len(r) > 3:
        c = r[3]
        spread = max(max(b) - min(b), max(c) - min(c))
        gap = float(np.median(c) - np.median(b))
        verdict = "(b) BELOW (c) by more than the spread" if gap > spread else ("(b) ABOVE (c)" if gap < 0 else "(b) below (c) by LESS than the spread")
        line += f"   (c) emulation, parent library {cell(c)}   (c) - (b) {gap:+.3f}, spread {spread:.3f}: {verdict}"
    say(line)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    f.write("\n".join(lines) + "\n")
