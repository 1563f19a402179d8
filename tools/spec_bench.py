"""What tgx_verify_row costs and what it can return (profiles/verify_row.txt): Llama-3.2-1B bf16 synthetic at context ~2060 (the bench's region), unpaged and paged
cache in ONE process.  Every timed call starts from the same state — the 2048-token prompt prefilled, its first greedy token sampled — rebuilt before the call, so
the figures of one column differ only in the call; the cases are interleaved over the repeats and the medians are reported, with the spread (min .. max).

  per n_draft in {1, 3, 7, 15}:
    verify      tgx_verify_row of n_draft tokens (n_draft + 1 positions); drafts from a prior plain greedy run of the same prompt: all correct, the first wrong, the
                middle one wrong — and, untimed, a wrong token at each position, to check the produced count against the plain run
    extend      tgx_extend_row of the same n_draft + 1 positions: the pass alone (the parent commit's code) — the difference is the all-position lm_head + accept
    step        one plain tgx_decode step, synchronised like the two calls above; and the streamed rate of tgx_decode(64) for the project's headline figure
  derived: break-even accepted drafts = verify / step - 1; tokens/s at acceptance 0, half, full = (1, n_draft // 2 + 1, n_draft + 1) / verify
  free-running: the host engine, speculate 0 against 7 with prompt lookup on a prompt made of a repeated span, with the histogram of tokens per verify pass

usage: python tools/spec_bench.py [--reps 9] [--out profiles/verify_row.txt]

--sampler T,K,P,M (profiles/verify_sampled.txt): tgx_verify_row_sampled under that sampler instead.  Per pass at 4 / 8 / 16 positions, interleaved over the repeats:
the sampled verify (drafts from the row's own sampled run: all accepted, as far as the two paths agree), the greedy verify of the same build, one sampled and one
greedy tgx_decode_rows step of this build and — with --parent-lib, a libtgx_mi355x.so built from the parent commit, loaded beside this one — one sampled step of the
parent.  Then the host engine free-running with speculateSampled on the repetitive prompt: tokens per pass and acceptance.
usage: python tools/spec_bench.py --sampler 0.8,0,0.9,0 [--parent-lib PATH] [--reps 9] [--out profiles/verify_sampled.txt]

--rows B[,B..] (profiles/verify_rows.txt): tgx_verify_rows over B rows at context 2048 — 4 and 8 positions per row, greedy and T 0.8 / top-p 0.9, extend.attn_splits
0, -1, the split count min(32, 2 * 256 CUs / (B * heads)) of the automatic rule and 2 / 4 / 8 — against B sequential tgx_verify_row_sampled calls and one B-row tgx_decode_rows step
of the parent commit's library (--parent-lib; without it, of this build), and the accepted drafts per row from which the joint call beats plain stepping.
usage: python tools/spec_bench.py --rows 2,4,8 [--parent-lib PATH] [--reps 9] [--out profiles/verify_rows.txt]

--tree (profiles/verify_tree.txt): tgx_verify_tree at context 2048, greedy and T 0.8 / top-p 0.9.  COST: ms per tree pass at 4 / 8 / 16 positions (two branches
interleaved in index order, the second one right: the accepted path is non-contiguous and the compaction moves every accepted row) against tgx_verify_row_sampled
of the same number of positions on the parent commit's library (--parent-lib; without it, on this build) — the median of --reps calls, and beside it the spread of
the parent's own figure over three repeated medians.  ACCEPTANCE: the host engine free-running with speculate 7, speculateTree 0 against 3, on a text the tool
generates — a few phrases that share a stem and go on differently, in random order — tokens produced per verify pass, tree passes, ids against speculate 0.
usage: python tools/spec_bench.py --tree [--parent-lib PATH] [--reps 10] [--out profiles/verify_tree.txt]

--processors (profiles/verify_processed.txt): the verify calls on a row with logit processors on (option verify.processors), at context 2048.  COST: ms per
tgx_verify_row at 4 / 8 / 16 positions with a bias list, penalties and an automaton on the row, against the same build's call with no processor on and against one
tgx_decode_rows step of the processed row on the parent commit's library (--parent-lib; without it, on this build).  Three rounds of --reps interleaved calls:
the median over all of them, and beside it the spread of the three rounds' medians.  ACCEPTANCE: tgx_cli on a text a regular expression forces (the GPT-2
geometry with the GPT-2 tokenizer fixture, the one full tokenizer in the tree), --regex --speculate 8 --speculate-processed against --regex alone on the parent
commit's tgx_cli (--parent-cli; without it, this build's): tokens per verify pass and decode-only tokens per second.
usage: python tools/spec_bench.py --processors [--parent-lib PATH] [--parent-cli PATH] [--reps 9] [--out profiles/verify_processed.txt]"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import GREEDY, Model

S = 2048
NDRAFT = [1, 3, 7, 15]


def fresh(m, prompt):
    m.reset_cache()
    m.forward(prompt[None, :])
    return int(m.sample(GREEDY)[0])


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def med(xs):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


def measure(paged, reps, lines):
    d = known_desc("llama-3.2-1b", "bf16")
    d.max_batch = 1
    m = Model(d)
    if paged:
        m.set_option("kv.budget_tokens", 4096)
    m.load_synthetic(1234, 0.02).finalize()
    V = d.vocab
    prompt = synth.synth_prompt(V, S, 1234)
    t0 = fresh(m, prompt)
    ref = [int(t) for t in m.decode(40, GREEDY)[:, 0]]       # the plain greedy run: ref[i] follows t0, ref[0], ..
    wrong = lambda ids, j: [t if i != j else (t + 1) % V for i, t in enumerate(ids)]
    # ---- untimed: the produced count for a wrong token at each position (and none), against the plain run.  A count that differs is a step whose top-2 gap is
    # inside the band between the two kernel paths: it is reported, not hidden
    lines.append("cache: %s" % ("paged (kv.budget_tokens 4096)" if paged else "unpaged"))
    for n in NDRAFT:
        bad = []
        for j in list(range(n)) + [None]:
            assert fresh(m, prompt) == t0
            ids, fin = m.verify_row(0, wrong(ref[:n], j))
            want = n + 1 if j is None else j + 1
            if len(ids) != want or list(ids[:want - 1]) != ref[:want - 1]:
                bad.append((j, len(ids)))
        lines.append("  n_draft %2d: produced count == index of the wrong token + 1 at every position and n_draft + 1 with none wrong: %s" % (n, "yes" if not bad else "NO %s" % bad))
    # ---- timed
    tv = {(n, k): [] for n in NDRAFT for k in ("all", "first", "mid")}
    te = {n: [] for n in NDRAFT}
    ts, tstream = [], []
    for rep in range(reps + 2):                                # two warm-up rounds (workspaces, graphs), discarded
        keep = rep >= 2
        for n in NDRAFT:
            for k, j in (("all", None), ("first", 0), ("mid", n // 2)):
                fresh(m, prompt)
                ms, _ = timed(lambda: m.verify_row(0, wrong(ref[:n], j)))
                if keep:
                    tv[(n, k)].append(ms)
            fresh(m, prompt)
            ms, _ = timed(lambda: m.extend_row(0, [t0] + ref[:n]))
            if keep:
                te[n].append(ms)
        fresh(m, prompt)
        ms, _ = timed(lambda: m.decode(1, GREEDY))
        if keep:
            ts.append(ms)
        fresh(m, prompt)
        ms, _ = timed(lambda: m.decode(64, GREEDY))
        if keep:
            tstream.append(ms / 64)
    step = statistics.median(ts)
    lines.append("  one plain step, synchronised        ms: %s" % med(ts))
    lines.append("  plain steps, streamed (64 per call) ms/token: %s   -> %.0f tok/s" % (med(tstream), 1e3 / statistics.median(tstream)))
    lines.append("  n_draft | verify ms: all correct / first wrong / middle wrong (medians) | extend ms | verify - extend | break-even accepted | tok/s at acceptance 0 / half / full | plain tok/s sync / streamed")
    for n in NDRAFT:
        v = statistics.median(tv[(n, "all")] + tv[(n, "first")] + tv[(n, "mid")])
        e = statistics.median(te[n])
        lines.append("  %7d | %.3f / %.3f / %.3f | %s | %+.3f | %.2f | %.0f / %.0f / %.0f | %.0f / %.0f" % (
            n, statistics.median(tv[(n, "all")]), statistics.median(tv[(n, "first")]), statistics.median(tv[(n, "mid")]), med(te[n]), v - e, v / step - 1,
            1e3 / v, 1e3 * (n // 2 + 1) / v, 1e3 * (n + 1) / v, 1e3 / step, 1e3 / statistics.median(tstream)))
    out = {n: statistics.median(tv[(n, "all")]) for n in NDRAFT}
    m.close()
    return out, step, statistics.median(tstream)


def free_running(lines):
    from ctypes import POINTER, c_int, c_int64, c_void_p
    from host_util import HostEngine, host_lib
    lib = host_lib()
    lib.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    lib.tgxe_spec_stats.restype = c_int
    lib.tgxe_spec_stats.argtypes = [c_void_p, POINTER(c_int64), c_int]
    e = HostEngine(lib, synthetic="llama-3.2-1b", device="mi355x", dtype=1, max_batch=1)
    assert e.prepare(), e.error()
    span = synth.synth_prompt(128256, 64, 99).astype(np.int32)
    prompt = np.tile(span, S // 64)                            # 2048 tokens: one 64-token span, repeated
    n_new = 256
    res = {}
    for rep in range(3):
        for spec in (0, 7):
            lib.tgxe_set_speculate(e.h, spec)
            e.reconfigure(max_new=n_new)
            t = time.perf_counter()
            ids, new, fin = e.generate_sync([prompt])
            res.setdefault(spec, []).append(((time.perf_counter() - t) * 1e3, ids[0, len(prompt):].tolist()))
    buf = (c_int64 * 32)()
    lib.tgxe_spec_stats(e.h, buf, 32)
    st = list(buf[:21])
    same = res[0][0][1] == res[7][0][1]
    first_diff = next((i for i, (a, b) in enumerate(zip(res[0][0][1], res[7][0][1])) if a != b), None)
    lines.append("free-running generateSync, %d new tokens after a %d-token prompt (a 64-token span repeated), unpaged, whole call incl. prefill, ms: speculate 0 %s | speculate 7 %s" % (
        n_new, med([r[0] for r in res[0]]), med([r[0] for r in res[7]])))
    lines.append("  ids equal: %s%s" % ("yes" if same else "no", "" if same else " (first difference at new token %d: a step whose top-2 gap is inside the band between the kernel paths)" % first_diff))
    lines.append("  over the 3 speculate-7 runs: %d verify passes, %d of %d draft tokens accepted, %d ordinary steps; tokens produced per verify pass 1..16: %s" % (st[0], st[2], st[1], st[3], st[5:21]))
    e.close()


def measure_sampled(cfg, reps, lines, parent_lib):
    from tinygpt_amd.ffi import ABI, Backend, SamplerCfg
    d = known_desc("llama-3.2-1b", "bf16")
    d.max_batch = 1
    seed = 7
    m = Model(d).load_synthetic(1234, 0.02).finalize()
    old = None
    if parent_lib:      # the parent commit's library beside this one: every symbol it has (it lacks the new ones)
        old = Model(d, backend=Backend(parent_lib, "tgx_", required=[n for n in ABI if n not in ("verify_row_sampled", "read_pass_logits")])).load_synthetic(1234, 0.02).finalize()
    V = d.vocab
    prompt = synth.synth_prompt(V, S, 1234)

    def fresh_row(mm, c):
        mm.reset_cache()
        mm.forward_row(0, prompt)
        mm.set_row_sampler(0, c, seed)
        return int(mm.sample_row(0, c, seed))

    fresh_row(m, cfg)
    ref_s = [int(t) for t in m.decode_rows(16)[0][:, 0]]       # the row's own sampled run
    fresh_row(m, GREEDY)
    ref_g = [int(t) for t in m.decode_rows(16)[0][:, 0]]
    lines.append("sampler: T %g top-k %d top-p %g min-p %g, row seed %d; unpaged; ms per call, synchronised: median (min .. max) over %d interleaved repeats" % (
        cfg.temperature, cfg.top_k, cfg.top_p, cfg.min_p, seed, reps))
    ND = [3, 7, 15]
    tv = {(n, k): [] for n in ND for k in ("sampled", "greedy")}
    acc = {n: [] for n in ND}
    ts = {k: [] for k in ("step sampled", "step greedy", "parent step sampled")}
    for rep in range(reps + 2):                                # two warm-up rounds, discarded
        keep = rep >= 2
        for n in ND:
            fresh_row(m, cfg)
            ms, r = timed(lambda: m.verify_row_sampled(0, ref_s[:n]))
            if keep:
                tv[(n, "sampled")].append(ms); acc[n].append(len(r[0]))
            fresh_row(m, GREEDY)
            ms, _ = timed(lambda: m.verify_row(0, ref_g[:n]))
            if keep:
                tv[(n, "greedy")].append(ms)
        for k, mm, c in (("step sampled", m, cfg), ("parent step sampled", old, cfg), ("step greedy", m, GREEDY)):      # A / B side by side
            if mm is None:
                continue
            fresh_row(mm, c)
            ms, _ = timed(lambda: mm.decode_rows(1))
            if keep:
                ts[k].append(ms)
    for k in ts:
        if ts[k]:
            lines.append("  one tgx_decode_rows step, %-20s %s" % (k + ":", med(ts[k])))
    chain = statistics.median(ts["step sampled"]) - statistics.median(ts["step greedy"])
    lines.append("  one row's sampler chain (sampled step - greedy step, this build): %+.3f ms" % chain)
    lines.append("  positions | sampled verify | greedy verify | surcharge | surcharge / one row's chain | sampled verify / parent's sampled step | tokens produced by the all-right draft (median)")
    base = statistics.median(ts["parent step sampled"] or ts["step sampled"])
    for n in ND:
        a_, g_ = statistics.median(tv[(n, "sampled")]), statistics.median(tv[(n, "greedy")])
        lines.append("  %9d | %s | %s | %+.3f | %.2f | %.2f | %d of %d" % (n + 1, med(tv[(n, "sampled")]), med(tv[(n, "greedy")]), a_ - g_, (a_ - g_) / chain if chain > 0 else float("nan"),
                                                                  a_ / base, statistics.median(acc[n]), n + 1))
    m.close()
    if old is not None:
        old.close()


def free_running_sampled(cfg, lines):
    from ctypes import POINTER, c_int, c_int64, c_void_p
    from host_util import HostEngine, host_lib
    lib = host_lib()
    lib.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    lib.tgxe_set_speculate_sampled.argtypes = [c_void_p, c_int]
    lib.tgxe_spec_stats.restype = c_int
    lib.tgxe_spec_stats.argtypes = [c_void_p, POINTER(c_int64), c_int]
    e = HostEngine(lib, synthetic="llama-3.2-1b", device="mi355x", dtype=1, max_batch=1)
    assert e.prepare(), e.error()
    span = synth.synth_prompt(128256, 64, 99).astype(np.int32)
    prompt = np.tile(span, S // 64)
    n_new = 256
    res = {}
    for rep in range(3):
        for on in (0, 1):
            lib.tgxe_set_speculate(e.h, 7)
            lib.tgxe_set_speculate_sampled(e.h, on)
            e.reconfigure(temperature=cfg.temperature, top_k=cfg.top_k, top_p=cfg.top_p, min_p=cfg.min_p, max_new=n_new)
            t = time.perf_counter()
            ids, new, fin = e.generate_sync([prompt])
            res.setdefault(on, []).append(((time.perf_counter() - t) * 1e3, ids[0, len(prompt):].tolist()))
    buf = (c_int64 * 32)()
    lib.tgxe_spec_stats(e.h, buf, 32)
    st = list(buf[:21])
    first_diff = next((i for i, (a, b) in enumerate(zip(res[0][0][1], res[1][0][1])) if a != b), None)
    lines.append("free-running generateSync under that sampler, speculate 7, %d new tokens after a %d-token prompt (a 64-token span repeated), whole call incl. prefill, ms: speculateSampled off %s | on %s" % (
        n_new, len(prompt), med([r[0] for r in res[0]]), med([r[0] for r in res[1]])))
    lines.append("  ids equal: %s" % ("yes" if first_diff is None else "up to new token %d (a draw inside the band between the kernel paths)" % first_diff))
    passes = max(st[0], 1)
    lines.append("  over the 3 runs with it on: %d verify passes, %d of %d draft tokens accepted (%.0f %%), %d ordinary steps; %.2f tokens per pass; tokens produced per verify pass 1..16: %s" % (
        st[0], st[2], st[1], 100.0 * st[2] / max(st[1], 1), st[3], (st[2] + st[0]) / passes, st[5:21]))
    e.close()


def measure_rows(B_list, reps, lines, parent_lib):
    """--rows (profiles/verify_rows.txt): ms per tgx_verify_rows call over B rows at context 2048, 4 and 8 positions per row, greedy and T 0.8 / top-p 0.9, with
    extend.attn_splits 0, -1 and the split counts the automatic rule would pick; against B sequential tgx_verify_row_sampled calls and one B-row tgx_decode_rows
    step — both of the parent commit's library with --parent-lib, else of this build.  Derived: the mean number of accepted draft tokens per row from which the
    joint call beats plain stepping = joint / step - 1."""
    from tinygpt_amd.ffi import ABI, Backend, SamplerCfg
    Bmax = max(B_list)
    d = known_desc("llama-3.2-1b", "bf16")
    d.max_batch, d.max_ctx = Bmax, S + 64
    new = ("verify_rows",)
    m = Model(d).load_synthetic(1234, 0.02).finalize()
    old = Model(d, backend=Backend(parent_lib, "tgx_", required=[n for n in ABI if n not in new])).load_synthetic(1234, 0.02).finalize() if parent_lib else m
    V = d.vocab
    prompts = [synth.synth_prompt(V, S, 1234 + r) for r in range(Bmax)]
    samplers = {"greedy": GREEDY, "T 0.8 / top-p 0.9": SamplerCfg(0.8, 0, 0.9, 0.0)}
    cus = 256

    def fresh_rows(mm, B, c):
        mm.reset_cache()
        mm.forward_rows(range(B), prompts[:B])
        for r in range(B):
            mm.set_row_sampler(r, c, 7 + r)
        return [int(mm.sample_row(r, c, 7 + r)) for r in range(B)]

    lines.append("baselines from: %s; ms per call, synchronised: median (min .. max) over %d interleaved repeats" % ("the parent commit's library" if parent_lib else "this build (no --parent-lib)", reps))
    lines.append("  B | positions/row | sampler | one B-row step | B one-row verify calls | joint, splits 0 | joint, splits -1 (what the rule picks) | joint at explicit split counts | joint(-1) / sequential | break-even accepted drafts per row (joint(-1) / step - 1) | form")
    for B in B_list:
        ns_rule = min(32, 2 * cus // (B * d.heads))
        for P in (4, 8):
            n = P - 1
            for sname, c in samplers.items():
                fresh_rows(m, B, c)
                ref = m.decode_rows(n)[0]                       # every row's own continuation: all accepted, as far as the paths agree
                drafts = [[int(t) for t in ref[:, r]] for r in range(B)]
                variants = [("0", 0), ("-1", -1)] + [(str(k), k) for k in sorted({2, 4, 8} | ({ns_rule} if ns_rule >= 2 else set()))]
                t = {k: [] for k in ["step", "seq"] + [v[0] for v in variants]}
                form = picked = 0
                for rep in range(reps + 2):                     # two warm-up rounds, discarded
                    keep = rep >= 2
                    fresh_rows(old, B, c)
                    ms, _ = timed(lambda: old.decode_rows(1))
                    if keep:
                        t["step"].append(ms)
                    fresh_rows(old, B, c)
                    ms, _ = timed(lambda: [old.verify_row_sampled(r, drafts[r]) for r in range(B)])
                    if keep:
                        t["seq"].append(ms)
                    for k, ns in variants:
                        m.set_option("extend.attn_splits", ns)
                        fresh_rows(m, B, c)
                        ms, _ = timed(lambda: m.verify_rows(range(B), drafts))
                        form = m.get_option("verify.last_form")
                        if k == "-1":
                            picked = m.get_option("verify.last_splits")
                        if keep:
                            t[k].append(ms)
                    m.set_option("extend.attn_splits", -1)
                step, seq, auto = statistics.median(t["step"]), statistics.median(t["seq"]), statistics.median(t["-1"])
                lines.append("  %d | %d | %s | %s | %s | %s | %s | %s | %.2f | %.2f | %d" % (
                    B, P, sname, med(t["step"]), med(t["seq"]), med(t["0"]), "%s (%s)" % (med(t["-1"]), picked or "unsplit"),
                    "; ".join("%s: %.3f" % (k, statistics.median(t[k])) for k, _ in variants[2:]),
                    auto / seq, auto / step - 1, form))
    m.close()
    if old is not m:
        old.close()


def measure_tree(reps, lines, parent_lib):
    from tinygpt_amd.ffi import ABI, Backend, SamplerCfg
    d = known_desc("llama-3.2-1b", "bf16")
    d.max_batch = 1
    seed = 7
    m = Model(d).load_synthetic(1234, 0.02).finalize()
    old = Model(d, backend=Backend(parent_lib, "tgx_", required=[n for n in ABI if n != "verify_tree"])).load_synthetic(1234, 0.02).finalize() if parent_lib else m
    V = d.vocab
    prompt = synth.synth_prompt(V, S, 1234)

    def fresh_row(mm, c):
        mm.reset_cache()
        mm.forward_row(0, prompt)
        mm.set_row_sampler(0, c, seed)
        return int(mm.sample_row(0, c, seed))

    lines.append("COST.  chain baseline from: %s; ms per call, synchronised; median (min .. max) of %d calls, the cases interleaved; the parent's figure three times over" % (
        "the parent commit's library" if parent_lib else "this build (no --parent-lib)", reps))
    lines.append("  sampler | positions | tree pass (this build) | chain pass tgx_verify_row_sampled (parent): three medians | spread of the parent's medians | tree - parent's middle median | tokens the tree pass produced")
    for sname, c in (("greedy", GREEDY), ("T 0.8 / top-p 0.9", SamplerCfg(0.8, 0, 0.9, 0.0))):
        fresh_row(m, c)
        ref = [int(t) for t in m.decode_rows(16)[0][:, 0]]     # the row's own run
        for P in (4, 8, 16):
            n = P - 1
            parent = [-1, -1] + list(range(n - 2))             # two branches interleaved in index order
            depth = [1, 1] + [0] * (n - 2)
            for i in range(2, n):
                depth[i] = depth[parent[i]] + 1
            # the second branch (odd nodes) carries the row's own continuation, the first one tokens it will not produce
            tokens = [ref[depth[i] - 1] if i % 2 == 1 else (ref[depth[i] - 1] + 1) % V for i in range(n)]
            tt, tp, got = [], [[], [], []], []
            for rep in range(reps + 2):                        # two warm-up rounds, discarded
                keep = rep >= 2
                fresh_row(m, c)
                ms, r = timed(lambda: m.verify_tree(0, tokens, parent))
                if keep:
                    tt.append(ms); got.append(len(r[0]))
                for k in range(3):
                    fresh_row(old, c)
                    ms, _ = timed(lambda: old.verify_row_sampled(0, ref[:n]))
                    if keep:
                        tp[k].append(ms)
            meds = sorted(statistics.median(x) for x in tp)
            lines.append("  %s | %d | %s | %.3f  %.3f  %.3f | %.3f | %+.3f | %d of at most %d" % (
                sname, P, med(tt), meds[0], meds[1], meds[2], meds[2] - meds[0], statistics.median(tt) - meds[1], statistics.median(got), n // 2 + 1))
    m.close()
    if old is not m:
        old.close()


def free_running_tree(lines):
    from ctypes import POINTER, c_int, c_int64, c_void_p
    from host_util import HostEngine, host_lib
    lib = host_lib()
    lib.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    lib.tgxe_set_speculate_sampled.argtypes = [c_void_p, c_int]
    lib.tgxe_set_speculate_tree.argtypes = [c_void_p, c_int]
    lib.tgxe_spec_tree_passes.restype = c_int64
    lib.tgxe_spec_tree_passes.argtypes = [c_void_p]
    lib.tgxe_spec_stats.restype = c_int
    lib.tgxe_spec_stats.argtypes = [c_void_p, POINTER(c_int64), c_int]
    # the text: four phrases of 16 tokens that share a 4-token stem and go on differently, 128 of them in random order — the tail of the text has been continued
    # in several ways before, which is where a tree can hold what a chain cannot
    rng = np.random.default_rng(99)
    stem = synth.synth_prompt(128256, 4, 98).astype(np.int32)
    phrases = [np.concatenate([stem, synth.synth_prompt(128256, 12, 100 + k).astype(np.int32)]) for k in range(4)]
    prompt = np.concatenate([phrases[int(k)] for k in rng.integers(0, 4, S // 16)])
    n_new = 256
    lines.append("ACCEPTANCE.  free-running generateSync, speculate 7, %d new tokens after a %d-token prompt (four 16-token phrases sharing a 4-token stem, in random order), unpaged" % (n_new, len(prompt)))
    for sname, sampler in (("greedy", {}), ("T 0.8 / top-p 0.9", dict(temperature=0.8, top_p=0.9))):
        res = {}
        for branches in (None, 0, 3):                          # None: speculate 0, the ids to compare against
            e = HostEngine(lib, synthetic="llama-3.2-1b", device="mi355x", dtype=1, max_batch=1)      # a fresh engine per variant: its statistics count from zero
            assert e.prepare(), e.error()
            lib.tgxe_set_speculate(e.h, 0 if branches is None else 7)
            lib.tgxe_set_speculate_sampled(e.h, 1 if sampler else 0)
            lib.tgxe_set_speculate_tree(e.h, branches or 0)
            times = []
            for rep in range(3):
                e.reconfigure(max_new=n_new, **sampler)
                t = time.perf_counter()
                ids, new, fin = e.generate_sync([prompt])
                times.append((time.perf_counter() - t) * 1e3)
            buf = (c_int64 * 32)()
            lib.tgxe_spec_stats(e.h, buf, 32)
            res[branches] = (times, ids[0, len(prompt):].tolist(), list(buf[:21]), int(lib.tgxe_spec_tree_passes(e.h)))
            e.close()
        for branches in (0, 3):
            times, ids, st, trees = res[branches]
            first_diff = next((i for i, (a, b) in enumerate(zip(res[None][1], ids)) if a != b), None)
            lines.append("  %s | %s | whole call incl. prefill ms %s (speculate 0: %s) | over 3 runs: %d verify passes (%d of them trees), %d of %d draft tokens accepted, %d ordinary steps | %.3f tokens produced per verify pass | produced per pass 1..16: %s | ids equal to speculate 0: %s" % (
                sname, "tree, 3 branches" if branches else "chain", med(times), med(res[None][0]), st[0], trees, st[2], st[1], st[3], (st[2] + st[0]) / max(st[0], 1), st[5:21],
                "yes" if first_diff is None else "up to new token %d" % first_diff))


def measure_processed(reps, lines, parent_lib):
    from tinygpt_amd.ffi import ABI, Backend
    d = known_desc("llama-3.2-1b", "bf16")
    d.max_batch = 1
    m = Model(d).load_synthetic(1234, 0.02).finalize()
    m.set_option("verify.processors", 1)
    old = Model(d, backend=Backend(parent_lib, "tgx_", required=list(ABI))).load_synthetic(1234, 0.02).finalize() if parent_lib else None
    V = d.vocab
    prompt = synth.synth_prompt(V, S, 1234)
    rng = np.random.default_rng(5)
    bias = {int(t): float(v) for t, v in zip(rng.choice(V, size=64, replace=False), rng.uniform(-2, 2, size=64))}
    table = np.full((4, V), 0xFFFF, np.uint16)      # four states, each allowing two thirds of the vocabulary
    for s_ in range(4):
        ok = (np.arange(V) + s_) % 3 != 0
        table[s_, ok] = (s_ + 1) % 4
    aid = {id(mm): mm.automaton_create(table, start=0) for mm in (m, old) if mm is not None}

    def fresh_row(mm, processed):
        mm.reset_cache()
        mm.forward_row(0, prompt)
        if processed:
            mm.set_row_penalties(0, 1.1, 0.1, 0.1).set_row_logit_bias(0, bias).set_row_history(0, prompt_ids=prompt)
            mm.set_row_automaton(0, aid[id(mm)], 0)
        mm.set_row_sampler(0, GREEDY, 0)
        return int(mm.sample_row(0, GREEDY, 0))

    fresh_row(m, True)
    ref_p = [int(t) for t in m.decode_rows(16)[0][:, 0]]       # the processed row's own run: the all-right draft
    fresh_row(m, False)
    ref_u = [int(t) for t in m.decode_rows(16)[0][:, 0]]
    ND, ROUNDS = [3, 7, 15], 3
    lines.append("the row: a bias list of 64 ids, penalties (repetition 1.1, presence 0.1, frequency 0.1) over a history seeded from the prompt, an automaton of 4 states that each "
                 "allow two thirds of the vocabulary; greedy; unpaged")
    lines.append("ms per call, synchronised: median over %d rounds x %d interleaved repeats (min .. max) [the rounds' medians: min .. max]" % (ROUNDS, reps))
    keys = [(n, k) for n in ND for k in ("processed", "plain")] + ["step processed", "parent step processed", "step plain"]
    t = {k: [[] for _ in range(ROUNDS)] for k in keys}
    acc = {n: [] for n in ND}
    for rnd in range(ROUNDS):
        for rep_ in range(reps + (2 if rnd == 0 else 0)):          # two warm-up repeats, discarded
            keep = rnd > 0 or rep_ >= 2
            for n in ND:
                fresh_row(m, True)
                ms, r = timed(lambda: m.verify_row(0, ref_p[:n]))
                if keep:
                    t[(n, "processed")][rnd].append(ms); acc[n].append(len(r[0]))
                fresh_row(m, False)
                ms, _ = timed(lambda: m.verify_row(0, ref_u[:n]))
                if keep:
                    t[(n, "plain")][rnd].append(ms)
            for k, mm, processed in (("step processed", m, True), ("parent step processed", old, True), ("step plain", m, False)):
                if mm is None:
                    continue
                fresh_row(mm, processed)
                ms, _ = timed(lambda: mm.decode_rows(1))
                if keep:
                    t[k][rnd].append(ms)

    def fig(k):
        flat = [x for r in t[k] for x in r]
        meds = [statistics.median(r) for r in t[k]]
        return "%s [%.3f .. %.3f]" % (med(flat), min(meds), max(meds))

    def mid(k):
        return statistics.median([x for r in t[k] for x in r])
    for k in ("step plain", "step processed", "parent step processed"):
        if t[k][0]:
            lines.append("  one tgx_decode_rows step, %-22s %s" % (k + ":", fig(k)))
    base_k = "parent step processed" if old is not None else "step processed"
    lines.append("  positions | verify, processors on | verify, no processor (this build) | surcharge | processed verify / %s | break-even accepted drafts | tokens produced by the all-right draft (median)" % base_k)
    for n in ND:
        a_, g_ = mid((n, "processed")), mid((n, "plain"))
        lines.append("  %9d | %s | %s | %+.3f | %.2f | %.2f | %d of %d" % (n + 1, fig((n, "processed")), fig((n, "plain")), a_ - g_, a_ / mid(base_k), a_ / mid(base_k) - 1,
                                                                    statistics.median(acc[n]), n + 1))
    m.close()
    if old is not None:
        old.close()


def free_running_processed(lines, parent_cli):
    import re
    from tinygpt_amd import build
    from constraint_util import GPT2_DIR
    _, cli = build.build_host()
    pattern = r'(\{"answer": "(yes|no)", "sure": (true|false)\}, )+'
    prompt = 'Answers: {"answer": "yes", "sure": true}, {"answer": "no", "sure": false}, '
    n_new = 192
    base = ["--synthetic", "gpt2", "--tokenizer", GPT2_DIR, "--prompt", prompt, "--regex", pattern, "--stop-ids", "50256", "--max-tokens", str(n_new), "--temperature", "0", "--top-p", "1"]
    runs = {"regex alone (%s)" % ("the parent commit's tgx_cli" if parent_cli else "this build's tgx_cli"): [parent_cli or cli] + base,
            "regex, speculate 8 (no flag)": [cli] + base + ["--speculate", "8"],
            "regex, speculate 8, speculate-processed": [cli] + base + ["--speculate", "8", "--speculate-processed"]}
    lines.append("free-running tgx_cli, GPT-2 geometry (synthetic weights) with the GPT-2 tokenizer, greedy, %d new tokens, pattern %s" % (n_new, pattern))
    outs = {}
    for name, cmd in runs.items():
        rates, stat, text = [], "", ""
        for _ in range(3):
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                lines.append("  %s: FAILED: %s" % (name, r.stderr.strip()[-200:]))
                break
            rates.append(float(re.search(r"decode-only rate: ([0-9.]+) token/s", r.stdout).group(1)))
            sp = [l for l in r.stdout.splitlines() if l.startswith("speculate:")]
            stat = sp[0] if sp else ""
            text = next((l for l in r.stdout.splitlines() if l.startswith("Output:")), "")
        if not rates:
            continue
        outs[name] = text
        line = "  %-45s decode-only tokens/s over 3 runs: %s" % (name + ":", med(rates))
        mt = re.search(r"speculate: (\d+) verify passes, (\d+) of (\d+) draft tokens accepted, (\d+) ordinary steps", stat)
        if mt:
            p_, a_, dt, st = (int(x) for x in mt.groups())
            line += " | %d verify passes, %d of %d draft tokens accepted, %d ordinary steps" % (p_, a_, dt, st)
            if p_:
                line += ", %.2f tokens per pass" % ((a_ + p_) / p_)
        lines.append(line)
    lines.append("  the three outputs are the same text: %s" % ("yes" if len(set(outs.values())) == 1 and len(outs) == 3 else "NO"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    ap.add_argument("--rows", default="", help="B[,B..]: measure tgx_verify_rows over B rows instead (profiles/verify_rows.txt), e.g. --rows 2,4,8")
    ap.add_argument("--sampler", default="", help="T,K,P,M: measure tgx_verify_row_sampled under this sampler instead")
    ap.add_argument("--tree", action="store_true", help="measure tgx_verify_tree instead (profiles/verify_tree.txt)")
    ap.add_argument("--parent-lib", default="", help="with --sampler / --rows: a libtgx_mi355x.so of the parent commit, for the A/B baselines")
    ap.add_argument("--processors", action="store_true", help="measure the verify calls on a processed row instead (profiles/verify_processed.txt)")
    ap.add_argument("--parent-cli", default="", help="with --processors: the parent commit's tgx_cli (beside its libraries), for the regex-alone baseline")
    a = ap.parse_args()
    if a.processors:
        import torch
        lines = ["tools/spec_bench.py --processors --reps %d%s%s   device: %s   Llama-3.2-1B bf16 synthetic, prompt %d tokens" % (
            a.reps, " --parent-lib <parent build>" if a.parent_lib else "", " --parent-cli <parent build>" if a.parent_cli else "", torch.cuda.get_device_name(0), S)]
        measure_processed(a.reps, lines, a.parent_lib)
        free_running_processed(lines, a.parent_cli)
        text = "\n".join(lines) + "\n"
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
    if a.tree:
        import torch
        lines = ["tools/spec_bench.py --tree --reps %d%s   device: %s   Llama-3.2-1B bf16 synthetic, prompt %d tokens, unpaged" % (
            a.reps, " --parent-lib <parent build>" if a.parent_lib else "", torch.cuda.get_device_name(0), S)]
        measure_tree(a.reps, lines, a.parent_lib)
        free_running_tree(lines)
        text = "\n".join(lines) + "\n"
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
    if a.rows:
        import torch
        lines = ["tools/spec_bench.py --rows %s --reps %d%s   device: %s   Llama-3.2-1B bf16 synthetic, %d-token prompts, unpaged" % (
            a.rows, a.reps, " --parent-lib <parent build>" if a.parent_lib else "", torch.cuda.get_device_name(0), S)]
        measure_rows([int(b) for b in a.rows.split(",")], a.reps, lines, a.parent_lib)
        text = "\n".join(lines) + "\n"
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
    if a.sampler:
        import torch
        from tinygpt_amd.ffi import SamplerCfg
        T, K, P, M = a.sampler.split(",")
        cfg = SamplerCfg(float(T), int(K), float(P), float(M))
        lines = ["tools/spec_bench.py --sampler %s --reps %d%s   device: %s   Llama-3.2-1B bf16 synthetic, prompt %d tokens" % (
            a.sampler, a.reps, " --parent-lib <parent build>" if a.parent_lib else "", torch.cuda.get_device_name(0), S)]
        measure_sampled(cfg, a.reps, lines, a.parent_lib)
        free_running_sampled(cfg, lines)
        text = "\n".join(lines) + "\n"
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "working tree"
    except OSError:
        commit = "working tree"
    import torch
    lines = ["tools/spec_bench.py --reps %d   device: %s   commit: %s (+ this change)   Llama-3.2-1B bf16 synthetic, prompt %d tokens" % (a.reps, torch.cuda.get_device_name(0), commit, S)]
    for paged in (0, 1):
        measure(paged, a.reps, lines)
    free_running(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
