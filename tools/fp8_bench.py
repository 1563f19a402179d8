#!/usr/bin/env python3
"""What a quantized-weights option (weights.fp8, weights.fp4) buys and what it costs, measured on one box: writes profiles/<option>.txt.

    python tools/fp8_bench.py [--option weights.fp8] [--base-opts KEY=V,...] [--parent-lib PATH] [--models llama-3.2-1b,mistral-7b-v0.3] [--rounds 3] [--out FILE]

--option is the option under test (set to 1 on this library; the labels below say fp8 for it).  --base-opts adds a second base context with those options set
(on the parent library when --parent-lib names it), e.g. --option weights.fp4 --base-opts weights.fp8=1: the FP4 step against the parent's FP8 step and
against its defaults, all contexts side by side and alternating.  --bpc 2,6,8 adds, per model, the step of the option under test at those workgroups per CU
of its three launches (options <class>.packed_bpc) beside the defaults, contexts alternating.

Per model (the bench.py point: a 2048-token prefill, 16 warm-up steps, 256 timed greedy steps; Mistral-7B is BASELINE.json config 3's geometry):
  * ms per step with the option under test (weights.fp8 in what follows) = 1 against the BASE context — the parent commit's library at its defaults when --parent-lib names it, else this library with
    the option off (the same launches and bits: a default context is unchanged) — as the median of the rounds' medians, with the spread of the rounds;
    the two contexts live side by side and take turns within every round, so clock drift hits both;
  * the per-class kernel times of tgx_profile_decode for both and the effective TB/s of the gate_up / down / lm_head launches (bytes the launch streams / time);
  * what the option does to the model: the largest and the RMS difference of the unrounded last-position logits against the base context over the timed
    steps (both contexts fed the BASE context's greedy ids, so every step compares the same position), and where the free-running greedy ids first differ.
The figures are reported, not asserted: synthetic weights say little about a trained model's quality.

    python tools/fp8_bench.py --rows [--parent-lib PATH]       # option weights.fp8_rows: writes profiles/weights_fp8_rows.txt
    python tools/fp8_bench.py --rows --option weights.fp4      # option weights.fp4_rows: writes profiles/weights_fp4_rows.txt

--rows: ms per tgx_decode_rows step at 4, 8, 16, 32 and 64 rows and ms per 16-position tgx_verify_row pass, Llama-3.2-1B bf16, every row at context --prompt;
base = weights.fp8 = 1 with weights.fp8_rows = 0 (the parent's launches; with --parent-lib the parent commit's library with weights.fp8 = 1 is timed beside it),
against weights.fp8_rows = 64 on the SAME context, the two settings alternating, median of the rounds' medians with the spread.  Same bits either way.
With --option weights.fp4 the context under test is weights.fp4 = 1 with weights.fp4_rows 0 / 64, and a third context, weights.fp8 = 1 with weights.fp8_rows 64,
takes its turn in every round."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth  # noqa: E402
from tinygpt_amd.ffi import ABI, GREEDY, Backend, Model, TgxError, product_backend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--option", default="weights.fp8", help="the option under test: weights.fp8 or weights.fp4")
ap.add_argument("--base-opts", default="", help="KEY=V,...: a second base context with these options")
ap.add_argument("--bpc", default="", help="N,...: also time the option under test at these workgroups per CU of gate_up / down / lm_head")
ap.add_argument("--parent-lib", default=None, help="the parent commit's libtgx_mi355x.so (default: this library with weights.fp8 = 0)")
ap.add_argument("--models", default="llama-3.2-1b,mistral-7b-v0.3")
ap.add_argument("--prompt", type=int, default=2048)
ap.add_argument("--warmup", type=int, default=16)
ap.add_argument("--steps", type=int, default=256)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3, help="timed regions per context and round (the round's figure is their median)")
ap.add_argument("--out", default=None)
ap.add_argument("--rows", action="store_true", help="measure option weights.fp8_rows instead (profiles/weights_fp8_rows.txt)")
args = ap.parse_args()
args.out = args.out or os.path.join(ROOT, "profiles", args.option.replace(".", "_") + "_rows.txt" if args.rows else args.option.replace(".", "_") + ".txt")
TAG = args.option.split(".")[-1]                                                            # fp8 / fp4: the label of the context under test
BASE_OPTS = [(kv.split("=")[0], int(kv.split("=")[1])) for kv in args.base_opts.split(",") if kv]

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(m, prompt):
    """one bench.py region: prefill, sample, warm-up, `steps` timed steps -> ms per step"""
    m.reset_cache()
    m.forward(prompt)
    m.sample(GREEDY)
    m.decode(args.warmup, GREEDY, fetch=False)
    m.synchronize()
    t0 = time.perf_counter()
    m.decode(args.steps, GREEDY, fetch=False)
    m.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.steps


def greedy_ids(m, prompt):
    m.reset_cache()
    m.forward(prompt)
    first = m.sample(GREEDY).copy()
    rest = m.decode(args.warmup + args.steps - 1, GREEDY)[:, 0]
    return np.concatenate([first, rest])


def get_or_0(m, key):
    try:
        return m.get_option(key)
    except TgxError:       # (a parent library that does not know the key)
        return 0


def class_table(m, d):
    """per-class kernel us per launch, and the stream bytes of the three weight launches of ONE layer / the head"""
    prof = m.profile_decode(8)
    H, I, V = d.hidden, d.inter, d.vocab
    packed = m.get_option("weights.packed_classes") if m.get_option("weights.packed") else 0
    q8 = m.get_option("weights.fp8_classes") if get_or_0(m, "weights.fp8") else 0
    q4 = m.get_option("weights.fp4_classes") if get_or_0(m, "weights.fp4") else 0
    weights = {"gateup": 2 * I * H, "down": H * I, "lmhead": V * H}
    out = {}
    for bit, cls in enumerate(("gateup", "down", "lmhead")):
        # (nominal: scales, escape records and padding left out — but 0.53125 is what an FP4 stream holds, scales included, wherever K % (512 ks) == 0)
        per_weight = 0.53125 if q4 >> bit & 1 else 1.0 if q8 >> bit & 1 else (1.5 if packed >> bit & 1 else 2.0)      # (nominal: scales, escape records and padding left out)
        n, ms = prof[cls]
        us = ms / n * 1e3 if n else float("nan")
        out[cls] = (us, weights[cls] * per_weight / (us * 1e-6) / 1e12 if n else float("nan"), per_weight)
    return prof, out


parent = Backend(args.parent_lib, "tgx_", required=list(ABI)) if args.parent_lib else None


def rows_bench():
    """option weights.fp8_rows / weights.fp4_rows (args.option + "_rows") on the batched step and a verify pass"""
    rows_key, other = args.option + "_rows", args.option == "weights.fp4"
    steps, ROWS = min(args.steps, 64), (4, 8, 16, 32, 64)
    d = known_desc("llama-3.2-1b", "bf16")
    d.max_ctx, d.max_batch = args.prompt + 256, max(ROWS)
    ctxs = {"this": Model(d, product_backend())}
    if parent:
        ctxs["parent"] = Model(d, parent)
    if other:
        ctxs["fp8"] = Model(d, product_backend())
    for key, m in ctxs.items():
        m.set_option("weights.fp8" if key == "fp8" else args.option, 1)
        for tname, bits in synth.synth_checkpoint(d, 1234, 0.02):
            m.upload(tname, bits)
        m.finalize()
    prompt = synth.synth_prompt(d.vocab, args.prompt, 1234)

    def step_ms(m, rows, fp8_rows):
        if fp8_rows is not None:
            m.set_option(rows_key, fp8_rows)
        m.reset_cache()
        for r in range(rows):
            m.forward_row(r, prompt)
            m.sample_row(r, GREEDY)
        m.decode_rows(args.warmup)
        m.synchronize()
        t0 = time.perf_counter()
        m.decode_rows(steps)
        m.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def verify_ms(m, rows, fp8_rows):
        """one 16-position pass (15 draft tokens; all rejected or not, the pass is the same work), timed over `steps` passes on a row kept at the prompt"""
        if fp8_rows is not None:
            m.set_option(rows_key, fp8_rows)
        ts = []
        for _ in range(8):
            m.reset_cache()
            m.forward_row(0, prompt)
            first = m.sample_row(0, GREEDY)
            m.synchronize()
            t0 = time.perf_counter()
            m.verify_row(0, [first] * 15)
            m.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts[1:])

    say(f"# option {rows_key}: batched steps and verify passes stream the {TAG.upper()} codes on the matrix cores (kernels/skinny_{TAG}.h) — tools/fp8_bench.py --rows" + (" --option weights.fp4" if other else ""))
    say(f"# Llama-3.2-1B bf16, every row at context {args.prompt}; {args.warmup} warm-up + {steps} timed tgx_decode_rows steps; {args.rounds} rounds, settings alternating; ms (spread of the rounds)")
    say(f"# base = {args.option} 1, {rows_key} 0 (the parent's launches); rows64 = {rows_key} 64; parent = the parent commit's library with {args.option} 1" + ("; fp8rows64 = weights.fp8 1, weights.fp8_rows 64" if other else ""))
    settings = [("base", "this", 0), ("rows64", "this", 64)] + ([("parent", "parent", None)] if parent else []) + ([("fp8rows64", "fp8", None)] if other else [])
    if other:
        ctxs["fp8"].set_option("weights.fp8_rows", 64)
    for what, fn, points in (("tgx_decode_rows step", step_ms, ROWS), ("16-position tgx_verify_row pass (host call included)", verify_ms, (1,))):
        for rows in points:
            for label, key, v in settings:
                fn(ctxs[key], rows, v)                          # untimed: workspaces, graphs
            got = {label: [] for label, _, _ in settings}
            for _ in range(args.rounds):
                for label, key, v in settings:
                    got[label].append(fn(ctxs[key], rows, v))
            med = {k: statistics.median(v) for k, v in got.items()}
            spread = max(max(v) - min(v) for v in got.values())
            verdict = "faster" if med["base"] - med["rows64"] > spread else ("SLOWER" if med["rows64"] - med["base"] > spread else "within the spread")
            say(f"{what}, {rows} rows: " + "   ".join(f"{k} {med[k]:.4f} ({max(got[k]) - min(got[k]):.4f})" for k in got) +
                f"   rows64 - base {med['rows64'] - med['base']:+.4f} ms = {100 * (med['rows64'] - med['base']) / med['base']:+.1f} %: {verdict}")
    m = ctxs["this"]
    say(f"code-stream products issued {m.get_option(rows_key[:-1] + '_products')}, fallbacks {m.get_option(rows_key[:-1] + '_fallbacks')}")
    say("per-launch us of gate_up / down / lm_head: not from this tool (tgx_profile_decode times the batch-1 step only); a kernel trace of its own")


if args.rows:
    rows_bench()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)
say(f"# option {args.option}: quantized gate_up / down / lm_head streams at batch 1 — tools/fp8_bench.py --option {args.option}" + (f" --base-opts {args.base_opts}" if BASE_OPTS else ""))
say(f"# base contexts: {'the parent commit library' if parent else 'this library'} at its defaults" + (f", and the same with {args.base_opts}" if BASE_OPTS else ""))
say(f"# point: {args.prompt}-token prefill, {args.warmup} warm-up steps, {args.steps} timed greedy steps; {args.rounds} rounds x {args.reps} regions per context, contexts alternating")
for name in args.models.split(","):
    d = known_desc(name, "bf16")
    d.max_ctx = min(d.max_ctx, 4096)
    ctx = {"base": Model(d, parent or product_backend())}
    if BASE_OPTS:
        ctx["base+" + args.base_opts] = Model(d, parent or product_backend())
        for k, v in BASE_OPTS:
            ctx["base+" + args.base_opts].set_option(k, v)
    ctx[TAG] = Model(d, product_backend())
    ctx[TAG].set_option(args.option, 1)
    base, q = ctx["base"], ctx[TAG]
    t0 = time.time()
    for tname, bits in synth.synth_checkpoint(d, 1234, 0.02):
        for m in ctx.values():
            m.upload(tname, bits)
    for m in ctx.values():
        m.finalize()
    say()
    say(f"## {name} bf16 ({d.param_count() / 1e9:.2f} B parameters; load + quantize {time.time() - t0:.0f} s)")
    T = args.prompt + args.warmup + args.steps // 2
    say(f"{TAG} streams {q.get_option(args.option + '_matrices')}, fallbacks {q.get_option(args.option + '_fallbacks')}; bytes per token at context {T}: " +
        ", ".join(f"{k} {m.bytes_per_token(T) / 1e6:.1f} MB" for k, m in ctx.items()))
    prompt = synth.synth_prompt(d.vocab, args.prompt, 1234)[None, :]
    for m in ctx.values():
        timed(m, prompt)                                    # untimed: workspaces, code objects, graphs
    rounds = {k: [] for k in ctx}
    for r in range(args.rounds):
        got = {k: [] for k in ctx}
        for _ in range(args.reps):
            for k, m in ctx.items():
                got[k].append(timed(m, prompt))
        for k in got:
            rounds[k].append(statistics.median(got[k]))
        say(f"round {r}: " + "   ".join(f"{k} {rounds[k][-1]:.4f} ms/step" for k in ctx))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    spread = {k: max(v) - min(v) for k, v in rounds.items()}
    say("ms per step, median of the rounds' medians (spread of the rounds): " + "   ".join(f"{k} {med[k]:.4f} ({spread[k]:.4f})" for k in ctx))
    for k in ctx:
        if k != TAG:
            mb, mq = med[k], med[TAG]
            say(f"{TAG} against {k}: difference {mb - mq:+.4f} ms = {100 * (mb - mq) / mb:+.1f} %   tok/s {1e3 / mb:.0f} -> {1e3 / mq:.0f}: " +
                ("faster by more than the spread" if mb - mq > max(spread[k], spread[TAG]) else "NOT faster by more than the spread"))
    for label, m in ctx.items():
        m.reset_cache(); m.forward(prompt); m.sample(GREEDY); m.decode(args.warmup, GREEDY, fetch=False)
        prof, cls = class_table(m, d)
        say(f"{label}: kernel us per launch  " + "  ".join(f"{k} {ms / n * 1e3:.2f}" for k, (n, ms) in prof.items() if n) +
            f"   sum per token {sum(ms for n, ms in prof.values()) / 8 * 1e3:.1f} us")
        say(f"{label}: effective TB/s  " + "  ".join(f"{k} {tb:.2f} (at {pw} B/weight)" for k, (us, tb, pw) in cls.items()))
    # the model: base's greedy ids fed to both contexts, the logits of every timed step compared
    ids_b, ids_q = greedy_ids(base, prompt), greedy_ids(q, prompt)
    differ = np.nonzero(ids_b != ids_q)[0]
    for m in (base, q):
        m.reset_cache(); m.forward(prompt)
    worst, sq_sum, count, ref_max = 0.0, 0.0, 0, 0.0
    for i in range(args.warmup + args.steps):
        tok = ids_b[i:i + 1][None, :]
        base.forward(tok); q.forward(tok)
        if i < args.warmup:
            continue
        lb, lq = base.logits(rounded=False).astype(np.float64), q.logits(rounded=False).astype(np.float64)
        worst = max(worst, float(np.abs(lb - lq).max())); sq_sum += float(((lb - lq) ** 2).sum()); count += lb.size
        ref_max = max(ref_max, float(np.abs(lb).max()))
    say(f"logits against the unquantized context over the {args.steps} timed steps (teacher-forced with its ids): largest |difference| {worst:.4g}, RMS {np.sqrt(sq_sum / count):.4g} "
        f"(largest |logit| {ref_max:.4g})")
    say(f"free-running greedy ids ({args.warmup + args.steps} tokens): " +
        ("all agree" if differ.size == 0 else f"first differ at token {int(differ[0])}, {int(differ.size)} of {ids_b.size} differ"))
    for m in ctx.values():
        m.close()
    if args.bpc:      # the option under test at other workgroups per CU of its three launches
        ctx = {"defaults": None, **{v: int(v) for v in args.bpc.split(",")}}
        for k, bpc in list(ctx.items()):
            ctx[k] = m = Model(d, product_backend())
            m.set_option(args.option, 1)
            for cls in ("gateup", "down", "lmhead"):
                if bpc:
                    m.set_option(cls + ".packed_bpc", bpc)
        for tname, bits in synth.synth_checkpoint(d, 1234, 0.02):
            for m in ctx.values():
                m.upload(tname, bits)
        rounds = {k: [] for k in ctx}
        for m in ctx.values():
            m.finalize(); timed(m, prompt)
        for r in range(args.rounds):
            for k, m in ctx.items():
                rounds[k].append(statistics.median(timed(m, prompt) for _ in range(args.reps)))
        say(f"{TAG} by workgroups per CU of gate_up / down / lm_head, ms per step, median of the rounds (spread): " +
            "   ".join(f"{k}: {statistics.median(v):.4f} ({max(v) - min(v):.4f})" for k, v in rounds.items()))
        for m in ctx.values():
            m.close()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
