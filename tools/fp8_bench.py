#!/usr/bin/env python3
"""What option weights.fp8 buys and what it costs, measured on one box: writes profiles/weights_fp8.txt.

    python tools/fp8_bench.py [--parent-lib PATH] [--models llama-3.2-1b,mistral-7b-v0.3] [--rounds 3] [--out profiles/weights_fp8.txt]

Per model (the bench.py point: a 2048-token prefill, 16 warm-up steps, 256 timed greedy steps; Mistral-7B is BASELINE.json config 3's geometry):
  * ms per step with weights.fp8 = 1 against the BASE context — the parent commit's library at its defaults when --parent-lib names it, else this library with
    the option off (the same launches and bits: a default context is unchanged) — as the median of the rounds' medians, with the spread of the rounds;
    the two contexts live side by side and take turns within every round, so clock drift hits both;
  * the per-class kernel times of tgx_profile_decode for both and the effective TB/s of the gate_up / down / lm_head launches (bytes the launch streams / time);
  * what the option does to the model: the largest and the RMS difference of the unrounded last-position logits against the base context over the timed
    steps (both contexts fed the BASE context's greedy ids, so every step compares the same position), and where the free-running greedy ids first differ.
The figures are reported, not asserted: synthetic weights say little about a trained model's quality."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth  # noqa: E402
from tinygpt_amd.ffi import ABI, GREEDY, Backend, Model, product_backend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None, help="the parent commit's libtgx_mi355x.so (default: this library with weights.fp8 = 0)")
ap.add_argument("--models", default="llama-3.2-1b,mistral-7b-v0.3")
ap.add_argument("--prompt", type=int, default=2048)
ap.add_argument("--warmup", type=int, default=16)
ap.add_argument("--steps", type=int, default=256)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3, help="timed regions per context and round (the round's figure is their median)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weights_fp8.txt"))
args = ap.parse_args()

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


def class_table(m, d, fp8):
    """per-class kernel us per launch, and the stream bytes of the three weight launches of ONE layer / the head"""
    prof = m.profile_decode(8)
    H, I, V = d.hidden, d.inter, d.vocab
    packed = m.get_option("weights.packed_classes") if m.get_option("weights.packed") else 0
    q8 = m.get_option("weights.fp8_classes") if fp8 else 0
    weights = {"gateup": 2 * I * H, "down": H * I, "lmhead": V * H}
    out = {}
    for bit, cls in enumerate(("gateup", "down", "lmhead")):
        per_weight = 1.0 if q8 >> bit & 1 else (1.5 if packed >> bit & 1 else 2.0)      # (nominal: scales, escape records and padding left out)
        n, ms = prof[cls]
        us = ms / n * 1e3 if n else float("nan")
        out[cls] = (us, weights[cls] * per_weight / (us * 1e-6) / 1e12 if n else float("nan"), per_weight)
    return prof, out


parent = Backend(args.parent_lib, "tgx_", required=list(ABI)) if args.parent_lib else None
say("# option weights.fp8: FP8 (E4M3, one power-of-two scale per row) gate_up / down / lm_head streams at batch 1 — tools/fp8_bench.py")
say(f"# base context: {'the parent commit library at its defaults' if parent else 'this library with weights.fp8 = 0 (the parent launches and bits)'}")
say(f"# point: {args.prompt}-token prefill, {args.warmup} warm-up steps, {args.steps} timed greedy steps; {args.rounds} rounds x {args.reps} regions per context, contexts alternating")
for name in args.models.split(","):
    d = known_desc(name, "bf16")
    d.max_ctx = min(d.max_ctx, 4096)
    base, q = Model(d, parent or product_backend()), Model(d, product_backend())
    q.set_option("weights.fp8", 1)
    t0 = time.time()
    for tname, bits in synth.synth_checkpoint(d, 1234, 0.02):
        base.upload(tname, bits); q.upload(tname, bits)
    base.finalize(); q.finalize()
    say()
    say(f"## {name} bf16 ({d.param_count() / 1e9:.2f} B parameters; load + quantize {time.time() - t0:.0f} s)")
    say(f"fp8 streams {q.get_option('weights.fp8_matrices')}, fallbacks {q.get_option('weights.fp8_fallbacks')}; "
        f"bytes per token at context {args.prompt + args.warmup + args.steps // 2}: base {base.bytes_per_token(args.prompt + args.warmup + args.steps // 2) / 1e6:.1f} MB, "
        f"fp8 {q.bytes_per_token(args.prompt + args.warmup + args.steps // 2) / 1e6:.1f} MB")
    prompt = synth.synth_prompt(d.vocab, args.prompt, 1234)[None, :]
    for m in (base, q):
        timed(m, prompt)                                    # untimed: workspaces, code objects, graphs
    rounds = {"base": [], "fp8": []}
    for r in range(args.rounds):
        got = {"base": [], "fp8": []}
        for _ in range(args.reps):
            got["base"].append(timed(base, prompt)); got["fp8"].append(timed(q, prompt))
        for k in got:
            rounds[k].append(statistics.median(got[k]))
        say(f"round {r}: base {rounds['base'][-1]:.4f} ms/step   fp8 {rounds['fp8'][-1]:.4f} ms/step")
    mb, mq = statistics.median(rounds["base"]), statistics.median(rounds["fp8"])
    sb, sq = max(rounds["base"]) - min(rounds["base"]), max(rounds["fp8"]) - min(rounds["fp8"])
    say(f"ms per step, median of the rounds' medians (spread of the rounds): base {mb:.4f} ({sb:.4f})   fp8 {mq:.4f} ({sq:.4f})   "
        f"difference {mb - mq:+.4f} ms = {100 * (mb - mq) / mb:+.1f} %   tok/s {1e3 / mb:.0f} -> {1e3 / mq:.0f}")
    say("faster than the base by more than the spread" if mb - mq > max(sb, sq) else "NOT faster than the base by more than the spread")
    for label, m, fp8 in (("base", base, 0), ("fp8", q, 1)):
        m.reset_cache(); m.forward(prompt); m.sample(GREEDY); m.decode(args.warmup, GREEDY, fetch=False)
        prof, cls = class_table(m, d, fp8)
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
    base.close(); q.close()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
