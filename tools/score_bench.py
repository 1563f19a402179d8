#!/usr/bin/env python3
"""score_bench.py — what scoring every position costs on top of the prompt pass (include/tgx.h tgx_score_row): ms of tgx_forward_row alone and of tgx_score_row with
top_n 0 and 20 on the same prompt, row 0 of one context, and the added ms against the 2 * seq * hidden * V flops of the all-position lm_head.  The forms alternate
inside every repetition; every shape is warmed up first; each figure is the median of --reps repetitions with their min .. max, each timed from a synchronised
device to the call's own return (both calls synchronise like an admission; the row reset is outside the window).

    python tools/score_bench.py [--models llama-3.2-1b,qwen2.5-0.5b] [--seqs 256,2048,8192] [--reps 7]
    python tools/score_bench.py --sweep [--model llama-3.2-1b --seq 2048]        # score.rows x score.vocab_chunk around the defaults
    python tools/score_bench.py --once --model llama-3.2-1b --seq 2048 --top-n 20   # two calls (the second warmed), for a kernel trace
"""
import argparse, dataclasses, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import Model, product_backend

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="llama-3.2-1b,qwen2.5-0.5b")
ap.add_argument("--model", default="llama-3.2-1b", help="--sweep / --once")
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--seqs", default="256,2048,8192")
ap.add_argument("--seq", type=int, default=2048, help="--sweep / --once")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sweep", action="store_true", help="score.rows x score.vocab_chunk")
ap.add_argument("--rows", default="512,1024,2048")
ap.add_argument("--chunks", default="8192,16384,32768")
ap.add_argument("--once", action="store_true")
ap.add_argument("--top-n", type=int, default=20)
args = ap.parse_args()


def model(name, ctx):
    desc = dataclasses.replace(known_desc(name, args.dtype), max_batch=1, max_ctx=ctx)
    return Model(desc, product_backend()).load_synthetic(1234, 0.02).finalize(), desc


def timed(m, fn):
    m.reset_row(0); m.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def cell(v):
    return f"{np.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]"


if args.once:
    m, desc = model(args.model, args.seq)
    ids = synth.synth_prompt(desc.vocab, args.seq, 900)
    for _ in range(2):
        m.reset_row(0); m.score_row(0, ids, args.top_n)
    m.close()
    sys.exit(0)

if args.sweep:
    m, desc = model(args.model, args.seq)
    ids = synth.synth_prompt(desc.vocab, args.seq, 900)
    combos = [(int(r), int(c)) for r in args.rows.split(",") for c in args.chunks.split(",")]
    t = {k: [] for k in combos}
    for rep in range(args.reps + 1):
        for r, c in combos:
            m.set_option("score.rows", r); m.set_option("score.vocab_chunk", c)
            dt = timed(m, lambda: m.score_row(0, ids, args.top_n))
            if rep:
                t[(r, c)].append(dt)
    for (r, c), v in t.items():
        print(f"{desc.name} {args.dtype} seq {args.seq} top_n {args.top_n}  score.rows {r:5d}  score.vocab_chunk {c:6d}  ms {cell(v)}", flush=True)
    m.close()
    sys.exit(0)

seqs = [int(x) for x in args.seqs.split(",")]
for name in args.models.split(","):
    m, desc = model(name, max(seqs))
    for S in seqs:
        ids = synth.synth_prompt(desc.vocab, S, 900)
        forms = {"forward_row": lambda: m.forward_row(0, ids), "score top_n 0": lambda: m.score_row(0, ids, 0), "score top_n 20": lambda: m.score_row(0, ids, 20)}
        t = {k: [] for k in forms}
        for rep in range(args.reps + 1):
            for k, fn in forms.items():
                dt = timed(m, fn)
                if rep:
                    t[k].append(dt)
        flops = 2.0 * S * desc.hidden * desc.vocab
        base = np.median(t["forward_row"])
        line = f"{desc.name} {args.dtype} V {desc.vocab} seq {S:5d} ms  " + "  ".join(f"{k}: {cell(v)}" for k, v in t.items())
        for k in ("score top_n 0", "score top_n 20"):
            add = np.median(t[k]) - base
            line += f"  | {k}: +{add:.3f} ms = {flops / max(add, 1e-9) / 1e9:.1f} TFLOP/s of lm_head"
        print(line + f"  (form {m.get_option('score.last_form')})", flush=True)
    m.close()
