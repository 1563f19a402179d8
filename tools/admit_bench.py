#!/usr/bin/env python3
"""admit_bench.py — the cost of bringing k prompts into a running batch: k sequential tgx_forward_row calls against ONE tgx_forward_rows call on the same prompts
(include/tgx.h), on one context, unpaged and paged.  Both forms alternate in the same process; every shape is warmed up first; each figure is the median of --reps
repetitions, each timed from a synchronised device to the call's own device synchronise (the row resets before each repetition are outside the window).

    python tools/admit_bench.py [--model llama-3.2-1b] [--dtype bf16] [--reps 10] [--sets 8x64,4x256,16x32,mixed]
"""
import argparse, dataclasses, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import GREEDY, Model, product_backend

SETS = {"8x64": [64] * 8, "4x256": [256] * 4, "16x32": [32] * 16, "mixed": [500, 300, 120, 40, 16, 8]}
ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama-3.2-1b")
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--sets", default=",".join(SETS))
ap.add_argument("--max-ctx", type=int, default=1024)
args = ap.parse_args()
sets = [(name, SETS[name]) for name in args.sets.split(",")]
B = max(len(lens) for _, lens in sets)

for paged in (0, 1):
    desc = dataclasses.replace(known_desc(args.model, args.dtype), max_batch=B, max_ctx=args.max_ctx)
    m = Model(desc, product_backend())
    if paged:
        m.set_option("kv.budget_tokens", B * args.max_ctx // 2)
    m.load_synthetic(1234, 0.02).finalize()
    m.forward(np.zeros((B, 1), dtype=np.int64)); m.sample(GREEDY)           # a batch of B rows, all retired below before every admission
    for name, lens in sets:
        prompts = [synth.synth_prompt(desc.vocab, n, 900 + i) for i, n in enumerate(lens)]
        rows = list(range(len(lens)))

        def run(joint):
            for r in range(B):
                m.reset_row(r)
            m.synchronize()
            t0 = time.perf_counter()
            if joint:
                m.forward_rows(rows, prompts)
            else:
                for r, p in zip(rows, prompts):
                    m.forward_row(r, p)
            m.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(2):
            run(False); run(True)
        seq, joint = [], []
        for _ in range(args.reps):
            seq.append(run(False)); joint.append(run(True))
        s, j = float(np.median(seq)), float(np.median(joint))
        print(f"{desc.name} {args.dtype} {'paged' if paged else 'slabs'} {name:6s} ({sum(lens)} tokens): {len(lens)} x tgx_forward_row {s:7.2f} ms, "
              f"tgx_forward_rows {j:7.2f} ms, ratio {j / s:.2f}", flush=True)
    m.close()
