#!/usr/bin/env python3
"""Cost of the per-token log-probability records (tgx_set_row_logprobs) inside the per-row decode step: ms/step of tgx_decode_rows, greedy rows, with logprobs
off, top_n 0 / 5 / 20 on every row, and top_n 5 on one row of the batch.

    python tools/logprobs_cost.py [--model llama-3.2-1b] [--prompt 256] [--steps 128] [--batches 1,32] [--reps 4]
"""
import argparse, dataclasses, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import Model, product_backend

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama-3.2-1b")
ap.add_argument("--prompt", type=int, default=256)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--batches", default="1,32")
ap.add_argument("--reps", type=int, default=4)
args = ap.parse_args()
batches = [int(b) for b in args.batches.split(",")]
desc = dataclasses.replace(known_desc(args.model), max_batch=max(batches), max_ctx=args.prompt + 2 * args.steps + 64)
m = Model(desc, product_backend())
for name, bits in synth.synth_checkpoint(desc, 1234, 0.02):
    m.upload(name, bits)
m.finalize()


def start(ids, tops):
    m.reset_cache(); m.forward(ids)
    for b, top_n in enumerate(tops):
        m.set_row_logprobs(b, top_n); m.sample_row(b)


for B in batches:
    ids = np.stack([synth.synth_prompt(desc.vocab, args.prompt, 77 + b) for b in range(B)])
    legs = [("off", [-1] * B), ("top_n 0, all rows", [0] * B), ("top_n 5, all rows", [5] * B), ("top_n 20, all rows", [20] * B)]
    if B > 1:
        legs.append((f"top_n 5, one row of {B}", [5] + [-1] * (B - 1)))
    times = {label: [] for label, _ in legs}
    for rep in range(args.reps):        # the legs alternate (the clock the power manager grants drifts over a run): every repetition is printed, the best is compared
        for label, tops in legs:
            start(ids, tops); m.decode_rows(16 + args.steps); m.synchronize()      # (untimed: every graph the timed steps replay is captured here)
            start(ids, tops); m.decode_rows(16); m.synchronize()
            t0 = time.perf_counter(); m.decode_rows(args.steps); m.synchronize()
            times[label].append((time.perf_counter() - t0) / args.steps)
    base = min(times["off"])
    for label, _ in legs:
        ts = times[label]
        print(f"B={B:<3d} logprobs {label:24s} {min(ts) * 1e3:.4f} ms/step (reps {' '.join(f'{t * 1e3:.4f}' for t in ts)})  adds {(min(ts) - base) * 1e6:6.1f} us", flush=True)
