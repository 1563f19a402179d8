#!/usr/bin/env python3
"""Cost of the per-row logit processors (tgx_set_row_penalties / tgx_set_row_logit_bias) inside the per-row decode step: ms/step of tgx_decode_rows, greedy rows,
with no processor set (twice: the A/A spread of the measurement), with one row of the batch processed, and with every row processed.

    python tools/logit_proc_cost.py [--model llama-3.2-1b] [--prompt 300] [--steps 128] [--batches 1,8,32] [--reps 4] [--lib other/libtgx_mi355x.so]

--lib: measure another build of the library (the parent commit's, for the "nothing set costs nothing" comparison); a library without the processor calls runs
the unprocessed legs only.
"""
import argparse, ctypes, dataclasses, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import ABI, Backend, Model, product_backend

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama-3.2-1b")
ap.add_argument("--prompt", type=int, default=300)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--batches", default="1,8,32")
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--lib", default=None)
args = ap.parse_args()
batches = [int(b) for b in args.batches.split(",")]
if args.lib:
    probe = ctypes.CDLL(args.lib)
    be = Backend(args.lib, "tgx_", required=[n for n in ABI if hasattr(probe, "tgx_" + n)])
else:
    be = product_backend()
has_proc = be.has("set_row_penalties")
desc = dataclasses.replace(known_desc(args.model), max_batch=max(batches), max_ctx=args.prompt + 2 * args.steps + 64)
m = Model(desc, be)
for name, bits in synth.synth_checkpoint(desc, 1234, 0.02):
    m.upload(name, bits)
m.finalize()
BIAS = {i * 397 % desc.vocab: (-1.0 if i % 3 else float("-inf")) for i in range(1, 33)}      # 32 ids across the vocabulary, a third of them banned


def start(ids, on):
    m.reset_cache(); m.forward(ids)
    for b, p in enumerate(on):
        if p:
            m.set_row_penalties(b, 1.3, 0.2, 0.1).set_row_logit_bias(b, BIAS).set_row_history(b, prompt_ids=ids[b])
        m.sample_row(b)


for B in batches:
    ids = np.stack([synth.synth_prompt(desc.vocab, args.prompt, 77 + b) for b in range(B)])
    legs = [("off", [False] * B), ("off (A/A)", [False] * B)]
    if has_proc:
        if B > 1:
            legs.append((f"one row of {B}", [True] + [False] * (B - 1)))
        legs.append(("all rows", [True] * B))
    times = {label: [] for label, _ in legs}
    for rep in range(args.reps):        # the legs alternate (the clock the power manager grants drifts over a run): every repetition is printed, the best is compared
        for label, on in legs:
            start(ids, on); m.decode_rows(16 + args.steps); m.synchronize()      # (untimed: every graph the timed steps replay is captured here)
            start(ids, on); m.decode_rows(16); m.synchronize()
            t0 = time.perf_counter(); m.decode_rows(args.steps); m.synchronize()
            times[label].append((time.perf_counter() - t0) / args.steps)
    base = min(times["off"])
    for label, _ in legs:
        ts = times[label]
        print(f"B={B:<3d} processors {label:16s} {min(ts) * 1e3:.4f} ms/step (reps {' '.join(f'{t * 1e3:.4f}' for t in ts)})  vs off {(min(ts) - base) * 1e6:+7.1f} us", flush=True)
