#!/usr/bin/env python3
"""Decode rate vs batch size (rows share each weight pass through the batched GEMV): aggregate tokens/s for B = 1, 2, 4, 8.

    python tools/batch_bench.py [--model llama-3.2-1b] [--prompt 512] [--steps 128]
"""
import argparse, dataclasses, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import GREEDY, Model, product_backend

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama-3.2-1b")
ap.add_argument("--prompt", type=int, default=512)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--batches", default="1,2,4,8")
ap.add_argument("--opts", default="", help="tgx_set_option pairs applied after finalize, e.g. 'gateup.ks=4;oproj.ks=2'")
ap.add_argument("--kv-budget", type=int, default=0, help="paged KV: option kv.budget_tokens (set before finalize); 0 = one max_ctx slab per row")
ap.add_argument("--sampler", default="", help="e.g. 'temperature=0.8,top_p=0.9' (default: greedy)")
ap.add_argument("--rows-api", action="store_true", help="the per-row path: every row's settings = --sampler (tgx_set_row_sampler), steps by tgx_decode_rows")
ap.add_argument("--mix", action="store_true", help="(per-row path) rows cycle greedy, T 0.8/p 0.9, T 1.0/k 50, T 0.7/min-p 0.05, all four filters")
args = ap.parse_args()
args.rows_api = args.rows_api or args.mix
batches = [int(b) for b in args.batches.split(",")]
desc = dataclasses.replace(known_desc(args.model), max_batch=max(batches), max_ctx=args.prompt + 2 * args.steps + 64)
m = Model(desc, product_backend())
if args.kv_budget:
    m.set_option("kv.budget_tokens", args.kv_budget)
for name, bits in synth.synth_checkpoint(desc, 1234, 0.02):
    m.upload(name, bits)
m.finalize()
for kv in filter(None, args.opts.split(";")):
    k, v = kv.split("="); m.set_option(k, int(v))
cfg = GREEDY
if args.sampler:
    from tinygpt_amd.ffi import SamplerCfg
    kw = {}
    for item in args.sampler.split(","):
        k, v = item.split("="); kw[k] = int(v) if k == "top_k" else float(v)
    cfg = SamplerCfg(**kw)
from tinygpt_amd.ffi import SamplerCfg
MIX = [GREEDY, SamplerCfg(0.8, 0, 0.9, 0.0), SamplerCfg(1.0, 50, 1.0, 0.0), SamplerCfg(0.7, 0, 1.0, 0.05), SamplerCfg(0.9, 40, 0.95, 0.05)]


def start(ids):
    m.reset_cache(); m.forward(ids); m.sample(cfg, seed=1)
    if args.rows_api:
        for b in range(ids.shape[0]):
            m.set_row_sampler(b, MIX[b % len(MIX)] if args.mix else cfg, 1 + b if args.mix else 1)


def run(n):
    if args.rows_api:
        m.decode_rows(n)
    else:
        m.decode(n, cfg, seed=1, fetch=False)


for B in batches:
    ids = np.stack([synth.synth_prompt(desc.vocab, args.prompt, 77 + b) for b in range(B)])
    start(ids)
    run(16 + args.steps); m.synchronize()      # (untimed: every graph the timed steps replay is captured here)
    start(ids)
    run(16); m.synchronize()
    t0 = time.perf_counter(); run(args.steps); m.synchronize(); dt = time.perf_counter() - t0
    tag = ("mixed rows " if args.mix else "rows ") if args.rows_api else ""
    print(f"{'paged ' if args.kv_budget else ''}{tag}{args.sampler + ' ' if args.sampler else ''}B={B}: {dt / args.steps * 1e3:.3f} ms/step, {B * args.steps / dt:.0f} tokens/s aggregate", flush=True)
