#!/usr/bin/env python3
"""embed_bench.py — the cost of tgx_embed_rows (include/tgx.h) against tgx_forward_rows on the same prompts: the embedding call runs the same prompt passes without
lm_head and adds one pooling pass (kernels/embed_pool.h).  Both forms alternate inside every repetition on ONE context (two contexts of one process were measured 2-4 % apart on the
same tgx_forward_rows call, in either direction from run to run: profiles/embed_rows.txt); every shape is warmed up first; each figure is the median of --reps repetitions with their min .. max beside it — the run-to-run spread a difference has to exceed — each timed
from a synchronised device to the call's own synchronise (the row resets before a repetition are outside the window).

    python tools/embed_bench.py [--model llama-3.2-1b] [--dtype bf16] [--reps 10] [--sets 32x128,4x2048] [--pool mean] [--parent-lib PATH] [--out profiles/embed_rows.txt]

--parent-lib: also time tgx_forward_rows of that library (a build without tgx_embed_rows) on a second context, as a third alternating form.
The pooling kernels' own time is not visible from the host: run the tool under `rocprofv3 --kernel-trace --stats` and read embed_pool_kernel / embed_finish_kernel.
The lines are printed and appended to --out."""
import argparse, dataclasses, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import ABI, Backend, Model, product_backend

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama-3.2-1b")
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--sets", default="32x128,4x2048", help="texts x tokens, comma separated")
ap.add_argument("--pool", default="mean", choices=["last", "mean", "first"])
ap.add_argument("--parent-lib", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed_rows.txt"))
args = ap.parse_args()

sets = [tuple(int(v) for v in s.split("x")) for s in args.sets.split(",")]
B, ctx = max(n for n, _ in sets), max(L for _, L in sets) + 64
desc = dataclasses.replace(known_desc(args.model, args.dtype), max_batch=B, max_ctx=ctx)
emb = Model(desc, product_backend()).load_synthetic(1234, 0.02).finalize()
old = Model(desc, Backend(args.parent_lib, "tgx_", required=[n for n in ABI if n != "embed_rows"])).load_synthetic(1234, 0.02).finalize() if args.parent_lib else None
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def timed(m, call, rows):
    for r in rows:
        if m.past_length_row(r):
            m.reset_row(r)
    m.synchronize()
    t0 = time.perf_counter()
    call()
    m.synchronize()
    return (time.perf_counter() - t0) * 1e3


say(f"# tools/embed_bench.py --model {args.model} --dtype {args.dtype} --reps {args.reps} --sets {args.sets} --pool {args.pool}"
    f"{' --parent-lib <parent build>' if args.parent_lib else ''}")
for n, L in sets:
    prompts = [synth.synth_prompt(desc.vocab, L, 900 + i) for i in range(n)]
    rows = list(range(n))
    forms = {"forward_rows": lambda: timed(emb, lambda: emb.forward_rows(rows, prompts), rows),
             "embed_rows": lambda: timed(emb, lambda: emb.embed_rows(rows, prompts, args.pool, release=True), rows)}
    if old:
        forms["parent"] = lambda: timed(old, lambda: old.forward_rows(rows, prompts), rows)
    for _ in range(2):
        for f in forms.values():
            f()
    t = {k: [] for k in forms}
    for _ in range(args.reps):
        for k, f in forms.items():
            t[k].append(f())
    cell = lambda v: f"{np.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]"
    fw, em = float(np.median(t["forward_rows"])), float(np.median(t["embed_rows"]))
    spread = max(t["forward_rows"]) - min(t["forward_rows"])
    verdict = "within" if em <= fw + spread else "SLOWER than"
    parent = f"   tgx_forward_rows (parent library, second context) {cell(t['parent'])}" if old else ""
    say(f"{desc.name} {args.dtype} {n} texts x {L} tokens, pool {args.pool}, ms: tgx_forward_rows {cell(t['forward_rows'])}   "
        f"tgx_embed_rows {cell(t['embed_rows'])}   embed - forward {em - fw:+.3f} ({verdict} forward_rows' median + its spread {spread:.3f}){parent}; "
        f"pooling launches {emb.get_option('embed.last_pool_launches')}")
emb.close()
if old:
    old.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    f.write("\n".join(lines) + "\n")
