#!/usr/bin/env python3
"""admit_bench.py — the cost of bringing k prompts into a running batch: k sequential tgx_forward_row calls against ONE tgx_forward_rows call on the same prompts
(include/tgx.h), on one context, unpaged and paged.  Both forms alternate in the same process; every shape is warmed up first; each figure is the median of --reps
repetitions, each timed from a synchronised device to the call's own device synchronise (the row resets before each repetition are outside the window).

    python tools/admit_bench.py [--model llama-3.2-1b] [--dtype bf16] [--reps 10] [--sets 8x64,4x256,16x32,mixed]

--fork N[,N..] measures n-best admission instead (include/tgx.h tgx_fork_row): ONE tgx_forward_row plus ONE tgx_fork_row into N - 1 rows against tgx_forward_rows with
N copies of the prompt, for every prompt length of --fork-prompts; the fork call is also timed alone, and on slabs its copy rate (bytes read once + written N - 1 times
over that time) is printed beside it.

    python tools/admit_bench.py --fork 4,16 [--fork-prompts 256,2048]

--extend measures a continuation (include/tgx.h tgx_extend_row): S new tokens after P cached ones, with the attention of the pass on the per-row prompt kernel
(extend.attn_splits 0), on the automatic choice (-1) and on 4 / 8 / 16 / 32 forced key splits (kernels/attn_extend.h) — and beside them tgx_reset_row +
tgx_forward_row(P + S), what a caller without tgx_extend_row does.  The forms alternate inside every repetition; the row is rolled back (tgx_truncate_row) outside the
timed window.  Each figure is the median of --reps repetitions with their min .. max beside it: the spread a difference has to exceed.

    python tools/admit_bench.py --extend [--model llama-3.2-1b] [--layers 0] [--extend-pasts 512,2048,8192] [--extend-lens 16,64,128]
    python tools/admit_bench.py --extend --model mistral-7b-v0.3 --dtype bf16 --layers 2        # head_dim 128 at two layers

--snapshot measures moving a row off the device and back (include/tgx.h tgx_save_row / tgx_restore_row): for a prompt of P tokens (--fork-prompts plus 8192), on
slabs and paged, tgx_save_row into a pageable host buffer, tgx_reset_row + tgx_restore_row from it, and tgx_reset_row + tgx_forward_row(P) — what a caller without
snapshots does to bring the sequence back.  The three alternate inside every repetition; median [min .. max] of --reps, and the GB/s each copy direction reached.

    python tools/admit_bench.py --snapshot [--fork-prompts 256,2048]

--mixed measures chunked prefill (include/tgx.h tgx_advance_rows): B live rows at a context of ~--mixed-ctx tokens take one step while one more row, which holds
--mixed-past positions, is fed a chunk of S tokens — as ONE tgx_advance_rows call on this build, per value of --mixed-tiles (option advance.attn_tiles), against
tgx_decode_rows(1) + tgx_extend_row(chunk) on --parent-lib (a library without the call; default: this build's).  The baseline's chunk row has to hold a token for
tgx_decode_rows, so it steps too: B + 1 rows.  The forms alternate inside every repetition on two contexts of one process; the chunk's row is rebuilt outside the timed
window; the step rows grow by one position per call.  Median [min .. max] of --reps.

    python tools/admit_bench.py --mixed [--mixed-rows 8,32] [--mixed-chunks 128,256,512] [--mixed-tiles 0,4,8,16,-1] [--parent-lib PATH]

--splice measures cutting the middle out of a row (include/tgx.h tgx_splice_row), the context shift "keep 4, drop the first half of the rest": 2048 -> 4 + 1024 and
8192 -> 4 + 4096 positions, on slabs and paged.  Per repetition, each from a synchronised device to the call's own synchronise: ONE tgx_splice_row; the one-token
tgx_extend_row that re-feeds the current token behind it; and tgx_reset_row + tgx_forward_row of the kept tokens, what a caller without the call does.  The row is
prefilled again outside the timed window.  Median [min .. max] of --reps; the lines are also written to --splice-out (default profiles/splice_row.txt).

    python tools/admit_bench.py --splice [--splice-out FILE]
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
ap.add_argument("--fork", default="", help="n-best admission: forward_row + fork_row into N - 1 rows against forward_rows of N copies (e.g. 4,16)")
ap.add_argument("--fork-prompts", default="256,2048")
ap.add_argument("--extend", action="store_true", help="a continuation of S tokens after P cached ones: tgx_extend_row per attention form against reset + forward_row(P + S)")
ap.add_argument("--extend-pasts", default="512,2048,8192")
ap.add_argument("--extend-lens", default="16,64,128")
ap.add_argument("--extend-splits", default="0,-1,4,8,16,32")
ap.add_argument("--layers", type=int, default=0, help="--extend: cut the model to this many layers (0 = all)")
ap.add_argument("--snapshot", action="store_true", help="tgx_save_row, reset + tgx_restore_row and reset + forward_row(P) for the P of --fork-prompts plus 8192")
ap.add_argument("--mixed", action="store_true", help="B step rows + one prompt chunk: ONE tgx_advance_rows call against tgx_decode_rows(1) + tgx_extend_row(chunk)")
ap.add_argument("--mixed-rows", default="8,32")
ap.add_argument("--mixed-chunks", default="128,256,512")
ap.add_argument("--mixed-ctx", type=int, default=300, help="--mixed: the step rows' context")
ap.add_argument("--mixed-past", type=int, default=256, help="--mixed: the positions the chunk's row already holds")
ap.add_argument("--mixed-tiles", default="-1", help="--mixed: the advance.attn_tiles values to time the joint call with (e.g. 0,4,8,16,-1)")
ap.add_argument("--parent-lib", default="", help="--mixed: the library the two-call baseline runs on (default: this build's)")
ap.add_argument("--splice", action="store_true", help="tgx_splice_row (2048 -> 4 + 1024, 8192 -> 4 + 4096) and the one-token extend_row behind it against reset + forward_row of the kept tokens")
ap.add_argument("--splice-out", default=os.path.join(ROOT, "profiles", "splice_row.txt"))
args = ap.parse_args()


def splice_bench():
    shapes = [(2048, 4, 1024), (8192, 4, 4096)]      # (past, kept at the front, kept at the end)
    ctx = max(s[0] for s in shapes) + 64
    lines = [f"# tools/admit_bench.py --splice --model {args.model} --dtype {args.dtype} --reps {args.reps}: one synchronised call each, ms, median [min .. max]"]
    for paged in (0, 1):
        desc = dataclasses.replace(known_desc(args.model, args.dtype), max_batch=1, max_ctx=ctx)
        m = Model(desc, product_backend())
        if paged:
            m.set_option("kv.budget_tokens", ((ctx + 127) // 128 + 1) * 128)
        m.load_synthetic(1234, 0.02).finalize()
        for P, head, tail in shapes:
            p = synth.synth_prompt(desc.vocab, P, 900)
            ranges = [(0, head), (P - tail, tail)]
            kept = np.concatenate([p[:head], p[P - tail:]])

            def timed(call):
                m.synchronize()
                t0 = time.perf_counter()
                call()
                m.synchronize()
                return (time.perf_counter() - t0) * 1e3

            t = {"splice": [], "extend": [], "forward": []}
            for rep in range(2 + args.reps):
                m.reset_row(0); m.forward_row(0, p)
                tok = int(m.sample_row(0, GREEDY))
                a = timed(lambda: m.splice_row(0, ranges))
                b = timed(lambda: m.extend_row(0, [tok]))
                c = timed(lambda: (m.reset_row(0), m.forward_row(0, kept)))
                if rep >= 2:
                    t["splice"].append(a); t["extend"].append(b); t["forward"].append(c)
            cell = lambda v: f"{np.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]"
            sp, ex, fw = (float(np.median(t[k])) for k in ("splice", "extend", "forward"))
            mib = 2 * desc.layers * desc.kv_heads * desc.head_dim * (4 if args.dtype == 'fp32' else 2) * tail / 2**20
            lines.append(f"{desc.name} {args.dtype} {'paged' if paged else 'slabs'} {P:5d} -> {head} + {tail:4d} ({mib:6.1f} MiB moved)  splice_row {cell(t['splice'])}   "
                         f"extend_row(1) {cell(t['extend'])}   reset + forward_row({head + tail}) {cell(t['forward'])}   splice / forward {sp / fw:.3f}   (splice + extend) / forward {(sp + ex) / fw:.3f}")
            print(lines[-1], flush=True)
        m.close()
    with open(args.splice_out, "w") as f:
        f.write("\n".join(lines) + "\n")


if args.splice:
    splice_bench()
    sys.exit(0)


def snapshot_bench():
    import ctypes
    plens = sorted(set([int(x) for x in args.fork_prompts.split(",")] + [8192]))
    ctx = max(plens) + 64
    for paged in (0, 1):
        desc = dataclasses.replace(known_desc(args.model, args.dtype), max_batch=1, max_ctx=ctx)
        m = Model(desc, product_backend())
        if paged:
            m.set_option("kv.budget_tokens", ((max(plens) + 127) // 128 + 1) * 128)
        m.load_synthetic(1234, 0.02).finalize()
        for P in plens:
            p = synth.synth_prompt(desc.vocab, P, 900)
            m.reset_row(0); m.forward_row(0, p)
            n = m.row_snapshot_bytes(0)
            buf = np.zeros(n, dtype=np.uint8)              # pageable, touched
            ptr, wrote = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(0)

            def timed(call, reset):
                if reset:
                    m.reset_row(0)
                m.synchronize()
                t0 = time.perf_counter()
                call()
                m.synchronize()
                return (time.perf_counter() - t0) * 1e3

            forms = {"save": (lambda: m._check(m.be.save_row(m._ctx, 0, ptr, n, ctypes.byref(wrote))), False),
                     "restore": (lambda: m._check(m.be.restore_row(m._ctx, 0, ptr, n)), True),
                     "forward": (lambda: m.forward_row(0, p), True)}
            t = {k: [] for k in forms}
            for rep in range(2 + args.reps):
                for k, (call, reset) in forms.items():      # save (the row is live), reset + restore, reset + forward_row: each leaves the row live for the next
                    dt = timed(call, reset)
                    if rep >= 2:
                        t[k].append(dt)
            cell = lambda v: f"{np.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]"
            sv, rs, fw = (float(np.median(t[k])) for k in ("save", "restore", "forward"))
            print(f"{desc.name} {args.dtype} {'paged' if paged else 'slabs'} prompt {P:5d} ({n / 2**20:7.1f} MiB) ms  save_row {cell(t['save'])} = {n / sv / 1e6:5.1f} GB/s   "
                  f"reset + restore_row {cell(t['restore'])} = {n / rs / 1e6:5.1f} GB/s   reset + forward_row({P}) {cell(t['forward'])}   restore / forward {rs / fw:.2f}", flush=True)
        m.close()


if args.snapshot:
    snapshot_bench()
    sys.exit(0)


def mixed_bench():
    from tinygpt_amd.ffi import ABI, ADV_FEED, ADV_STEP, Backend
    new_syms = ("advance_rows",)
    rows_l, chunks = [int(x) for x in args.mixed_rows.split(",")], [int(x) for x in args.mixed_chunks.split(",")]
    tiles_l = [int(x) for x in args.mixed_tiles.split(",")]
    C0, P = args.mixed_ctx, args.mixed_past
    old_be = Backend(args.parent_lib, "tgx_", required=[n for n in ABI if n not in new_syms]) if args.parent_lib else product_backend()
    for paged in (0, 1):
        for B in rows_l:
            ctx = max(C0 + 8 * (4 + args.reps), P + max(chunks) + 8) + 64
            desc = dataclasses.replace(known_desc(args.model, args.dtype), max_batch=B + 1, max_ctx=ctx)
            ms = []
            for be in (product_backend(), old_be):
                m = Model(desc, be)
                if paged:
                    m.set_option("kv.budget_tokens", (B + 1) * ((ctx + 127) // 128) * 128)
                m.load_synthetic(1234, 0.02).finalize()
                for r in range(B):
                    m.forward_row(r, synth.synth_prompt(desc.vocab, C0 - (r % 7), 900 + r))
                    m.set_row_sampler(r, GREEDY, 0); m.sample_row(r, GREEDY)
                ms.append(m)
            new, old = ms
            prefix = synth.synth_prompt(desc.vocab, P, 77)
            for S in chunks:
                chunk = [int(t) for t in synth.synth_prompt(desc.vocab, S, 78)]

                def joint(tiles):
                    new.reset_row(B); new.forward_row(B, prefix)
                    new.set_option("advance.attn_tiles", tiles)
                    new.synchronize()
                    t0 = time.perf_counter()
                    new.advance_rows(list(range(B + 1)), [ADV_STEP] * B + [ADV_FEED], [[]] * B + [chunk])
                    new.synchronize()
                    return (time.perf_counter() - t0) * 1e3

                def apart():
                    old.reset_row(B); old.forward_row(B, prefix); old.sample_row(B, GREEDY)
                    old.synchronize()
                    t0 = time.perf_counter()
                    old.decode_rows(1)
                    old.extend_row(B, chunk)
                    old.synchronize()
                    return (time.perf_counter() - t0) * 1e3

                for _ in range(2):
                    apart()
                    for tl in tiles_l:
                        joint(tl)
                t = {tl: [] for tl in tiles_l}
                base = []
                for _ in range(args.reps):
                    base.append(apart())
                    for tl in tiles_l:
                        t[tl].append(joint(tl))
                cell = lambda v: f"{np.median(v):6.3f} [{min(v):6.3f} .. {max(v):6.3f}]"
                cells = "  ".join(f"tiles {'auto' if tl < 0 else tl}: {cell(v)}" for tl, v in t.items())
                print(f"{desc.name} {args.dtype} {'paged' if paged else 'slabs'} {B:2d} step rows at ~{C0} + a chunk of {S:3d} at past {P} ms  "
                      f"decode_rows(1) + extend_row ({'parent' if args.parent_lib else 'this'} library) {cell(base)}  |  one tgx_advance_rows  {cells}"
                      f"  (advance.last_tiles {new.get_option('advance.last_tiles')})", flush=True)
            new.close(); old.close()


if args.mixed:
    mixed_bench()
    sys.exit(0)


def extend_bench():
    pasts, lens = [int(x) for x in args.extend_pasts.split(",")], [int(x) for x in args.extend_lens.split(",")]
    forms = [int(x) for x in args.extend_splits.split(",")]
    desc = dataclasses.replace(known_desc(args.model, args.dtype), max_batch=1, max_ctx=max(pasts) + max(lens) + 64)
    if args.layers:
        desc = dataclasses.replace(desc, layers=args.layers)
    m = Model(desc, product_backend()).load_synthetic(1234, 0.02).finalize()
    tag = f"{desc.name} {args.dtype} {desc.layers} layers head_dim {desc.head_dim}"
    for P in pasts:
        for S in lens:
            seq = synth.synth_prompt(desc.vocab, P + S, 900)
            m.reset_cache(); m.forward_row(0, seq[:P])

            def ext(ns):
                m.set_option("extend.attn_splits", ns)
                m.synchronize()
                t0 = time.perf_counter()
                m.extend_row(0, seq[P:])
                m.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                m.truncate_row(0, P)
                return dt

            for ns in forms:
                ext(ns); ext(ns)
            t = {ns: [] for ns in forms}
            for _ in range(args.reps):
                for ns in forms:
                    t[ns].append(ext(ns))
            full = []
            for i in range(2 + max(3, args.reps // 3)):
                m.reset_row(0); m.synchronize()
                t0 = time.perf_counter()
                m.forward_row(0, seq)
                m.synchronize()
                if i >= 2:
                    full.append((time.perf_counter() - t0) * 1e3)
            cells = "  ".join(f"{'auto' if ns < 0 else ns}: {np.median(v):6.3f} [{min(v):6.3f} .. {max(v):6.3f}]" for ns, v in t.items())
            print(f"{tag} past {P:5d} S {S:3d} ms  {cells}  | reset + forward_row({P + S}): {np.median(full):7.3f}", flush=True)
    m.close()


if args.extend:
    extend_bench()
    sys.exit(0)


def fork_bench():
    ns, plens = [int(x) for x in args.fork.split(",")], [int(x) for x in args.fork_prompts.split(",")]
    B, ctx = max(ns), max(args.max_ctx, max(plens) + 64)
    for paged in (0, 1):
        desc = dataclasses.replace(known_desc(args.model, args.dtype), max_batch=B, max_ctx=ctx)
        m = Model(desc, product_backend())
        if paged:
            m.set_option("kv.budget_tokens", B * ((max(plens) + 127) // 128 + 1) * 128)      # room for N separate copies of the longest prompt
        m.load_synthetic(1234, 0.02).finalize()
        m.forward(np.zeros((B, 1), dtype=np.int64)); m.sample(GREEDY)
        esz = 4 if args.dtype == "fp32" else 2
        for P in plens:
            p = synth.synth_prompt(desc.vocab, P, 900)
            for N in ns:
                def run(fork):
                    for r in range(B):
                        m.reset_row(r)
                    m.synchronize()
                    t0 = time.perf_counter()
                    if fork:
                        m.forward_row(0, p)
                        t1 = time.perf_counter()
                        m.fork_row(0, range(1, N))
                    else:
                        t1 = t0
                        m.forward_rows(range(N), [p] * N)
                    m.synchronize()
                    t2 = time.perf_counter()
                    return (t2 - t0) * 1e3, (t2 - t1) * 1e3
                for _ in range(2):
                    run(True); run(False)
                whole, call, copies = [], [], []
                for _ in range(args.reps):
                    a, b = run(True); whole.append(a); call.append(b)
                    copies.append(run(False)[0])
                w, c, j = float(np.median(whole)), float(np.median(call)), float(np.median(copies))
                moved = 2 * desc.layers * desc.kv_heads * (P % 128 if paged else P) * desc.head_dim * esz      # bytes read once, written N - 1 times
                print(f"{desc.name} {args.dtype} {'paged' if paged else 'slabs'} prompt {P:5d} n {N:3d}: forward_row + fork_row {w:7.2f} ms (the fork call {c * 1e3:7.0f} us, "
                      f"{moved * N / 1e6:7.1f} MB moved = {moved * N / max(c, 1e-9) / 1e6:6.1f} GB/s), forward_rows of {N} copies {j:7.2f} ms, ratio {w / j:.2f}", flush=True)
        m.close()


if args.fork:
    fork_bench()
    sys.exit(0)
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
