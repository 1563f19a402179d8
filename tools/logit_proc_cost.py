#!/usr/bin/env python3
"""Cost of the per-row logit processors (tgx_set_row_penalties / tgx_set_row_logit_bias) inside the per-row decode step: ms/step of tgx_decode_rows, greedy rows,
with no processor set (twice: the A/A spread of the measurement), with one row of the batch processed, and with every row processed.

    python tools/logit_proc_cost.py [--model llama-3.2-1b] [--prompt 300] [--steps 128] [--batches 1,8,32] [--reps 4] [--lib other/libtgx_mi355x.so]

--lib: measure another build of the library (the parent commit's, for the "nothing set costs nothing" comparison); a library without the processor calls runs
the unprocessed legs only.

--automaton: the constrained-decoding leg (tgx_automaton_create / tgx_set_row_automaton) instead: per batch size no processor (twice), a bias list on every row
(the existing processor cost) and an automaton on every row (a 64-state table, every state allowing a random half of the vocabulary, so that the rows keep
running); then the cost of tgx_automaton_create for that table and, with --tokenizer DIR (a directory with tokenizer.json), the host compile time of three
patterns over it.  --out FILE appends the lines to FILE as well (profiles/automaton.txt).  With --lib (a library without the calls) only the "off" legs run.
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
ap.add_argument("--automaton", action="store_true")
ap.add_argument("--tokenizer", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--stop-id", type=int, default=0)      # --tokenizer: the id allowed where a match may end (the tokenizer's EOS)
args = ap.parse_args()
batches = [int(b) for b in args.batches.split(",")]
if args.lib:
    probe = ctypes.CDLL(args.lib)
    be = Backend(args.lib, "tgx_", required=[n for n in ABI if hasattr(probe, "tgx_" + n)])
else:
    be = product_backend()
has_proc = be.has("set_row_penalties")
has_auto = be.has("automaton_create")
_print = print


def print(*a, **kw):      # every line to --out as well
    _print(*a, **kw)
    if args.out:
        with open(args.out, "a") as f:
            _print(*a, file=f)


desc = dataclasses.replace(known_desc(args.model), max_batch=max(batches), max_ctx=args.prompt + 2 * args.steps + 64)
m = Model(desc, be)
for name, bits in synth.synth_checkpoint(desc, 1234, 0.02):
    m.upload(name, bits)
m.finalize()
BIAS = {i * 397 % desc.vocab: (-1.0 if i % 3 else float("-inf")) for i in range(1, 33)}      # 32 ids across the vocabulary, a third of them banned


AUTO_STATES = 64
auto_id = None


def auto_table():
    rng = np.random.default_rng(5)
    t = rng.integers(0, AUTO_STATES, size=(AUTO_STATES, desc.vocab)).astype(np.uint16)
    t[rng.random((AUTO_STATES, desc.vocab)) < 0.5] = 0xFFFF
    return t


def start(ids, on):
    m.reset_cache(); m.forward(ids)
    for b, p in enumerate(on):
        if p == "auto":
            m.set_row_automaton(b, auto_id, b % AUTO_STATES)
        elif p == "bias":
            m.set_row_logit_bias(b, BIAS)
        elif p:
            m.set_row_penalties(b, 1.3, 0.2, 0.1).set_row_logit_bias(b, BIAS).set_row_history(b, prompt_ids=ids[b])
        m.sample_row(b)


if args.automaton:
    print(f"# tools/logit_proc_cost.py --automaton: {args.model} bf16, prompt {args.prompt}, {args.steps} timed steps per repetition, {args.reps} repetitions, library {args.lib or 'this build'}")
    if has_auto:
        table = auto_table()
        ts = []
        for _ in range(5):
            m.synchronize(); t0 = time.perf_counter(); a = m.automaton_create(table); ts.append(time.perf_counter() - t0); m.automaton_destroy(a)
        print(f"tgx_automaton_create, {AUTO_STATES} states x V {desc.vocab} ({table.nbytes / 2 ** 20:.1f} MiB, host validation + allocation + copy): best {min(ts) * 1e3:.2f} ms (reps {' '.join(f'{t * 1e3:.2f}' for t in ts)})")
        auto_id = m.automaton_create(table)


for B in batches:
    ids = np.stack([synth.synth_prompt(desc.vocab, args.prompt, 77 + b) for b in range(B)])
    legs = [("off", [False] * B), ("off (A/A)", [False] * B)]
    if args.automaton:
        if has_auto:
            legs += [("bias, all rows", ["bias"] * B), ("automaton, all rows", ["auto"] * B)]
    elif has_proc:
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

if args.automaton and args.tokenizer:      # the host compile (tinygpt_amd/host/constraint.cpp) of three patterns over the tokenizer in that directory
    from tinygpt_amd import build
    lib = ctypes.CDLL(build.build_host()[0])
    lib.tgxe_constraint_compile.restype = ctypes.c_void_p
    lib.tgxe_constraint_compile.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.c_int32, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.tgxe_constraint_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int32)] * 3
    lib.tgxe_constraint_destroy.argtypes = [ctypes.c_void_p]
    for pat in (r"(yes|no|maybe)", r"\d{4}-\d{2}-\d{2}", r'\{"name": "[a-z]+", "age": \d+\}'):
        err = ctypes.create_string_buffer(512)
        t0 = time.perf_counter()
        h = lib.tgxe_constraint_compile(args.tokenizer.encode(), pat.encode(), (ctypes.c_int32 * 1)(args.stop_id), 1, 0, 0, err, 512)
        dt = time.perf_counter() - t0
        if not h:
            print(f"compile {pat!r} over {args.tokenizer}: refused: {err.value.decode()}")
            continue
        n, s0, v = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        lib.tgxe_constraint_info(h, ctypes.byref(n), ctypes.byref(s0), ctypes.byref(v))
        lib.tgxe_constraint_destroy(h)
        print(f"compile {pat!r} over {args.tokenizer} (tokenizer load included): {dt * 1e3:.1f} ms, {n.value} states x {v.value} ids")
elif args.automaton:
    print("host compile time over a 128k vocabulary: not measured (no --tokenizer given: no tokenizer of that size at hand)")
