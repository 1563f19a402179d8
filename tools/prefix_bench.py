#!/usr/bin/env python3
"""What option attn.shared_prefix buys on batched steps whose rows share a prompt, measured on one box: writes profiles/shared_prefix.txt.

    python tools/prefix_bench.py [--parent-lib PATH] [--rounds 3] [--out FILE]

Llama-3.2-1B bf16 geometry (synthetic weights), paged cache.  Cases: a 2048-token prompt forked into 8 rows (one group); four 2048-token prompts forked into 8
rows each (32 rows, 4 groups); 8 rows that share only their first 256 tokens of 2048 (a 256-token prompt forked, every row extended by 1792 tokens of its own);
an 8192-token prompt forked into 8 rows (where the shared stream is four times as long).
Per case: ms per tgx_decode_rows step with attn.shared_prefix 0 and 128 on ONE context, the settings taking turns within every round in the order 0, 128, 128, 0
(the rows grow by 48 tokens per region: the order gives both settings the same mean context); a region = 16 warm-up steps (setting the option drops the step
graphs: they are captured here) + 32 timed steps.  Reported: the median of the rounds' medians with the spread of the rounds.
With --parent-lib: the option-0 step of this library against the parent commit's library on the 32-row case, two contexts taking turns the same way."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth  # noqa: E402
from tinygpt_amd.ffi import ABI, GREEDY, Backend, Model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None, help="the parent commit's libtgx_mi355x.so")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=16)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_prefix.txt"))
args = ap.parse_args()
PROMPT, LONG, ROWS = 2048, 8192, 32
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def context(backend=None):
    d = known_desc("llama-3.2-1b", "bf16")
    d.max_batch, d.max_ctx = ROWS, LONG + 1024
    m = Model(d, backend) if backend else Model(d)
    m.set_option("kv.budget_tokens", LONG + 4 * PROMPT + ROWS * 1152)
    return m.load_synthetic(1234, 0.02).finalize()


def forked(m, n_prompts, per, shared=PROMPT, total=PROMPT):
    """n_prompts prompts of `shared` tokens, each forked into `per` rows; rows then extended to `total` tokens with tokens of their own"""
    m.reset_cache()
    for p in range(n_prompts):
        m.forward_row(p * per, synth.synth_prompt(m.desc.vocab, shared, 10 + p))
        m.fork_row(p * per, range(p * per + 1, (p + 1) * per))
    for r in range(n_prompts * per if shared < total else 0):
        m.extend_row(r, synth.synth_prompt(m.desc.vocab, total - shared, 500 + r))
    for r in range(n_prompts * per):      # (after every pass: a pass leaves the batch without current tokens)
        m.sample_row(r, GREEDY)


def region(m):
    m.decode_rows(args.warmup)
    m.synchronize()
    t0 = time.perf_counter()
    m.decode_rows(args.steps)
    m.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.steps


def take_turns(label, setters):
    """setters: [(name, callable that selects the setting and returns the context)] x 2 -> the table line; order a, b, b, a within every round"""
    per_round, groups = {name: [] for name, _ in setters}, [None]
    for _ in range(args.rounds):
        got = {name: [] for name, _ in setters}
        for i in (0, 1, 1, 0):
            name, select = setters[i]
            ctx = select()
            got[name].append(region(ctx))
            if name == "128":
                groups[0] = ctx.get_option("attn.last_prefix_groups")
        for name in got:
            per_round[name].append(statistics.median(got[name]))
    cells = []
    for name, _ in setters:
        v = per_round[name]
        cells.append("%s %.3f ms (rounds %.3f .. %.3f)" % (name, statistics.median(v), min(v), max(v)))
    a, b = (statistics.median(per_round[name]) for name, _ in setters)
    say("%-44s %s   %s   ratio %.3f%s" % (label, cells[0], cells[1], b / a, "" if groups[0] is None else "   groups %d" % groups[0]))


def main():
    import subprocess
    box = subprocess.run(["bash", "-c", "(rocminfo 2>/dev/null | grep -m1 -E 'Marketing Name:.*(Instinct|MI3)' || echo) ; uname -r"], capture_output=True, text=True).stdout.split("\n")
    say("attn.shared_prefix 0 against 128: ms per tgx_decode_rows step, Llama-3.2-1B bf16 (16 layers, synthetic weights), paged cache, every row at context ~%d (the last case: ~%d)" % (PROMPT, LONG))
    say("box: %s | kernel %s | %s" % (box[0].strip() or "unknown GPU", box[1].strip() if len(box) > 1 else "?", time.strftime("%Y-%m-%d")))
    say("region = %d warm-up + %d timed steps; %d rounds, settings in the order 0, 128, 128, 0 within a round; median of the rounds' medians" % (args.warmup, args.steps, args.rounds))
    m = context()

    def setting(v):
        def select():
            m.set_option("attn.shared_prefix", v)
            return m
        return select
    # (the 32-row case last: tgx_reset_cache keeps the batch's row count, and rows that are not refilled hold no token)
    for label, n_prompts, per, shared, total in (("8 rows, one 2048-token prompt", 1, 8, PROMPT, PROMPT), ("8 rows sharing 256 of 2048 tokens", 1, 8, 256, PROMPT),
                                                 ("8 rows, one 8192-token prompt", 1, 8, LONG, LONG), ("32 rows, four 2048-token prompts", 4, 8, PROMPT, PROMPT)):
        forked(m, n_prompts, per, shared, total)
        take_turns(label, [("off", setting(0)), ("128", setting(128))])
    if args.parent_lib:
        m.set_option("attn.shared_prefix", 0)
        p = context(Backend(args.parent_lib, "tgx_", required=list(ABI)))
        forked(m, 4, 8); forked(p, 4, 8)
        take_turns("option off, 32 rows: parent library / this one", [("parent", lambda: p), ("this", lambda: m)])
        p.close()
    m.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


main()
