#!/usr/bin/env python3
"""Bit identity of the continuation calls (include/tgx.h: tgx_extend_row, tgx_score_row on a held row, tgx_verify_row, tgx_verify_row_sampled, tgx_verify_rows,
tgx_advance_rows) between this build and another library of the same ABI — the parent commit's, when the calls' host side is refactored.

One seeded script per configuration: Llama-3.2-1B bf16 with synthetic weights, on slabs and with kv.budget_tokens and extend.attn_splits set (the skinny and tiled routes, the key-split and
the mixed attention), and the gpt2_hd64 fixture's geometry in fp32, as it is and with prefill.mfma 0 (the fp32 and by-steps routes; the row-by-row and piecewise forms: *.last_form 2).  The script runs twice, each
time on a fresh context — the first pass finds the token row 3 produces in the tgx_verify_rows call, the second sets it as that row's stop id — and calls: extend_row of 3, 8 and a
long run of ids; score_row on a held row, short and long; verify_row; verify_row_sampled; verify_rows with greedy and sampled rows, a row without a draft, a row recording
log-probabilities and the row with the stop id; a decode step with that row retired; advance_rows with two STEPs, a FEED, a FEED_MORE into a new row and a FEED into
the retired row; the closing FEED; four decode_rows steps.  After every call it dumps the returned ids and finish flags, the pass logits, every row's logits, the
lengths, kv.free_tokens, the log-probability ring of the recording row and the *.last_* options.

    python tools/continuation_identity.py [--parent-lib PATH] [--out FILE]

With --parent-lib the same script runs on that library beside this build's and every dumped array is compared byte for byte (exit status 1 on a difference).
Without it the digest of the dump is printed, for a comparison across processes."""
import argparse, copy, hashlib, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from tinygpt_amd import known_desc, synth
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import ABI, ADV_FEED, ADV_FEED_MORE, ADV_STEP, GREEDY, Backend, Model, SamplerCfg, TgxError, product_backend

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default="", help="a libtgx_mi355x.so of the parent commit, run beside this build's")
ap.add_argument("--out", default="", help="append the verdict lines to this file")
args = ap.parse_args()

SAMPLED = SamplerCfg(0.8, 0, 0.9, 0.0)
OPTIONS = ["verify.last_form", "verify.last_splits", "advance.last_form", "advance.last_tiles", "score.last_form"]
B = 6


def llama(be, budget):
    d = copy.deepcopy(known_desc("llama-3.2-1b", "bf16"))
    d.max_batch, d.max_ctx = B, 1024
    m = Model(d, be)
    if budget:
        m.set_option("kv.budget_tokens", budget)
    m.load_synthetic(1234, 0.02).finalize()
    if budget:
        m.set_option("extend.attn_splits", 4)      # the key-split attention at these short contexts as well (verify.last_splits > 0)
    return m, dict(prompts=(40, 63, 129, 200), long=200, feed=20, more=50, admit=140)


def gpt2_fp32(be, mfma):
    with open(os.path.join(ROOT, "tests", "golden", "gpt2_hd64", "config.json")) as f:
        cfg = json.load(f)
    d = desc_from_hf_config(dict(cfg, n_positions=256, n_ctx=256), "fp32", max_batch=B)      # (the fixture has 64 learned positions; synthetic weights)
    d.max_ctx = 256
    m = Model(d, be).load_synthetic(1234, 0.02).finalize()
    m.set_option("prefill.mfma", mfma)
    return m, dict(prompts=(20, 21, 33, 40), long=40, feed=9, more=17, admit=30)


def script(m, sz, stop_tok, dump):
    """one pass of the script on a fresh context; returns the token row 3 produced in the verify_rows call"""
    V = m.desc.vocab
    ids = lambda n, seed: [int(t) for t in synth.synth_prompt(V, n, seed)]
    recorded = [0]

    def snap(what, got=None):
        for k, (i, f) in enumerate(got or []):
            dump(f"{what} ids[{k}]", np.asarray(i, np.int64)); dump(f"{what} finish[{k}]", np.asarray([f], np.int32))
        try:
            dump(f"{what} pass_logits", m.pass_logits())
        except TgxError:
            dump(f"{what} pass_logits", np.zeros(0, np.float32))
        dump(f"{what} logits", m.logits(rounded=False))
        dump(f"{what} state", np.asarray([m.past_length_row(r) for r in range(B)] + [m.get_option("kv.free_tokens")] + [m.get_option(o) for o in OPTIONS], np.int64))
        for n in range(min(recorded[0], 16), 0, -1):      # the ring's last records, as many of them as it holds
            try:
                ring = m.row_logprobs(2, n)
            except TgxError:
                continue
            for k, a in enumerate(ring):
                dump(f"{what} logprobs[{k}]", a)
            break

    cfgs = [(GREEDY, 0), (SAMPLED, 977), (GREEDY, 0), (GREEDY, 0)]
    for r, p in enumerate(sz["prompts"]):
        m.forward_row(r, synth.synth_prompt(V, p, 1 + r))
    for r, (cfg, seed) in enumerate(cfgs):
        m.set_row_sampler(r, cfg, seed); m.set_row_stop(r, 0, []); m.set_row_logprobs(r, 3 if r == 2 else -1)
    for r, (cfg, seed) in enumerate(cfgs):
        m.sample_row(r, cfg, seed)
    recorded[0] = 1
    snap("admitted")
    for n in (3, 8, sz["long"]):
        m.extend_row(0, ids(n, 20 + n)); snap(f"extend_row {n}")
    m.sample_row(0, GREEDY)
    for n in (12, sz["long"]):
        for k, a in enumerate(m.score_row(2, ids(n, 31), 2)):
            dump(f"score_row {n} [{k}]", a)
        snap(f"score_row {n}")
    m.sample_row(2, GREEDY); recorded[0] += 1
    snap("verify_row", [m.verify_row(0, ids(5, 41))])
    snap("verify_row_sampled", [m.verify_row_sampled(1, ids(7, 42))])
    if stop_tok is not None:
        m.set_row_stop(3, 0, [stop_tok])
    got = m.verify_rows([0, 1, 2, 3], [[], ids(7, 43), ids(3, 44), ids(2, 45)])
    recorded[0] += len(got[2][0])
    snap("verify_rows", got)
    tok3 = int(got[3][0][0])
    m.reset_row(3)                                   # retired: it rides along the next step
    out = m.decode_rows(1); recorded[0] += 1
    for k, a in enumerate(out):
        dump(f"step with row 3 retired [{k}]", a)
    got = m.advance_rows([2, 0, 4, 1, 3], [ADV_FEED, ADV_STEP, ADV_FEED_MORE, ADV_STEP, ADV_FEED], [ids(sz["feed"], 51), ids(2, 52), ids(sz["more"], 53), ids(4, 54), ids(sz["admit"], 55)])
    snap("advance_rows", got)
    got = m.advance_rows([4, 0], [ADV_FEED, ADV_STEP], [ids(5, 56), []])
    snap("advance_rows, the closing feed", got)
    for r in (2, 3, 4):
        m.sample_row(r, GREEDY)
    recorded[0] += 1
    out = m.decode_rows(4); recorded[0] += 4
    for k, a in enumerate(out):
        dump(f"decode_rows [{k}]", a)
    snap("decode_rows")
    return tok3


def run(be, make, budget):
    arrays, tok3 = [], None
    for n in (1, 2):
        m, sz = make(be, budget)
        tok3 = script(m, sz, tok3, lambda name, a: arrays.append((f"pass {n}: {name}", np.ascontiguousarray(a).copy())))
        m.close()
    return arrays


lines, bad = [], 0
mine = product_backend()
parent = Backend(args.parent_lib, "tgx_", required=[n for n in ABI if n != "verify_tree"]) if args.parent_lib else None      # (the parent commit has no tgx_verify_tree)
for name, make, budget in (("Llama-3.2-1B bf16, slabs", llama, 0), ("Llama-3.2-1B bf16, kv.budget_tokens 4096, extend.attn_splits 4", llama, 4096), ("gpt2_hd64 geometry fp32", gpt2_fp32, 1), ("gpt2_hd64 geometry fp32, prefill.mfma 0", gpt2_fp32, 0)):
    a = run(mine, make, budget)
    h = hashlib.sha256()
    for what, x in a:
        h.update(what.encode()); h.update(str((x.dtype, x.shape)).encode()); h.update(x.tobytes())
    forms = sorted({tuple(int(v) for v in x[B + 1:]) for what, x in a if what.endswith(" state")})
    line = f"{name}: {len(a)} arrays, sha256 {h.hexdigest()[:16]}; (verify form, splits, advance form, tiles, score form) seen: {forms}"
    if parent:
        b = run(parent, make, budget)
        diff = [wa for (wa, xa), (wb, xb) in zip(a, b) if wa != wb or xa.dtype != xb.dtype or xa.shape != xb.shape or xa.tobytes() != xb.tobytes()]
        if len(a) != len(b):
            diff.append(f"{len(a)} arrays against the parent's {len(b)}")
        bad += len(diff)
        line += "; against the parent library: " + ("every array equal byte for byte" if not diff else f"{len(diff)} DIFFER: {diff[:8]}")
    print(line, flush=True)
    lines.append(line)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
