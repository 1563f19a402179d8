#!/usr/bin/env python3
"""Cost of the sampler inside the decode step (one run with the CLI defaults T=0.8 / top-p 0.9):
ms/step greedy vs sampled configurations, Llama-3.2-1B, batch 1, context ~300."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import GREEDY, Model, SamplerCfg, product_backend
desc = known_desc(sys.argv[1] if len(sys.argv) > 1 else "llama-3.2-1b")
m = Model(desc, product_backend())
for name, bits in synth.synth_checkpoint(desc, 1234, 0.02):
    m.upload(name, bits)
m.finalize()
for kv in filter(None, os.environ.get("TGX_OPTS", "").split(";")):      # e.g. TGX_OPTS="sampler.one_pass=0"
    k, v = kv.split("="); m.set_option(k, int(v))
prompt = synth.synth_prompt(desc.vocab, 256, 1)[None, :]
CFGS = [("greedy", GREEDY), ("T=0.8 top-p 0.9 (CLI default)", SamplerCfg(temperature=0.8, top_p=0.9)),
        ("T=0.7 top-p 0.9 (server default)", SamplerCfg(temperature=0.7, top_p=0.9)),
        ("T=0.8 top-k 50", SamplerCfg(temperature=0.8, top_k=50)), ("T=1.0 min-p 0.05", SamplerCfg(temperature=1.0, min_p=0.05)),
        ("T=0.8 top-k 50 top-p 0.9 min-p 0.05", SamplerCfg(temperature=0.8, top_k=50, top_p=0.9, min_p=0.05)), ("T=1.0 only", SamplerCfg(temperature=1.0))]
best = {}
for rep in range(4):            # the configurations alternate (the clock the power manager grants drifts over a run): best of four per configuration
    for label, cfg in CFGS:
        # an untimed pass over the same contexts first: a context that crosses an attention-form limit captures a new step graph (~2.5 ms), and seven
        # configurations x two forms thrash the six-entry graph cache — inside the timed region that read as +20 us per step for whoever paid it
        m.reset_cache(); m.forward(prompt); m.sample(cfg, seed=1); m.decode(16 + 128, cfg, seed=1, fetch=False); m.synchronize()
        m.reset_cache(); m.forward(prompt); m.sample(cfg, seed=1)
        m.decode(16, cfg, seed=1, fetch=False); m.synchronize()
        t0 = time.perf_counter(); m.decode(128, cfg, seed=1, fetch=False); m.synchronize(); dt = (time.perf_counter() - t0) / 128
        best[label] = min(best.get(label, 1e9), dt)
LP_LEGS = []
# the log-probability records (tgx_set_row_logprobs) ride behind a step's publish: tgx_decode_rows greedy with logprobs off / top_n 0 / 5 / 20
for rep in range(4):
    for top_n in (-1, 0, 5, 20):
        # (an untimed pass over the same contexts first, as above: the timed region captures no graph)
        m.reset_cache(); m.forward(prompt); m.set_row_logprobs(0, top_n); m.sample_row(0); m.decode_rows(16 + 128); m.synchronize()
        m.reset_cache(); m.forward(prompt); m.set_row_logprobs(0, top_n); m.sample_row(0)
        m.decode_rows(16); m.synchronize()
        t0 = time.perf_counter(); m.decode_rows(128); m.synchronize(); dt = (time.perf_counter() - t0) / 128
        label = "decode_rows greedy, logprobs " + ("off" if top_n < 0 else f"top_n {top_n}")
        best[label] = min(best.get(label, 1e9), dt)
        if rep == 0: LP_LEGS.append(label)
base = best["greedy"]
for label, _ in CFGS:
    dt = best[label]
    print(f"{label:40s} {dt * 1e3:.4f} ms/step  {1 / dt:7.1f} tok/s  sampler adds {(dt - base) * 1e6:6.1f} us", flush=True)
base = best[LP_LEGS[0]]          # the records' cost is read against the same per-row step with every row off
for label in LP_LEGS:
    dt = best[label]
    print(f"{label:40s} {dt * 1e3:.4f} ms/step  {1 / dt:7.1f} tok/s  logprobs add {(dt - base) * 1e6:6.1f} us", flush=True)
