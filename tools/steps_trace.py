#!/usr/bin/env python3
"""The launches of a per-row decode step, for a kernel trace: Llama-3.2-1B, a 256-token prefill, every row's first token, then STEPS eager steps of
tgx_decode_rows with every row on its defaults (greedy, logprobs off).  The difference between two traces (STEPS 32 and 16) is 16 steps' launches.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/steps_trace.py STEPS BATCH [TREE]      (TREE: another checkout to import from)
"""
import dataclasses, os, sys
steps, B = int(sys.argv[1]), int(sys.argv[2])
tree = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
import numpy as np
import tinygpt_amd
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import Model, product_backend
assert os.path.abspath(tinygpt_amd.__file__).startswith(tree), tinygpt_amd.__file__
desc = dataclasses.replace(known_desc("llama-3.2-1b"), max_batch=B, max_ctx=512)
m = Model(desc, product_backend())
for name, bits in synth.synth_checkpoint(desc, 1234, 0.02):
    m.upload(name, bits)
m.finalize()
m.set_option("graph", 0)           # eager launches: the trace lists every kernel of a step (a captured step issues the same ones)
ids = np.stack([synth.synth_prompt(desc.vocab, 256, 77 + b) for b in range(B)])
m.forward(ids)
for b in range(B):
    m.sample_row(b)
out, new, fin = m.decode_rows(steps)
m.synchronize()
print("tree", tree, "steps", steps, "B", B, "last ids", out[-1][:4].tolist(), flush=True)
