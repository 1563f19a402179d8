"""The mixed attention's work-list builder (tinygpt_amd/csrc/attn_worklist.h; tgx_advance_rows) without a GPU: tests/attn_worklist_check.cpp, a stand-alone
program, audits it under the address and undefined-behaviour sanitizers — the pass of test_hip_advance_rows.py's first test at tile targets 0 / 1 / 3 (at 0 item
for item the list of tgx_forward_rows' ragged pass), the 32-split cap, the automatic target, and a random run (n <= 8, lens 1..600, pasts 0..900, heads 1..4,
targets 0..9) against a naive model: every key tile a query block's causal range needs covered exactly once, <= 32 splits per block, heaviest first, partial
slots distinct and inside the reported size."""
import subprocess

from tinygpt_amd import build


def test_attn_worklist_check():
    exe = build.build_attn_worklist_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "attn_worklist_check: ok" in r.stdout
