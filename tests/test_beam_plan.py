"""The planner of tgx_beam_advance (tinygpt_amd/csrc/beam_plan.h) and the KvPool calls the entry point makes, without a GPU: tests/beam_plan_check.cpp, a
stand-alone program, audits them under the address and undefined-behaviour sanitizers — the pinned placement on hand-written cases (1 -> 4 from a fresh prefill, the
identity, a permutation with a repeated parent, all children of one parent, a shrink and the regrowth through retired rows) and on random groups against a
restatement of the rule, the blocks taken and given back against a KvPool driven beside the planner with KvPool::check after every plan, the one-entry-per-index
changes list, and every refusal (a refusal leaves the pool as it was)."""
import subprocess

from tinygpt_amd import build


def test_beam_plan_check():
    exe = build.build_beam_plan_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "beam_plan_check: ok" in r.stdout
