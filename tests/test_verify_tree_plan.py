"""The planner of tgx_verify_tree (tinygpt_amd/csrc/verify_tree_plan.h) without a GPU: tests/verify_tree_plan_check.cpp, a stand-alone program, audits it under the
address and undefined-behaviour sanitizers — depths, parent positions, the 16-bit ancestor-or-self masks, the chain test and the sibling-duplicate refusal of every
tree of up to 6 nodes and of random trees of 15 against a naive walk along the parent pointers, the shapes the GPU tests use, and every refusal."""
import subprocess

from tinygpt_amd import build


def test_verify_tree_plan_check():
    exe = build.build_verify_tree_plan_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "verify_tree_plan_check: ok" in r.stdout
