"""The planner of tgx_splice_row (tinygpt_amd/csrc/splice_plan.h) and the KvPool calls the entry point makes, without a GPU: tests/splice_plan_check.cpp, a
stand-alone program, audits them under the address and undefined-behaviour sanitizers — the shapes of tests/test_hip_splice_row.py alone and beside a forked
sibling, touching ranges merged, every refusal, the truncation and no-op forms against tgx_truncate_row's pool, copy on write with and without a free block, and
a random run against a naive model (rows as vectors of token tags read back through the block tables)."""
import subprocess

from tinygpt_amd import build


def test_splice_plan_check():
    exe = build.build_splice_plan_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "splice_plan_check: ok" in r.stdout
