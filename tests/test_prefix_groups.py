"""The planner of the shared-prefix decode attention (tinygpt_amd/csrc/prefix_groups.h), without a GPU: tests/prefix_groups_check.cpp, a stand-alone program beside a
real KvPool under the address and undefined-behaviour sanitizers — the pinned grouping rules on hand-written pools, the cut at 32 / G rows, G = 9, the splits."""
import subprocess

from tinygpt_amd import build


def test_prefix_groups_check():
    r = subprocess.run([build.build_prefix_groups_check()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "" and "prefix_groups_check: ok" in r.stdout, r.stdout + r.stderr
