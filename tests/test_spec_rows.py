"""SpecInputs::verifyRows (tinygpt_amd/host/spec_mode.h) without a GPU: a stand-alone program under the address and undefined-behaviour sanitizers
(tests/spec_rows_check.cpp).  verifyRows false reproduces the table of tests/spec_mode_check.cpp for every input; verifyRows true lets a batch of several sequences
speculate exactly where one sequence does."""
import subprocess

from tinygpt_amd import build


def test_spec_rows_check_under_sanitizers():
    exe = build.build_spec_rows_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "spec_rows_check: ok" in r.stdout
