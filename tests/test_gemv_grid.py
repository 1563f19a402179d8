"""The grid arithmetic of the batch-1..4 GEMV launches (tinygpt_amd/csrc/gemv_grid.h) without a GPU: tests/gemv_grid_check.cpp, a stand-alone program, audits
it under the address and undefined-behaviour sanitizers over every units in 1..70000, units per workgroup in {1, 2, 4} and cap in {256, 512, 768, 1024}."""
import subprocess

from tinygpt_amd import build


def test_gemv_grid_check():
    exe = build.build_gemv_grid_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "gemv_grid_check: ok" in r.stdout
