"""The paged-KV block pool (tinygpt_amd/csrc/kv_pool.h) without a GPU: tests/kv_pool_check.cpp, a stand-alone program, audits it under the address and
undefined-behaviour sanitizers — scripted cases (the figures of test_hip_fork_row.py::test_block_accounting, the states the entry points cannot reach, truncation,
the table's end) and a random run against a naive model."""
import subprocess

from tinygpt_amd import build


def test_kv_pool_check():
    exe = build.build_kv_pool_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "kv_pool_check: ok" in r.stdout
