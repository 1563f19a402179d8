"""The owner of a context's device allocations (tinygpt_amd/csrc/dev_mem.h) without a GPU: tests/dev_mem_check.cpp, a stand-alone program, binds it to a counting
malloc / free pair under the address and undefined-behaviour sanitizers — a scripted case for each rule of grow, release(nullptr), release_all, and a random run
of alloc / release / grow with injected allocation failures against a naive model.  LeakSanitizer at exit is part of the verdict."""
import subprocess

from tinygpt_amd import build


def test_dev_mem_check():
    exe = build.build_dev_mem_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "dev_mem_check: ok" in r.stdout
