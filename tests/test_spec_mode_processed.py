"""SpecInputs::verifyProcessed (tinygpt_amd/host/spec_mode.h; GPTConfig::speculateProcessed) on a CPU, under the address and undefined-behaviour sanitizers
(tests/spec_mode_processed_check.cpp): every input the function saw before the field existed gives the old answer, and processors with verifyProcessed set follow
the greedy, sampled and rows rules."""
import subprocess

from tinygpt_amd import build


def test_spec_mode_processed_check_under_sanitizers():
    exe = build.build_spec_mode_processed_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spec_mode_processed_check: ok" in r.stdout
