"""The byte format of a row snapshot (tinygpt_amd/csrc/row_snapshot.h; include/tgx.h tgx_save_row / tgx_restore_row) without a GPU: tests/row_snapshot_check.cpp, a
stand-alone program under the address and undefined-behaviour sanitizers — the 64-bit size formula against a naive sum on the released geometries (one beyond 2^32
bytes), a header round trip, every prefix of a valid snapshot refused, every single-field corruption refused with its status, and 20,000 random blobs that are never
read outside their buffer and never accepted unless every section is consistent."""
import subprocess

from tinygpt_amd import build


def test_row_snapshot_check():
    exe = build.build_row_snapshot_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "row_snapshot_check: ok" in r.stdout
