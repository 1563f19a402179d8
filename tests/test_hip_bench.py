"""bench.py's plain run (the headline figure only) and --dump-outputs: the line carries the timed decode and nothing measured by --full, and the
dumped arrays are what the timed call computed — K greedy ids, and the last step's logits whose argmax is the last id."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    steps = 8
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "qwen2.5-0.5b", "--prompt", "16", "--steps", str(steps),
           "--warmup", "2", "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == 2 and line["unit"] == "tokens/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["full"] is False
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) / line["value"] < 1e-3
    assert line["roofline"] is None and line["cpu_baseline"] is None and "prefill_ms" not in line["config"]

    toks = np.load(tmp_path / "out" / "tokens.npy")
    logits = np.load(tmp_path / "out" / "logits.npy")
    assert toks.dtype == np.float64 and toks.shape == (steps, 1)
    assert logits.dtype == np.float32 and logits.shape == (1, 151936)
    assert (toks == np.round(toks)).all() and (toks >= 0).all() and (toks < logits.shape[1]).all()
    assert np.isfinite(logits).all()
    assert int(np.argmax(logits[0])) == int(toks[-1, 0])          # greedy: the last timed step sampled the argmax of its own logits
