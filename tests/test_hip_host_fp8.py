"""GPTConfig::weightsFp8 on the GPU: the host engine (C view, tgxe_create3) and the CLI's --weights-fp8 produce the ids of a Model with option weights.fp8 set —
and not those of the unquantized model, where the two differ."""
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from fp8_host_util import Fp8Engine
from host_util import host_lib, write_model_dir
from tinygpt_amd import build, known_desc
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, PRODUCT_LIB, Model, product_backend

pytestmark = pytest.mark.gpu
PROMPT = [5, 6, 7, 8, 9]


def model_ids(d, seed, std, fp8, prompt, n):
    m = Model(d, product_backend())
    m.set_option("weights.fp8", fp8)
    m.load_synthetic(seed, std).finalize()
    assert m.get_option("weights.fp8_matrices") == (2 * d.layers + 1 if fp8 else 0)
    m.forward(np.asarray(prompt)[None, :])
    ids = [int(m.sample(GREEDY)[0])] + [int(t) for t in m.decode(n - 1, GREEDY)[:, 0]]
    m.close()
    return ids


def test_engine_with_the_flag_gives_the_quantized_models_ids(tmp_path):
    cfg, g = load_golden("llama_tiny")
    seed, std = int(g["seed"]), float(g["std"])
    write_model_dir(str(tmp_path), cfg, seed, std)
    d = desc_from_hf_config(cfg, "bf16", max_batch=4)
    n = 12
    want = {fp8: model_ids(d, seed, std, fp8, g["prompt"][0], n) for fp8 in (0, 1)}
    for fp8 in (0, 1):
        e = Fp8Engine(host_lib(), fp8, model_dir=str(tmp_path), dtype=1)
        assert e.prepare(), e.error()
        e.reconfigure(max_new=n)
        ids, new, fin = e.generate_sync([g["prompt"][0]])
        assert list(ids[0, g["prompt"].shape[1]:]) == want[fp8]
        e.close()


def test_an_unsupported_dtype_fails_prepare(tmp_path):
    cfg, g = load_golden("llama_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    e = Fp8Engine(host_lib(), 1, model_dir=str(tmp_path), dtype=2)      # fp16 storage
    assert not e.prepare() and "weights.fp8" in e.error()
    e.close()


def test_cli_weights_fp8_gives_the_ids_of_model_with_the_option():
    _, cli = build.build_host(test_hooks=True)       # tgx_cli_test: bound to the product library by name
    n = 8
    out = subprocess.run([cli, "--synthetic", "qwen2.5-0.5b", "--backend-lib", PRODUCT_LIB, "--backend-prefix", "tgx_", "--weights-fp8", "--max-tokens", str(n),
                          "--temperature", "0", "--top-p", "1", "--prompt-ids", ",".join(map(str, PROMPT))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = [[int(t) for t in l.split(":")[1].split()] for l in out.stdout.splitlines() if l.startswith("Output ids:")]
    assert len(rows) == 1
    d = known_desc("qwen2.5-0.5b", "bf16", max_batch=4)
    assert rows[0] == model_ids(d, 1234, 0.02, 1, PROMPT, n)
