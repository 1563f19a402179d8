"""GPTConfig::speculateTree in the host engine and tgx_cli --speculate-tree (host/engine.h; include/tgx.h tgx_verify_tree): with speculate = 7 and 3 branches the
ids and callbacks are those of speculate = 0, greedy and under the CLI's default sampler, and tree passes are known to have run (tgxe_spec_tree_passes, the CLI's
speculate-tree line).  The drafter looks at the sequence INCLUDING the tokens generated so far, so a tree needs generated text whose tail has been continued in
different ways before.  The prompt is 22 tokens over an alphabet of 6 (rng seed 14 of a search over such prompts): on the CPU oracle, whose greedy and T 0.8 /
top-p 0.9 generations of this peaked checkpoint coincide, the engine's loop restated over the generated ids (tgxh_ngram_tree, the draft walked against the ids)
runs 14 tree passes, 5 chain passes and 2 plain steps per generate call; the test asks for at least one per call."""
import subprocess
from ctypes import POINTER, c_int, c_int64, c_void_p

import pytest

from conftest import load_golden
from tinygpt_amd import build

pytestmark = pytest.mark.gpu
TREE_PROMPT = [204, 176, 24, 176, 24, 24, 91, 24, 204, 162, 24, 162, 176, 176, 204, 24, 24, 24, 91, 162, 204, 176]


def tree_engine(tmp_path):
    from host_util import HostEngine, host_lib, write_model_dir
    cfg, g = load_golden("llama_tiny")
    cfg = dict(cfg, tie_word_embeddings=False)
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]), peaked=True, eos=[cfg["vocab_size"] - 1])
    lib = host_lib()
    lib.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    lib.tgxe_set_speculate_sampled.argtypes = [c_void_p, c_int]
    lib.tgxe_set_speculate_tree.argtypes = [c_void_p, c_int]
    lib.tgxe_spec_tree_passes.restype = c_int64
    lib.tgxe_spec_tree_passes.argtypes = [c_void_p]
    lib.tgxe_spec_stats.restype = c_int
    lib.tgxe_spec_stats.argtypes = [c_void_p, POINTER(c_int64), c_int]
    e = HostEngine(lib, model_dir=str(tmp_path), device="mi355x", dtype=1)
    assert e.prepare(), e.error()
    return e, lib


def stats(e):
    buf = (c_int64 * 32)()
    e.lib.tgxe_spec_stats(e.h, buf, 32)
    return list(buf[:21])


@pytest.mark.parametrize("sampled", [0, 1])
def test_host_engine_speculate_tree_equals_plain(tmp_path, sampled):
    e, lib = tree_engine(tmp_path)
    n_new = 40
    sampler = dict(temperature=0.8, top_p=0.9) if sampled else {}
    lib.tgxe_set_speculate_sampled(e.h, sampled)
    runs = {}
    for spec, branches in ((0, 0), (7, 0), (7, 3)):
        lib.tgxe_set_speculate(e.h, spec)
        lib.tgxe_set_speculate_tree(e.h, branches)
        e.reconfigure(max_new=n_new, **sampler)
        ids, new, fin = e.generate_sync([TREE_PROMPT])
        e.reconfigure(max_new=n_new, **sampler)
        aids, anew, afin, seen = e.generate_async(TREE_PROMPT)
        runs[(spec, branches)] = (ids.tolist(), new, fin, aids.tolist(), anew, afin, seen)
        if branches == 0:
            assert lib.tgxe_spec_tree_passes(e.h) == 0                    # off: no tree pass, whatever speculate says
    assert runs[(0, 0)] == runs[(7, 0)] == runs[(7, 3)]
    assert lib.tgxe_spec_tree_passes(e.h) >= 2, (lib.tgxe_spec_tree_passes(e.h), stats(e))      # both generate calls ran at least one tree pass
    assert stats(e)[0] >= lib.tgxe_spec_tree_passes(e.h)                  # ... which count among the verify passes
    # an extra stop id that the generation produces: Stop at that token on both paths, the same callbacks
    gen = runs[(0, 0)][3][len(TREE_PROMPT):]
    stop = gen[len(gen) // 2]
    res = []
    for spec, branches in ((0, 0), (7, 3)):
        lib.tgxe_set_speculate(e.h, spec)
        lib.tgxe_set_speculate_tree(e.h, branches)
        e.reconfigure(max_new=n_new, extra_stop=[stop], **sampler)
        aids, anew, afin, seen = e.generate_async(TREE_PROMPT)
        res.append((aids.tolist(), anew, afin, seen))
    assert res[0] == res[1] and res[0][2] == "stop"
    e.close()


@pytest.mark.parametrize("sampled", [0, 1])
def test_cli_speculate_tree_equals_plain(tmp_path, sampled):
    from host_util import write_model_dir
    cfg, g = load_golden("llama_tiny")
    cfg = dict(cfg, tie_word_embeddings=False)
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]), peaked=True)
    _, cli = build.build_host()
    sampler = ["--temperature", "0.8", "--top-p", "0.9", "--speculate-sampled"] if sampled else ["--temperature", "0", "--top-p", "1"]
    base = [cli, "--model", str(tmp_path), "--device", "mi355x", "--dtype", "bf16", "--max-tokens", "40", "--prompt-ids", ",".join(str(t) for t in TREE_PROMPT)] + sampler
    outs = []
    for extra in ([], ["--speculate", "7", "--speculate-tree", "3"]):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        outs.append(out.stdout)
    rows = [[l for l in o.splitlines() if l.startswith("Output ids:")] for o in outs]
    assert rows[0] == rows[1] and len(rows[0]) == 1
    assert "speculate-tree:" not in outs[0]
    line = [l for l in outs[1].splitlines() if l.startswith("speculate-tree:")][0].split()
    assert int(line[1]) >= 1, line                                        # "speculate-tree: N of the verify passes ran a tree ..."
