"""GPTConfig::speculate on a batch (host/engine.cpp): when the device shim exports tgx_verify_rows, generateSync on several prompts advances every unfinished row
through one tgx_verify_rows call per iteration — its own prompt-lookup draft (host/spec_draft.h), or none.  The ids are those of the plain batch loop, greedy
and under GPTConfig::speculateSampled; verify passes are known to have run (SpecStats).  tgx_cli --speculate with two prompts prints the plain run's text."""
import subprocess

import pytest

from conftest import load_golden
from test_hip_verify_sampled import SPEC_PROMPT, spec_engine, stats
from tinygpt_amd import build

pytestmark = pytest.mark.gpu
# three prompts of one length (no padding enters the comparison): the repeated span of SPEC_PROMPT, the same span shifted, and a prompt without a repeat (no draft
# until the generation itself repeats)
PROMPTS = [SPEC_PROMPT, SPEC_PROMPT[3:] + SPEC_PROMPT[:3], [21 + 3 * i for i in range(len(SPEC_PROMPT))]]


@pytest.mark.parametrize("sampled", [0, 1])
def test_host_engine_speculate_on_a_batch_equals_plain(tmp_path, sampled, oracle_lib):
    e, lib, vocab = spec_engine(tmp_path)
    n_new = 24
    sampler = dict(temperature=0.8, top_p=0.9) if sampled else {}
    runs = {}
    for spec in (0, 7):
        lib.tgxe_set_speculate(e.h, spec)
        lib.tgxe_set_speculate_sampled(e.h, sampled)
        e.reconfigure(max_new=n_new, **sampler)
        ids, new, fin = e.generate_sync(PROMPTS)
        runs[spec] = (ids.tolist(), new, fin)
        if spec == 0:
            assert stats(e) == [0] * 21
    assert runs[0] == runs[7], (runs[0], runs[7])
    s = stats(e)
    assert s[0] >= 1, s                                                   # SpecStats.verifyCalls: joint passes with a draft ran
    assert s[1] >= 1, s                                                   # ... and carried draft tokens
    e.close()


def test_cli_speculate_with_two_prompts(tmp_path):
    from host_util import write_model_dir
    cfg, g = load_golden("llama_tiny")
    cfg = dict(cfg, tie_word_embeddings=False)
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]), peaked=True)
    _, cli = build.build_host()
    two = ";".join(",".join(str(t) for t in p) for p in PROMPTS[:2])
    base = [cli, "--model", str(tmp_path), "--device", "mi355x", "--dtype", "bf16", "--max-tokens", "24", "--temperature", "0", "--top-p", "1", "--prompt-ids", two]
    outs = []
    for extra in ([], ["--speculate", "7"]):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        outs.append(out.stdout)
    rows = [[l for l in o.splitlines() if l.startswith("Output ids:")] for o in outs]
    assert rows[0] == rows[1] and len(rows[0]) == 2, rows
    line = [l for l in outs[1].splitlines() if l.startswith("speculate:")][0].split()
    assert int(line[1]) >= 1, line                                        # "speculate: N verify passes, ..."
