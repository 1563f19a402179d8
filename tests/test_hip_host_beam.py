"""Beam search in the host engine (tinygpt_amd/host/engine.h GPTConfig::numBeams; host/beam.h the rules): generateSync with numBeams 4 returns the ids and scores of
the same search driven from Python through ffi — the same calls, kernels and batch sizes, so bit for bit; numBeams 1 is the greedy loop it always was; under a
regex every returned text matches; every configuration the header refuses fails with its message; tgx_cli --num-beams 4 --num-return 2 prints two texts."""
import ctypes
import subprocess
from ctypes import POINTER, c_double, c_float, c_int, c_void_p

import numpy as np
import pytest

from conftest import load_golden
from host_util import HostEngine, host_lib, write_model_dir
from test_beam_host import Scorer
from tinygpt_amd import build
from tinygpt_amd.ffi import Model, product_backend

pytestmark = pytest.mark.gpu

SEED, STD, EOS = 1234, 0.05, 255
PROMPT = [5, 9, 17, 5, 9, 17, 5, 9, 17, 5, 9]


@pytest.fixture(scope="module")
def lib():
    h = host_lib()
    h.tgxe_set_beams.argtypes = [c_void_p, c_int, c_float, c_int, c_int]
    h.tgxe_last_beam_scores.argtypes = [c_void_p, POINTER(c_double), c_int]
    h.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    h.tgxe_set_logprobs.argtypes = [c_void_p, c_int]
    h.tgxe_set_context_shift.argtypes = [c_void_p, c_int, c_int]
    h.tgxe_set_regex.argtypes = [c_void_p, ctypes.c_char_p]
    return h


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    cfg, _ = load_golden("llama_tiny")
    path = str(tmp_path_factory.mktemp("beam") / "llama_tiny")
    return path, write_model_dir(path, cfg, SEED, STD, eos=EOS)


def beam_scores(lib, e):
    buf = (c_double * 8)()
    n = lib.tgxe_last_beam_scores(e.h, buf, 8)
    return list(buf[:n])


def python_search(m, prompt, K, lp, early, max_new, ends):
    """the engine's loop through ffi: prefill, select with n = 1, advance 1 -> K, then tgx_decode_rows(1) + select + advance per step"""
    m.reset_cache()
    m.forward_row(0, prompt)
    sc = Scorer(K, lp, early, max_new, ends)
    rows, group = [0], list(range(K))
    for step in range(max_new + 1):
        beam, tok, score, lpv = m.beam_select(rows, sc.scores, K, ends)
        sc.step(list(zip(beam.tolist(), tok.tolist(), score.tolist(), lpv.tolist())))
        if sc.done:
            break
        rows = m.beam_advance(rows if step else group, sc.parents, sc.tokens).tolist()
        m.decode_rows(1)
    return sorted(sc.kept, key=lambda h: (-h["score"], h["order"]))


@pytest.mark.parametrize("lp,early,max_new", [(1.0, False, 8), (0.0, True, 6), (2.0, False, 5)])
def test_engine_equals_the_search_driven_through_ffi(lib, model_dir, lp, early, max_new):
    path, d = model_dir
    K = 4
    e = HostEngine(lib, model_dir=path, max_batch=K)
    assert e.prepare(), e.error()
    assert e.eos_ids() == [EOS]
    e.reconfigure(max_new=max_new)
    plain, _, _ = e.generate_sync([PROMPT])
    lib.tgxe_set_beams(e.h, K, lp, int(early), K)
    e.reconfigure(max_new=max_new)
    got, new, fin = e.generate_sync([PROMPT], pad=0)
    scores = beam_scores(lib, e)
    d.max_batch = K
    m = Model(d, product_backend()).load_synthetic(SEED, STD).finalize()
    want = python_search(m, PROMPT, K, lp, early, max_new, [EOS])
    got = got.reshape(len(want), -1)
    S = len(PROMPT)
    assert new == max_new and got.shape == (len(want), S + max_new) and len(scores) == len(want)
    for b, h in enumerate(want):
        np.testing.assert_array_equal(got[b, :S], PROMPT)
        np.testing.assert_array_equal(got[b, S:], h["tokens"] + [0] * (max_new - len(h["tokens"])), err_msg=str(b))
        assert scores[b] == h["score"], (b, scores[b], h["score"])
    assert fin == ("length" if want[0]["length"] else "stop")
    assert scores == sorted(scores, reverse=True)
    # numBeams 1: the loop it always was
    lib.tgxe_set_beams(e.h, 1, 1.0, 0, 1)
    e.reconfigure(max_new=max_new)
    again, _, _ = e.generate_sync([PROMPT])
    np.testing.assert_array_equal(again, plain)
    assert beam_scores(lib, e) == []
    m.close(); e.close()


def refused(lib, e, prompts, needle):
    flat = np.concatenate([np.asarray(p, np.int32) for p in prompts])
    lens = np.asarray([len(p) for p in prompts], np.int32)
    out = np.zeros(1 << 12, np.int32)
    n, new, fin = ctypes.c_int64(), ctypes.c_int64(), c_int()
    rc = lib.tgxe_generate_sync(e.h, flat.ctypes.data_as(POINTER(ctypes.c_int32)), lens.ctypes.data_as(POINTER(ctypes.c_int32)), len(prompts), 0,
                                out.ctypes.data_as(POINTER(ctypes.c_int32)), len(out), ctypes.byref(n), ctypes.byref(new), ctypes.byref(fin))
    assert rc == 1 and needle in e.error(), (rc, e.error())


def test_refused_configurations_fail_with_their_message(lib, model_dir):
    path, _ = model_dir
    e = HostEngine(lib, model_dir=path, max_batch=4)
    assert e.prepare(), e.error()
    lib.tgxe_set_beams(e.h, 4, 1.0, 0, 2)
    e.reconfigure(temperature=0.8, top_p=0.9, max_new=4)
    refused(lib, e, [PROMPT], "greedy sampler")
    e.reconfigure(max_new=4)
    refused(lib, e, [PROMPT, PROMPT], "one prompt")
    with pytest.raises(AssertionError, match="generateAsync"):
        e.generate_async(PROMPT)
    lib.tgxe_set_speculate(e.h, 4)
    refused(lib, e, [PROMPT], "does not combine")
    lib.tgxe_set_speculate(e.h, 0)
    lib.tgxe_set_logprobs(e.h, 0)
    refused(lib, e, [PROMPT], "does not combine")
    lib.tgxe_set_logprobs(e.h, -1)
    lib.tgxe_set_context_shift(e.h, 1, 0)
    refused(lib, e, [PROMPT], "does not combine")
    lib.tgxe_set_context_shift(e.h, 0, 0)
    e.reconfigure(max_new=4, extra_stop=list(range(100, 108)))      # 8 extra ids + the model's EOS
    refused(lib, e, [PROMPT], "EOS / stop ids")
    e.reconfigure(max_new=4)
    lib.tgxe_set_beams(e.h, 4, 1.0, 0, 5)
    refused(lib, e, [PROMPT], "numReturn")
    lib.tgxe_set_beams(e.h, 9, 1.0, 0, 1)
    refused(lib, e, [PROMPT], "TGX_MAX_BEAMS")
    lib.tgxe_set_beams(e.h, 4, 1.0, 0, 2)
    got, new, _ = e.generate_sync([PROMPT])                         # ... and the engine still serves what it can
    assert got.size == 2 * (len(PROMPT) + 4)
    e.close()
    small = HostEngine(lib, model_dir=path, max_batch=2)
    assert small.prepare(), small.error()
    lib.tgxe_set_beams(small.h, 4, 1.0, 0, 1)
    small.reconfigure(max_new=4)
    refused(lib, small, [PROMPT], "maxBatch")
    small.close()


def test_regex_every_returned_text_matches(lib):
    from constraint_util import GPT2_DIR, fullmatch
    e = HostEngine(lib, synthetic="gpt2", tokenizer_dir=GPT2_DIR, max_batch=4)
    assert e.prepare(), e.error()
    for pat in ("(yes|no|maybe)", r"\d{2}-\d{2}"):
        lib.tgxe_set_regex(e.h, pat.encode())
        lib.tgxe_set_beams(e.h, 4, 1.0, 0, 3)
        e.reconfigure(max_new=12, extra_stop=[50256])
        ids, new, texts = e.generate_sync_text(["Answer:"])
        assert len(texts) == 3 and len(beam_scores(lib, e)) == 3
        for t in texts:
            assert fullmatch(pat, t.decode("utf-8")), (pat, t)
        rows = ids.reshape(3, -1)      # (hypotheses differ as token sequences; two tokenisations of one text are two hypotheses)
        assert len(set(tuple(r) for r in rows.tolist())) == 3
    e.close()


def test_cli_prints_two_texts():
    from constraint_util import GPT2_DIR
    _, cli = build.build_host()
    out = subprocess.run([cli, "--synthetic", "gpt2", "--tokenizer", GPT2_DIR, "--prompt", "The date:", "--num-beams", "4", "--num-return", "2", "--max-tokens", "6",
                          "--temperature", "0", "--top-p", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert sum(l.startswith("Output:") for l in lines) == 2, out.stdout
    scores = [float(l.split()[-1]) for l in lines if l.startswith("beam ")]
    assert len(scores) == 2 and scores[0] >= scores[1]
