"""GPTEngine::saveSession / loadSession (tinygpt_amd/host/engine.h) and tgx_cli --session-save / --session-load: row 0's conversation cache written to a file (a small
header with the cached token ids, then the row's snapshot — include/tgx.h tgx_save_row) and restored by another process.  Through the C view, on a synthetic llama
cut with the gpt2 tokenizer fixture (peaked checkpoint: no greedy choice sits on a near-tie): engine X runs turn 1, saves and is destroyed, a fresh X loads and runs
turn 2; engine Y runs both turns in one process.  Both turn 2s are prefix-reuse runs on the extend route over the same cached prefix: the same ids, the same
tgxe_last_reused.  Files that cannot be loaded leave the engine as it was; the CLI prints the same text with and without a session file."""
import os
import subprocess
from ctypes import c_char_p, c_int, c_int64, c_void_p

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from host_util import HostEngine, host_lib, write_model_dir
from tinygpt_amd import build

pytestmark = pytest.mark.gpu

TOK = os.path.join(GOLDEN, "tokenizer", "gpt2")
TURN1 = "The capital of France is"
MORE = " And the capital of Spain is"


def bound_lib():
    lib = host_lib()
    lib.tgxe_set_reuse_prefix.argtypes = [c_void_p, c_int]
    lib.tgxe_set_reuse_prefix.restype = None
    lib.tgxe_last_reused.argtypes = [c_void_p]
    lib.tgxe_last_reused.restype = c_int64
    for fn in (lib.tgxe_save_session, lib.tgxe_load_session):
        fn.argtypes = [c_void_p, c_char_p]
        fn.restype = c_int
    return lib


def model_dir(path, fam):
    cfg, g = load_golden(fam)
    cfg = dict(cfg, vocab_size=50257, tie_word_embeddings=False)      # the tokenizer's vocabulary; an untied lm_head holds the peaked checkpoint's loud rows
    write_model_dir(str(path), cfg, int(g["seed"]), float(g["std"]), eos=50256, peaked=True)
    return str(path)


def engine(lib, mdir, reuse=1):
    e = HostEngine(lib, model_dir=mdir, tokenizer_dir=TOK, device="mi355x", dtype=1, max_batch=1)
    assert e.prepare(), e.error()
    lib.tgxe_set_reuse_prefix(e.h, reuse)
    return e


def turn(e, text, max_new=12):
    e.reconfigure(max_new=max_new)
    ids, new, fin, chunks = e.generate_async_text(text)
    return ids.copy(), new, fin, b"".join(chunks), int(e.lib.tgxe_last_reused(e.h))


def test_session_file_across_engines(tmp_path):
    lib = bound_lib()
    mdir = model_dir(tmp_path / "llama", "llama_tiny")
    path = str(tmp_path / "turn1.session").encode()
    # ---- turn 1: X saves and goes away; Y stays
    X, Y = engine(lib, mdir), engine(lib, mdir)
    (ix, nx, fx, tx, rx), (iy, ny, fy, ty, ry) = turn(X, TURN1), turn(Y, TURN1)
    np.testing.assert_array_equal(ix, iy)
    assert (nx, fx, tx, rx) == (ny, fy, ty, ry) and rx == 0
    assert lib.tgxe_save_session(X.h, path) == 0, X.error()
    X.close()
    blob = open(path, "rb").read()
    held = len(ix) - 1                                    # every position of the cache: the last token was never fed back
    assert blob[:8] == b"TGXSESS\0" and int.from_bytes(blob[12:16], "little") == held
    np.testing.assert_array_equal(np.frombuffer(blob, "<i4", held, 16), ix[:held])
    snap = blob[16 + 4 * held + 8:]
    assert snap[:8] == b"TGXSNAP\0" and int.from_bytes(snap[60:64], "little") == 0 and int.from_bytes(snap[64:72], "little") == held      # no logits in the file
    # ---- files that cannot be loaded
    other = engine(lib, model_dir(tmp_path / "mistral", "mistral_tiny"))
    turn(other, TURN1, max_new=4)
    other_path = str(tmp_path / "other.session").encode()
    assert lib.tgxe_save_session(other.h, other_path) == 0, other.error()
    other.close()
    cut_path = str(tmp_path / "cut.session").encode()
    open(cut_path, "wb").write(blob[:-100])
    short_path = str(tmp_path / "short.session").encode()
    open(short_path, "wb").write(blob[:40])
    bad = (cut_path, short_path, other_path, str(tmp_path / "missing.session").encode())
    # ---- a fresh X: the good file, then the bad ones (which leave it as it is), then turn 2
    text2 = TURN1 + tx.decode("utf-8", errors="replace") + MORE
    X = engine(lib, mdir)
    assert lib.tgxe_load_session(X.h, path) == 0, X.error()
    for p in bad:
        assert lib.tgxe_load_session(X.h, p) == 1 and X.error(), p
    (ix2, nx2, fx2, tx2, rx2), (iy2, ny2, fy2, ty2, ry2) = turn(X, text2), turn(Y, text2)
    print("turn 2: reused", rx2, ry2, "of a cache of", held, "positions; prompt", len(ix2) - nx2)
    np.testing.assert_array_equal(ix2, iy2)
    assert (nx2, fx2, tx2) == (ny2, fy2, ty2)
    assert rx2 == ry2 > len(ix) // 2
    # ---- an engine whose load failed serves turn 2 from scratch, and says so
    Z = engine(lib, mdir)
    noreuse = engine(lib, mdir, reuse=0)
    assert lib.tgxe_load_session(noreuse.h, path) == 1 and "reuse" in noreuse.error()
    for p in bad:
        assert lib.tgxe_load_session(Z.h, p) == 1 and Z.error(), p
    iz2, nz2, fz2, tz2, rz2 = turn(Z, text2)
    np.testing.assert_array_equal(iz2, iy2)
    assert (nz2, fz2, tz2, rz2) == (ny2, fy2, ty2, 0)
    # ---- a run that ends with the row finished on the device (speculation steps through the per-row calls) keeps no cache: nothing to save, and a message
    lib.tgxe_set_speculate.argtypes = [c_void_p, c_int]
    lib.tgxe_set_speculate.restype = None
    lib.tgxe_set_speculate(Z.h, 4)
    turn(Z, TURN1)
    assert lib.tgxe_save_session(Z.h, str(tmp_path / "spec.session").encode()) == 1 and "saveSession" in Z.error()
    assert not os.path.exists(tmp_path / "spec.session")
    for e in (X, Y, Z, noreuse):
        e.close()


def test_cli_session_flags(tmp_path):
    mdir = model_dir(tmp_path / "llama", "llama_tiny")
    _, cli = build.build_host()
    f = str(tmp_path / "cli.session")
    base = [cli, "--model", mdir, "--tokenizer", TOK, "--max-tokens", "12", "--temperature", "0", "--top-p", "1", "--prompt", TURN1]
    refused = subprocess.run(base + ["--session-save", f], capture_output=True, timeout=120)      # not the streaming path
    assert refused.returncode == 1 and b"--stream" in refused.stderr and not os.path.exists(f)
    refused = subprocess.run(base + ["--stream", "--session-save", f, "--speculate", "4"], capture_output=True, timeout=120)      # the row would finish on the device
    assert refused.returncode == 1 and b"--speculate" in refused.stderr and not os.path.exists(f)
    runs = []
    for extra in ([], ["--session-save", f], ["--session-load", f]):
        out = subprocess.run(base + ["--stream"] + extra, capture_output=True, timeout=300)
        assert out.returncode == 0, out.stderr
        runs.append(out)
    text = [r.stdout.split(b"\nTime cost")[0] for r in runs]
    assert text[0].startswith(TURN1.encode()) and len(text[0]) > len(TURN1)
    assert text[0] == text[1] == text[2]
    assert os.path.getsize(f) > 128
    assert b"session: 0 prompt tokens" in runs[1].stderr
    assert b"session: 4 prompt tokens served from the cache" in runs[2].stderr      # the prompt's five tokens but the last, whose logits the pass computes
