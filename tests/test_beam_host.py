"""The hypothesis bookkeeping of beam search (tinygpt_amd/host/beam.h BeamScorer) without a GPU: tests/beam_check.cpp, a stand-alone program built under the
address and undefined-behaviour sanitizers, runs the scorer over random candidate streams; what it decides — every step's next beams, the kept hypotheses with their
scores as bit patterns, their order and finish reasons — must equal, character for character, the restatement of the header's rules below."""
import struct
import subprocess

import numpy as np

from tinygpt_amd import build


def bits32(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def bits64(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


class Scorer:
    """the rules of host/beam.h, restated"""

    def __init__(self, K, lp, early, max_new, ends):
        self.K, self.lp, self.early, self.max_new, self.ends = K, float(np.float32(lp)), early, max_new, set(ends)
        self.run, self.scores, self.kept, self.len, self.added, self.done = [[]], [np.float32(0)], [], 0, 0, False

    def add(self, seq, sum_lp, length):
        h = {"tokens": seq, "sum": np.float32(sum_lp), "score": float(np.float32(sum_lp)) / (float(len(seq)) ** self.lp), "length": length, "order": self.added}
        self.added += 1
        if len(self.kept) < self.K:
            self.kept.append(h)
            return
        w = self.worst()
        if h["score"] > self.kept[w]["score"]:
            self.kept[w] = h

    def worst(self):
        return min(range(len(self.kept)), key=lambda i: (self.kept[i]["score"], -self.kept[i]["order"]))

    def step(self, cands):
        nxt, line = [], []
        self.parents, self.tokens = [], []      # the next beams: what tgx_beam_advance is given
        self.len += 1
        for i, (beam, tok, score, _) in enumerate(cands):
            if len(nxt) >= self.K:
                break
            if not 0 <= beam < len(self.run):
                continue
            seq = self.run[beam] + [tok]
            if tok in self.ends:
                if i < self.K:
                    self.add(seq, score, False)
                continue
            nxt.append((seq, np.float32(score)))
            line.append(f"{beam}:{tok}:{bits32(score)}")
            self.parents.append(beam); self.tokens.append(tok)
        self.run, self.scores = [s for s, _ in nxt], [x for _, x in nxt]
        if not self.run:
            self.done = True
        elif len(self.kept) >= self.K and (self.early or not (float(self.scores[0]) / (float(self.max_new if self.lp > 0 else self.len) ** self.lp) > self.kept[self.worst()]["score"])):
            self.done = True
        elif self.len >= self.max_new:
            for seq, s in zip(self.run, self.scores):
                self.add(seq, s, True)
            self.done = True
        return " ".join([f"S {int(self.done)} {len(self.run)}"] + line)

    def finish(self):
        return [f"H {int(h['length'])} {bits32(h['sum'])} {bits64(h['score'])} " + " ".join(str(t) for t in h["tokens"]) for h in sorted(self.kept, key=lambda h: (-h["score"], h["order"]))]


def stream(rng):
    """one random search: its parameters and, per step, a candidate list shaped like tgx_beam_select's (best first, ending at the K-th candidate that is no end id,
    at 32 entries, or early — the candidates ran out); now and then scores tie, a beam index is out of range, or the stream goes on after the search is done"""
    K = int(rng.integers(1, 9))
    lp = [0.0, 1.0, 0.6, 2.0, -0.5][int(rng.integers(0, 5))]
    early = bool(rng.integers(0, 2))
    max_new = int(rng.integers(1, 12))
    vocab = int(rng.integers(4, 40))
    ends = sorted(set(int(t) for t in rng.integers(0, vocab, size=int(rng.integers(0, 4)))))
    steps, running, base = [], 1, 0.0
    for _ in range(max_new + int(rng.integers(0, 2))):
        n_max = int(rng.integers(0, 33)) if rng.integers(0, 6) == 0 else 32
        cands, live, score = [], 0, base
        while len(cands) < n_max and live < K:
            score -= float(rng.choice([0.0, 0.25, 0.5, rng.uniform(0, 3)]))
            beam = int(rng.integers(0, running)) if rng.integers(0, 40) else running + 1
            tok = int(rng.integers(0, vocab)) if rng.integers(0, 3) or not ends else int(rng.choice(ends))
            cands.append((beam, tok, float(np.float32(score)), float(np.float32(-rng.uniform(0, 5)))))
            live += tok not in ends and 0 <= beam < running
        steps.append(cands)
        running = max(1, min(K, live))
        base = cands[0][2] if cands else base
    return K, lp, early, max_new, ends, steps


def test_beam_scorer_against_the_restated_rules():
    exe = build.build_beam_check()
    rng = np.random.default_rng(20260)
    streams = [stream(rng) for _ in range(400)]
    text, want = [str(len(streams))], []
    for K, lp, early, max_new, ends, steps in streams:
        text.append(" ".join(str(x) for x in [K, bits32(lp), int(early), max_new, len(ends)] + ends + [len(steps)]))
        ref = Scorer(K, lp, early, max_new, ends)
        for cands in steps:
            text.append(" ".join([str(len(cands))] + [f"{b} {t} {bits32(s)} {bits32(l)}" for b, t, s, l in cands]))
            if not ref.done:
                want.append(ref.step(cands))
        want += ref.finish() + ["E"]
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = [l.rstrip() for l in r.stdout.splitlines()]
    want = [l.rstrip() for l in want]
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    kinds = "".join(l[0] for l in want)
    assert "H 1" in r.stdout and "H 0" in r.stdout and "S 1" in r.stdout and kinds.count("E") == 400      # both finish reasons and early ends occur


def test_a_backend_without_the_calls_fails_the_generate_call(oracle_lib, tmp_path):
    """the host engine bound to a library that does not export tgx_beam_select / tgx_beam_advance (the CPU oracle, through the test-hook build): numBeams > 1 fails
    generateSync with a message, numBeams 1 runs the loop it always ran"""
    import ctypes
    from conftest import load_golden
    from host_util import HostEngine, host_lib, write_model_dir
    lib = host_lib(test_hooks=True)
    lib.tgxe_set_beams.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int]
    cfg, g = load_golden("llama_tiny")
    write_model_dir(str(tmp_path), cfg, int(g["seed"]), float(g["std"]))
    e = HostEngine(lib, model_dir=str(tmp_path), backend_lib=oracle_lib.path, prefix="tgxo_", dtype=0, max_batch=4)
    assert e.prepare(), e.error()
    e.reconfigure(max_new=4)
    plain, _, _ = e.generate_sync([g["prompt"][0]])
    lib.tgxe_set_beams(e.h, 4, 1.0, 0, 1)
    e.reconfigure(max_new=4)
    try:
        e.generate_sync([g["prompt"][0]])
        raise RuntimeError("the call went through")
    except AssertionError as err:
        assert "lacks tgx_beam_select / tgx_beam_advance" in str(err)
    lib.tgxe_set_beams(e.h, 1, 1.0, 0, 1)
    e.reconfigure(max_new=4)
    again, _, _ = e.generate_sync([g["prompt"][0]])
    np.testing.assert_array_equal(again, plain)
    e.close()
