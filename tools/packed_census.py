#!/usr/bin/env python
"""Escape census of a synthetic checkpoint under the exponent-packed format's window (kernels/gemv_packed.h), per class, on the CPU:
weights, escapes, the most in one row, and how many matrices fall back to the plain kernel at a record of four entries.  Printed for the live "HL" window
(exponent fields [2 E0h, 2 E0h + 15], E0h = max((Emax >> 1) - 7, 0)) next to the replaced S/C window (E0 + 1 .. E0 + 15, E0 = max(Emax - 15, 0)).
The records are kept per (row, K-part) of the class's batch-1 launch (ks waves share a row pair; K-part p holds chunks [p * per, p * per + per), per = 64 NX):
a second table gives, for the HL window, the share of rows and of (row, K-part) with a non-empty record, the most escapes in one (row, K-part) and the
matrices that fall back under a record of four per row (the earlier layout) and per (row, K-part) (the live one).

  python tools/packed_census.py                                  # the benchmark's checkpoint: llama-3.2-1b, seed 1234, std 0.02
  python tools/packed_census.py --layers 1 --vocab 1024          # the descriptor of tests/test_hip_packed_hl.py
"""
import argparse
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tinygpt_amd import known_desc, synth  # noqa: E402

RECORD = 4


def escapes_hl(W):
    e = ((W >> 7) & 0xFF).astype(np.int32)
    emax = int(e[e < 255].max())
    d = (e >> 1) - max((emax >> 1) - 7, 0)
    return (d < 0) | (d > 7) | (e == 0) | (e == 255), emax


def escapes_sc(W):
    e = ((W >> 7) & 0xFF).astype(np.int32)
    emax = int(e[e < 255].max())
    c = e - max(emax - 15, 0)
    return (c < 1) | (c > 15), emax


def launch_ks(cls, K, inter):
    """the K split of the class's batch-1 launch (tgx_create's Tune::ks, then gemv_auto_ks in decode.hip)"""
    ks = (4 if inter >= 8192 else 2) if cls == "down" else 1
    while ks < 4 and ((K // 8) + ks * 64 - 1) // (ks * 64) > 8:
        ks *= 2
    return ks


def per_part(esc, ks):
    """escapes per (row, K-part): [N][ks]"""
    N, K = esc.shape
    nchunk = K // 8
    per = ((nchunk + ks * 64 - 1) // (ks * 64)) * 64
    part = np.minimum((np.arange(K) // 8) // per, ks - 1)
    return np.stack([esc[:, part == p].sum(axis=1) for p in range(ks)], axis=1)


def classify(name, tied):
    if name.endswith("mlp.gate_proj.weight") or name.endswith("mlp.up_proj.weight"):
        return "gate_up"
    if name.endswith("mlp.down_proj.weight"):
        return "down"
    if name == "lm_head.weight" or (tied and name == "model.embed_tokens.weight"):
        return "lm_head"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3.2-1b")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--std", type=float, default=0.02)
    ap.add_argument("--layers", type=int, default=0, help="override the descriptor's depth")
    ap.add_argument("--vocab", type=int, default=0, help="override the descriptor's vocabulary")
    a = ap.parse_args()
    d = copy.deepcopy(known_desc(a.model))
    if a.layers:
        d.layers = a.layers
    if a.vocab:
        d.vocab = a.vocab
    # gate and up are one matrix on the device (rows of up after the rows of gate): a fallback is per launch matrix, so their overflows are merged per layer
    stat = {c: {w: dict(tensors=0, weights=0, esc=0, most=0, over=set(), emax=set()) for w in ("HL", "S/C")} for c in ("lm_head", "gate_up", "down")}
    kp = {c: dict(ks=set(), rows=0, rows_rec=0, parts=0, parts_rec=0, most=0, over=set()) for c in stat}
    for name, bits in synth.synth_checkpoint(d, a.seed, a.std):
        cls = classify(name, d.tied)
        if cls is None:
            continue
        mat = name.rsplit(".", 2)[0] if cls == "gate_up" else name
        for w, fn in (("HL", escapes_hl), ("S/C", escapes_sc)):
            esc, emax = fn(bits)
            per_row = esc.sum(axis=1)
            s = stat[cls][w]
            s["tensors"] += 1; s["weights"] += bits.size; s["esc"] += int(per_row.sum()); s["most"] = max(s["most"], int(per_row.max())); s["emax"].add(emax)
            if per_row.max() > RECORD:
                s["over"].add(mat)
            if w == "HL" and bits.shape[1] % 8 == 0:
                ks = launch_ks(cls, bits.shape[1], d.inter)
                pp, k = per_part(esc, ks), kp[cls]
                k["ks"].add(ks); k["rows"] += pp.shape[0]; k["rows_rec"] += int((per_row > 0).sum()); k["parts"] += pp.size; k["parts_rec"] += int((pp > 0).sum())
                k["most"] = max(k["most"], int(pp.max()))
                if pp.max() > RECORD:
                    k["over"].add(mat)
    print(f"{a.model} layers {d.layers} vocab {d.vocab} seed {a.seed} std {a.std}; record of {RECORD} entries")
    print(f"{'class':8} {'window':6} {'tensors':>7} {'weights':>13} {'escapes':>9} {'rate':>9} {'most in one row':>15} {'matrices falling back':>21}  Emax")
    for cls, ws in stat.items():
        for w, s in ws.items():
            if s["tensors"]:
                print(f"{cls:8} {w:6} {s['tensors']:7d} {s['weights']:13d} {s['esc']:9d} {s['esc'] / s['weights']:9.2e} {s['most']:15d} {len(s['over']):21d}  {sorted(s['emax'])}")
    print(f"{'class':8} {'ks':>6} {'rows with a record':>18} {'(row, K-part) with one':>22} {'most in one (row, K-part)':>25} {'falling back: per row':>21} {'per (row, K-part)':>17}")
    for cls, k in kp.items():
        if k["rows"]:
            print(f"{cls:8} {str(sorted(k['ks'])):>6} {k['rows_rec'] / k['rows']:18.1%} {k['parts_rec'] / k['parts']:22.1%} {k['most']:25d} {len(stat[cls]['HL']['over']):21d} {len(k['over']):17d}")


if __name__ == "__main__":
    main()
