"""ctypes binding of the C ABI in include/tgx.h and the host-side model wrapper used by
bench.py and the parity tests.

`Model` mirrors the engine-facing interface of the reference's GPTModel
(src/model/GPTModel.h:80-106: forward / resetCache / load / numLayers / contextSize) plus
Sampler::sample (src/engine/Sampler.cpp:23-79) on top of one opaque `tgx_ctx`.

The product library is tinygpt_amd/lib/libtgx_mi355x.so (built by tinygpt_amd.build); loading
fails loudly if it is missing — there is no CPU fallback in this package.  `Backend` binds any
library exporting the same entry points under a symbol prefix (the test infrastructure reuses it).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint64, c_void_p

import numpy as np

from .desc import CDesc, ModelDesc, DTYPE_BF16, DTYPE_F32, DTYPE_F16
from . import synth

HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(HERE, "lib", "libtgx_mi355x.so")

STATUS_NAMES = {0: "TGX_OK", 1: "TGX_ERR_INVALID", 2: "TGX_ERR_UNSUPPORTED", 3: "TGX_ERR_DEVICE", 4: "TGX_ERR_STATE",
                5: "TGX_ERR_NOMEM", 6: "TGX_ERR_NAME", 7: "TGX_ERR_SHAPE", 8: "TGX_ERR_CONTEXT"}

MAX_LOGPROBS, LOGPROB_RING = 20, 256      # TGX_MAX_LOGPROBS, TGX_LOGPROB_RING
KERNEL_CLASSES = ["qkv", "attn", "oproj", "gateup", "down", "lmhead"]


class SamplerCfg(ctypes.Structure):
    """struct tgx_sampler_cfg == SamplerConfig (src/engine/Sampler.h:13-22)."""
    _fields_ = [("temperature", c_float), ("top_k", c_int64), ("top_p", c_float), ("min_p", c_float)]

    def __init__(self, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0):
        super().__init__(temperature, top_k, top_p, min_p)

    @property
    def greedy(self):   # Sampler.cpp:15-21
        return not (self.temperature > 0 or self.top_k > 0 or self.top_p < 1 or self.min_p > 0)


GREEDY = SamplerCfg()


class PenaltyCfg(ctypes.Structure):
    """tgx_penalty_cfg; neutral: repetition 1, presence 0, frequency 0"""
    _fields_ = [("repetition", c_float), ("presence", c_float), ("frequency", c_float)]

    def __init__(self, repetition=1.0, presence=0.0, frequency=0.0):
        super().__init__(repetition, presence, frequency)


MAX_LOGIT_BIAS = 320     # TGX_MAX_LOGIT_BIAS
ADV_STEP, ADV_FEED, ADV_FEED_MORE = 0, 1, 2      # TGX_ADV_*: the kinds of tgx_advance_rows
MAX_ADVANCE_POSITIONS = 8192                     # TGX_MAX_ADVANCE_POSITIONS


MAX_BEAMS, MAX_BEAM_CAND, MAX_STOP_IDS = 8, 32, 8    # TGX_MAX_BEAMS, TGX_MAX_BEAM_CAND, TGX_MAX_STOP_IDS


class BeamCand(ctypes.Structure):
    """tgx_beam_cand"""
    _fields_ = [("beam", c_int32), ("token", c_int32), ("score", c_float), ("lp", c_float)]


POOL_MODES = {"last": 0, "mean": 1, "first": 2}      # TGX_POOL_*


class EmbedCfg(ctypes.Structure):
    """tgx_embed_cfg"""
    _fields_ = [("pool", c_int32), ("normalize", c_int32), ("dims", c_int32), ("release", c_int32)]


class TgxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


# name -> (restype, argtypes); every symbol include/tgx.h declares
ABI = {
    "device_count": (c_int, [POINTER(c_int)]),
    "create": (c_int, [POINTER(CDesc), c_int, POINTER(c_void_p)]),
    "upload": (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int, c_int]),
    "finalize": (c_int, [c_void_p]),
    "destroy": (None, [c_void_p]),
    "forward": (c_int, [c_void_p, POINTER(c_int64), c_int, c_int]),
    "read_logits": (c_int, [c_void_p, POINTER(c_float), c_int]),
    "sample": (c_int, [c_void_p, POINTER(SamplerCfg), c_uint64, POINTER(c_int64)]),
    "decode": (c_int, [c_void_p, POINTER(SamplerCfg), c_uint64, c_int, POINTER(c_int64)]),
    "step_async": (c_int, [c_void_p, POINTER(SamplerCfg), c_uint64, POINTER(c_int64)]),
    "fetch_token": (c_int, [c_void_p, c_int64, POINTER(c_int32)]),
    "reset_cache": (c_int, [c_void_p]),
    "past_length": (c_int64, [c_void_p]),
    "reset_row": (c_int, [c_void_p, c_int]),
    "forward_row": (c_int, [c_void_p, c_int, POINTER(c_int64), c_int]),
    "forward_rows": (c_int, [c_void_p, c_int, POINTER(c_int32), POINTER(c_int64), POINTER(c_int32)]),
    "embed_rows": (c_int, [c_void_p, c_int, POINTER(c_int32), POINTER(c_int64), POINTER(c_int32), POINTER(EmbedCfg), POINTER(c_float)]),
    "fork_row": (c_int, [c_void_p, c_int, c_int, POINTER(c_int32)]),
    "beam_select": (c_int, [c_void_p, c_int, POINTER(c_int32), POINTER(c_float), c_int, POINTER(c_int32), c_int, POINTER(BeamCand), POINTER(c_int32)]),
    "beam_advance": (c_int, [c_void_p, c_int, POINTER(c_int32), c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "extend_row": (c_int, [c_void_p, c_int, POINTER(c_int64), c_int]),
    "truncate_row": (c_int, [c_void_p, c_int, c_int64]),
    "splice_row": (c_int, [c_void_p, c_int, c_int, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "row_snapshot_bytes": (c_int, [c_void_p, c_int, POINTER(c_int64)]),
    "save_row": (c_int, [c_void_p, c_int, c_void_p, c_int64, POINTER(c_int64)]),
    "restore_row": (c_int, [c_void_p, c_int, c_void_p, c_int64]),
    "verify_row": (c_int, [c_void_p, c_int, POINTER(c_int64), c_int, POINTER(c_int64), POINTER(c_int32), POINTER(c_int32)]),
    "verify_row_sampled": (c_int, [c_void_p, c_int, POINTER(c_int64), c_int, POINTER(c_int64), POINTER(c_int32), POINTER(c_int32)]),
    "verify_tree": (c_int, [c_void_p, c_int, POINTER(c_int64), POINTER(c_int32), c_int, POINTER(c_int64), POINTER(c_int32), POINTER(c_int32)]),
    "read_pass_logits": (c_int, [c_void_p, POINTER(c_float), c_int, POINTER(c_int32)]),
    "verify_rows": (c_int, [c_void_p, c_int, POINTER(c_int32), POINTER(c_int64), POINTER(c_int32), POINTER(c_int64), POINTER(c_int32), POINTER(c_int32)]),
    "advance_rows": (c_int, [c_void_p, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int64), POINTER(c_int32), POINTER(c_int64), POINTER(c_int32), POINTER(c_int32)]),
    "sample_row": (c_int, [c_void_p, c_int, POINTER(SamplerCfg), c_uint64, POINTER(c_int64)]),
    "past_length_row": (c_int64, [c_void_p, c_int]),
    "set_row_sampler": (c_int, [c_void_p, c_int, POINTER(SamplerCfg), c_uint64]),
    "set_row_stop": (c_int, [c_void_p, c_int, c_int32, POINTER(c_int32), c_int]),
    "decode_rows": (c_int, [c_void_p, c_int, POINTER(c_int64), POINTER(c_int32), POINTER(c_int32)]),
    "set_row_logprobs": (c_int, [c_void_p, c_int, c_int]),
    "read_row_logprobs": (c_int, [c_void_p, c_int, c_int, POINTER(c_float), POINTER(c_int32), POINTER(c_float), POINTER(c_int32)]),
    "score_row": (c_int, [c_void_p, c_int, POINTER(c_int64), c_int, c_int, POINTER(c_float), POINTER(c_int32), POINTER(c_float)]),
    "set_row_penalties": (c_int, [c_void_p, c_int, POINTER(PenaltyCfg)]),
    "set_row_logit_bias": (c_int, [c_void_p, c_int, c_int, POINTER(c_int32), POINTER(c_float)]),
    "set_row_history": (c_int, [c_void_p, c_int, POINTER(c_int64), c_int, POINTER(c_int64), c_int]),
    "automaton_create": (c_int, [c_void_p, c_int32, c_int32, POINTER(ctypes.c_uint16), POINTER(c_int32)]),
    "automaton_destroy": (c_int, [c_void_p, c_int32]),
    "set_row_automaton": (c_int, [c_void_p, c_int, c_int32, c_int32]),
    "read_row_automaton": (c_int, [c_void_p, c_int, POINTER(c_int32), POINTER(c_int32)]),
    "context_size": (c_int64, [c_void_p]),
    "num_layers": (c_int32, [c_void_p]),
    "last_error": (c_char_p, [c_void_p]),
    "synchronize": (c_int, [c_void_p]),
    "read_kv": (c_int, [c_void_p, c_int, c_int, POINTER(c_float), POINTER(c_float)]),
    "write_kv": (c_int, [c_void_p, c_int, c_int, POINTER(c_float), POINTER(c_float), c_int64]),
    "profile_decode": (c_int, [c_void_p, c_int, POINTER(c_int64), POINTER(c_double)]),
    "set_option": (c_int, [c_void_p, c_char_p, c_int]),
    "get_option": (c_int, [c_void_p, c_char_p, POINTER(c_int)]),
    "read_probs": (c_int, [c_void_p, POINTER(c_float)]),
    "set_logits": (c_int, [c_void_p, POINTER(c_float), c_int]),
    "bytes_per_token": (c_int64, [c_void_p, c_int64]),
    "abi_version": (c_int, []),
}


class Backend:
    """A loaded shared library exporting `<prefix><name>` for (a subset of) ABI."""

    def __init__(self, path: str, prefix: str = "tgx_", required=None, extra=None):
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} not found — build it first (python -c 'import __graft_entry__ as g; g.build()'). "
                "tinygpt_amd has no CPU fallback.")
        self.path = path
        self.prefix = prefix
        self.lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        table = dict(ABI)
        if extra:
            table.update(extra)
        names = required if required is not None else list(ABI)
        if extra:
            names = list(names) + list(extra)
        for name in names:
            res, args = table[name]
            fn = getattr(self.lib, prefix + name)   # AttributeError if the symbol is missing: loud by design
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)

    def has(self, name):
        return hasattr(self, name)


_product = None


def product_backend() -> Backend:
    global _product
    if _product is None:
        _product = Backend(PRODUCT_LIB, "tgx_")
    return _product


def _as_bits(arr: np.ndarray):
    """ndarray -> (contiguous array, tgx_dtype).  uint16 is taken as bf16 bit patterns."""
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint16:
        return a, DTYPE_BF16
    if a.dtype == np.float32:
        return a, DTYPE_F32
    if a.dtype == np.float16:
        return a.view(np.uint16), DTYPE_F16
    raise TypeError(f"unsupported tensor dtype {a.dtype}")


class Model:
    """One model instance on one device behind the C ABI."""

    def __init__(self, desc: ModelDesc, backend: Backend | None = None, device: int = 0):
        self.be = backend or product_backend()
        self.desc = desc
        self._ctx = c_void_p()
        cd = desc.to_c()
        st = self.be.create(ctypes.byref(cd), device, ctypes.byref(self._ctx))
        if st != 0:
            msg = self.be.last_error(self._ctx if self._ctx else None)
            raise TgxError(st, (msg or b"").decode())
        self.batch = 0

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, st):
        if st != 0:
            raise TgxError(st, (self.be.last_error(self._ctx) or b"").decode())

    def close(self):
        if self._ctx:
            self.be.destroy(self._ctx)
            self._ctx = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- load (== GPTModel::load -> SafeTensors::load) ---------------------------------------
    def upload(self, name: str, arr: np.ndarray, strict: bool = True):
        if hasattr(arr, "error") and hasattr(arr, "dtype") and not isinstance(arr, np.ndarray):
            # checkpoint.UnsupportedTensor: a file dtype this path cannot convert (I64 / BOOL / U8 ...).  The ABI's name probe (ndim < 0, include/tgx.h)
            # tells a parameter the model needs (TGX_ERR_SHAPE: raise) from a key it ignores or does not know (skipped like the reference, SafeTensors.cpp:176-182)
            one = (c_int64 * 1)(0)
            st = self.be.upload(self._ctx, name.encode(), ctypes.cast(one, c_void_p), one, -1, 0)   # 0 = TGX_F32
            if st == 7 or (st == 6 and strict):
                raise arr.error()
            return False
        a, dt = _as_bits(arr)
        shape = (c_int64 * a.ndim)(*a.shape)
        st = self.be.upload(self._ctx, name.encode(), a.ctypes.data_as(c_void_p), shape, a.ndim, dt)
        if st == 6 and not strict:   # "Unexpected key" is a warning in the reference (non-strict load, GPTModel.h:96)
            return False
        self._check(st)
        return True

    def load_synthetic(self, seed: int = 1234, std: float = 0.02, peaked: bool = False):
        for name, bits in synth.synth_checkpoint(self.desc, seed, std, peaked):
            self.upload(name, bits)
        return self

    def load_state(self, tensors: "dict[str, np.ndarray]", strict: bool = False):
        for name, arr in tensors.items():
            self.upload(name, arr, strict=strict)
        return self

    def finalize(self):
        self._check(self.be.finalize(self._ctx))
        return self

    # -- hot path ---------------------------------------------------------------------------
    def forward(self, ids):
        ids = np.ascontiguousarray(np.atleast_2d(np.asarray(ids, dtype=np.int64)))
        B, S = ids.shape
        self._check(self.be.forward(self._ctx, ids.ctypes.data_as(POINTER(c_int64)), B, S))
        self.batch = B
        return self

    def logits(self, rounded: bool = True) -> np.ndarray:
        out = np.empty((self.batch, self.desc.vocab), dtype=np.float32)
        self._check(self.be.read_logits(self._ctx, out.ctypes.data_as(POINTER(c_float)), int(rounded)))
        return out

    def sample(self, cfg: SamplerCfg = GREEDY, seed: int = 0) -> np.ndarray:
        out = np.empty(self.batch, dtype=np.int64)
        self._check(self.be.sample(self._ctx, ctypes.byref(cfg), seed, out.ctypes.data_as(POINTER(c_int64))))
        return out

    def decode(self, n_steps: int, cfg: SamplerCfg = GREEDY, seed: int = 0, fetch: bool = True):
        out = np.empty((n_steps, self.batch), dtype=np.int64) if fetch else None
        ptr = out.ctypes.data_as(POINTER(c_int64)) if fetch else None
        self._check(self.be.decode(self._ctx, ctypes.byref(cfg), seed, n_steps, ptr))
        return out

    def step_async(self, cfg: SamplerCfg = GREEDY, seed: int = 0) -> int:
        t = c_int64()
        self._check(self.be.step_async(self._ctx, ctypes.byref(cfg), seed, ctypes.byref(t)))
        return t.value

    def fetch_token(self, ticket: int) -> int:
        v = c_int32()
        self._check(self.be.fetch_token(self._ctx, ticket, ctypes.byref(v)))
        return v.value

    def reset_cache(self):
        self._check(self.be.reset_cache(self._ctx))

    # -- per-row sequence lifecycle (include/tgx.h, ABI 3) ------------------------------------
    def reset_row(self, row: int):
        self._check(self.be.reset_row(self._ctx, row))
        return self

    def forward_row(self, row: int, ids):
        """prefill one prompt into `row` of the live batch (a retired row, or the next free one); the other rows keep their state"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        self._check(self.be.forward_row(self._ctx, row, ids.ctypes.data_as(POINTER(c_int64)), len(ids)))
        self.batch = max(self.batch, row + 1)
        return self

    def forward_rows(self, rows, prompts):
        """prefill prompts[i] into rows[i] of the live batch, all in ONE pass (include/tgx.h tgx_forward_rows); the other rows keep their state"""
        rows = np.ascontiguousarray(np.asarray(list(rows), dtype=np.int32).reshape(-1))
        ps = [np.asarray(p, dtype=np.int64).reshape(-1) for p in prompts]
        assert len(ps) == len(rows), "one prompt per row"
        lens = np.ascontiguousarray(np.array([len(p) for p in ps], dtype=np.int32))
        ids = np.ascontiguousarray(np.concatenate(ps) if ps else np.zeros(1, dtype=np.int64))
        self._check(self.be.forward_rows(self._ctx, len(rows), rows.ctypes.data_as(POINTER(c_int32)), ids.ctypes.data_as(POINTER(c_int64)),
                                         lens.ctypes.data_as(POINTER(c_int32))))
        if len(rows):
            self.batch = max(self.batch, int(rows.max()) + 1)
        return self

    def embed_rows(self, rows, prompts, pool="last", normalize=True, dims=0, release=False) -> np.ndarray:
        """the pooled final-norm hidden state of prompts[i], prefilled into rows[i] in ONE pass without lm_head (include/tgx.h tgx_embed_rows): float32
        [n][dims or hidden].  release=False leaves the rows holding their positions without logits; release=True retires them"""
        rows = np.ascontiguousarray(np.asarray(list(rows), dtype=np.int32).reshape(-1))
        ps = [np.asarray(p, dtype=np.int64).reshape(-1) for p in prompts]
        assert len(ps) == len(rows), "one prompt per row"
        lens = np.ascontiguousarray(np.array([len(p) for p in ps], dtype=np.int32))
        ids = np.ascontiguousarray(np.concatenate(ps) if ps else np.zeros(1, dtype=np.int64))
        cfg = EmbedCfg(POOL_MODES[pool] if isinstance(pool, str) else int(pool), int(bool(normalize)), int(dims), int(bool(release)))
        width = int(dims) if 0 < int(dims) else self.desc.hidden
        out = np.zeros((max(len(rows), 1), max(width, 1)), dtype=np.float32)
        self._check(self.be.embed_rows(self._ctx, len(rows), rows.ctypes.data_as(POINTER(c_int32)), ids.ctypes.data_as(POINTER(c_int64)),
                                       lens.ctypes.data_as(POINTER(c_int32)), ctypes.byref(cfg), out.ctypes.data_as(POINTER(c_float))))
        if len(rows):
            self.batch = max(self.batch, int(rows.max()) + 1)
        return out[:len(rows), :width]

    def fork_row(self, src: int, dst_rows):
        """make every row of dst_rows (retired rows or the next free ones) a copy of the live row `src` (include/tgx.h tgx_fork_row): same length, cache, logits and
        current token; on a paged cache the full blocks are shared, only the partial tail block is copied"""
        rows = np.ascontiguousarray(np.asarray(list(dst_rows), dtype=np.int32).reshape(-1))
        ptr = rows.ctypes.data_as(POINTER(c_int32)) if len(rows) else (c_int32 * 1)()
        self._check(self.be.fork_row(self._ctx, src, len(rows), ptr))
        if len(rows):
            self.batch = max(self.batch, int(rows.max()) + 1)
        return self

    # -- beam search (include/tgx.h tgx_beam_select / tgx_beam_advance) ---------------------------
    def beam_select(self, rows, scores, k: int, end_ids=()):
        """the joint ranking of rows' next-token distributions plus their running scores (include/tgx.h tgx_beam_select): the prefix of the joint order that ends at
        the k-th candidate whose token is no end id -> (beam [m] int32 — an index into rows —, token [m] int32, score [m] float32, lp [m] float32)"""
        rows = np.ascontiguousarray(np.asarray(list(rows), dtype=np.int32).reshape(-1))
        sc = np.ascontiguousarray(np.asarray(list(scores), dtype=np.float32).reshape(-1))
        assert len(sc) == len(rows), "one score per row"
        ends = np.ascontiguousarray(np.asarray(list(end_ids), dtype=np.int32).reshape(-1))
        out = (BeamCand * MAX_BEAM_CAND)()
        n = c_int32(0)
        self._check(self.be.beam_select(self._ctx, len(rows), rows.ctypes.data_as(POINTER(c_int32)) if len(rows) else None, sc.ctypes.data_as(POINTER(c_float)) if len(sc) else None,
                                        int(k), ends.ctypes.data_as(POINTER(c_int32)) if len(ends) else None, len(ends), out, ctypes.byref(n)))
        a = np.frombuffer(out, dtype=np.dtype([("beam", np.int32), ("token", np.int32), ("score", np.float32), ("lp", np.float32)]), count=MAX_BEAM_CAND)[:n.value]
        return a["beam"].copy(), a["token"].copy(), a["score"].copy(), a["lp"].copy()

    def beam_advance(self, rows, parent, tokens):
        """re-seat the group `rows` (sources and spares) on its next hypotheses (include/tgx.h tgx_beam_advance): hypothesis j continues rows[parent[j]] with current
        token tokens[j] -> the rows the hypotheses live in, by the header's pinned placement"""
        rows = np.ascontiguousarray(np.asarray(list(rows), dtype=np.int32).reshape(-1))
        par = np.ascontiguousarray(np.asarray(list(parent), dtype=np.int32).reshape(-1))
        tok = np.ascontiguousarray(np.asarray(list(tokens), dtype=np.int32).reshape(-1))
        assert len(par) == len(tok), "one token per parent"
        out = np.full(max(len(par), 1), -1, dtype=np.int32)
        self._check(self.be.beam_advance(self._ctx, len(rows), rows.ctypes.data_as(POINTER(c_int32)) if len(rows) else None, len(par),
                                         par.ctypes.data_as(POINTER(c_int32)) if len(par) else None, tok.ctypes.data_as(POINTER(c_int32)) if len(tok) else None,
                                         out.ctypes.data_as(POINTER(c_int32))))
        out = out[:len(par)]
        if len(out):
            self.batch = max(self.batch, int(out.max()) + 1)
        return out

    def extend_row(self, row: int, ids):
        """append ids at positions past .. past + len(ids) - 1 of the live (or finished) row `row` in one causal pass (include/tgx.h tgx_extend_row); the row's current
        token, if any, is discarded"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        self._check(self.be.extend_row(self._ctx, row, ids.ctypes.data_as(POINTER(c_int64)), len(ids)))
        return self

    def truncate_row(self, row: int, n: int):
        """roll `row` back to its first n positions (include/tgx.h tgx_truncate_row); it then holds no logits until extend_row"""
        self._check(self.be.truncate_row(self._ctx, row, int(n)))
        return self

    def splice_row(self, row: int, ranges) -> int:
        """keep the positions in `ranges` — (start, length) pairs, sorted and disjoint — of `row` and slide them together, the keys re-rotated to where they land
        (include/tgx.h tgx_splice_row); returns the new length.  The row then holds no logits until extend_row"""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
        starts, lens = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
        n = c_int64(0)
        self._check(self.be.splice_row(self._ctx, row, len(r), starts.ctypes.data_as(POINTER(c_int64)), lens.ctypes.data_as(POINTER(c_int64)), ctypes.byref(n)))
        return n.value

    # -- row snapshots (include/tgx.h tgx_save_row / tgx_restore_row) -----------------------------
    def row_snapshot_bytes(self, row: int) -> int:
        n = c_int64(0)
        self._check(self.be.row_snapshot_bytes(self._ctx, row, ctypes.byref(n)))
        return n.value

    def save_row(self, row: int) -> bytes:
        """the live row `row` as a snapshot (include/tgx.h tgx_save_row): its cache positions, position and token words and, if it holds them, hidden row and logits;
        the row stays as it is"""
        buf = np.empty(self.row_snapshot_bytes(row), dtype=np.uint8)
        n = c_int64(0)
        self._check(self.be.save_row(self._ctx, row, buf.ctypes.data_as(c_void_p), buf.size, ctypes.byref(n)))
        return buf[:n.value].tobytes()

    def restore_row(self, row: int, blob):
        """`row` (a retired or empty row, or the next free one) becomes the row `blob` was saved from (include/tgx.h tgx_restore_row); settings are the caller's"""
        a = np.frombuffer(blob, dtype=np.uint8)
        ptr = a.ctypes.data_as(c_void_p) if a.size else ctypes.cast((ctypes.c_ubyte * 1)(), c_void_p)
        self._check(self.be.restore_row(self._ctx, row, ptr, a.size))
        self.batch = max(self.batch, row + 1)
        return self

    def verify_row(self, row: int, draft):
        """verify `draft` (1 .. 15 guessed next tokens) on the live row `row` in one pass (include/tgx.h tgx_verify_row): the row takes the draft's greedy-matching
        prefix plus the model's own next token and stands as after that many greedy decode steps -> (produced ids, finish: 0 running, 1 stop id, 2 max_new)"""
        draft = np.ascontiguousarray(np.asarray(draft, dtype=np.int64).reshape(-1))
        out = np.empty(len(draft) + 1, dtype=np.int64)
        n, fin = c_int32(0), c_int32(0)
        ptr = draft.ctypes.data_as(POINTER(c_int64)) if len(draft) else (c_int64 * 1)()
        self._check(self.be.verify_row(self._ctx, row, ptr, len(draft), out.ctypes.data_as(POINTER(c_int64)), ctypes.byref(n), ctypes.byref(fin)))
        return out[:n.value].copy(), fin.value

    def verify_row_sampled(self, row: int, draft):
        """verify_row under the row's OWN sampler (include/tgx.h tgx_verify_row_sampled; set_row_sampler: cfg and seed): the row takes the draft's prefix that equals
        its draws plus its own draw at the first mismatch, the ids decode_rows would have produced -> (produced ids, finish).  A greedy row: verify_row itself"""
        draft = np.ascontiguousarray(np.asarray(draft, dtype=np.int64).reshape(-1))
        out = np.empty(len(draft) + 1, dtype=np.int64)
        n, fin = c_int32(0), c_int32(0)
        ptr = draft.ctypes.data_as(POINTER(c_int64)) if len(draft) else (c_int64 * 1)()
        self._check(self.be.verify_row_sampled(self._ctx, row, ptr, len(draft), out.ctypes.data_as(POINTER(c_int64)), ctypes.byref(n), ctypes.byref(fin)))
        return out[:n.value].copy(), fin.value

    def verify_tree(self, row: int, tokens, parent):
        """verify a token TREE of 1 .. 15 guesses on the live row `row` in one pass (include/tgx.h tgx_verify_tree): tokens[i] is node i's token, parent[i] its parent
        node (-1: a child of the row's current token, else an index < i).  Every node attends its own branch alone; the row takes the branch its own settings
        produce (greedy, or its sampler's draws) and stands as after that many decode steps -> (produced ids, finish).  A chain (parent[i] == i - 1) is
        verify_row_sampled itself"""
        tokens = np.ascontiguousarray(np.asarray(tokens, dtype=np.int64).reshape(-1))
        parent = np.ascontiguousarray(np.asarray(parent, dtype=np.int32).reshape(-1))
        assert len(tokens) == len(parent), (len(tokens), len(parent))
        out = np.empty(len(tokens) + 1, dtype=np.int64)
        n, fin = c_int32(0), c_int32(0)
        tptr = tokens.ctypes.data_as(POINTER(c_int64)) if len(tokens) else (c_int64 * 1)()
        pptr = parent.ctypes.data_as(POINTER(c_int32)) if len(parent) else (c_int32 * 1)()
        self._check(self.be.verify_tree(self._ctx, row, tptr, pptr, len(tokens), out.ctypes.data_as(POINTER(c_int64)), ctypes.byref(n), ctypes.byref(fin)))
        return out[:n.value].copy(), fin.value

    def pass_logits(self) -> np.ndarray:
        """the fp32 logits [M][vocab] of the last verify pass's M positions (include/tgx.h tgx_read_pass_logits; test / diagnostic use)"""
        out = np.empty((64, self.desc.vocab), dtype=np.float32)      # TGX_MAX_VERIFY_POSITIONS at the most (a one-row pass: TGX_MAX_DRAFT + 1)
        m = c_int32(0)
        self._check(self.be.read_pass_logits(self._ctx, out.ctypes.data_as(POINTER(c_float)), 64, ctypes.byref(m)))
        return out[:m.value].copy()

    def verify_rows(self, rows, drafts):
        """verify_row_sampled for several rows in ONE joint pass (include/tgx.h tgx_verify_rows): drafts[i] = row rows[i]'s draft ids, possibly empty (the row then
        produces one token, as a decode_rows step would) -> a list of (produced ids, finish), one per row in call order"""
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
        ds = [np.asarray(d, dtype=np.int64).reshape(-1) for d in drafts]
        assert len(ds) == len(rows), (len(ds), len(rows))
        n_draft = np.ascontiguousarray(np.array([len(d) for d in ds], dtype=np.int32))
        flat = np.ascontiguousarray(np.concatenate(ds + [np.zeros(1, dtype=np.int64)]))      # (never empty: the pointer stays valid)
        n = len(rows)
        out = np.zeros((max(n, 1), 16), dtype=np.int64)      # [n][TGX_MAX_DRAFT + 1]
        out_n, fin = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.be.verify_rows(self._ctx, n, rows.ctypes.data_as(POINTER(c_int32)), flat.ctypes.data_as(POINTER(c_int64)), n_draft.ctypes.data_as(POINTER(c_int32)),
                                        out.ctypes.data_as(POINTER(c_int64)), out_n.ctypes.data_as(POINTER(c_int32)), fin.ctypes.data_as(POINTER(c_int32))))
        return [(out[i, :out_n[i]].copy(), int(fin[i])) for i in range(n)]

    def advance_rows(self, rows, kinds, ids_per_row):
        """prompt chunks and live rows' steps in ONE ragged pass (include/tgx.h tgx_advance_rows).  kinds[i]: ADV_STEP — rows[i] is a live row with a current token,
        ids_per_row[i] its draft (possibly empty: one plain step); ADV_FEED — ids_per_row[i] is appended to (or admitted into) rows[i] and the last position's logits
        land in its slot; ADV_FEED_MORE — the same without logits, more of the prompt follows -> a list of (produced ids, finish), one per row in call order (FEED
        rows: no ids, 0)"""
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
        kinds = np.ascontiguousarray(np.asarray(kinds, dtype=np.int32).reshape(-1))
        ps = [np.asarray(p, dtype=np.int64).reshape(-1) for p in ids_per_row]
        assert len(ps) == len(rows) == len(kinds), (len(ps), len(rows), len(kinds))
        lens = np.ascontiguousarray(np.array([len(p) for p in ps], dtype=np.int32))
        flat = np.ascontiguousarray(np.concatenate(ps + [np.zeros(1, dtype=np.int64)]))      # (never empty: the pointer stays valid)
        n = len(rows)
        out = np.zeros((max(n, 1), 16), dtype=np.int64)      # [n][TGX_MAX_DRAFT + 1]
        out_n, fin = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.be.advance_rows(self._ctx, n, rows.ctypes.data_as(POINTER(c_int32)), kinds.ctypes.data_as(POINTER(c_int32)), flat.ctypes.data_as(POINTER(c_int64)),
                                         lens.ctypes.data_as(POINTER(c_int32)), out.ctypes.data_as(POINTER(c_int64)), out_n.ctypes.data_as(POINTER(c_int32)),
                                         fin.ctypes.data_as(POINTER(c_int32))))
        if n:
            self.batch = max(self.batch, int(rows.max()) + 1)
        return [(out[i, :out_n[i]].copy(), int(fin[i])) for i in range(n)]

    @property
    def advance_attn_tiles(self) -> int:
        """option advance.attn_tiles: the tile target of tgx_advance_rows' attention (-1 automatic, 0 never split, N tiles per work item)"""
        return self.get_option("advance.attn_tiles")

    @advance_attn_tiles.setter
    def advance_attn_tiles(self, value: int):
        self.set_option("advance.attn_tiles", value)

    @property
    def advance_last_form(self) -> int:
        """read-only option advance.last_form: 0 no advance_rows call yet, 1 the joint pass, 2 piecewise"""
        return self.get_option("advance.last_form")

    def sample_row(self, row: int, cfg: SamplerCfg = GREEDY, seed: int = 0) -> int:
        out = c_int64()
        self._check(self.be.sample_row(self._ctx, row, ctypes.byref(cfg), seed, ctypes.byref(out)))
        return out.value

    def past_length_row(self, row: int) -> int:
        return self.be.past_length_row(self._ctx, row)

    # -- per-row sampler settings and device-side stop (include/tgx.h tgx_decode_rows) ---------
    def set_row_sampler(self, row: int, cfg: SamplerCfg = GREEDY, seed: int = 0):
        self._check(self.be.set_row_sampler(self._ctx, row, ctypes.byref(cfg) if cfg is not None else None, seed))
        return self

    def set_row_stop(self, row: int, max_new: int = 0, stop_ids=()):
        ids = np.ascontiguousarray(np.asarray(list(stop_ids), dtype=np.int32).reshape(-1))
        ptr = ids.ctypes.data_as(POINTER(c_int32)) if len(ids) else None
        self._check(self.be.set_row_stop(self._ctx, row, max_new, ptr, len(ids)))
        return self

    def decode_rows(self, n_steps: int):
        """n_steps steps, every row with its own settings -> (ids [n_steps][batch] (-1 after a row finished), produced [batch], finish [batch]:
        0 running, 1 stop id, 2 max_new)"""
        out = np.empty((n_steps, self.batch), dtype=np.int64)
        new = np.empty(self.batch, dtype=np.int32)
        fin = np.empty(self.batch, dtype=np.int32)
        self._check(self.be.decode_rows(self._ctx, n_steps, out.ctypes.data_as(POINTER(c_int64)), new.ctypes.data_as(POINTER(c_int32)),
                                        fin.ctypes.data_as(POINTER(c_int32))))
        return out, new, fin

    # -- per-token log-probabilities (include/tgx.h tgx_set_row_logprobs) ------------------------
    def set_row_logprobs(self, row: int, top_n: int = 0):
        """-1 off, 0 the produced token's log-probability, 1 .. MAX_LOGPROBS that many alternatives as well"""
        self._check(self.be.set_row_logprobs(self._ctx, row, top_n))
        return self

    def row_logprobs(self, row: int, n: int):
        """the row's last n records, oldest first -> (lp [n], top ids [n][MAX_LOGPROBS] (-1 beyond top_n), top lp [n][MAX_LOGPROBS], top_n [n])"""
        m = max(n, 1)
        lp = np.empty(m, dtype=np.float32)
        ids = np.empty((m, MAX_LOGPROBS), dtype=np.int32)
        tlp = np.empty((m, MAX_LOGPROBS), dtype=np.float32)
        tn = np.empty(m, dtype=np.int32)
        self._check(self.be.read_row_logprobs(self._ctx, row, n, lp.ctypes.data_as(POINTER(c_float)), ids.ctypes.data_as(POINTER(c_int32)),
                                              tlp.ctypes.data_as(POINTER(c_float)), tn.ctypes.data_as(POINTER(c_int32))))
        return lp[:n], ids[:n], tlp[:n], tn[:n]

    # -- per-row logit processors (include/tgx.h tgx_set_row_penalties) --------------------------
    def set_row_penalties(self, row: int, repetition: float = 1.0, presence: float = 0.0, frequency: float = 0.0):
        cfg = PenaltyCfg(repetition, presence, frequency)
        self._check(self.be.set_row_penalties(self._ctx, row, ctypes.byref(cfg)))
        return self

    def set_row_logit_bias(self, row: int, bias=None):
        """bias: {id: value} or a sequence of (id, value) pairs; empty / None clears.  -inf bans an id"""
        pairs = list(bias.items()) if isinstance(bias, dict) else list(bias or ())
        ids = np.ascontiguousarray(np.asarray([p[0] for p in pairs], dtype=np.int32).reshape(-1))
        val = np.ascontiguousarray(np.asarray([p[1] for p in pairs], dtype=np.float32).reshape(-1))
        self._check(self.be.set_row_logit_bias(self._ctx, row, len(ids), ids.ctypes.data_as(POINTER(c_int32)) if len(ids) else None,
                                               val.ctypes.data_as(POINTER(c_float)) if len(ids) else None))
        return self

    # -- token automata (include/tgx.h tgx_automaton_create) ------------------------------------
    def automaton_create(self, next, start: int = 0) -> int:
        """next: uint16 [n_states][vocab], 0xFFFF = not allowed; returns the table's id"""
        t = np.ascontiguousarray(next)
        if t.dtype != np.uint16 or t.ndim != 2 or t.shape[1] != self.desc.vocab:
            raise ValueError(f"automaton table: uint16 [n_states][{self.desc.vocab}] expected, got {t.dtype} {t.shape}")
        out = c_int32(-1)
        self._check(self.be.automaton_create(self._ctx, t.shape[0], start, t.ctypes.data_as(POINTER(ctypes.c_uint16)), ctypes.byref(out)))
        return out.value

    def automaton_destroy(self, aid: int):
        self._check(self.be.automaton_destroy(self._ctx, aid))
        return self

    def set_row_automaton(self, row: int, aid: int = -1, state: int = -1):
        """aid -1 switches the row off; state -1 is the table's start"""
        self._check(self.be.set_row_automaton(self._ctx, row, aid, state))
        return self

    def read_row_automaton(self, row: int):
        """(id, state) of the row as it stands (-1, -1: none); synchronises"""
        i, s = c_int32(-1), c_int32(-1)
        self._check(self.be.read_row_automaton(self._ctx, row, ctypes.byref(i), ctypes.byref(s)))
        return i.value, s.value

    def set_row_history(self, row: int, prompt_ids=(), produced_ids=()):
        """REPLACES the row's history words: the prompt bit of every id in prompt_ids, the produced count of every id in produced_ids"""
        p = np.ascontiguousarray(np.asarray(list(prompt_ids), dtype=np.int64).reshape(-1))
        g = np.ascontiguousarray(np.asarray(list(produced_ids), dtype=np.int64).reshape(-1))
        self._check(self.be.set_row_history(self._ctx, row, p.ctypes.data_as(POINTER(c_int64)) if len(p) else None, len(p),
                                            g.ctypes.data_as(POINTER(c_int64)) if len(g) else None, len(g)))
        return self

    def score_row(self, row: int, ids, top_n: int = 0):
        """tgx_forward_row (an empty row) or tgx_extend_row (a row that holds a sequence) of `ids`, plus the log-probability of every supplied token (include/tgx.h
        tgx_score_row): (lp [n], top_ids [n][TGX_MAX_LOGPROBS], top_lp likewise), n = len(ids) - 1; lp[i] is ids[i + 1]'s under position i's distribution"""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        n = max(len(ids) - 1, 0)
        lp = np.empty(n, np.float32)
        top_ids = np.empty((n, MAX_LOGPROBS), np.int32)
        top_lp = np.empty((n, MAX_LOGPROBS), np.float32)
        self._check(self.be.score_row(self._ctx, row, ids.ctypes.data_as(POINTER(c_int64)), len(ids), top_n, lp.ctypes.data_as(POINTER(c_float)),
                                      top_ids.ctypes.data_as(POINTER(c_int32)), top_lp.ctypes.data_as(POINTER(c_float))))
        self.batch = max(self.batch, row + 1)
        return lp, top_ids, top_lp

    @property
    def past_length(self) -> int:
        return self.be.past_length(self._ctx)

    @property
    def context_size(self) -> int:
        return self.be.context_size(self._ctx)

    def synchronize(self):
        self._check(self.be.synchronize(self._ctx))

    def read_kv(self, row: int, layer: int):
        T = self.be.past_length_row(self._ctx, row) if self.be.has("past_length_row") else self.past_length
        shape = (T, self.desc.kv_heads, self.desc.head_dim)
        k = np.empty(shape, dtype=np.float32)
        v = np.empty(shape, dtype=np.float32)
        self._check(self.be.read_kv(self._ctx, row, layer, k.ctypes.data_as(POINTER(c_float)), v.ctypes.data_as(POINTER(c_float))))
        return k, v

    def write_kv(self, row: int, layer: int, k: np.ndarray, v: np.ndarray):
        """overwrite cache rows [0, len(k)) of (row, layer) from fp32 [T][kv_heads][head_dim] arrays (the layout read_kv returns)"""
        k = np.ascontiguousarray(k, dtype=np.float32); v = np.ascontiguousarray(v, dtype=np.float32)
        assert k.shape == v.shape and k.shape[1:] == (self.desc.kv_heads, self.desc.head_dim)
        self._check(self.be.write_kv(self._ctx, row, layer, k.ctypes.data_as(POINTER(c_float)), v.ctypes.data_as(POINTER(c_float)), k.shape[0]))

    def profile_decode(self, n_steps: int):
        n = len(KERNEL_CLASSES)
        launches = (c_int64 * n)()
        ms = (c_double * n)()
        self._check(self.be.profile_decode(self._ctx, n_steps, launches, ms))
        return {k: (launches[i], ms[i]) for i, k in enumerate(KERNEL_CLASSES)}

    def probs(self) -> np.ndarray:
        out = np.empty((self.batch, self.desc.vocab), dtype=np.float32)
        self._check(self.be.read_probs(self._ctx, out.ctypes.data_as(POINTER(c_float))))
        return out

    def set_logits(self, logits):
        l = np.ascontiguousarray(np.atleast_2d(np.asarray(logits, dtype=np.float32)))
        self._check(self.be.set_logits(self._ctx, l.ctypes.data_as(POINTER(c_float)), l.shape[0]))
        self.batch = l.shape[0]
        return self

    def set_option(self, key: str, value: int):
        self._check(self.be.set_option(self._ctx, key.encode(), int(value)))
        return self

    def get_option(self, key: str) -> int:
        out = c_int(0)
        self._check(self.be.get_option(self._ctx, key.encode(), ctypes.byref(out)))
        return out.value

    def bytes_per_token(self, T: int) -> int:
        return self.be.bytes_per_token(self._ctx, T)
