"""The layout space of the FP8 / MXFP4 weight streams (kernels/gemv_fp8.h, gemv_fp4.h, skinny_fp8.h, skinny_fp4.h): a table of small models whose gate_up, down
and lm_head meet every layout the kernels index, and the host rules that decide which kernel serves each product, written out again in Python.  No GPU.

tests/test_stream_shapes.py holds the table to the reach list below; tests/test_hip_stream_shapes.py runs every case bit for bit against the master path and
holds the counters to predict_step().

The rules are transcriptions: stream_nx (csrc/ctx.h) / gemv_auto_ks / launch_gemv's R = 2 rules (csrc/decode.hip), the quantizer's layout choice per form
(quantize_weights), launch_skinny's split rule, skinny_fp8_covers / skinny_fp4_covers, and the branches of launch_decode_step_mfma that hand a product to
launch_skinny (csrc/skinny.hip).  A change to one of those shows here as a counter mismatch on the GPU, with both geometries printed.

Shapes: only the dimension under test is large.  K = hidden cases take intermediate 512 and a vocabulary of a few hundred; K = intermediate cases take hidden
512.  Family qwen3 lets heads * head_dim (128) differ from hidden.  The FP8 rows kernel takes split ranges of whole 512-k runs only, which launch_skinny gives a
512-row down from K = 8192 on: that, not the layout, is why the largest cases hold 8192 .. 14336 columns."""
from dataclasses import dataclass

from tinygpt_amd.desc import ModelDesc

SEED, STD = 77, 0.05                     # tests/test_hip_fuzz.py's weight std: its 6e-3 bound against the oracle is for such models
BUDGET_BYTES = 56 << 20                  # bf16 bytes of all tensors of a case: two layers of 512 x 8192 (the smallest two-layer model whose FP8 down streams) fit
CLASSES = ("gateup", "down", "lmhead")
SKINNY_WGS = 256
M_VALUES = (3, 16, 17, 32, 33, 48, 49, 64)


@dataclass(frozen=True)
class Case:
    name: str
    hidden: int
    inter: int
    vocab: int
    ks: tuple = (None, None, None)       # gateup.ks / down.ks / lmhead.ks set before finalize (None: the default)
    rows: tuple = (5,)                   # row counts of forward_rows + decode_rows
    layers: int = 1
    tied: bool = True
    plant: bool = False                  # plant_all_codes / scales apart on every quantized matrix
    oracle: bool = False                 # also against the CPU oracle
    passes: bool = False                 # verify_row (M = 3) and extend_row (M = 16)
    opts: tuple = ()                     # further options of both contexts, set after finalize
    family: str = "qwen3"
    heads: int = 2
    kv_heads: int = 1
    head_dim: int = 64

    def desc(self, max_batch=None):
        return ModelDesc(family=self.family, hidden=self.hidden, layers=self.layers, heads=self.heads, kv_heads=self.kv_heads, head_dim=self.head_dim,
                         inter=self.inter, vocab=self.vocab, max_ctx=96, qkv_bias=False, tied=self.tied, compute_dtype="bf16", norm_eps=1e-5,
                         rope_theta=10000.0, n_positions=0, max_batch=max_batch or max(self.rows), qk_norm=True)

    def weight_bytes(self):
        return 2 * sum(int(s[0]) * (int(s[1]) if len(s) > 1 else 1) for s in self.desc().tensor_shapes().values())


# K = hidden (gate_up and lm_head; unsplit on the rows kernels).  hidden x ks from {512, 1024, 1536, 2560, 3584, 4096, 4608} x {1, 2, 4}, less what the reach
# list does not need, plus 3072 (NX = 6 is on neither axis of the issue's list).  Down has K = 512 throughout: NX = 1 at ks = 2, its second k-part all padding.
HIDDEN_CASES = [
    Case("h512", 512, 512, 200, rows=(3, 64), plant=True),                                    # NX 1: one run in the whole product
    Case("h1024_ks2", 1024, 512, 320, ks=(2, None, 2), rows=(16,)),                           # NX 1, ks 2
    Case("h1024", 1024, 512, 200, rows=(33,)),                                                # NX 2
    Case("h1536", 1536, 512, 200, rows=(5, 17), plant=True, passes=True),                     # NX 3
    Case("h3584_ks2", 3584, 512, 200, ks=(2, None, 2), rows=(32,)),                           # NX 4 (3.5: padded)
    Case("h2560", 2560, 512, 200, rows=(48,)),                                                # NX 5
    Case("h3072", 3072, 512, 200, rows=(49,)),                                                # NX 6
    Case("h3584", 3584, 512, 200, rows=(5,)),                                                 # NX 7
    Case("h4096", 4096, 512, 200, rows=(5, 33), plant=True, oracle=True),                     # NX 8: the 7B / 8B gate_up and lm_head
    Case("h2560_ks4", 2560, 512, 200, ks=(4, None, 4), rows=(17,)),                           # NX 2, ks 4: k-part 2 half padding, k-part 3 all padding
    Case("h4608", 4608, 512, 200, rows=(5,)),                                                 # ks 1 asked, 2 laid out (gemv_auto_ks): NX 5 (4.5: padded)
]
# K = intermediate (down; split by launch_skinny) at hidden 512
DOWN_CASES = [
    Case("d1536_ks1", 512, 1536, 200, ks=(None, 1, None), rows=(5,)),                         # NX 3; ranges of 256 k
    Case("d2048", 512, 2048, 200, rows=(16,)),                                                # NX 2 at the default ks 2
    Case("d4096_ks1", 512, 4096, 200, ks=(None, 1, None), rows=(5,)),                         # NX 8; ranges of 256 k
    Case("d8192_ks2_x2", 512, 8192, 200, ks=(None, 2, None), rows=(5, 49), layers=2, tied=False, oracle=True),      # NX 8; ranges of 512 k; two layers, own head
    Case("d10240", 512, 10240, 200, rows=(5,), oracle=True),                                  # NX 5 (ks 4); ranges of 768 k
    Case("d14336", 512, 14336, 200, rows=(5,)),                                               # NX 7 (ks 4); ranges of 1024 k
]
# paths no default reaches at these sizes.  launch_skinny leaves down unsplit (GEMM_RESIDUAL in the stream kernel) only from hidden ~11000 on or with the
# split rule off; a batch above 64 rows runs as ONE eight-block pass unless decode.step_rows is 64
OPTION_CASES = [
    Case("h512_unsplit", 512, 512, 200, rows=(5,), opts=(("prefill.splitk", 0),)),
    Case("h512_b67", 512, 512, 200, rows=(67,), opts=(("decode.step_rows", 64),)),
]
SHAPES = HIDDEN_CASES + DOWN_CASES + OPTION_CASES
FORMS = ("fp8", "fp4")
CASES = [(form, c) for form in FORMS for c in SHAPES]


def case_id(fc):
    return f"{fc[0]}-{fc[1].name}"


# ---- csrc/decode.hip ----------------------------------------------------------------------------------------------------------------------------------
def gemv_nx(K, ks):
    return (K // 8 + ks * 64 - 1) // (ks * 64)


def gemv_auto_ks(K, want):
    ks = want
    while ks < 4 and gemv_nx(K, ks) > 8:
        ks *= 2
    return ks


def default_ks(cls, case):
    """tgx_create's Tune::ks at bf16 storage"""
    return (4 if case.inter >= 8192 else 2) if cls == "down" else 1


def wanted_ks(cls, case):
    return case.ks[CLASSES.index(cls)] or default_ks(cls, case)


def gemv_launch_ks(K, want, R, cls):
    """the K split launch_gemv runs a class at for R batch rows"""
    ks = gemv_auto_ks(K, want)
    while R > 1 and ks < 4 and gemv_nx(K, ks) > 4:
        ks *= 2
    if R == 2 and cls == "gateup" and ks == 1 and gemv_nx(K, 1) == 4:
        ks = 2
    return ks


@dataclass(frozen=True)
class Layout:
    """the stream quantize_weights lays out for one matrix"""
    form: str
    N: int
    K: int
    ks: int
    nx: int
    stream: bool

    @property
    def row_bytes(self):
        return self.ks * ((self.nx + 1) // 2) * 1024 if self.form == "fp8" else self.ks * self.nx * 272

    @property
    def full(self):
        return self.nx >> 2

    @property
    def rem(self):
        return self.nx & 3

    @property
    def padded(self):
        """the last k-part holds fewer than 64 NX chunks"""
        return self.ks * self.nx * 64 > self.K // 8

    def geometry(self):
        return f"{self.form} N={self.N} K={self.K} ks={self.ks} NX={self.nx} FULL={self.full} REM={self.rem} padded={int(self.padded)} stream={int(self.stream)}"


def dims(cls, case):
    """(N, K) of a class's matrix"""
    return {"gateup": (2 * case.inter, case.hidden), "down": (case.hidden, case.inter), "lmhead": (case.vocab, case.hidden)}[cls]


def layout(form, cls, case):
    N, K = dims(cls, case)
    assert K <= 16384                    # (down beyond 16384 columns is laid out as several K ranges: tests/test_hip_fp4.py's 28672)
    ks = gemv_auto_ks(K, wanted_ks(cls, case))
    nx = gemv_nx(K, ks)
    return Layout(form, N, K, ks, nx, nx <= 8 and K % (8 if form == "fp8" else 32) == 0)


def gemv_streams(lay, cls, case, R):
    """launch_gemv: the batch-1 stream kernel, for one row and a stream laid out for the launch's K split"""
    return lay.stream and R == 1 and lay.ks == gemv_launch_ks(lay.K, wanted_ks(cls, case), R, cls)


# ---- csrc/skinny.hip ----------------------------------------------------------------------------------------------------------------------------------
def skinny_cfg(N, num_cus):
    return 2 if (N + 127) // 128 >= 2 * num_cus else 0


def skinny_split(M, N, K, allow_split, num_cus=256, splitk=1):
    """launch_skinny for a two-term product on stored terms: (mb, cfg, kp, nsplit, k_per); k_per 0: unsplit.  (The slab buffer holds 16 splits of the widest
    product, ensure_skinny_ws, so its size never cuts a split here.)"""
    mb = 8 if M > 64 else 4 if M > 32 else 2 if M > 16 else 1
    cfg = skinny_cfg(N, num_cus)
    kp = 128 if cfg == 1 else 256
    panels = (K + kp - 1) // kp
    rows = 128 if cfg == 2 else 64
    gx = (N + rows - 1) // rows
    nsplit, k_per = 1, 0
    if allow_split and splitk and gx < SKINNY_WGS:
        nsplit = max(1, min(16, panels, (SKINNY_WGS + gx // 2) // gx))
    if nsplit > 1:
        k_per = (panels + nsplit - 1) // nsplit * kp
        nsplit = (K + k_per - 1) // k_per
    return mb, cfg, kp, nsplit, k_per


def covers(lay, M, k_per):
    """skinny_fp8_covers / skinny_fp4_covers at bf16 storage"""
    if not lay.stream or M < 1 or M > 64 or lay.K < 512 or lay.K % 512:
        return False
    if k_per and k_per % (512 if lay.form == "fp8" else 64):
        return False
    return lay.nx <= 8


@dataclass(frozen=True)
class Product:
    cls: str
    lay: Layout
    M: int
    counted: bool            # inside the row limit and handed the quantized matrix: one of the two row counters moves
    streams: bool
    epi: str
    mb: int
    nsplit: int
    k_per: int

    @property
    def ranges(self):
        if not self.k_per:
            return [(0, self.lay.K)]
        return [(s * self.k_per, min(self.lay.K, (s + 1) * self.k_per)) for s in range(self.nsplit)]

    def geometry(self):
        r = self.ranges
        return (f"{self.cls} M={self.M} MB={self.mb} {self.epi} {'STREAM' if self.streams else 'fallback' if self.counted else 'uncounted'} "
                f"{len(r)} range(s) of {r[0][1] - r[0][0]} k | {self.lay.geometry()}")


def option(case, key, default):
    return dict(case.opts).get(key, default)


def predict_product(form, cls, case, M, limit=64):
    """one product of launch_decode_step_mfma for M rows under weights.fp8_rows / weights.fp4_rows = limit"""
    lay = layout(form, cls, case)
    N, K = dims(cls, case)
    # fp8_rows_mat hands out every quantized matrix, fp4_rows_mat only one that owns a stream
    handed = 3 <= M <= limit and (form == "fp8" or lay.stream)
    # gate_up and lm_head never split (allow_split false); a product that covers unsplit bypasses the K-split kernel and takes stored terms: gate_up through
    # the `terms || gu_q8` branch, lm_head because `terms` holds from 3 rows on at hidden % 64 == 0 (skinny.dma is on)
    mb, cfg, kp, nsplit, k_per = skinny_split(M, N, K, cls == "down", splitk=option(case, "prefill.splitk", 1))
    streams = handed and mb <= 4 and covers(lay, M, k_per)
    epi = "PARTIAL" if nsplit > 1 else {"gateup": "SILU", "down": "RESIDUAL", "lmhead": "STORE"}[cls]
    return Product(cls, lay, M, handed, streams, epi, mb, nsplit, k_per)


def step_passes(case, rows):
    """the row counts of the launch_decode_step_mfma calls of one step of `rows` live rows (launch_decode_step; the defaults make wide_ok true)"""
    per = option(case, "decode.step_rows", 128)
    return [min(per, rows - r0) for r0 in range(0, rows, per)]


def predict_step(form, case, rows, limit=64):
    """every quantized product of one eager decode step and the counter deltas (row_products, row_fallbacks)"""
    prods = []
    for M in step_passes(case, rows):
        for _ in range(case.layers):
            prods += [predict_product(form, "gateup", case, M, limit), predict_product(form, "down", case, M, limit)]
        prods.append(predict_product(form, "lmhead", case, M, limit))
    return prods, (sum(p.streams for p in prods), sum(p.counted and not p.streams for p in prods))


def predict_finalize(form, case):
    """(<form>_matrices, <form>_fallbacks) after tgx_finalize"""
    lays = [layout(form, cls, case) for cls in ("gateup", "down")] * case.layers + [layout(form, "lmhead", case)]
    return sum(l.stream for l in lays), sum(not l.stream for l in lays)


# ---- the reach list -------------------------------------------------------------------------------------------------------------------------------------
def reach_list():
    """the features a streamed product must meet at least once, per form (the issue's list; K no multiple of 512 stays with the tiny families' modules)"""
    out = []
    for form in FORMS:
        b1 = [f"nx{n}" for n in range(1, 9)] + [f"ks{k}" for k in (1, 2, 4)] + ["padded"]
        rows = ([f"nx{n}" for n in range(1, 9)] + ["nx1_single_run"] + [f"ks{k}" for k in (1, 2, 4)] + ["padded", "unsplit", "split_whole_runs"] +
                [f"mb{m}" for m in (1, 2, 4)] + [f"m{m}" for m in M_VALUES] + [f"epi_{e}" for e in ("SILU", "RESIDUAL", "PARTIAL", "STORE")] +
                ["vocab_odd", "two_layers_untied", "batch_over_64"])
        if form == "fp4":
            rows += ["split_inside_run", "range_from_second_half"] + [f"rem{r}_full{f}" for r in (1, 2, 3) for f in (0, 1)]
        out += [f"{form}.b1.{f}" for f in b1] + [f"{form}.rows.{f}" for f in rows]
    return out


def features(form, case):
    """the features of the reach list that this case's streamed products meet"""
    got = set()
    for cls in CLASSES:
        lay = layout(form, cls, case)
        if gemv_streams(lay, cls, case, 1):
            got |= {f"b1.nx{lay.nx}", f"b1.ks{lay.ks}"} | ({"b1.padded"} if lay.padded else set())
    for rows in case.rows:
        prods, _ = predict_step(form, case, rows)
        live = [p for p in prods if p.streams]
        for p in live:
            lay = p.lay
            got |= {f"rows.nx{lay.nx}", f"rows.ks{lay.ks}", f"rows.mb{p.mb}", f"rows.epi_{p.epi}", f"rows.m{p.M}"}
            if lay.padded: got.add("rows.padded")
            if lay.K == 512 and not p.k_per: got.add("rows.nx1_single_run")
            if not p.k_per: got.add("rows.unsplit")
            elif p.k_per % 512 == 0: got.add("rows.split_whole_runs")
            else: got.add("rows.split_inside_run")
            if lay.rem and lay.full <= 1: got.add(f"rows.rem{lay.rem}_full{lay.full}")
            # a range whose first run is slot 2 or 3 of its quad: the kernel's first load is a quad's second half, which then brings the scales
            if lay.nx != 4 and any(((b >> 9) % lay.nx) & 2 for b, _ in p.ranges): got.add("rows.range_from_second_half")
            if p.cls == "lmhead" and case.vocab % 64 and case.vocab != 129: got.add("rows.vocab_odd")
        per_cls = {c: all(p.streams for p in prods if p.cls == c) for c in CLASSES}
        if case.layers >= 2 and not case.tied and per_cls["gateup"] and per_cls["down"]: got.add("rows.two_layers_untied")
        passes = step_passes(case, rows)
        if rows > 64 and passes[0] == 64 and 3 <= passes[-1] <= 6 and {p.M for p in live} == set(passes): got.add("rows.batch_over_64")
    return {f"{form}.{f}" for f in got}


def step_table(form, case):
    """the summary's row of a case: class -> NX, ks, ranges and streamed or not, per row count"""
    lines = []
    for rows in case.rows:
        prods, delta = predict_step(form, case, rows)
        seen = []
        for p in prods:
            if p.geometry() not in seen:
                seen.append(p.geometry())
        lines.append(f"{form}-{case.name} rows={rows} products/fallbacks={delta}: " + "; ".join(seen))
    return lines
