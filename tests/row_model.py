"""A host-only model of the per-row contract of include/tgx.h, a test double that answers the row calls from it, and the driver that fuzzes a device with random
call sequences against both (tests/test_row_model.py on a CPU, tests/test_hip_row_fuzz.py on the GPU).

  RowModel      per row: state (empty / retired / live / finished), has_logits / has_token, the token list in the cache and the current token, sampler and stop
                settings, produced count, logprob switch and record count.  Per context: batch, max_batch, max_ctx and — paged — an abstract block pool (block ids
                with reference counts) that follows the header's rules.  status(kind, ...) is the status code the header promises, apply(kind, ...) the new state;
                free_tokens() the exact kv.free_tokens.  Written from the TEXT of include/tgx.h: where two refusal reasons with different codes would hold at once
                the header does not say which wins, and status() asserts that no such call is made.
  OracleDevice  tinygpt_amd.ffi.Model's row methods answered by a RowModel plus one batch-1 CPU oracle per row: what makes the driver, the model and the coverage
                conditions testable without a GPU.  What a reader sees of a row (cache rows, logits, records) is held here, so copies are copies bit for bit.
  Mirror        the reference of the numeric checks: per row an oracle and its reordered twin, fed the row's token list.
  run_sequence  draws operations, predicts each with the model, runs it on the device and checks what include/tgx.h promises after every one.
"""
from __future__ import annotations

import pickle
import time

import numpy as np

from conftest import load_golden, rel_err
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, SamplerCfg, TgxError

OK, INVALID, UNSUPPORTED, STATE, CONTEXT = 0, 1, 2, 4, 8
BLK = 128
MAX_STOP, MAX_DRAFT, MAX_LOGPROBS, LOGPROB_RING = 8, 15, 20, 256
EMPTY, RETIRED, LIVE, FINISHED = "empty", "retired", "live", "finished"
GREEDY_T = (0.0, 0, 1.0, 0.0)
LENS = [1, 2, 17, 33, 100, 126, 127, 128, 129, 200, 255, 256, 257]
FAMS = ["llama_tiny", "qwen2_tiny", "mistral_tiny", "qwen3_tiny", "gpt2_hd64"]
ARMS = ["f32_slab", "h16_slab", "h16_paged"]
MAX_CTX = 384


def is_greedy(s):
    return not (s[0] > 0 or s[1] > 0 or s[2] < 1 or s[3] > 0)


def blocks_for(n):
    return (n + BLK - 1) // BLK


class Snap:
    """what a snapshot holds of a row, as far as the contract goes"""
    def __init__(self, row):
        self.tokens = list(row.tokens); self.has_logits = row.has_logits; self.has_token = row.has_logits and row.has_token
        self.tok = row.tok if self.has_token else None


class Row:
    def __init__(self):
        self.state = EMPTY; self.blocks = []; self.fin_code = 0
        self.settings_default(); self.drop_sequence()

    def settings_default(self):
        self.sampler, self.seed = GREEDY_T, 0
        self.max_new, self.stop_ids, self.produced = 0, (), 0
        self.lp, self.lp_count = -1, 0

    def drop_sequence(self):
        self.tokens = []; self.tok = None; self.has_logits = False; self.has_token = False

    @property
    def holds(self):
        return self.state in (LIVE, FINISHED)

    @property
    def length(self):
        return len(self.tokens) if self.holds else 0

    def note_produced(self, t):
        """the stop rule of tgx_set_row_stop: 1 a stop id (it takes precedence), 2 the max_new-th token, 0 running"""
        self.produced += 1
        if t in self.stop_ids:
            return 1
        return 2 if self.max_new > 0 and self.produced >= self.max_new else 0


class Pool:
    """block ids with reference counts; a block is free at count 0"""
    def __init__(self, budget_tokens):
        self.total = blocks_for(budget_tokens)
        self.free = list(range(self.total - 1, -1, -1)); self.ref = {}

    def take(self):
        b = self.free.pop(); self.ref[b] = 1
        return b

    def drop(self, b):
        self.ref[b] -= 1
        if self.ref[b] == 0:
            del self.ref[b]; self.free.append(b)

    def shared(self, b):
        return self.ref[b] > 1


class RowModel:
    def __init__(self, max_batch, max_ctx, vocab, budget_tokens=0):
        self.max_batch, self.max_ctx, self.vocab = max_batch, max_ctx, vocab
        self.batch = 0
        self.rows = [Row() for _ in range(max_batch)]
        self.pool = Pool(budget_tokens) if budget_tokens else None
        self.budget = self.pool.total * BLK if self.pool else -1
        self.cov = {}          # coverage counters of what the pool and the rows went through

    # ---- figures a reader of the device sees
    def free_tokens(self):
        return len(self.pool.free) * BLK if self.pool else -1

    def past_length_row(self, r):
        return self.rows[r].length

    def past_length(self):
        return max([x.length for x in self.rows[:self.batch] if x.state == LIVE] + [0])

    def note(self, what):
        self.cov[what] = self.cov.get(what, 0) + 1

    # ---- the pool rules of include/tgx.h
    def _given_back(self, rows):
        return sum(1 for r in rows for b in self.rows[r].blocks if not self.pool.shared(b))

    def _release(self, r):
        self._trim(r, 0)

    def _trim(self, r, tokens):
        row = self.rows[r]
        while len(row.blocks) > blocks_for(tokens):
            self.pool.drop(row.blocks.pop())

    def _grow(self, r, tokens):
        row = self.rows[r]
        while len(row.blocks) < blocks_for(tokens):
            row.blocks.append(self.pool.take())

    def _more(self, r, tokens):
        return max(0, blocks_for(tokens) - len(self.rows[r].blocks))

    def _short(self, need, have, reasons):
        if self.pool and need > have:
            reasons.append((CONTEXT, "pool"))

    # ---- status: every reason the header gives for refusing the call
    def _in(self, r):
        return 0 <= r < self.max_batch

    def _targets(self, rows, reasons, src=None):
        if any(not self._in(r) for r in rows):
            reasons.append((INVALID, "row_range")); return
        if len(set(rows)) != len(rows) or src in rows:
            reasons.append((INVALID, "row_twice")); return
        new = sorted(r for r in rows if r >= self.batch)
        if new != list(range(self.batch, self.batch + len(new))):
            reasons.append((INVALID, "new_row_not_batch"))
        if any(self.rows[r].holds for r in rows):
            reasons.append((STATE, "target_live"))

    def _source(self, r, reasons, what):
        """a live, unfinished row of the batch that holds >= 1 positions"""
        if not self._in(r):
            reasons.append((INVALID, "row_range")); return False
        row = self.rows[r]
        if row.state == FINISHED:
            reasons.append((STATE, what + "_finished"))
        elif row.state != LIVE:
            reasons.append((STATE, what + "_retired"))
        return row.state == LIVE

    def reasons(self, kind, *a):
        rs = []
        getattr(self, "_why_" + kind)(rs, *a)
        return rs

    def status(self, kind, *a):
        rs = self.reasons(kind, *a)
        codes = {c for c, _ in rs}
        assert len(codes) <= 1, f"{kind}{a}: the header does not say which of {rs} wins — the generator must not draw this call"
        return (rs[0][0], rs[0][1]) if rs else (OK, "")

    def _why_forward_rows(self, rs, rows, prompts):
        if len(rows) < 1:
            rs.append((INVALID, "n")); return
        self._targets(rows, rs)
        if any(len(p) < 1 for p in prompts):
            rs.append((INVALID, "len"))
        if any(len(p) > self.max_ctx for p in prompts):
            rs.append((CONTEXT, "max_ctx"))
        if not rs:
            self._short(sum(blocks_for(len(p)) for p in prompts), len(self.pool.free) + self._given_back(rows) if self.pool else 0, rs)

    def _why_forward_row(self, rs, row, ids):
        self._why_forward_rows(rs, [row], [ids])

    def _why_reset_row(self, rs, row):
        if not self._in(row):
            rs.append((INVALID, "row_range"))

    def _why_set_row_sampler(self, rs, row, sampler, seed):
        if not self._in(row):
            rs.append((INVALID, "row_range"))

    def _why_set_row_stop(self, rs, row, max_new, stop_ids):
        if not self._in(row):
            rs.append((INVALID, "row_range"))
        if len(stop_ids) > MAX_STOP:
            rs.append((INVALID, "n_stop"))

    def _why_set_row_logprobs(self, rs, row, top_n):
        if not self._in(row):
            rs.append((INVALID, "row_range"))
        if not -1 <= top_n <= MAX_LOGPROBS:
            rs.append((INVALID, "top_n"))

    def _why_sample_row(self, rs, row):
        # the header defines the call for a live row of the batch that holds logits, and refuses a truncated one; nothing else is drawn
        assert self._in(row) and row < self.batch and self.rows[row].state == LIVE, "sample_row is drawn on live rows only"
        if not self.rows[row].has_logits:
            rs.append((STATE, "truncated"))

    def _stepping(self):
        return [r for r in range(self.batch) if self.rows[r].state == LIVE]

    def _why_steps(self, rs, n, rows_call):
        live = self._stepping()
        if not live:
            rs.append((STATE, "nothing_to_step"))
        if any(not self.rows[r].has_logits for r in live):
            rs.append((STATE, "truncated"))
        elif any(not self.rows[r].has_token for r in live):
            rs.append((STATE, "no_token"))
        fin = [r for r in range(self.batch) if self.rows[r].state == FINISHED]
        if fin and not rows_call:
            rs.append((STATE, "finished_row"))
        if live and max(self.rows[r].length for r in live) + n > self.max_ctx:
            rs.append((CONTEXT, "max_ctx"))
        if rows_call and any(self.rows[r].length >= self.max_ctx for r in fin):
            rs.append((CONTEXT, "finished_at_max_ctx"))
        if not rs and self.pool:
            self._short(sum(self._more(r, self.rows[r].length + n) for r in live), len(self.pool.free), rs)

    def _why_decode_rows(self, rs, n):
        assert n >= 1
        self._why_steps(rs, n, True)

    def _why_decode(self, rs, n):
        assert n >= 1
        self._why_steps(rs, n, False)

    def _why_fork_row(self, rs, src, dsts):
        if len(dsts) < 1:
            rs.append((INVALID, "n")); return
        if self._source(src, rs, "src") and not self.rows[src].has_logits:
            rs.append((STATE, "truncated"))
        self._targets(dsts, rs, src)
        if not rs and self.pool:
            tail = self.rows[src].length % BLK != 0
            self._short(len(dsts) if tail else 0, len(self.pool.free) + self._given_back(dsts), rs)

    def _why_extend_row(self, rs, row, ids):
        if not self._in(row):
            rs.append((INVALID, "row_range")); return
        if len(ids) < 1:
            rs.append((INVALID, "len"))
        x = self.rows[row]
        if not x.holds:
            rs.append((STATE, "extend_retired")); return
        if x.length + len(ids) > self.max_ctx:
            rs.append((CONTEXT, "max_ctx"))
        if not rs and self.pool:
            self._short(self._more(row, x.length + len(ids)), len(self.pool.free), rs)

    def _why_score_row(self, rs, row, ids):
        if self._in(row) and self.rows[row].holds:
            self._why_extend_row(rs, row, ids)
        else:
            self._why_forward_row(rs, row, ids)

    def _cow(self, row, new_len):
        x = self.rows[row]
        return bool(self.pool) and new_len % BLK != 0 and self.pool.shared(x.blocks[blocks_for(new_len) - 1])

    def _why_truncate_row(self, rs, row, new_len):
        if not self._in(row):
            rs.append((INVALID, "row_range")); return
        x = self.rows[row]
        if not x.holds:
            rs.append((STATE, "truncate_retired")); return
        if new_len < 1 or new_len > x.length:
            rs.append((INVALID, "new_len")); return
        assert not (new_len == x.length and x.state == FINISHED), "the header does not say what new_len == past does to a finished row"
        if new_len == x.length and x.has_logits:
            return
        if self._cow(row, new_len) and not self.pool.free:
            rs.append((CONTEXT, "pool"))

    def _why_verify_row(self, rs, row, draft):
        if not self._in(row):
            rs.append((INVALID, "row_range")); return
        if not 1 <= len(draft) <= MAX_DRAFT:
            rs.append((INVALID, "n_draft"))
        if not self._source(row, rs, "verify"):
            return
        x = self.rows[row]
        if not x.has_logits:
            rs.append((STATE, "truncated"))
        elif not x.has_token:
            rs.append((STATE, "no_token"))
        if not is_greedy(x.sampler):
            rs.append((UNSUPPORTED, "sampled_row"))
        if x.length + len(draft) + 1 > self.max_ctx:
            rs.append((CONTEXT, "max_ctx"))
        if not rs and self.pool:
            self._short(self._more(row, x.length + len(draft) + 1), len(self.pool.free), rs)

    def _why_save_row(self, rs, row):
        self._source(row, rs, "save")

    def _why_restore_row(self, rs, row, snap):
        self._targets([row], rs)
        if len(snap.tokens) > self.max_ctx:
            rs.append((CONTEXT, "max_ctx"))
        if not rs and self.pool:
            self._short(blocks_for(len(snap.tokens)), len(self.pool.free) + self._given_back([row]), rs)

    # ---- apply: the state after a call that returned TGX_OK.  `out` is what the device produced (ids); the counts it reported are checked against the stop rules
    def apply(self, kind, *a, out=None):
        return getattr(self, "_do_" + kind)(*a) if out is None else getattr(self, "_do_" + kind)(*a, out)

    def _admit(self, r, tokens, has_logits=True, has_token=False, tok=None):
        x = self.rows[r]
        x.state = LIVE; x.tokens = list(tokens); x.has_logits = has_logits; x.has_token = has_token; x.tok = tok
        x.produced = 0; x.lp_count = 0
        self.batch = max(self.batch, r + 1)

    def _do_forward_rows(self, rows, prompts):
        if self.pool:
            for r in rows:
                self._release(r)
            for r, p in zip(rows, prompts):
                self._grow(r, len(p))
        for r, p in zip(rows, prompts):
            self._admit(r, p)

    def _do_forward_row(self, row, ids):
        self._do_forward_rows([row], [ids])

    def _do_reset_row(self, row):
        x = self.rows[row]
        if self.pool:
            self._release(row)
        x.state = RETIRED if row < self.batch else EMPTY
        x.drop_sequence(); x.settings_default()

    def _do_set_row_sampler(self, row, sampler, seed):
        self.rows[row].sampler, self.rows[row].seed = tuple(sampler), seed

    def _do_set_row_stop(self, row, max_new, stop_ids):
        x = self.rows[row]
        x.max_new, x.stop_ids, x.produced = max_new, tuple(stop_ids), 0

    def _do_set_row_logprobs(self, row, top_n):
        self.rows[row].lp = top_n

    def _do_sample_row(self, row, tok):
        x = self.rows[row]
        x.has_token, x.tok = True, int(tok)
        if x.lp >= 0:
            x.lp_count += 1

    def _do_decode_rows(self, n, out):
        ids, new, fin = out
        live = self._stepping()
        for r in live:
            if self.pool:
                self._grow(r, self.rows[r].length + n)
        for r in range(self.batch):
            x = self.rows[r]
            if r not in live:
                assert (ids[:, r] == -1).all() and new[r] == 0, f"row {r} ({x.state}) rides along: ids -1, out_new 0, got {ids[:, r]}, {new[r]}"
                assert fin[r] == (x.fin_code if x.state == FINISHED else 0), f"out_finish {fin[r]} for the {x.state} row {r}"
                continue
            start, code, k = x.length, 0, 0
            for s in range(n):
                t = int(ids[s, r])
                if code:
                    assert t == -1, f"row {r} finished at step {k - 1} and reports id {t} at step {s}"
                    continue
                assert 0 <= t < self.vocab, f"row {r} step {s}: id {t}"
                x.tokens.append(x.tok); x.tok = t; k += 1
                code = x.note_produced(t)
            assert new[r] == k and fin[r] == code, f"row {r}: out_new {new[r]} / out_finish {fin[r]}, the stop rules give {k} / {code}"
            if x.lp >= 0:
                x.lp_count += k
            if blocks_for(start) != blocks_for(x.length):
                self.note("decode_rows_crosses_block")
            if code:
                x.state, x.fin_code = FINISHED, code
                if self.pool:
                    if blocks_for(x.length) < len(x.blocks):
                        self.note("finished_row_surplus_block")
                    self._trim(r, x.length)
        return live

    def _do_decode(self, n, ids):
        live = self._stepping()
        for r in live:
            x = self.rows[r]
            if self.pool:
                self._grow(r, x.length + n)
            for s in range(n):
                x.tokens.append(x.tok); x.tok = int(ids[s, r])
        return live

    def _do_fork_row(self, src, dsts):
        s = self.rows[src]
        self.note("fork_tail" if s.length % BLK else "fork_no_tail")
        if self.pool:
            for d in dsts:
                self._release(d)
            for d in dsts:
                for b in s.blocks[:s.length // BLK]:
                    self.pool.ref[b] += 1; self.rows[d].blocks.append(b)
                if s.length % BLK:
                    self.rows[d].blocks.append(self.pool.take())
        for d in dsts:
            self._admit(d, s.tokens, True, s.has_token, s.tok)

    def _do_extend_row(self, row, ids):
        x = self.rows[row]
        if x.state == FINISHED:
            self.note("finished_then_extended")
        if self.pool:
            self._grow(row, x.length + len(ids))
        lp_count = x.lp_count
        self._admit(row, x.tokens + list(ids))
        x.lp_count = lp_count

    def _do_score_row(self, row, ids):
        (self._do_extend_row if self.rows[row].holds else self._do_forward_row)(row, ids)

    def _do_truncate_row(self, row, new_len):
        x = self.rows[row]
        if new_len == x.length and x.has_logits:
            return
        if self._cow(row, new_len):
            self.note("cow_truncation")
            i = blocks_for(new_len) - 1
            old = x.blocks[i]; x.blocks[i] = self.pool.take(); self.pool.drop(old)
        if self.pool:
            self._trim(row, new_len)
        x.state = LIVE; x.tokens = x.tokens[:new_len]; x.has_logits = x.has_token = False; x.tok = None

    def _do_verify_row(self, row, draft, out):
        ids, fin = out
        x = self.rows[row]
        n, start = len(ids), x.length
        assert 1 <= n <= len(draft) + 1, f"out_n {n} for a draft of {len(draft)}"
        assert list(ids[:n - 1]) == list(draft[:n - 1]), f"out_ids {list(ids)} does not start with the accepted draft {list(draft[:n - 1])}"
        if self.pool:
            self._grow(row, x.length + len(draft) + 1)
        code = 0
        for i, t in enumerate(ids):
            assert code == 0, f"verify_row went on after the token that finished the row: {list(ids)}"
            x.tokens.append(x.tok); x.tok = int(t)
            code = x.note_produced(int(t))
        assert code == fin, f"out_finish {fin}, the stop rules give {code} for {list(ids)}"
        if not code and n < len(draft) + 1:
            assert int(ids[-1]) != int(draft[n - 1]), "acceptance ended on a token that equals the draft's"
        if x.lp >= 0:
            x.lp_count += n
        if code:
            x.state, x.fin_code = FINISHED, code
        if blocks_for(start) != blocks_for(x.length):
            self.note("verify_crosses_block")
        if self.pool:
            self._trim(row, x.length)

    def _do_save_row(self, row):
        return Snap(self.rows[row])

    def _do_restore_row(self, row, snap):
        if self.pool:
            self._release(row); self._grow(row, len(snap.tokens))
        self._admit(row, snap.tokens, snap.has_logits, snap.has_token, snap.tok)


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# the random stream behind a (seed, arm), where it is not the seed's own number: chosen in the CPU dry run (tests/test_row_model.py) so that the oracle stays far enough
# from its reordered twin on every sequence
STREAM = {(2, "f32_slab"): 402, (7, "f32_slab"): 407}      # mistral_tiny (hidden 512, head_dim 128) in fp32: 8.5e-6 and 7.0e-6 from the twin, under the 1e-5 the arm asks for


def case(seed, arm):
    """the fixture, dtype and geometry of one (seed, arm)"""
    fam = FAMS[seed % len(FAMS)]
    dtype = "fp32" if arm == "f32_slab" else ("fp16" if seed % 4 == 2 else "bf16")
    rng = np.random.default_rng(90000 + 17 * STREAM.get((seed, arm), seed) + ARMS.index(arm))
    max_batch = int(rng.integers(4, 7))
    budget = blocks_for(int(1.5 * max_batch * BLK)) * BLK if arm == "h16_paged" else 0
    return dict(seed=seed, arm=arm, fam=fam, dtype=dtype, max_batch=max_batch, max_ctx=MAX_CTX, budget=budget, rng=rng)


def make_desc(fam, dtype, max_batch, max_ctx=MAX_CTX):
    cfg, g = load_golden(fam)
    d = desc_from_hf_config(cfg, dtype, max_batch=max_batch)
    d.max_ctx = max_ctx
    if d.n_positions:
        d.n_positions = max_ctx
    return d, int(g["seed"]), float(g["std"])


def new_oracle(fam, dtype, reorder=False):
    from oracle.oracle_ffi import OracleModel
    d, seed, std = make_desc(fam, dtype, 1)
    m = OracleModel(d).load_synthetic(seed, std)
    if reorder:
        m.set_reorder(True)
    return m.finalize()


def lsm64(v, t):
    v = np.asarray(v, np.float64)
    return float(v[t] - (v.max() + np.log(np.exp(v - v.max()).sum())))


class OracleSeq:
    """one batch-1 oracle following a token list: several tokens only into an empty cache, one at a time behind it"""
    def __init__(self, fam, dtype, reorder=False):
        self.o = new_oracle(fam, dtype, reorder); self.toks = []

    def sync(self, tokens, each=None):
        """make the cache hold `tokens`; each(i, logits) is called after token i went in as a single-token forward"""
        tokens = [int(t) for t in tokens]
        n = len(self.toks)
        if n == 0 or self.toks != tokens[:n]:          # nothing to build on: one forward of the whole list
            self.o.reset_cache(); self.toks = []
            if tokens:
                self.o.forward(np.array([tokens], dtype=np.int64)); self.toks = list(tokens)
            return self
        for i in range(n, len(tokens)):
            self.o.forward(np.array([[tokens[i]]], dtype=np.int64)); self.toks.append(tokens[i])
            if each is not None:
                each(i, self.logits())
        return self

    def clear(self):
        self.o.reset_cache(); self.toks = []

    def logits(self):
        return self.o.logits(rounded=False)[0].copy()

    def kv(self, layer):
        return self.o.read_kv(0, layer)


def draw_token(lg, sampler, seed, pos, row):
    """the test double's sampler: any fixed function of (logits, settings, seed, position, row) will do — the driver follows the ids, it never predicts a draw"""
    if is_greedy(sampler):
        return int(np.argmax(lg))
    t, k, p, _ = sampler
    l = np.asarray(lg, np.float64) / (t if t > 0 else 1.0)
    if k > 0:
        l[l < np.sort(l)[-min(k, l.size)]] = -np.inf
    pr = np.exp(l - l.max()); pr /= pr.sum()
    if p < 1:
        order = np.argsort(-pr, kind="stable"); c = np.cumsum(pr[order])
        pr[order[(c - pr[order]) >= p]] = 0; pr /= pr.sum()
    return int(np.random.default_rng([seed, pos, row]).choice(l.size, p=pr))


class OracleDevice:
    """the row calls of tinygpt_amd.ffi.Model answered by a RowModel and one batch-1 CPU oracle per row"""
    blob_is_private = True      # its snapshots are no tgx snapshots: two contexts need not write the same bytes

    def __init__(self, fam, dtype, max_batch, max_ctx=MAX_CTX, budget=0):
        self.desc, _, _ = make_desc(fam, dtype, max_batch, max_ctx)
        self.fam, self.dtype = fam, dtype
        self.m = RowModel(max_batch, max_ctx, self.desc.vocab, budget)
        self.seq = [None] * max_batch
        self.kv = [None] * max_batch           # per row: [layer] -> [K rows, V rows], what read_kv returns
        self.lg = [None] * max_batch
        self.lens = [0] * max_batch
        self.rec = [[] for _ in range(max_batch)]
        self.any_logits = False

    @property
    def batch(self):
        return self.m.batch

    def close(self):
        pass

    def _gate(self, kind, *a):
        st, why = self.m.status(kind, *a)
        if st:
            raise TgxError(st, f"{kind}: {why}")

    def _oracle(self, r):
        if self.seq[r] is None:
            self.seq[r] = OracleSeq(self.fam, self.dtype)
        return self.seq[r]

    def _run(self, r, base, new):
        """the row's oracle over base + new; the cache rows of `new` and the last logits become the row's"""
        o = self._oracle(r)
        base, new = list(base), [int(t) for t in new]
        if base:
            o.sync(base); o.sync(base + new)
        else:
            o.clear(); o.sync(new)
        fresh = [o.kv(l) for l in range(self.desc.layers)]
        self.kv[r] = [[np.concatenate([self.kv[r][l][j][:len(base)], fresh[l][j][len(base):]]) if base else fresh[l][j].copy() for j in range(2)] for l in range(self.desc.layers)]
        self.lg[r] = o.logits(); self.lens[r] = len(base) + len(new); self.any_logits = True

    def _record(self, r, t):
        if self.m.rows[r].lp >= 0:
            self.rec[r].append(np.float32(lsm64(self.lg[r], t)))

    # ---- admissions
    def forward_rows(self, rows, prompts):
        rows = [int(r) for r in rows]; prompts = [[int(t) for t in p] for p in prompts]
        self._gate("forward_rows", rows, prompts)
        for r, p in zip(rows, prompts):
            self.rec[r] = []; self._run(r, [], p)
        self.m.apply("forward_rows", rows, prompts)
        return self

    def forward_row(self, row, ids):
        return self.forward_rows([row], [ids])

    def reset_row(self, row):
        self._gate("reset_row", row)
        self.m.apply("reset_row", row); self.rec[row] = []; self.lens[row] = 0
        return self

    def extend_row(self, row, ids):
        ids = [int(t) for t in ids]
        self._gate("extend_row", row, ids)
        self._run(row, self.m.rows[row].tokens, ids)
        self.m.apply("extend_row", row, ids)
        return self

    def score_row(self, row, ids, top_n=0):
        ids = [int(t) for t in ids]
        self._gate("score_row", row, ids)
        if self.m.rows[row].holds:
            self.extend_row(row, ids)
        else:
            self.forward_row(row, ids)
        n = len(ids) - 1
        return np.full(n, -1.0, np.float32), np.full((n, MAX_LOGPROBS), -1, np.int32), np.full((n, MAX_LOGPROBS), -np.inf, np.float32)

    def truncate_row(self, row, n):
        self._gate("truncate_row", row, int(n))
        x = self.m.rows[row]
        if not (n == x.length and x.has_logits):
            self.kv[row] = [[k[:n].copy(), v[:n].copy()] for k, v in self.kv[row]]
            self.lens[row] = int(n)
        self.m.apply("truncate_row", row, int(n))
        return self

    # ---- settings
    def set_row_sampler(self, row, cfg=GREEDY, seed=0):
        s = (float(cfg.temperature), int(cfg.top_k), float(cfg.top_p), float(cfg.min_p))
        self._gate("set_row_sampler", row, s, seed); self.m.apply("set_row_sampler", row, s, seed)
        return self

    def set_row_stop(self, row, max_new=0, stop_ids=()):
        self._gate("set_row_stop", row, max_new, tuple(stop_ids)); self.m.apply("set_row_stop", row, max_new, tuple(stop_ids))
        return self

    def set_row_logprobs(self, row, top_n=0):
        self._gate("set_row_logprobs", row, top_n); self.m.apply("set_row_logprobs", row, top_n)
        return self

    def row_logprobs(self, row, n):
        if not self.rec[row]:
            raise TgxError(STATE, "the row has recorded nothing")
        if not 1 <= n <= min(len(self.rec[row]), LOGPROB_RING):
            raise TgxError(INVALID, "n")
        return np.array(self.rec[row][-n:], np.float32), None, None, None

    # ---- tokens
    def sample_row(self, row, cfg=GREEDY, seed=0):
        self._gate("sample_row", row)
        s = (float(cfg.temperature), int(cfg.top_k), float(cfg.top_p), float(cfg.min_p))
        t = draw_token(self.lg[row], s, seed, self.lens[row], row)
        self._record(row, t); self.m.apply("sample_row", row, out=t)
        return t

    def _step(self, r, toks, x):
        self._run(r, toks, [x])

    def decode_rows(self, n):
        self._gate("decode_rows", n)
        B = self.m.batch
        ids = np.full((n, B), -1, np.int64); new = np.zeros(B, np.int32); fin = np.zeros(B, np.int32)
        for r in self.m._stepping():
            x = self.m.rows[r]
            toks, cur, shadow = list(x.tokens), x.tok, Row()
            shadow.max_new, shadow.stop_ids, shadow.produced = x.max_new, x.stop_ids, x.produced
            for s in range(n):
                self._step(r, toks, cur); toks.append(cur)
                cur = draw_token(self.lg[r], x.sampler, x.seed, len(toks), r)
                self._record(r, cur)
                ids[s, r] = cur; new[r] += 1
                fin[r] = shadow.note_produced(cur)
                if fin[r]:
                    break
        for r in range(B):
            if self.m.rows[r].state == FINISHED:
                fin[r] = self.m.rows[r].fin_code
        self.m.apply("decode_rows", n, out=(ids, new, fin))
        return ids, new, fin

    def decode(self, n, cfg=GREEDY, seed=0):
        self._gate("decode", n)
        ids = np.zeros((n, self.m.batch), np.int64)
        for r in self.m._stepping():
            toks, cur = list(self.m.rows[r].tokens), self.m.rows[r].tok
            for s in range(n):
                self._step(r, toks, cur); toks.append(cur)
                cur = ids[s, r] = int(np.argmax(self.lg[r]))
        self.m.apply("decode", n, out=ids)
        return ids

    def verify_row(self, row, draft):
        draft = [int(t) for t in draft]
        self._gate("verify_row", row, draft)
        x = self.m.rows[row]
        toks, cur, shadow, out, fin = list(x.tokens), x.tok, Row(), [], 0
        shadow.max_new, shadow.stop_ids, shadow.produced = x.max_new, x.stop_ids, x.produced
        for i in range(len(draft) + 1):
            self._step(row, toks, cur); toks.append(cur)
            cur = int(np.argmax(self.lg[row])); out.append(cur); self._record(row, cur)
            fin = shadow.note_produced(cur)
            if fin or i == len(draft) or cur != draft[i]:
                break
        self._verified(row)
        out = np.array(out, np.int64)
        self.m.apply("verify_row", row, draft, out=(out, fin))
        return out, fin

    def _verified(self, row):
        pass

    # ---- copies
    def _copy_rows(self, src_kv, n):
        return [[k[:n].copy(), v[:n].copy()] for k, v in src_kv]

    def fork_row(self, src, dsts):
        dsts = [int(d) for d in dsts]
        self._gate("fork_row", src, dsts)
        for d in dsts:
            self.kv[d] = self._copy_rows(self.kv[src], self.lens[src]); self.lg[d] = self.lg[src].copy(); self.lens[d] = self.lens[src]; self.rec[d] = []
        self.m.apply("fork_row", src, dsts)
        return self

    def save_row(self, row):
        self._gate("save_row", row)
        x = self.m.rows[row]
        return pickle.dumps(dict(snap=Snap(x), kv=self._copy_rows(self.kv[row], self.lens[row]), lg=self.lg[row].copy() if x.has_logits else None, rec=list(self.rec[row])))

    def restore_row(self, row, blob):
        b = pickle.loads(blob)
        self._gate("restore_row", row, b["snap"])
        self.kv[row] = self._copy_rows(b["kv"], len(b["snap"].tokens)); self.lens[row] = len(b["snap"].tokens)
        if b["lg"] is not None:
            self.lg[row] = b["lg"].copy(); self.any_logits = True
        self.rec[row] = self._restored_records(b)
        self.m.apply("restore_row", row, b["snap"])
        return self

    def _restored_records(self, b):
        return []

    # ---- readers
    def logits(self, rounded=False):
        V = self.desc.vocab
        return np.stack([self.lg[r] if self.lg[r] is not None else np.zeros(V, np.float32) for r in range(self.m.batch)])

    def read_kv(self, row, layer):
        k, v = self.kv[row][layer]
        return k[:self.lens[row]], v[:self.lens[row]]

    def past_length_row(self, row):
        return self.lens[row] if self.m.rows[row].holds else 0

    @property
    def past_length(self):
        return self.m.past_length()

    def get_option(self, key):
        assert key == "kv.free_tokens"
        return self.m.free_tokens()


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
class Mirror:
    """the reference: per row an oracle and its reordered twin (every reduction last-to-first) fed the row's token list.  An admission is one forward; decode, verify
    and extend tokens are single-token forwards; a truncation resets and forwards the kept prefix; a fork or restore target forwards its token list"""
    def __init__(self, fam, dtype, max_batch):
        self.fam, self.dtype = fam, dtype
        self.a = [None] * max_batch; self.b = [None] * max_batch
        self.lg = [None] * max_batch
        self.floor = [0.0] * max_batch
        self.spare = None

    def _pair(self, r):
        if self.a[r] is None:
            self.a[r] = OracleSeq(self.fam, self.dtype); self.b[r] = OracleSeq(self.fam, self.dtype, reorder=True)
        return self.a[r], self.b[r]

    def clear(self, r):
        if self.a[r] is not None:
            self.a[r].clear(); self.b[r].clear()
        self.lg[r] = None

    def _seen(self, r, la, lb):
        self.floor[r] = max(self.floor[r], rel_err(lb[None, :], la[None, :]))

    def follow(self, r, tokens, each=None):
        """the row's cache now holds `tokens`; each(i, logits) sees the oracle's logits behind every token that went in on its own"""
        a, b = self._pair(r)
        seen = []
        b.sync(tokens, each=(lambda i, lg: seen.append(lg)) if each else None)

        def one(i, lg):
            self._seen(r, lg, seen.pop(0))
            each(i, lg)
        a.sync(tokens, each=one if each else None)
        la, lb = a.logits(), b.logits()
        self._seen(r, la, lb)
        self.lg[r] = la

    def greedy_continuation(self, tokens, tok, n):
        """the reference's next n greedy tokens behind tokens + [tok] (a spare context: the rows' own stay where they are)"""
        if self.spare is None:
            self.spare = OracleSeq(self.fam, self.dtype)
        out, toks = [], list(tokens)
        for _ in range(n):
            toks.append(int(tok))
            self.spare.sync(toks)
            tok = int(np.argmax(self.spare.logits())); out.append(tok)
        return out


def clear_gap(lg, frac=4e-3):
    top2 = np.sort(lg)[-2:]
    return (top2[1] - top2[0]) > frac * np.abs(lg).max()


class Stats:
    def __init__(self):
        self.max_err = 0.0; self.floor = 0.0; self.greedy = 0; self.compared = 0
        self.accepted = {}; self.refused = {}; self.classes = {}; self.cov = {}; self.wall = 0.0

    def line(self):
        share = self.compared / max(self.greedy, 1)
        ops = " ".join(f"{k}:{self.accepted.get(k, 0)}/{self.refused.get(k, 0)}" for k in sorted(set(self.accepted) | set(self.refused)))
        return f"max_err {self.max_err:.3e} floor {self.floor:.3e} ids_compared {self.compared}/{self.greedy} ({share:.2f}) wall {self.wall:.2f}s ops(ok/refused) {ops}"


class Ctx:
    """one context under test: the device, its model, its mirror, what the last look at the device saw"""
    def __init__(self, device, model, mirror, name):
        self.dev, self.m, self.mir, self.name = device, model, mirror, name
        self.layers = device.desc.layers
        self.logits_exist = False


class Failure(AssertionError):
    pass


class Driver:
    KINDS = ["forward_row", "forward_rows", "reset_row", "sample_row", "set_row_sampler", "set_row_stop", "decode_rows", "decode", "fork_row", "extend_row",
             "truncate_row", "verify_row", "save_row", "restore_row", "score_row", "set_row_logprobs"]
    WEIGHTS = dict(forward_row=2.0, forward_rows=1.2, reset_row=1.0, sample_row=1.5, set_row_sampler=0.6, set_row_stop=1.4, decode_rows=4.0, decode=0.8, fork_row=3.0,
                   extend_row=1.5, truncate_row=1.6, verify_row=2.0, snapshot=1.3, score_row=0.8, set_row_logprobs=1.0, finish_short_of_block=1.0)

    def __init__(self, main, aux, rng, bound, gap, lp_tol, tag):
        self.c, self.aux, self.rng = main, aux, rng
        self.bound, self.gap, self.lp_tol, self.tag = bound, gap, lp_tol, tag
        self.log, self.stats, self.drawn = [], Stats(), {}
        self.pending, self.fixup = [], False
        self.saved = []            # (blob, Snap, what the device showed of the row when it was saved, origin row, origin context)

    # ---- looking at the device
    def observe(self, c):
        m, d = c.m, c.dev
        o = dict(lens=[int(d.past_length_row(r)) for r in range(m.max_batch)], past=int(d.past_length), free=int(d.get_option("kv.free_tokens")))
        o["lg"] = d.logits(rounded=False) if c.logits_exist and m.batch else None
        o["kv"] = {r: [tuple(a.copy() for a in d.read_kv(r, l)) for l in range(c.layers)] for r in range(m.batch) if m.rows[r].holds}
        return o

    def fail(self, what):
        raise Failure(f"{self.tag} op {len(self.log) - 1}: {what}\nfloors {[f'{f:.2e}' for f in self.c.mir.floor]}\nlog:\n" + "\n".join(f"  {i}: {l}" for i, l in enumerate(self.log)))

    def need(self, cond, what):
        if not cond:
            self.fail(what)

    def same_row(self, a, b, ra, rb, what, upto=None, logits=True):
        ka, kb = a["kv"][ra], b["kv"][rb]
        for l in range(len(ka)):
            for j in range(2):
                x, y = ka[l][j], kb[l][j]
                if upto is not None:
                    x, y = x[:upto], y[:upto]
                self.need(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{what}: cache rows of layer {l} ({'KV'[j]}) differ (rows {ra}, {rb})")
        if logits:
            self.need(np.array_equal(a["lg"][ra].view(np.uint32), b["lg"][rb].view(np.uint32)), f"{what}: logits differ (rows {ra}, {rb})")

    def call(self, c, kind, fn):
        try:
            return OK, fn()
        except TgxError as e:
            return e.status, None

    # ---- one operation on one context: predicted, run, checked
    def op(self, c, kind, args, run, named, out_to_model=None, illegal=None):
        """run(dev) makes the call; named = rows the call may change (None: worked out from the model after the call)"""
        m = c.m
        self.log.append(f"[{c.name}] {kind}{self._show(args)}" + (f"   (drawn illegal: {illegal})" if illegal else ""))
        want, why = m.status(kind, *args)
        before = self.observe(c)
        got, out = self.call(c, kind, lambda: run(c.dev))
        self.log[-1] += f" -> {got}" + (f" {why}" if want else "")
        self.need(got == want, f"status {got}, the header promises {want} ({why})")
        is_main = c is self.c
        if is_main:
            (self.stats.accepted if got == OK else self.stats.refused)[kind] = (self.stats.accepted if got == OK else self.stats.refused).get(kind, 0) + 1
            if got != OK:
                self.stats.classes[f"{kind}:{why}"] = self.stats.classes.get(f"{kind}:{why}", 0) + 1
        if got != OK:
            after = self.observe(c)
            self.need(after["lens"] == before["lens"] and after["past"] == before["past"] and after["free"] == before["free"], f"a refused call moved lengths or the pool: {before['lens']}/{before['free']} -> {after['lens']}/{after['free']}")
            for r in before["kv"]:
                self.same_row(before, after, r, r, "after a refusal", logits=before["lg"] is not None and m.rows[r].state == LIVE and m.rows[r].has_logits)
            return None
        was = {r: (m.rows[r].state, m.rows[r].has_logits, m.rows[r].length) for r in range(m.max_batch)}
        try:
            ret = m.apply(kind, *args, out=out_to_model(out)) if out_to_model else m.apply(kind, *args)
        except AssertionError as e:
            self.fail(f"the device's outputs contradict the header: {e}")
        if kind in ("forward_row", "forward_rows", "extend_row", "score_row", "restore_row", "fork_row", "decode", "decode_rows", "verify_row"):
            c.logits_exist = c.logits_exist or any(x.has_logits for x in m.rows)
        if named is None:
            named = ret
        after = self.observe(c)
        self.need(after["lens"] == [m.past_length_row(r) for r in range(m.max_batch)], f"lengths {after['lens']}, the model's {[m.past_length_row(r) for r in range(m.max_batch)]}")
        self.need(after["past"] == m.past_length(), f"past_length {after['past']}, the model's {m.past_length()}")
        self.need(after["free"] == m.free_tokens(), f"kv.free_tokens {after['free']}, the model's {m.free_tokens()}")
        for r, (state, had_logits, length) in was.items():       # bystanders
            if r in named or state not in (LIVE, FINISHED):
                continue
            self.same_row(before, after, r, r, f"bystander row {r}", logits=state == LIVE and had_logits and before["lg"] is not None)
        return dict(out=out, before=before, after=after, ret=ret)

    @staticmethod
    def _show(args):
        def s(a):
            if isinstance(a, Snap):
                return f"<snapshot of {len(a.tokens)}>"
            if isinstance(a, (list, tuple, np.ndarray)) and len(a) > 6 and not isinstance(a[0], (list, tuple, np.ndarray)):
                return f"<{len(a)} ids: {list(a[:3])}..>"
            if isinstance(a, (list, tuple)):
                return "[" + ", ".join(s(x) for x in a) + "]"
            return repr(a)
        return "(" + ", ".join(s(a) for a in args) + ")"

    # ---- numeric checks against the mirror
    def check_logits(self, c, after):
        for r in range(c.m.batch):
            x = c.m.rows[r]
            if x.state == LIVE and x.has_logits and c.mir.lg[r] is not None:
                e = rel_err(after["lg"][r][None, :], c.mir.lg[r][None, :])
                if c is self.c:
                    self.stats.max_err = max(self.stats.max_err, e)
                self.need(e < self.bound, f"row {r}: logits {e:.3e} from the oracle (bound {self.bound:g}, this row's oracle-to-twin floor {c.mir.floor[r]:.3e})")
        self.stats.floor = max([self.stats.floor] + self.c.mir.floor)

    def greedy_id(self, ref_lg, got, what):
        self.stats.greedy += 1
        if clear_gap(ref_lg, self.gap):
            self.stats.compared += 1
            self.need(int(np.argmax(ref_lg)) == int(got), f"{what}: greedy id {int(got)}, the oracle's {int(np.argmax(ref_lg))} on a clear top-2 gap")

    def follow_steps(self, c, r, base, inputs, produced, greedy, what):
        """the mirror takes `inputs` behind `base` one by one; the id produced behind input i is produced[i]"""
        def each(i, lg):
            j = i - len(base)
            if greedy and 0 <= j < len(produced):
                self.greedy_id(lg, produced[j], f"{what}, row {r}, token {j}")
        if c.mir.a[r] is None or c.mir.a[r].toks != list(base):
            c.mir.follow(r, list(base))
        c.mir.follow(r, list(base) + list(inputs), each=each)

    def check_lp(self, c, r, after, tok):
        x = c.m.rows[r]
        if x.lp < 0:
            return
        st, rec = self.call(c, "row_logprobs", lambda: c.dev.row_logprobs(r, 1))
        self.need(st == OK, f"row {r}: reading the last of {x.lp_count} logprob records returned {st}")
        want = lsm64(after["lg"][r], tok)
        self.need(abs(float(rec[0][0]) - want) <= self.lp_tol, f"row {r}: logprob record {float(rec[0][0]):.7f}, the fp64 log-softmax of its own logits at id {tok} is {want:.7f}")

    def check_lp_counts(self, c):
        for r in range(c.m.batch):
            x = c.m.rows[r]
            if x.lp < 0 or not x.holds:
                continue
            n = min(x.lp_count, LOGPROB_RING)
            if n == 0:
                st, _ = self.call(c, "row_logprobs", lambda: c.dev.row_logprobs(r, 1))
                self.need(st == STATE, f"row {r}: the model counts 0 logprob records, reading one returned {st}")
            else:
                st, _ = self.call(c, "row_logprobs", lambda: c.dev.row_logprobs(r, n))
                self.need(st == OK, f"row {r}: the model counts {x.lp_count} logprob records, reading {n} returned {st}")
                if n < LOGPROB_RING:
                    st, _ = self.call(c, "row_logprobs", lambda: c.dev.row_logprobs(r, n + 1))
                    self.need(st == INVALID, f"row {r}: the model counts {x.lp_count} logprob records, reading {n + 1} returned {st}")

    # ---- the operations
    def ids(self, n):
        return [int(t) for t in self.rng.integers(0, self.c.m.vocab, n)]

    def do_admit(self, c, rows, prompts, kind, illegal=None):
        if kind == "forward_row":
            res = self.op(c, kind, (rows[0], prompts[0]), lambda d: d.forward_row(rows[0], np.array(prompts[0], np.int64)), rows, illegal=illegal)
        elif kind == "score_row":
            res = self.op(c, kind, (rows[0], prompts[0]), lambda d: d.score_row(rows[0], np.array(prompts[0], np.int64)), rows, illegal=illegal)
        else:
            res = self.op(c, kind, (rows, prompts), lambda d: d.forward_rows(rows, [np.array(p, np.int64) for p in prompts]), rows, illegal=illegal)
        if res:
            for r, p in zip(rows, prompts):
                c.mir.clear(r); c.mir.follow(r, p)
            if kind == "score_row":
                self.check_scores(res["out"], len(prompts[0]))
            self.check_logits(c, res["after"])
        return res

    def check_scores(self, out, n):
        lp = out[0]
        self.need(len(lp) == n - 1 and np.isfinite(lp).all() and (lp <= 0).all(), f"score_row: {n - 1} log-probabilities <= 0 expected, got {lp}")

    def do_reset(self, c, row, illegal=None):
        res = self.op(c, "reset_row", (row,), lambda d: d.reset_row(row), [row], illegal=illegal)
        if res:
            c.mir.clear(row)
        return res

    def do_sample(self, c, row, illegal=None):
        x = c.m.rows[row]
        cfg = SamplerCfg(*x.sampler)
        res = self.op(c, "sample_row", (row,), lambda d: d.sample_row(row, cfg, x.seed), [row], out_to_model=lambda t: t, illegal=illegal)
        if res:
            self.need(np.array_equal(res["before"]["lg"][row].view(np.uint32), res["after"]["lg"][row].view(np.uint32)), f"sample_row changed the logits of row {row}")
            self.same_row(res["before"], res["after"], row, row, "sample_row", logits=False)
            if is_greedy(x.sampler) and c.mir.lg[row] is not None:
                self.greedy_id(c.mir.lg[row], res["out"], f"sample_row, row {row}")
            self.check_lp(c, row, res["after"], res["out"])
        return res

    def do_extend(self, c, row, ids, kind="extend_row", illegal=None):
        base = list(c.m.rows[row].tokens) if c.m._in(row) else []
        run = (lambda d: d.extend_row(row, np.array(ids, np.int64))) if kind == "extend_row" else (lambda d: d.score_row(row, np.array(ids, np.int64)))
        res = self.op(c, kind, (row, ids), run, [row], illegal=illegal)
        if res:
            self.same_row(res["before"], res["after"], row, row, "extend_row: the prefix", upto=len(base), logits=False)
            self.follow_steps(c, row, base, ids, [], False, kind)
            if kind == "score_row":
                self.check_scores(res["out"], len(ids))
            self.check_logits(c, res["after"])
        return res

    def do_truncate(self, c, row, n, illegal=None):
        res = self.op(c, "truncate_row", (row, n), lambda d: d.truncate_row(row, n), [row], illegal=illegal)
        if res:
            self.same_row(res["before"], res["after"], row, row, "truncate_row: rows [0, new_len)", upto=n, logits=False)
            if not c.m.rows[row].has_logits:
                c.mir.follow(row, c.m.rows[row].tokens); c.mir.lg[row] = None
        return res

    def do_decode_rows(self, c, n, illegal=None):
        m = c.m
        pre = {r: (list(m.rows[r].tokens), m.rows[r].tok, is_greedy(m.rows[r].sampler)) for r in m._stepping()}
        res = self.op(c, "decode_rows", (n,), lambda d: d.decode_rows(n), None, out_to_model=lambda o: o, illegal=illegal)
        if res:
            ids, new, fin = res["out"]
            for r, (base, tok, greedy) in pre.items():
                k = int(new[r])
                produced = [int(t) for t in ids[:k, r]]
                self.same_row(res["before"], res["after"], r, r, "decode_rows: the prefix", upto=len(base), logits=False)
                self.follow_steps(c, r, base, [tok] + produced[:-1], produced, greedy, "decode_rows")
                if m.rows[r].state == FINISHED:
                    c.mir.lg[r] = None
                if k == n:
                    self.check_lp(c, r, res["after"], produced[-1])
            self.check_logits(c, res["after"])
        return res

    def do_decode(self, c, n, illegal=None):
        m = c.m
        pre = {r: (list(m.rows[r].tokens), m.rows[r].tok) for r in m._stepping()}
        res = self.op(c, "decode", (n,), lambda d: d.decode(n, GREEDY), None, out_to_model=lambda o: o, illegal=illegal)
        if res:
            for r, (base, tok) in pre.items():
                produced = [int(t) for t in res["out"][:, r]]
                self.follow_steps(c, r, base, [tok] + produced[:-1], produced, True, "decode")
            self.check_logits(c, res["after"])
        return res

    def do_fork(self, c, src, dsts, illegal=None):
        res = self.op(c, "fork_row", (src, dsts), lambda d: d.fork_row(src, dsts), dsts, illegal=illegal)
        if res:
            for d in dsts:
                self.same_row(res["after"], res["after"], src, d, f"fork {src} -> {d}")
                c.mir.clear(d); c.mir.follow(d, c.m.rows[d].tokens)
            self.check_logits(c, res["after"])
        return res

    def do_verify(self, c, row, draft, illegal=None):
        x = c.m.rows[row] if c.m._in(row) else None
        base, tok = (list(x.tokens), x.tok) if x else ([], None)
        res = self.op(c, "verify_row", (row, draft), lambda d: d.verify_row(row, np.array(draft, np.int64)), [row], out_to_model=lambda o: o, illegal=illegal)
        if res:
            out = [int(t) for t in res["out"][0]]
            self.same_row(res["before"], res["after"], row, row, "verify_row: the prefix", upto=len(base), logits=False)
            self.follow_steps(c, row, base, [tok] + out[:-1], out, True, "verify_row")
            if c.m.rows[row].state == FINISHED:
                c.mir.lg[row] = None
            else:
                self.check_lp(c, row, res["after"], out[-1])
            self.check_logits(c, res["after"])
        return res

    def do_save(self, c, row, illegal=None):
        res = self.op(c, "save_row", (row,), lambda d: d.save_row(row), [], illegal=illegal)
        if res:
            self.same_row(res["before"], res["after"], row, row, "a save changes nothing", logits=c.m.rows[row].has_logits)
            shot = dict(kv={0: res["after"]["kv"][row]}, lg=[res["after"]["lg"][row].copy()] if c.m.rows[row].has_logits else None)
            return res["out"], res["ret"], shot
        return None

    def do_restore(self, c, row, saved, illegal=None):
        blob, snap, shot = saved
        res = self.op(c, "restore_row", (row, snap), lambda d: d.restore_row(row, blob), [row], illegal=illegal)
        if res:
            self.need(res["after"]["lens"][row] == len(snap.tokens), "restored length")
            self.same_row(shot, res["after"], 0, row, f"restore into row {row}", logits=snap.has_logits)
            c.mir.clear(row); c.mir.follow(row, snap.tokens)
            if not snap.has_logits:
                c.mir.lg[row] = None
            self.check_logits(c, res["after"])
        return res

    # ---- drawing
    def rows_where(self, c, pred):
        return [r for r in range(c.m.max_batch) if pred(r, c.m.rows[r])]

    def pick(self, xs):
        return xs[int(self.rng.integers(0, len(xs)))]

    def free_targets(self, c, k):
        """k rows an admission may name: retired rows and the next new rows"""
        m = c.m
        retired = self.rows_where(c, lambda r, x: r < m.batch and x.state == RETIRED)
        self.rng.shuffle(retired)
        out = []
        nb = m.batch
        for _ in range(k):
            if retired and (nb >= m.max_batch or self.rng.random() < 0.6):
                out.append(int(retired.pop()))
            elif nb < m.max_batch:
                out.append(nb); nb += 1
        return out

    def fit_len(self, room):
        ok = [n for n in LENS if n <= room]
        return int(self.pick(ok)) if ok else 0

    def draw_legal(self):
        c, m, rng = self.c, self.c.m, self.rng
        kinds = list(self.WEIGHTS); w = np.array([self.WEIGHTS[k] for k in kinds])
        if self.stats.greedy < 2 * len(self.log):                  # a run that has produced few tokens so far leans towards the calls that produce them
            w[kinds.index("decode_rows")] *= 3; w[kinds.index("verify_row")] *= 2
        w /= w.sum()
        for _ in range(40):
            kind = kinds[int(rng.choice(len(kinds), p=w))]
            live = self.rows_where(c, lambda r, x: x.state == LIVE)
            if kind == "forward_row":
                t = self.free_targets(c, 1)
                if t:
                    res = self.do_admit(c, t, [self.ids(self.pick(LENS))], "forward_row")
                    r = t[0]
                    if res and m.rows[r].length % BLK == 0 and rng.random() < 0.6:       # next: a fork on a block boundary, no tail to copy
                        self.pending.append(lambda: self.do_fork(c, r, self.free_targets(c, int(rng.integers(1, 3)))) if m.rows[r].state == LIVE and m.rows[r].has_logits and self.free_targets(c, 1) else None)
                    elif res and rng.random() < 0.15:
                        self.pending.append(lambda: self.draw_illegal(force="verify_notok"))
                    return res
            elif kind == "forward_rows":
                t = self.free_targets(c, int(rng.integers(2, 5)))
                if len(t) >= 2:
                    return self.do_admit(c, t, [self.ids(self.pick(LENS)) for _ in t], "forward_rows")
            elif kind == "score_row":
                holds = self.rows_where(c, lambda r, x: x.holds and x.length < m.max_ctx)
                if holds and rng.random() < 0.5:
                    r = self.pick(holds); n = self.fit_len(m.max_ctx - m.rows[r].length)
                    if m.rows[r].state == FINISHED or n:
                        return self.do_extend(c, r, self.ids(n), "score_row")
                t = self.free_targets(c, 1)
                if t:
                    return self.do_admit(c, t, [self.ids(self.pick(LENS))], "score_row")
            elif kind == "reset_row":
                holds = self.rows_where(c, lambda r, x: x.holds)
                if holds and (len(holds) > 2 or rng.random() < 0.3):
                    return self.do_reset(c, self.pick(holds))
            elif kind == "sample_row":
                cand = [r for r in live if m.rows[r].has_logits and not m.rows[r].has_token] or [r for r in live if m.rows[r].has_logits and rng.random() < 0.3]
                if cand:
                    return self.do_sample(c, self.pick(cand))
            elif kind == "set_row_sampler":
                r = int(rng.integers(0, m.max_batch))
                s = [(0.8, 0, 0.9, 0.0), (1.0, 50, 1.0, 0.0), GREEDY_T][int(rng.integers(0, 3))]
                seed = int(rng.integers(1, 1 << 30))
                return self.op(c, "set_row_sampler", (r, s, seed), lambda d: d.set_row_sampler(r, SamplerCfg(*s), seed), [r])
            elif kind == "set_row_stop":
                cand = [r for r in live if m.rows[r].has_token] or live
                if cand:
                    edge = [r for r in cand if m.rows[r].length % BLK >= BLK - 19 and m.rows[r].length + 21 <= m.max_ctx]
                    r = self.pick(edge) if edge and rng.random() < 0.7 else self.pick(cand)
                    x = m.rows[r]
                    max_new = int(rng.integers(1, 6)) if rng.random() < 0.7 else 0
                    if r in edge and rng.random() < 0.7:           # next: a row that finishes just short of a block boundary, inside a call that was given blocks beyond it
                        max_new = 1
                        n_cross = BLK - x.length % BLK + 1
                        self.pending.append(lambda: self.ready_and_decode(c, n_cross))
                    stops = []
                    if rng.random() < 0.6:
                        stops = self.ids(int(rng.integers(1, MAX_STOP)))
                        if x.has_token and is_greedy(x.sampler) and x.length + 7 < m.max_ctx:
                            stops[0] = c.mir.greedy_continuation(x.tokens, x.tok, int(rng.integers(1, 6)))[-1]
                    return self.op(c, "set_row_stop", (r, max_new, tuple(stops)), lambda d: d.set_row_stop(r, max_new, stops), [r])
            elif kind == "set_row_logprobs":
                r = int(self.pick(live)) if live and rng.random() < 0.7 else int(rng.integers(0, m.max_batch))
                top_n = int(self.pick([0, 0, 3, -1]))
                return self.op(c, "set_row_logprobs", (r, top_n), lambda d: d.set_row_logprobs(r, top_n), [r])
            elif kind in ("decode_rows", "decode"):
                if not live:
                    continue
                fix = [r for r in live if not m.rows[r].has_logits]
                self.fixup = True                                  # what makes the steps legal does not count as one of the run's operations
                if fix:                                            # a truncated row blocks every step: extend it
                    r = self.pick(fix); n = self.fit_len(m.max_ctx - m.rows[r].length)
                    if n:
                        return self.do_extend(c, r, self.ids(n))
                    return self.do_reset(c, r)
                fix = [r for r in live if not m.rows[r].has_token]
                if fix:
                    return self.do_sample(c, self.pick(fix))
                self.fixup = False
                room = m.max_ctx - max(m.rows[r].length for r in live)
                if kind == "decode":
                    if any(x.state == FINISHED for x in m.rows[:m.batch]):
                        return self.do_reset(c, self.pick(self.rows_where(c, lambda r, x: x.state == FINISHED)))
                    if room >= 1:
                        return self.do_decode(c, int(rng.integers(1, min(3, room) + 1)))
                elif room >= 1 and not any(x.state == FINISHED and x.length >= m.max_ctx for x in m.rows):
                    return self.do_decode_rows(c, int(rng.integers(1, min(20, room) + 1)))
                return self.do_reset(c, max(live, key=lambda r: m.rows[r].length))
            elif kind == "fork_row":
                cand = [r for r in live if m.rows[r].has_logits]
                if cand:
                    on_edge = [r for r in cand if m.rows[r].length % BLK == 0]
                    src = self.pick(on_edge) if on_edge and rng.random() < 0.7 else self.pick(cand)
                    t = self.free_targets(c, int(rng.integers(1, 4)))
                    if t:
                        res = self.do_fork(c, src, t)
                        if res and m.pool and m.rows[src].length >= BLK and rng.random() < 0.6:      # next: one sibling rolled back into a block the others map as well
                            r, n = int(self.pick(t + [src])), int(rng.integers(1, BLK)) + BLK * int(rng.integers(0, m.rows[src].length // BLK))
                            self.pending.append(lambda: self.do_truncate(c, r, n) if m.rows[r].holds and m.rows[r].length >= n else None)
                        return res
            elif kind == "extend_row":
                cand = self.rows_where(c, lambda r, x: x.holds and x.length < m.max_ctx)
                fin = [r for r in cand if m.rows[r].state == FINISHED]
                if cand:
                    r = self.pick(fin) if fin and rng.random() < 0.7 else self.pick(cand)
                    n = self.fit_len(m.max_ctx - m.rows[r].length)
                    if n:
                        ids = self.ids(n)
                        if m.rows[r].has_token and rng.random() < 0.5:
                            ids[0] = m.rows[r].tok
                        return self.do_extend(c, r, ids)
            elif kind == "truncate_row":
                cand = self.rows_where(c, lambda r, x: x.holds and x.length >= 2)
                if cand:
                    shared = [r for r in cand if m.pool and any(m.pool.shared(b) for b in m.rows[r].blocks)]
                    r = self.pick(shared) if shared and rng.random() < 0.7 else self.pick(cand)
                    L = m.rows[r].length
                    opts = [L - 1, max(1, L // 2), max(1, (L // BLK) * BLK), max(1, (L // BLK) * BLK - int(rng.integers(1, 100)))]
                    if r in shared:                                # into a block forked siblings map as well: copy on write
                        n_shared = sum(1 for b in m.rows[r].blocks if m.pool.shared(b))
                        opts += [int(rng.integers(1, BLK)) + BLK * int(rng.integers(0, n_shared))] * 3
                    if m.rows[r].state == LIVE and m.rows[r].has_logits:
                        opts.append(L)
                    n = int(self.pick([o for o in opts if 1 <= o <= L and not (o == L and m.rows[r].state == FINISHED)]))
                    if r in shared and rng.random() < 0.6:
                        n = opts[-1]
                    res = self.do_truncate(c, r, n)
                    if res and rng.random() < 0.5:                 # next: one of the calls a row without logits refuses
                        self.pending.append(lambda: self.draw_illegal(force=str(self.pick(["fork_trunc", "sample_trunc", "decode_rows_trunc"]))))
                    return res
            elif kind == "verify_row":
                cand = [r for r in live if m.rows[r].has_logits and m.rows[r].has_token and is_greedy(m.rows[r].sampler) and m.rows[r].length + 2 <= m.max_ctx]
                if cand:
                    edge = [r for r in cand if BLK - 16 <= m.rows[r].length % BLK]
                    r = self.pick(edge) if edge and rng.random() < 0.7 else self.pick(cand)
                    x = m.rows[r]
                    nd = int(rng.integers(1, min(MAX_DRAFT, m.max_ctx - x.length - 1) + 1))
                    draft = c.mir.greedy_continuation(x.tokens, x.tok, nd)
                    if rng.random() < 0.5:
                        i = int(rng.integers(0, nd)); draft[i] = (draft[i] + 1 + int(rng.integers(0, m.vocab - 1))) % m.vocab
                    return self.do_verify(c, r, draft)
            elif kind == "finish_short_of_block":
                # paged: a row one token short of finishing, a few positions short of a block boundary, in a call that is given blocks beyond the boundary
                if not m.pool:
                    continue
                edge = [r for r in live if m.rows[r].has_logits and m.rows[r].length % BLK >= BLK - 19 and m.rows[r].length + 21 <= m.max_ctx]
                if edge:
                    r = int(self.pick(edge)); n_cross = BLK - m.rows[r].length % BLK + 1
                    self.pending.append(lambda: self.ready_and_decode(c, n_cross))
                    return self.op(c, "set_row_stop", (r, 1, ()), lambda d: d.set_row_stop(r, 1, ()), [r])
                t = self.free_targets(c, 1)
                if t:
                    return self.do_admit(c, t, [self.ids(int(self.pick([126, 127])))], "forward_row")
            elif kind == "snapshot":
                cand = [r for r in live if m.rows[r].length >= 1]
                if cand:
                    return self.do_snapshot(self.pick(cand))
        return None

    def ready_and_decode(self, c, n):
        """decode_rows(n) behind whatever makes it legal: every live row that lacks a token is sampled first"""
        m = c.m
        live = self.rows_where(c, lambda r, x: x.state == LIVE)
        if not live or any(not m.rows[r].has_logits for r in live):
            return None
        for r in live:
            if not m.rows[r].has_token:
                self.do_sample(c, r)
        room = m.max_ctx - max(m.rows[r].length for r in live)
        if room < 1 or any(x.state == FINISHED and x.length >= m.max_ctx for x in m.rows):
            return None
        return self.do_decode_rows(c, min(n, room))

    def do_snapshot(self, r):
        """save a row, then restore it: into the same row, another row, or the second context (the other cache layout where there is one) and back"""
        c, m, rng = self.c, self.c.m, self.rng
        saved = self.do_save(c, r)
        if not saved:
            return None
        how = self.pick(["same", "other", "other", "cross", "cross", "cross"])
        if how == "cross" and self.aux is not None:
            a = self.aux
            t = self.free_targets(a, 1)
            if not t:
                t = [int(rng.integers(0, a.m.max_batch))]
                self.do_reset(a, t[0])
            res = self.do_restore(a, t[0], saved)
            if res:
                key = "restore_cross_layout" if bool(a.m.pool) != bool(c.m.pool) else "restore_cross_context"
                self.stats.cov[key] = self.stats.cov.get(key, 0) + 1
                again = self.do_save(a, t[0])
                self.need(again is not None, "the restored row cannot be saved")
                if isinstance(saved[0], bytes) and not getattr(c.dev, "blob_is_private", False):
                    self.need(again[0] == saved[0], "the same row saved on the two contexts is not the same bytes")
                saved = again
            else:
                return res
            if rng.random() < 0.4:
                self.do_reset(a, t[0])
            how = "other"
        if how == "same":
            self.do_reset(c, r)
            return self.do_restore(c, r, saved)
        t = self.free_targets(c, 1)
        if not t:
            victims = self.rows_where(c, lambda q, x: x.holds and q != r)
            if not victims:
                return None
            t = [self.pick(victims)]
            self.do_reset(c, t[0])
        res = self.do_restore(c, t[0], saved)
        if res and t[0] != r:
            self.stats.cov["restore_other_row"] = self.stats.cov.get("restore_other_row", 0) + 1
        if res and rng.random() < 0.5:                             # next: the restored row's records are asked for — it has none, whatever its source had
            row = t[0]
            self.pending.append(lambda: self.op(c, "set_row_logprobs", (row, 0), lambda d: d.set_row_logprobs(row, 0), [row]))
        return res

    RARE = ("_trunc", "_retired", "_finished", "_sampled", "new_row_not_batch")      # classes that need a state few operations leave a row in

    def draw_illegal(self, probe=False, force=None):
        """one call the header refuses in the current state, with exactly one reason (probe: is a class that needs a passing state open and not drawn yet?)"""
        c, m, rng = self.c, self.c.m, self.rng
        live = self.rows_where(c, lambda r, x: x.state == LIVE)
        holds = self.rows_where(c, lambda r, x: x.holds)
        trunc = [r for r in live if not m.rows[r].has_logits]
        retired = self.rows_where(c, lambda r, x: r < m.batch and x.state == RETIRED)
        fin = self.rows_where(c, lambda r, x: x.state == FINISHED)
        notok = [r for r in live if m.rows[r].has_logits and not m.rows[r].has_token]
        can_step = bool(live) and max(m.rows[r].length for r in live) + 1 <= m.max_ctx and not any(m.rows[r].length >= m.max_ctx for r in fin)
        sampled = [r for r in live if m.rows[r].has_logits and m.rows[r].has_token and not is_greedy(m.rows[r].sampler) and m.rows[r].length + 3 <= m.max_ctx]
        full = [r for r in holds if m.rows[r].length + 257 > m.max_ctx]
        free = self.free_targets(c, 1)
        opts = []
        if holds:
            opts += ["admit_live", "admit_live_rows", "restore_live", "score_live_ctx" if full else "admit_live"]
        if trunc:
            opts += ["sample_trunc", "fork_trunc" if free else "sample_trunc"] + (["decode_rows_trunc", "decode_trunc"] if can_step else [])
        if retired:
            opts += ["extend_retired", "truncate_retired", "save_retired"]
        if notok and not trunc and can_step:
            opts += ["decode_notok", "decode_rows_notok"]
        notok_v = [r for r in notok if is_greedy(m.rows[r].sampler) and m.rows[r].length + 4 <= m.max_ctx]
        if notok_v:
            opts += ["verify_notok"]
        if sampled:
            opts += ["verify_sampled"]
        if fin:
            opts += ["save_finished", "fork_finished" if free else "save_finished"]
        if m.batch + 1 < m.max_batch:
            opts += ["new_row_not_batch", "fork_new_row_not_batch" if [r for r in live if m.rows[r].has_logits] else "new_row_not_batch"]
        if full:
            opts += ["extend_ctx"]
        if holds:
            opts += ["truncate_beyond"]
        if not probe:
            opts += ["reset_range", "sampler_range", "stop_range", "logprobs_range"]
        rare = [o for o in opts if o.endswith(self.RARE) and not self.drawn.get(o)]
        if probe:
            return bool(rare)
        opts = [force] if force in opts else rare if rare and rng.random() < 0.7 else opts
        least = min(self.drawn.get(o, 0) for o in opts)            # the classes a run has drawn least come first: every class gets its turn
        what = self.pick(sorted({o for o in opts if self.drawn.get(o, 0) == least}))
        self.drawn[what] = self.drawn.get(what, 0) + 1
        if what == "admit_live":
            return self.do_admit(c, [self.pick(holds)], [self.ids(5)], "forward_row", illegal=what)
        if what == "admit_live_rows":
            rows = [self.pick(holds)] + [r for r in free if not m.rows[r].holds]
            return self.do_admit(c, rows, [self.ids(3) for _ in rows], "forward_rows", illegal=what)
        if what == "restore_live":
            src = [r for r in live]
            if not src:
                return self.do_admit(c, [self.pick(holds)], [self.ids(5)], "forward_row", illegal="admit_live")
            saved = self.do_save(c, self.pick(src))
            return self.do_restore(c, self.pick(holds), saved, illegal=what) if saved else None
        if what == "score_live_ctx":
            return self.do_extend(c, self.pick(full), self.ids(257), "score_row", illegal=what)
        if what == "sample_trunc":
            return self.do_sample(c, self.pick(trunc), illegal=what)
        if what == "fork_trunc":
            return self.do_fork(c, self.pick(trunc), free, illegal=what)
        if what == "decode_rows_trunc" or what == "decode_rows_notok":
            return self.do_decode_rows(c, 1, illegal=what)
        if what == "decode_trunc" or what == "decode_notok":
            return self.do_decode(c, 1, illegal=what)
        if what == "extend_retired":
            return self.do_extend(c, self.pick(retired), self.ids(3), illegal=what)
        if what == "truncate_retired":
            return self.do_truncate(c, self.pick(retired), 1, illegal=what)
        if what == "save_retired":
            return self.do_save(c, self.pick(retired), illegal=what)
        if what == "verify_notok":
            return self.do_verify(c, self.pick(notok_v), self.ids(3), illegal=what)
        if what == "verify_sampled":
            return self.do_verify(c, self.pick(sampled), self.ids(2), illegal=what)
        if what == "save_finished":
            return self.do_save(c, self.pick(fin), illegal=what)
        if what == "fork_finished":
            return self.do_fork(c, self.pick(fin), free, illegal=what)
        if what == "new_row_not_batch":
            return self.do_admit(c, [m.batch + 1], [self.ids(4)], "forward_row", illegal=what)
        if what == "fork_new_row_not_batch":
            return self.do_fork(c, self.pick([r for r in live if m.rows[r].has_logits]), [m.batch + 1], illegal=what)
        if what == "extend_ctx":
            return self.do_extend(c, self.pick(full), self.ids(257), illegal=what)
        if what == "truncate_beyond":
            r = self.pick(holds)
            return self.do_truncate(c, r, m.rows[r].length + 1, illegal=what)
        if what == "reset_range":
            return self.do_reset(c, m.max_batch, illegal=what)
        if what == "sampler_range":
            return self.op(c, "set_row_sampler", (m.max_batch, GREEDY_T, 0), lambda d: d.set_row_sampler(m.max_batch, GREEDY, 0), [], illegal=what)
        if what == "stop_range":
            return self.op(c, "set_row_stop", (-1, 2, ()), lambda d: d.set_row_stop(-1, 2, ()), [], illegal=what)
        return self.op(c, "set_row_logprobs", (0, MAX_LOGPROBS + 1), lambda d: d.set_row_logprobs(0, MAX_LOGPROBS + 1), [], illegal=what)

    def run(self, n_ops):
        t0 = time.time()
        c, was_illegal = self.c, False
        i = drawn = 0
        while i < n_ops and drawn < 3 * n_ops:
            drawn += 1; self.fixup = False
            # roughly one operation in seven is drawn to be illegal; a truncated, finished or retired row lives for an operation or two, so the refusal classes that
            # need one are drawn while it does
            if self.pending:
                self.pending.pop(0)(); was_illegal = False
            elif i >= 1 and self.rng.random() < (0.3 if not was_illegal and self.draw_illegal(probe=True) else 1.0 / 8.0):
                self.draw_illegal(); was_illegal = True
            else:
                self.draw_legal(); was_illegal = False
            i += 0 if self.fixup else 1
            self.check_lp_counts(c)
        # every row reset: the pool must be whole again
        for cc in [c] + ([self.aux] if self.aux else []):
            for r in range(cc.m.max_batch):
                if cc.m.rows[r].state != EMPTY:
                    self.do_reset(cc, r)
            self.need(cc.m.free_tokens() == cc.m.budget and int(cc.dev.get_option("kv.free_tokens")) == cc.m.budget, f"[{cc.name}] after every row was reset kv.free_tokens is {cc.dev.get_option('kv.free_tokens')}, the budget {cc.m.budget}")
        self.stats.wall = time.time() - t0
        for k, v in c.m.cov.items():
            self.stats.cov[k] = self.stats.cov.get(k, 0) + v
        self.stats.floor = max([self.stats.floor] + c.mir.floor + (self.aux.mir.floor if self.aux else []))
        return self.stats


def run_sequence(device, model, rng, n_ops, *, fam, dtype, bound, gap=4e-3, lp_tol=2e-5, aux=None, tag=""):
    """n_ops random operations on `device`, each predicted by `model` and checked; aux = (device, model) of the second context snapshots travel through"""
    main = Ctx(device, model, Mirror(fam, dtype, model.max_batch), "main")
    second = Ctx(aux[0], aux[1], Mirror(fam, dtype, aux[1].max_batch), "aux") if aux else None
    return Driver(main, second, rng, bound, gap, lp_tol, tag).run(n_ops)
