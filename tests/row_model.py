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

The arms whose name ends in _x draw the later row calls as well (tgx_splice_row, tgx_verify_rows, tgx_advance_rows, tgx_beam_select, tgx_beam_advance).  After a
splice a row's cache is no function of its token list any more: the oracles of such a row have their cache spliced (tests/splice_ref.py, rounded once to the storage
dtype), cut (set_past) and copied (read_kv / write_kv) instead of being forwarded again, until the row is admitted afresh (Row.spliced).
A negative
lens[i] of tgx_advance_rows cannot be passed through tinygpt_amd.ffi: the driver makes that one call on the C entry point (raw_advance_rows).
"""
from __future__ import annotations

import pickle
import time

import numpy as np

import beam_ref
import splice_ref
from conftest import load_golden, rel_err
from tinygpt_amd.desc import desc_from_hf_config
from tinygpt_amd.ffi import GREEDY, SamplerCfg, TgxError

OK, INVALID, UNSUPPORTED, STATE, CONTEXT = 0, 1, 2, 4, 8
BLK = 128
MAX_STOP, MAX_DRAFT, MAX_LOGPROBS, LOGPROB_RING = 8, 15, 20, 256
MAX_SPLICE_RANGES, MAX_VERIFY_POSITIONS, MAX_ADVANCE_POSITIONS, MAX_BEAMS, MAX_BEAM_CAND = 16, 64, 8192, 8, 32
STEP, FEED, FEED_MORE = 0, 1, 2
EMPTY, RETIRED, LIVE, FINISHED = "empty", "retired", "live", "finished"
GREEDY_T = (0.0, 0, 1.0, 0.0)
LENS = [1, 2, 17, 33, 100, 126, 127, 128, 129, 200, 255, 256, 257]
FAMS = ["llama_tiny", "qwen2_tiny", "mistral_tiny", "qwen3_tiny", "gpt2_hd64"]
ARMS = ["f32_slab", "h16_slab", "h16_paged", "f32_slab_x", "h16_slab_x", "h16_paged_x"]      # _x: the same dtype and layout, the kind table extended (Driver.WEIGHTS_X)
MAX_CTX = 384


def is_greedy(s):
    return not (s[0] > 0 or s[1] > 0 or s[2] < 1 or s[3] > 0)


def blocks_for(n):
    return (n + BLK - 1) // BLK


class Snap:
    """what a snapshot holds of a row, as far as the contract goes"""
    def __init__(self, row):
        self.tokens = list(row.tokens); self.has_logits = row.has_logits; self.has_token = row.has_logits and row.has_token
        self.spliced = row.spliced
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
        self.fed_more = False     # the row's last feed was a TGX_ADV_FEED_MORE: the rest of its prompt is still to come
        self.spliced = False      # tgx_splice_row has moved cache rows: the cache is no longer a function of the token list (until the row is admitted afresh)

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
    def __init__(self, max_batch, max_ctx, vocab, budget_tokens=0, gpt2=False):
        self.max_batch, self.max_ctx, self.vocab, self.gpt2 = max_batch, max_ctx, vocab, gpt2
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
        if new_len == x.length and x.has_logits and x.state != FINISHED:      # (on a finished row new_len == past is a truncation like any other)
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

    # ---- the later row calls: tgx_splice_row, tgx_verify_rows, tgx_advance_rows, tgx_beam_select, tgx_beam_advance
    @staticmethod
    def splice_src(ranges):
        """the source position of every kept position"""
        return [p for s, n in ranges for p in range(s, s + n)]

    def _splice_plan(self, row, ranges):
        """(new_len, f, no-op, the indices of the written blocks that forked siblings map as well) of a legal splice"""
        x = self.rows[row]
        src = self.splice_src(ranges)
        new_len = len(src)
        f = next((i for i, p in enumerate(src) if p != i), new_len)      # the end of the leading delta == 0 range; new_len for a truncation
        noop = new_len == x.length and f == new_len and x.has_logits and x.state != FINISHED      # (on a finished row it is a truncation: the state is cleared)
        swap = [i for i in range(f // BLK, blocks_for(new_len)) if self.pool.shared(x.blocks[i])] if self.pool and not noop else []
        return new_len, f, noop, swap

    def _why_splice_row(self, rs, row, ranges):
        if not self._in(row):
            rs.append((INVALID, "row_range")); return
        # the header's order: the row and n_keep; the row's state; GPT-2; then the ranges against the row's length
        if not 1 <= len(ranges) <= MAX_SPLICE_RANGES:
            rs.append((INVALID, "n_keep")); return
        x = self.rows[row]
        if not x.holds:                                             # a retired or empty row holds no positions: refused for its state whatever its ranges are
            rs.append((STATE, "splice_retired")); return
        if self.gpt2:                                               # learned positions: nothing to re-rotate
            rs.append((UNSUPPORTED, "gpt2")); return
        end = 0
        for s, n in ranges:                                          # empty, unsorted, overlapping, outside [0, past)
            if n < 1 or s < end or s + n > x.length:
                rs.append((INVALID, "bad_range")); return
            end = s + n
        new_len, f, noop, swap = self._splice_plan(row, ranges)
        if len(swap) > (len(self.pool.free) if self.pool else 0):   # against the free list ALONE: what the row gives back is not counted
            rs.append((CONTEXT, "pool"))

    def _do_splice_row(self, row, ranges, out_len):
        x = self.rows[row]
        new_len, f, noop, swap = self._splice_plan(row, ranges)
        assert int(out_len) == new_len, f"out_len {out_len}, the kept ranges hold {new_len}"
        if noop:
            return
        if self.pool:
            if swap:
                self.note("splice_cow_block" if f < new_len else "cow_truncation")
            for i in swap:
                old = x.blocks[i]; x.blocks[i] = self.pool.take(); self.pool.drop(old)
            self._trim(row, new_len)
            if f < new_len and any(self.pool.shared(b) for b in x.blocks[:f // BLK]):
                self.note("splice_shared_prefix_kept")
        src = self.splice_src(ranges)
        x.spliced = x.spliced or f < new_len
        x.state = LIVE; x.tokens = [x.tokens[p] for p in src]; x.has_logits = x.has_token = False; x.tok = None

    def _why_step_row(self, rs, r, n_draft, what):
        """tgx_verify_rows' per-row checks, in the one-row call's order"""
        if not self._in(r):
            rs.append((INVALID, "row_range")); return False
        if not 0 <= n_draft <= MAX_DRAFT:
            rs.append((INVALID, "n_draft"))
        if not self._source(r, rs, what):
            return False
        x = self.rows[r]
        if not x.has_logits:
            rs.append((STATE, "step_no_logits" if what == "step" else "truncated"))
        elif not x.has_token:
            rs.append((STATE, "step_no_token" if what == "step" else "no_token"))
        if x.length + n_draft + 1 > self.max_ctx:
            rs.append((CONTEXT, "max_ctx"))
        return True

    def _why_verify_rows(self, rs, rows, drafts):
        if not 1 <= len(rows) <= self.max_batch:
            rs.append((INVALID, "n")); return
        if any(not self._in(r) for r in rows):
            rs.append((INVALID, "row_range")); return
        if len(set(rows)) != len(rows):
            rs.append((INVALID, "row_twice"))
        for r, d in zip(rows, drafts):
            self._why_step_row(rs, r, len(d), "verify")
        if sum(len(d) + 1 for d in drafts) > MAX_VERIFY_POSITIONS:
            rs.append((INVALID, "positions"))
        if not rs and self.pool:                                    # the blocks of ALL named rows together
            self._short(sum(self._more(r, self.rows[r].length + len(d) + 1) for r, d in zip(rows, drafts)), len(self.pool.free), rs)

    def _do_verify_rows(self, rows, drafts, out):
        assert len(out) == len(rows), f"{len(out)} results for {len(rows)} rows"
        if all(len(d) == 0 for d in drafts):
            self.note("verify_rows_all_zero_drafts")
        for r, d, o in zip(rows, drafts, out):
            given = blocks_for(self.rows[r].length + len(d) + 1)
            self._do_verify_row(r, d, o)
            if self.pool and given > blocks_for(self.rows[r].length):
                self.note("verify_rows_rejects_tail_block")

    def _why_advance_rows(self, rs, rows, kinds, ids, lens=None):
        """lens: the call's lens[] where it is not the lengths of `ids` (only a raw call can pass a negative one)"""
        if not 1 <= len(rows) <= self.max_batch:
            rs.append((INVALID, "n")); return
        # first the call's own: kinds, lengths, the two position limits
        if any(not STEP <= k <= FEED_MORE for k in kinds):
            rs.append((INVALID, "kind")); return
        if lens is not None:
            assert any(n < 0 for n in lens) and all(n == len(d) for n, d in zip(lens, ids) if n >= 0), "explicit lens are for the negative-length refusal alone"
            rs.append((INVALID, "neg_len")); return
        if sum(len(d) + 1 for k, d in zip(kinds, ids) if k == STEP) > MAX_VERIFY_POSITIONS:
            rs.append((INVALID, "step_positions")); return
        if sum(len(d) + (k == STEP) for k, d in zip(kinds, ids)) > MAX_ADVANCE_POSITIONS:
            rs.append((INVALID, "positions")); return
        # then per row, each row's checks with the codes of its equivalent call
        if any(not self._in(r) for r in rows):
            rs.append((INVALID, "row_range")); return
        if len(set(rows)) != len(rows):
            rs.append((INVALID, "row_twice"))
        for r, k, d in zip(rows, kinds, ids):
            x = self.rows[r]
            if k == STEP:
                self._why_step_row(rs, r, len(d), "step")
                continue
            if len(d) < 1:
                rs.append((INVALID, "len"))
            if x.length + len(d) > self.max_ctx:                    # tgx_extend_row's past + seq, tgx_forward_row's seq
                rs.append((CONTEXT, "max_ctx"))
        new = sorted(r for r, k in zip(rows, kinds) if k != STEP and r >= self.batch)
        if new != list(range(self.batch, self.batch + len(new))):
            rs.append((INVALID, "gap"))
        if not rs and self.pool:                                    # ALL named rows together, against the free list plus what admission targets give back
            need = sum(self._more(r, self.rows[r].length + len(d) + (k == STEP)) for r, k, d in zip(rows, kinds, ids))
            self._short(need, len(self.pool.free) + self._given_back([r for r, k in zip(rows, kinds) if k != STEP and not self.rows[r].holds]), rs)

    def _do_advance_rows(self, rows, kinds, ids, out):
        assert len(out) == len(rows), f"{len(out)} results for {len(rows)} rows"
        has_step = STEP in kinds
        for r, k, d, o in zip(rows, kinds, ids, out):
            x = self.rows[r]
            if k == STEP:
                self._do_verify_row(r, d, o)
                continue
            assert len(o[0]) == 0 and o[1] == 0, f"a FEED row reports out_n {len(o[0])} / out_finish {o[1]}"
            if x.holds:
                if x.state == FINISHED and has_step:
                    self.note("advance_over_finished_row")
                if not x.has_logits and x.state == LIVE and x.fed_more and k == FEED:
                    self.note("advance_feed_more_then_feed")
                self._do_extend_row(r, d)
            else:
                if r >= self.batch:
                    self.note("advance_admits_new_row")
                self._do_forward_row(r, d)
            x.fed_more = k == FEED_MORE
            if k == FEED_MORE:                                      # "no logits and no current token"; an admission by FEED_MORE counts as an admission
                x.has_logits = x.has_token = False; x.tok = None

    def _why_beam_select(self, rs, rows, scores, k, end_ids):
        if not 1 <= len(rows) <= MAX_BEAMS or not 1 <= k <= MAX_BEAMS or len(end_ids) > MAX_STOP:
            rs.append((INVALID, "n_k_end")); return
        if any(not np.isfinite(s) for s in scores):
            rs.append((INVALID, "score"))
        if any(not self._in(r) for r in rows):
            rs.append((INVALID, "row_range")); return
        if len(set(rows)) != len(rows):
            rs.append((INVALID, "row_twice"))
        for r in rows:
            if self._source(r, rs, "beam") and not self.rows[r].has_logits:
                rs.append((STATE, "no_logits"))

    def _do_beam_select(self, rows, scores, k, end_ids):
        pass

    def beam_placement(self, rows, parent):
        """the PINNED rule -> (out_rows, the childless sources)"""
        n_next = len(parent)
        out = [None] * n_next
        sources = [i for i, r in enumerate(rows) if self.rows[r].state == LIVE]
        pinned = {}
        for j, p in enumerate(parent):
            pinned.setdefault(p, j)
        for p, j in pinned.items():
            out[j] = rows[p]
        childless = [i for i in sources if i not in pinned]
        empty = sorted(childless + [i for i in range(len(rows)) if i not in sources])      # empty once the childless sources are retired, in array order
        for j in range(n_next):
            if out[j] is None:
                out[j] = rows[empty.pop(0)]
        return out, [rows[i] for i in childless]

    def _why_beam_advance(self, rs, rows, parent, tokens):
        if not 1 <= len(rows) <= MAX_BEAMS or not 1 <= len(parent) <= len(rows):
            rs.append((INVALID, "n")); return
        if any(not self._in(r) for r in rows):
            rs.append((INVALID, "row_range")); return
        if len(set(rows)) != len(rows):
            rs.append((INVALID, "row_twice")); return
        if any(not 0 <= p < len(rows) for p in parent):
            rs.append((INVALID, "parent_range")); return
        if any(not 0 <= t < self.vocab for t in tokens):
            rs.append((INVALID, "token"))
        for r in rows:
            x = self.rows[r]
            if x.state == FINISHED:
                rs.append((STATE, "finished_source"))
            elif x.state == LIVE and not x.has_logits:
                rs.append((STATE, "no_logits"))
        if any(self.rows[rows[p]].state not in (LIVE, FINISHED) for p in parent):
            rs.append((STATE, "parent_is_spare"))
        if any(c == STATE for c, _ in rs):
            return
        out, childless = self.beam_placement(rows, parent)
        new = sorted(r for r in out if r >= self.batch)             # the new rows that RECEIVE a hypothesis
        if new != list(range(self.batch, self.batch + len(new))):
            rs.append((INVALID, "gap"))
        if not rs and self.pool:                                    # the fresh tail blocks against the free list plus what the childless sources give back
            pinned = set()
            tails = 0
            for j, p in enumerate(parent):
                if p in pinned:
                    tails += self.rows[rows[p]].length % BLK != 0
                pinned.add(p)
            self._short(tails, len(self.pool.free) + self._given_back(childless), rs)

    def _do_beam_advance(self, rows, parent, tokens, out_rows):
        want, childless = self.beam_placement(rows, parent)
        assert [int(r) for r in out_rows] == want, f"out_rows {[int(r) for r in out_rows]}, the pinned placement gives {want}"
        if self.pool and any(self.pool.shared(b) for r in rows for b in self.rows[r].blocks):
            self.note("beam_on_already_forked_rows")
        src = {rows[p]: Snap(self.rows[rows[p]]) for p in parent}
        for r in childless:                                         # retired first, as by tgx_reset_row
            self.note("beam_childless_source_retired")
            self._do_reset_row(r)
        seen = set()
        for j, p in enumerate(parent):
            r, d, s = rows[p], want[j], src[rows[p]]
            if p not in seen:                                       # its lowest-j child stays in place
                seen.add(p)
                self.rows[r].has_token, self.rows[r].tok = True, int(tokens[j])
                continue
            if d >= self.batch:
                self.note("beam_new_row_spare")
            if self.pool:                                           # tgx_fork_row's destination, word for word
                pb = self.rows[r].blocks
                self._release(d)
                for b in pb[:len(s.tokens) // BLK]:
                    self.pool.ref[b] += 1; self.rows[d].blocks.append(b)
                if len(s.tokens) % BLK:
                    self.note("beam_copied_child_tail_block")
                    self.rows[d].blocks.append(self.pool.take())
            self._admit(d, s.tokens, True, True, int(tokens[j])); self.rows[d].spliced = s.spliced
        return want, childless

    # ---- apply: the state after a call that returned TGX_OK.  `out` is what the device produced (ids); the counts it reported are checked against the stop rules
    def apply(self, kind, *a, out=None):
        return getattr(self, "_do_" + kind)(*a) if out is None else getattr(self, "_do_" + kind)(*a, out)

    def _admit(self, r, tokens, has_logits=True, has_token=False, tok=None):
        x = self.rows[r]
        x.state = LIVE; x.tokens = list(tokens); x.has_logits = has_logits; x.has_token = has_token; x.tok = tok
        x.produced = 0; x.lp_count = 0; x.fed_more = False
        self.batch = max(self.batch, r + 1)

    def _do_forward_rows(self, rows, prompts):
        if self.pool:
            for r in rows:
                self._release(r)
            for r, p in zip(rows, prompts):
                self._grow(r, len(p))
        for r, p in zip(rows, prompts):
            self._admit(r, p); self.rows[r].spliced = False

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
            self._admit(d, s.tokens, True, s.has_token, s.tok); self.rows[d].spliced = s.spliced

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
        if new_len == x.length and x.has_logits and x.state != FINISHED:
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
        self._admit(row, snap.tokens, snap.has_logits, snap.has_token, snap.tok); self.rows[row].spliced = snap.spliced


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# the random stream behind a (seed, arm), where it is not the seed's own number: chosen in the CPU dry run (tests/test_row_model.py) so that the oracle stays far enough
# from its reordered twin on every sequence
# mistral_tiny (hidden 512, head_dim 128) in fp32: these streams stay under the 1e-5 the arm asks for, where the seed's own number did not (the dry run prints each floor)
STREAM = {(2, "f32_slab"): 402, (7, "f32_slab"): 407, (2, "f32_slab_x"): 402}
BUDGET_X = 1.0      # blocks per row of the paged _x arm: forked and beam rows share their full blocks, so the pool lasts longer per row than in the old arm


def base_arm(arm):
    return arm[:-2] if arm.endswith("_x") else arm


def case(seed, arm):
    """the fixture, dtype and geometry of one (seed, arm)"""
    fam = FAMS[seed % len(FAMS)]
    x, base = arm.endswith("_x"), base_arm(arm)
    dtype = "fp32" if base == "f32_slab" else ("fp16" if seed % 4 == 2 else "bf16")
    rng = np.random.default_rng(90000 + 17 * STREAM.get((seed, arm), seed) + ARMS.index(arm))      # (an _x arm's index is its own: a stream of its own)
    max_batch = int(rng.integers(6, 9)) if x else int(rng.integers(4, 7))      # _x: a beam group of up to 4 + 2 spares next to bystanders
    budget = blocks_for(int(BUDGET_X * max_batch * BLK)) * BLK if x else blocks_for(int(1.5 * max_batch * BLK)) * BLK
    return dict(seed=seed, arm=arm, fam=fam, dtype=dtype, max_batch=max_batch, max_ctx=MAX_CTX, budget=budget if base == "h16_paged" else 0, rng=rng, extended=x)


def angle_table(fam, dtype):
    """the RoPE angles [MAX_CTX][hd / 2] tests/splice_ref.py rotates by: its own float32 table where the frequencies are unscaled; for Llama-3's scaled ones the
    angles of the oracle's cos / sin tables (only differences of two angles are used, so the branch of atan2 does not matter)"""
    if (fam, dtype) not in _angles:
        d, _, _ = make_desc(fam, dtype, 1)
        if d.rope_factor > 0:
            cos, sin = new_oracle(fam, dtype).rope_tables(MAX_CTX)
            _angles[(fam, dtype)] = np.arctan2(sin.astype(np.float64), cos.astype(np.float64))
        else:
            _angles[(fam, dtype)] = splice_ref.angles(d, MAX_CTX)
    return _angles[(fam, dtype)]


_angles = {}


def round_storage(x, dtype):
    """fp64 -> the storage dtype (round to nearest even), as float32"""
    x = np.asarray(x, np.float64).astype(np.float32)
    if dtype == "fp32":
        return x
    if dtype == "fp16":
        return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(x.shape)


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

    # ---- a cache that is no function of the token list (tgx_splice_row): set from cache rows, never re-forwarded
    def plant(self, kv, toks):
        """the cache becomes kv ([layer] -> (K rows, V rows), rounded once to the storage dtype by write_kv) and holds len(toks) positions"""
        self.o.reset_cache()
        for l, (k, v) in enumerate(kv):
            self.o.write_kv(0, l, k[:len(toks)], v[:len(toks)])
        self.o.set_past(len(toks)); self.toks = [int(t) for t in toks]

    def export(self, layers):
        return [tuple(a.copy() for a in self.o.read_kv(0, l)) for l in range(layers)]

    def splice(self, ranges, ang, layers):
        kv = []
        for l in range(layers):
            k, v = self.o.read_kv(0, l)
            kv.append(splice_ref.splice(k, v, ranges, ang))
        self.plant(kv, [self.toks[p] for p in RowModel.splice_src(ranges)])

    def cut(self, n):
        self.o.set_past(n); self.toks = self.toks[:n]

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


def raw_advance_rows(dev, rows, kinds, ids, lens):
    """tgx_advance_rows with a lens[] of the caller's own (tinygpt_amd.ffi.Model.advance_rows derives it from the arrays, so it cannot pass a negative one)"""
    if isinstance(dev, OracleDevice):
        return dev.advance_rows(rows, kinds, ids, lens=lens)
    from ctypes import POINTER, c_int32, c_int64
    a = lambda v, t: np.ascontiguousarray(np.asarray(v, dtype=t).reshape(-1))
    r, k, n = a(rows, np.int32), a(kinds, np.int32), a(lens, np.int32)
    flat = a([t for d in ids for t in d] + [0], np.int64)
    out, out_n, fin = np.zeros((len(r), MAX_DRAFT + 1), np.int64), np.zeros(len(r), np.int32), np.zeros(len(r), np.int32)
    p32, p64 = (lambda x: x.ctypes.data_as(POINTER(c_int32))), (lambda x: x.ctypes.data_as(POINTER(c_int64)))
    dev._check(dev.be.advance_rows(dev._ctx, len(r), p32(r), p32(k), p64(flat), p32(n), p64(out), p32(out_n), p32(fin)))
    return [(out[i, :out_n[i]].copy(), int(fin[i])) for i in range(len(r))]


class OracleDevice:
    """the row calls of tinygpt_amd.ffi.Model answered by a RowModel and one batch-1 CPU oracle per row"""
    blob_is_private = True      # its snapshots are no tgx snapshots: two contexts need not write the same bytes

    def __init__(self, fam, dtype, max_batch, max_ctx=MAX_CTX, budget=0):
        self.desc, _, _ = make_desc(fam, dtype, max_batch, max_ctx)
        self.fam, self.dtype = fam, dtype
        self.m = RowModel(max_batch, max_ctx, self.desc.vocab, budget, gpt2=self.desc.family == "gpt2")
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
        if base and self.m.rows[r].spliced:                         # the cache rows are the row's own: no token list gives them
            o.plant(self.kv[r], base); o.sync(base + new)
        elif base:
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
        if not (n == x.length and x.has_logits and x.state != FINISHED):
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

    # ---- the later row calls
    def splice_row(self, row, ranges):
        ranges = [(int(s), int(n)) for s, n in np.asarray(ranges, np.int64).reshape(-1, 2)]
        self._gate("splice_row", row, ranges)
        new_len, f, noop, _ = self.m._splice_plan(row, ranges)
        if not noop:
            ang = angle_table(self.fam, self.dtype)
            self.kv[row] = [[round_storage(a, self.dtype) for a in splice_ref.splice(k[:self.lens[row]], v[:self.lens[row]], ranges, ang)] for k, v in self.kv[row]]
            self.lens[row] = new_len
        self.m.apply("splice_row", row, ranges, out=new_len)
        return new_len

    def _verify_one(self, row, draft):
        """tgx_verify_row_sampled's walk on one row -> (ids, finish); the model is not moved"""
        x = self.m.rows[row]
        toks, cur, shadow, out, fin = list(x.tokens), x.tok, Row(), [], 0
        shadow.max_new, shadow.stop_ids, shadow.produced = x.max_new, x.stop_ids, x.produced
        for i in range(len(draft) + 1):
            self._step(row, toks, cur); toks.append(cur)
            cur = draw_token(self.lg[row], x.sampler, x.seed, len(toks), row); out.append(cur); self._record(row, cur)
            fin = shadow.note_produced(cur)
            if fin or i == len(draft) or cur != draft[i]:
                break
        self._verified(row)
        return np.array(out, np.int64), fin

    def verify_rows(self, rows, drafts):
        rows = [int(r) for r in rows]; drafts = [[int(t) for t in d] for d in drafts]
        self._gate("verify_rows", rows, drafts)
        out = [self._verify_one(r, d) for r, d in zip(rows, drafts)]
        self.m.apply("verify_rows", rows, drafts, out=out)
        return out

    def advance_rows(self, rows, kinds, ids, lens=None):
        rows = [int(r) for r in rows]; kinds = [int(k) for k in kinds]; ids = [[int(t) for t in d] for d in ids]
        self._gate("advance_rows", rows, kinds, ids, *([] if lens is None else [list(lens)]))
        out = []
        for r, k, d in zip(rows, kinds, ids):
            if k == STEP:
                out.append(self._verify_one(r, d)); continue
            x = self.m.rows[r]
            if x.holds:
                self._run(r, x.tokens, d)
            else:
                self.rec[r] = []; self._run(r, [], d)
            out.append((np.zeros(0, np.int64), 0))
        self.m.apply("advance_rows", rows, kinds, ids, out=out)
        return out

    def beam_select(self, rows, scores, k, end_ids=()):
        rows = [int(r) for r in rows]; scores = [float(x) for x in scores]; end_ids = [int(e) for e in end_ids]
        self._gate("beam_select", rows, scores, int(k), end_ids)
        prefix, _ = beam_ref.select([self.lg[r] for r in rows], scores, int(k), end_ids)
        return (np.array([c[1] for c in prefix], np.int32), np.array([c[3] for c in prefix], np.int32), np.array([c[0] for c in prefix], np.float32),
                np.array([c[4] for c in prefix], np.float32))

    def beam_advance(self, rows, parent, tokens):
        rows = [int(r) for r in rows]; parent = [int(p) for p in parent]; tokens = [int(t) for t in tokens]
        self._gate("beam_advance", rows, parent, tokens)
        out, childless = self.m.beam_placement(rows, parent)
        held = {rows[p]: (self._copy_rows(self.kv[rows[p]], self.lens[rows[p]]), self.lg[rows[p]].copy(), self.lens[rows[p]]) for p in parent}
        for r in childless:
            self.rec[r] = []; self.lens[r] = 0
        for j, p in enumerate(parent):
            if out[j] != rows[p]:
                kv, lg, n = held[rows[p]]
                self.kv[out[j]] = self._copy_rows(kv, n); self.lg[out[j]] = lg.copy(); self.lens[out[j]] = n; self.rec[out[j]] = []
        self.m.apply("beam_advance", rows, parent, tokens, out=out)
        return np.array(out, np.int32)

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
        if key in ("verify.last_form", "advance.last_form"):
            return 0                                                # no device pass is ever made here
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

    # ---- rows whose cache tgx_splice_row has moved: the oracle's cache is spliced, cut and copied; it is never rebuilt from the token list
    def splice(self, r, ranges, layers):
        ang = angle_table(self.fam, self.dtype)
        for o in self._pair(r):
            o.splice(ranges, ang, layers)
        self.lg[r] = None

    def cut(self, r, n):
        for o in self._pair(r):
            o.cut(n)
        self.lg[r] = None

    def export(self, r, layers):
        """what a copy of row r starts from: both oracles' cache rows, the token list, the logits"""
        a, b = self._pair(r)
        return dict(a=a.export(layers), b=b.export(layers), toks=list(a.toks), lg=None if self.lg[r] is None else self.lg[r].copy())

    def plant(self, r, e, has_logits=True):
        a, b = self._pair(r)
        a.plant(e["a"], e["toks"]); b.plant(e["b"], e["toks"])
        self.lg[r] = e["lg"].copy() if has_logits and e["lg"] is not None else None

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
        self.forms = {}            # (call, verify.last_form / advance.last_form) -> accepted calls

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

    # the _x arms: the 16 kinds above plus the later row calls, which carry about half of the weight (beam = tgx_beam_select, then tgx_beam_advance on its candidates)
    KINDS_X = ["splice_row", "verify_rows", "advance_rows", "beam_select", "beam_advance"]
    WEIGHTS_X = dict(splice_row=6.0, verify_rows=5.0, advance_rows=7.0, beam=7.0)
    LENS_X = [1, 2, 5, 17, 33, 100, 127, 128, 129]      # FEED lengths: every token goes through a per-row CPU oracle one by one behind a prefix
    # the matrix-core routes' minimum (prefill_min_rows, set in tgx_create, tinygpt_amd/csrc/abi.hip: 5 at hidden <= 2048, 4 above): calls of fewer positions run row
    # by row.  Every fixture of FAMS has hidden <= 512; a larger fixture needs its own value.  tgx_verify_rows' generator aims at it; tgx_advance_rows' FEED lengths
    # (LENS_X) pass it on their own
    MIN_JOINT = 5

    def __init__(self, main, aux, rng, bound, gap, lp_tol, tag, extended=False):
        self.c, self.aux, self.rng, self.extended = main, aux, rng, extended
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
        if kind in ("forward_row", "forward_rows", "extend_row", "score_row", "restore_row", "fork_row", "decode", "decode_rows", "verify_row", "verify_rows",
                    "advance_rows", "beam_advance"):
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
            if not c.m.rows[row].has_logits and c.m.rows[row].spliced:
                c.mir.cut(row, n); self.mark("truncate_spliced_row")
            elif not c.m.rows[row].has_logits:
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
                self.copy_mirror(c, src, d)
            if c.m.rows[src].spliced:
                self.mark("splice_then_fork")
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
            if c.m.rows[row].spliced:                               # no token list gives this cache: the reference's own travels with the snapshot
                res["ret"].planted = c.mir.export(row, c.layers)
            return res["out"], res["ret"], shot
        return None

    def do_restore(self, c, row, saved, illegal=None):
        blob, snap, shot = saved
        res = self.op(c, "restore_row", (row, snap), lambda d: d.restore_row(row, blob), [row], illegal=illegal)
        if res:
            self.need(res["after"]["lens"][row] == len(snap.tokens), "restored length")
            self.same_row(shot, res["after"], 0, row, f"restore into row {row}", logits=snap.has_logits)
            if snap.spliced:
                c.mir.plant(row, snap.planted, snap.has_logits)
            else:
                c.mir.clear(row); c.mir.follow(row, snap.tokens)
            if not snap.has_logits:
                c.mir.lg[row] = None
            self.check_logits(c, res["after"])
        return res

    # ---- the later row calls
    def mark(self, what):
        self.stats.cov[what] = self.stats.cov.get(what, 0) + 1

    def copy_mirror(self, c, src, dst):
        """the reference of a copy: a forward of the token list, or — behind a splice — the source oracle's cache rows"""
        if c.m.rows[dst].spliced:
            c.mir.plant(dst, c.mir.export(src, c.layers))
        else:
            c.mir.clear(dst); c.mir.follow(dst, c.m.rows[dst].tokens)

    def tally_form(self, c, call):
        if c is self.c:
            f = int(c.dev.get_option(call + ".last_form"))
            self.stats.forms[(call, f)] = self.stats.forms.get((call, f), 0) + 1

    def do_splice(self, c, row, ranges, illegal=None):
        from test_hip_splice_row import rotated_k_bound
        m = c.m
        ranges = [(int(s), int(n)) for s, n in ranges]
        legal = not m.reasons("splice_row", row, ranges)
        if legal:
            x = m.rows[row]
            plan, pre, was_spliced, was = m._splice_plan(row, ranges), list(x.tokens), x.spliced, (x.state, x.has_logits, x.has_token)
        elif c is self.c and m._in(row) and not m.rows[row].holds and 1 <= len(ranges) <= MAX_SPLICE_RANGES:
            self.mark("splice_refused_retired_row" if row < m.batch else "splice_refused_row_beyond_batch")
        res = self.op(c, "splice_row", (row, ranges), lambda d: d.splice_row(row, np.array(ranges, np.int64).reshape(-1, 2)), [row], out_to_model=lambda n: n, illegal=illegal)
        if not res:
            return res
        res["was"] = was
        new_len, f, noop, _ = plan
        if c is self.c:
            was = res["was"]
            self.mark("splice_on_finished_row" if was[0] == FINISHED else "splice_on_no_logits_row" if not was[1] else "splice_on_token_row" if was[2] else "splice_on_logits_only_row")
            if noop:
                self.mark("splice_noop")
            elif f == new_len:
                self.mark("splice_truncation_form")
            elif ranges[0][0] == 0:
                self.mark("splice_lead_on_block_edge" if f % BLK == 0 else "splice_lead_inside_block")
            if any(a[0] + a[1] == b[0] for a, b in zip(ranges, ranges[1:])):
                self.mark("splice_ranges_touch")
        if noop:
            self.same_row(res["before"], res["after"], row, row, "splice_row: the no-op")
            return res
        src = np.array(RowModel.splice_src(ranges)); moved = src != np.arange(new_len)
        ang = angle_table(c.mir.fam, c.mir.dtype)
        for l in range(c.layers):
            (k0, v0), (k1, v1) = res["before"]["kv"][row][l], res["after"]["kv"][row][l]
            self.need(v1.shape == v0[src].shape and np.array_equal(v1.view(np.uint32), v0[src].view(np.uint32)), f"splice_row: V rows of layer {l} are not the kept source rows")
            self.need(np.array_equal(k1[~moved].view(np.uint32), k0[src][~moved].view(np.uint32)), f"splice_row: K rows of layer {l} with delta 0 changed")
            if moved.any():
                ref, _ = splice_ref.splice(k0, v0, ranges, ang)
                err, bound = np.abs(k1 - ref)[moved], rotated_k_bound(ref, c.mir.dtype)[moved]
                self.need((err <= bound).all(), f"splice_row: rotated K rows of layer {l} are {float((err / bound).max()):.2f} of the bound from tests/splice_ref.py")
        if f < new_len:
            if not was_spliced and (c.mir.a[row] is None or c.mir.a[row].toks != pre):
                c.mir.follow(row, pre)
            c.mir.splice(row, ranges, c.layers)
        elif was_spliced:
            c.mir.cut(row, new_len); self.mark("truncate_spliced_row")
        else:
            c.mir.follow(row, m.rows[row].tokens); c.mir.lg[row] = None
        return res

    def _stepped(self, c, r, base, tok, greedy, o, what, before, after):
        """what the driver checks of a row that tgx_verify_row stepped, for every STEP row of the joint calls"""
        out = [int(t) for t in o[0]]
        self.same_row(before, after, r, r, what + ": the prefix", upto=len(base), logits=False)
        self.follow_steps(c, r, base, [tok] + out[:-1], out, greedy, what)
        if c.m.rows[r].state == FINISHED:
            c.mir.lg[r] = None
        else:
            self.check_lp(c, r, after, out[-1])

    def do_verify_rows(self, c, rows, drafts, illegal=None):
        m = c.m
        pre = {r: (list(m.rows[r].tokens), m.rows[r].tok, is_greedy(m.rows[r].sampler)) for r in rows if m._in(r)}
        res = self.op(c, "verify_rows", (rows, drafts), lambda d: d.verify_rows(rows, drafts), rows, out_to_model=lambda o: o, illegal=illegal)
        if res:
            for r, o in zip(rows, res["out"]):
                self._stepped(c, r, *pre[r], o, "verify_rows", res["before"], res["after"])
            self.check_logits(c, res["after"])
            self.tally_form(c, "verify")
        return res

    def do_advance_rows(self, c, rows, kinds, ids, lens=None, illegal=None):
        m = c.m
        pre = {r: (list(m.rows[r].tokens), m.rows[r].tok, is_greedy(m.rows[r].sampler), m.rows[r].holds) for r in rows if m._in(r)}
        if lens is not None:                                        # a lens[] of its own: the raw call, refused by the header whatever else it names
            return self.op(c, "advance_rows", (rows, kinds, ids, lens), lambda d: raw_advance_rows(d, rows, kinds, ids, lens), rows, out_to_model=lambda o: o, illegal=illegal)
        res = self.op(c, "advance_rows", (rows, kinds, ids), lambda d: d.advance_rows(rows, kinds, ids), rows, out_to_model=lambda o: o, illegal=illegal)
        if res:
            for r, k, d, o in zip(rows, kinds, ids, res["out"]):
                base, tok, greedy, held = pre[r]
                if k == STEP:
                    self._stepped(c, r, base, tok, greedy, o, "advance_rows", res["before"], res["after"])
                    continue
                if held:
                    self.same_row(res["before"], res["after"], r, r, "advance_rows: the prefix", upto=len(base), logits=False)
                    self.follow_steps(c, r, base, d, [], False, "advance_rows")
                else:
                    c.mir.clear(r); c.mir.follow(r, d)
                if k == FEED_MORE:
                    c.mir.lg[r] = None
            self.check_logits(c, res["after"])
            self.tally_form(c, "advance")
        return res

    def do_beam_select(self, c, rows, scores, k, ends, illegal=None):
        res = self.op(c, "beam_select", (rows, scores, k, ends), lambda d: d.beam_select(rows, scores, k, ends), [], illegal=illegal)
        if res:
            beam, token, score, lp = res["out"]
            vecs = [res["after"]["lg"][r] for r in rows]
            prefix, rest = beam_ref.select(vecs, scores, k, ends)
            self.need(len(beam) == len(prefix), f"beam_select returned {len(beam)} candidates, the reference on the device's own logits {len(prefix)}")
            seq = prefix + rest[:1]
            for j, (key, i, _, t, l) in enumerate(prefix):
                tied = (j > 0 and seq[j - 1][0] == key) or (j + 1 < len(seq) and seq[j + 1][0] == key)
                if not tied:                                        # (which of two equal keys comes first is the order's business; their score is the same number)
                    self.need((int(beam[j]), int(token[j])) == (i, t), f"beam_select: candidate {j} is {(int(beam[j]), int(token[j]))}, the reference's {(i, t)}")
                    self.need(abs(float(lp[j]) - l) <= self.lp_tol, f"beam_select: candidate {j} lp {float(lp[j]):.7f}, the reference's {l:.7f}")
                else:                                               # the device's own choice among the tied: its lp against that row's reference
                    self.need(0 <= int(beam[j]) < len(rows) and 0 <= int(token[j]) < c.m.vocab, f"beam_select: candidate {j} is {(int(beam[j]), int(token[j]))}")
                    own = float(beam_ref.log_softmax64(vecs[int(beam[j])])[int(token[j])])
                    self.need(abs(float(lp[j]) - own) <= self.lp_tol, f"beam_select: candidate {j} lp {float(lp[j]):.7f}, the fp64 log-softmax of its row gives {own:.7f}")
                # lp_tol plus the fp32 rounding of the key: tests/test_hip_beam.py's bound on a score
                self.need(abs(float(score[j]) - key) <= self.lp_tol + 2.0 ** -23 * abs(key), f"beam_select: candidate {j} score {float(score[j]):.7f}, the reference's {key:.7f}")
        return res

    def do_beam_advance(self, c, rows, parent, tokens, illegal=None):
        m = c.m
        lens = {r: m.rows[r].length for r in rows if m._in(r)}
        res = self.op(c, "beam_advance", (rows, parent, tokens), lambda d: d.beam_advance(rows, parent, tokens), rows, out_to_model=lambda o: [int(r) for r in o], illegal=illegal)
        if res:
            want, childless = res["ret"]
            for r in childless:
                self.need(r in want or res["after"]["lens"][r] == 0, f"beam_advance: the childless source {r} is not retired")
                c.mir.clear(r)
            for j, p in enumerate(parent):
                r, d = rows[p], want[j]
                self.need(res["after"]["lens"][d] == lens[r], f"beam_advance: hypothesis {j} in row {d} holds {res['after']['lens'][d]} positions, its parent held {lens[r]}")
                self.same_row(res["before"], res["after"], r, d, f"beam_advance: hypothesis {j} (row {r} -> {d})", upto=lens[r])
                if d != r:
                    self.copy_mirror(c, r, d)
            self.check_logits(c, res["after"])
        return res

    def drafts_for(self, c, r, nd):
        """as verify_row's generator: the oracle's greedy continuation, half of the time with one id replaced — accept lengths vary"""
        x = c.m.rows[r]
        if nd == 0:
            return []
        if not is_greedy(x.sampler) or x.spliced:
            return self.ids(nd)
        draft = c.mir.greedy_continuation(x.tokens, x.tok, nd)
        if self.rng.random() < 0.5:
            i = int(self.rng.integers(0, nd)); draft[i] = (draft[i] + 1 + int(self.rng.integers(0, c.m.vocab - 1))) % c.m.vocab
        return draft

    def splice_ranges(self, L):
        """1 .. 4 kept ranges of a row of L >= 2 positions, in one of the forms the header singles out"""
        rng = self.rng
        form = str(self.pick(["noop", "trunc", "lead_in_block", "lead_on_edge", "touch", "no_lead", "multi", "multi"]))
        cut = lambda lo, hi: int(rng.integers(lo, hi)) if hi > lo else lo
        if form == "noop":
            return [(0, L)]
        if form == "trunc":
            return [(0, cut(1, L))]
        if form == "no_lead":
            s = cut(1, L); return [(s, L - s)]
        if form == "lead_on_edge" and L > BLK + 1:
            a = BLK * cut(1, (L - 2) // BLK + 1); b = cut(a + 1, L)
            return [(0, a), (b, L - b)]
        if form == "touch" and L >= 4:
            a = cut(1, L - 2); b = cut(a + 1, L - 1); e = cut(b + 1, L + 1)
            return [(0, a), (a, b - a)] + ([(e, L - e)] if e < L else [])      # (without a third range: a truncation in two touching pieces)
        if form in ("lead_in_block", "lead_on_edge", "touch"):
            a = cut(1, L); a += a % BLK == 0 and a + 1 < L
            b = cut(min(a + 1, L - 1), L)
            return [(0, a), (b, L - b)] if b > a else [(0, a)]
        n = int(rng.integers(2, 5))
        pts = sorted(set(int(x) for x in rng.integers(0, L + 1, 2 * n)))
        out = [(pts[i], pts[i + 1] - pts[i]) for i in range(0, len(pts) - 1, 2)]
        return out or [(0, L)]

    def draw_legal_x(self, kind):
        """one of the later row calls, legal up to the pool (a shortfall is a refusal the model predicts)"""
        c, m, rng = self.c, self.c.m, self.rng
        live = self.rows_where(c, lambda r, x: x.state == LIVE)
        ready = [r for r in live if m.rows[r].has_logits and m.rows[r].has_token and m.rows[r].length + 1 <= m.max_ctx]
        if kind == "splice_row":
            cand = self.rows_where(c, lambda r, x: x.holds and x.length >= 2)
            if not cand:
                return None
            shared = [r for r in cand if m.pool and any(m.pool.shared(b) for b in m.rows[r].blocks)]
            r = int(self.pick(shared)) if shared and rng.random() < 0.6 else int(self.pick(cand))
            fin = [q for q in cand if m.rows[q].state == FINISHED]
            if fin and rng.random() < 0.7:
                r = int(self.pick(fin))
            x = m.rows[r]
            ranges = self.splice_ranges(x.length)
            if r in shared and x.length > BLK + 2 and rng.random() < 0.9:      # the identity prefix covers whole blocks the siblings map as well: they stay shared
                a = int(rng.integers(BLK, x.length - 1)); b = int(rng.integers(a + 1, x.length))
                ranges = [(0, a), (b, x.length - b)]
            if r in shared and not m.pool.free and rng.random() < 0.8:      # no free block: a splice that writes into a shared block is refused whatever the row gives back
                ranges = [(1, x.length - 1)]
            res = self.do_splice(c, r, ranges)
            if res and not m.gpt2 and not m.rows[r].has_logits:    # next: what the spliced row goes through — fed again and forked, saved and restored, rolled back
                nxt = str(self.pick(["fork", "fork", "snapshot", "snapshot", "truncate", "none"]))
                if nxt == "fork":
                    def feed_and_fork():
                        if m.rows[r].holds and m.rows[r].spliced and m.rows[r].length + 3 <= m.max_ctx and self.do_extend(c, r, self.ids(int(rng.integers(1, 4)))):
                            t = self.free_targets(c, int(rng.integers(1, 3)))
                            if t:
                                self.pending.append(lambda: self.do_fork(c, r, t) if m.rows[r].state == LIVE and m.rows[r].has_logits and not any(m.rows[d].holds for d in t) else None)
                    self.pending.append(feed_and_fork)
                elif nxt == "snapshot":
                    self.pending.append(lambda: self.do_snapshot(r) if m.rows[r].state == LIVE else None)
                elif nxt == "truncate" and m.rows[r].length >= 2:
                    n = int(rng.integers(1, m.rows[r].length))
                    self.pending.append(lambda: self.do_truncate(c, r, n) if m.rows[r].holds and m.rows[r].length >= n else None)
            return res
        if kind == "verify_rows":
            if not ready:
                return None
            rng.shuffle(ready)
            edge = [r for r in ready if m.rows[r].length % BLK >= BLK - MAX_DRAFT and m.rows[r].length + MAX_DRAFT + 1 <= m.max_ctx]
            if not edge and m.pool and rng.random() < 0.35 and self.free_targets(c, 1):      # no such row: one is admitted, and verified next with a draft of noise
                t = self.free_targets(c, 1)
                res = self.do_admit(c, t, [self.ids(int(self.pick([120, 125, 127])))], "forward_row")
                if res:
                    self.pending.append(lambda: self.do_sample(c, t[0]) if m.rows[t[0]].state == LIVE and m.rows[t[0]].has_logits else None)
                    self.pending.append(lambda: self.do_verify_rows(c, t, [self.ids(MAX_DRAFT)]) if m.rows[t[0]].state == LIVE and m.rows[t[0]].has_logits and m.rows[t[0]].has_token else None)
                return res
            if edge and rng.random() < 0.7:                        # a row whose draft reaches into the next block comes first
                ready = edge[:1] + [r for r in ready if r != edge[0]]
            rows = [int(r) for r in ready[:int(rng.integers(1, len(ready) + 1))]]
            zero, left, drafts = rng.random() < 0.2, MAX_VERIFY_POSITIONS, []
            for i, r in enumerate(rows):
                room = min(MAX_DRAFT, m.max_ctx - m.rows[r].length - 1, left - (len(rows) - i))
                nd = 0 if zero or room < 1 else int(rng.integers(0, room + 1))
                if i == 0 and not zero and rng.random() < 0.5:                 # at or above the joint pass's minimum whatever the other rows draw
                    nd = max(nd, min(room, self.MIN_JOINT - 1))
                if i == 0 and r in edge and not zero and rng.random() < 0.7:   # ... and is all noise: the block it was given for the draft goes back
                    drafts.append(self.ids(room)); left -= room + 1
                    continue
                drafts.append(self.drafts_for(c, r, nd)); left -= nd + 1
            return self.do_verify_rows(c, rows, drafts)
        if kind == "advance_rows":
            fin_now = any(x.state == FINISHED for x in m.rows)
            mode = "mixed" if fin_now else str(self.pick(["mixed", "mixed", "mixed", "mixed", "no_step", "no_feed"]))
            rows, kinds, ids, left, nb = [], [], [], MAX_VERIFY_POSITIONS, m.batch
            feed = lambda room: (FEED_MORE if rng.random() < 0.3 else FEED, self.ids(int(self.pick([n for n in self.LENS_X if n <= room]))))
            for r in rng.permutation(m.max_batch):
                r, x = int(r), m.rows[int(r)]
                if r >= m.batch:
                    continue
                if x.state == LIVE and x.has_logits and x.has_token and mode != "no_step" and rng.random() < (0.9 if fin_now else 0.6) and x.length + 1 <= m.max_ctx and left >= 1:
                    nd = int(rng.integers(0, min(MAX_DRAFT, m.max_ctx - x.length - 1, left - 1) + 1))
                    rows.append(r); kinds.append(STEP); ids.append(self.drafts_for(c, r, nd)); left -= nd + 1
                elif mode != "no_feed" and x.length < m.max_ctx and rng.random() < (0.8 if x.state == FINISHED or x.fed_more or x.state == RETIRED else 0.3):
                    k, d = feed(m.max_ctx - x.length)
                    rows.append(r); kinds.append(k); ids.append(d)
            while mode != "no_feed" and nb < m.max_batch and rng.random() < 0.4:      # new rows: exactly batch .. batch + k - 1
                k, d = feed(m.max_ctx)
                rows.append(nb); kinds.append(k); ids.append(d); nb += 1
            if not rows:
                return None
            return self.do_advance_rows(c, rows, kinds, ids)
        if kind == "beam":
            srcs = [r for r in live if m.rows[r].has_logits]
            if len(srcs) < 2:
                return None
            rng.shuffle(srcs)
            srcs = [int(r) for r in srcs[:int(rng.integers(2, min(4, len(srcs)) + 1))]]
            scores = [float(x) for x in -np.round(rng.uniform(0, 6, len(srcs)) * 64) / 64]
            k = int(rng.integers(1, len(srcs) + 3))
            ends = self.ids(int(rng.integers(1, 4))) if rng.random() < 0.3 else []
            sel = self.do_beam_select(c, srcs, scores, min(k, MAX_BEAMS), ends)
            retired = self.rows_where(c, lambda r, x: r < m.batch and x.state == RETIRED)
            spares = [int(r) for r in retired[:int(rng.integers(0, 3))]]
            nb = m.batch
            while len(spares) < 2 and nb < m.max_batch and rng.random() < 0.5:
                spares.append(nb); nb += 1
            rows = srcs + spares
            n_next = int(rng.integers(1, len(rows) + 1))
            parent = [int(p) for p in rng.integers(0, len(srcs), n_next)]
            tailed = [i for i, r in enumerate(srcs) if m.rows[r].length % BLK]
            if m.pool and len(m.pool.free) <= 2 and tailed and rng.random() < 0.9:      # a nearly empty pool: every row of the group a child of one parent, a fresh tail block each
                parent = [int(self.pick(tailed))] * len(rows)
            cand = {}
            if sel:
                for b, t in zip(sel["out"][0], sel["out"][1]):
                    cand.setdefault(int(b), []).append(int(t))
            tokens = [cand[p].pop(0) if cand.get(p) and rng.random() < 0.7 else int(rng.integers(0, m.vocab)) for p in parent]

            def advance():
                if all(m.rows[r].state == LIVE and m.rows[r].has_logits for r in srcs) and not any(m.rows[r].holds for r in spares) and [r for r in spares if r >= m.batch] == list(range(m.batch, m.batch + len([r for r in spares if r >= m.batch]))):
                    if self.do_beam_advance(c, rows, parent, tokens):
                        self.pending.append(lambda: self.ready_and_decode(c, 1))      # next: the step that makes the children differ
            self.pending.append(advance)
            return sel
        return None

    # the classes tests/test_row_model.py asks the seed set for: drawn first while a run has not drawn them (most need a state few operations leave a row in)
    REACH_X = ("splice_gpt2", "splice_empty", "splice_retired", "verify_rows_twice", "verify_rows_notok", "verify_rows_positions", "advance_gap", "advance_step_nolog",
               "advance_neg_len", "beam_parent_is_spare", "beam_finished", "beam_select_twice")

    def draw_illegal_x(self, force=None):
        """one of the later row calls that the header refuses in the current state for exactly one reason (None: no class is open)"""
        c, m, rng = self.c, self.c.m, self.rng
        live = self.rows_where(c, lambda r, x: x.state == LIVE)
        holds = self.rows_where(c, lambda r, x: x.holds and x.length >= 3)
        ready = [r for r in live if m.rows[r].has_logits and m.rows[r].has_token and m.rows[r].length + 2 <= m.max_ctx]
        nolog = [r for r in live if not m.rows[r].has_logits]
        notok = [r for r in live if m.rows[r].has_logits and not m.rows[r].has_token]
        fin = self.rows_where(c, lambda r, x: x.state == FINISHED)
        retired = self.rows_where(c, lambda r, x: r < m.batch and x.state == RETIRED)
        full = [r for r in ready if m.rows[r].length + MAX_DRAFT + 1 > m.max_ctx]
        srcs = [r for r in live if m.rows[r].has_logits]
        gap = m.batch + 1 < m.max_batch
        wide = [r for r in live if m.rows[r].has_logits and m.rows[r].length + MAX_DRAFT + 1 <= m.max_ctx]      # five of them exceed TGX_MAX_VERIFY_POSITIONS
        opts = []
        if m.gpt2:
            opts += ["splice_gpt2"] if holds else []
        else:
            opts += ["splice_empty", "splice_unsorted", "splice_overlap", "splice_beyond", "splice_n_keep"] if holds else []
            opts += ["splice_retired"] if retired or m.batch < m.max_batch else []
            opts += ["splice_row_range"]
        if ready:
            opts += ["verify_rows_twice"] + (["verify_rows_max_ctx"] if full else [])
            opts += ["verify_rows_notok"] if notok else []
            opts += ["verify_rows_nolog"] if nolog else []
            opts += ["verify_rows_finished"] if fin else []
            opts += ["verify_rows_positions", "advance_step_positions"] if len(wide) >= 5 else []
            opts += ["advance_kind", "advance_twice"]
            opts += ["advance_step_nolog"] if nolog else []
            opts += ["advance_step_notok"] if notok else []
        opts += ["advance_gap"] if gap else []
        opts += ["advance_positions", "advance_len0", "advance_neg_len"] if live else []
        if len(srcs) >= 2:
            opts += ["beam_twice", "beam_token", "beam_select_twice"]
            opts += ["beam_parent_is_spare"] if retired or m.batch < m.max_batch else []
            opts += ["beam_finished"] if fin else []
            opts += ["beam_gap"] if gap else []
            opts += ["beam_select_nolog"] if nolog else []
        if not opts:
            return None
        if force is not None:
            opts = [o for o in opts if o == force]
            if not opts:
                return None
        rare = [o for o in opts if o in self.REACH_X and not self.drawn.get(o)]
        if rare and rng.random() < 0.7:                             # classes that need a state few operations leave a row in
            opts = rare
        least = min(self.drawn.get(o, 0) for o in opts)
        what = str(self.pick(sorted({o for o in opts if self.drawn.get(o, 0) == least})))
        self.drawn[what] = self.drawn.get(what, 0) + 1
        if what in ("verify_rows_positions", "advance_step_positions"):
            ready = [int(r) for r in wide[:5]]
            for r in ready:
                if not m.rows[r].has_token:
                    self.do_sample(c, r)
        kind, args = self.illegal_call_x(what, live, holds, ready, nolog, notok, fin, retired, full, srcs)
        if len({code for code, _ in m.reasons(kind, *args)}) != 1:      # only calls the header refuses for one code (a pool already short adds a second)
            return None
        do = dict(splice_row=self.do_splice, verify_rows=self.do_verify_rows, advance_rows=self.do_advance_rows, beam_select=self.do_beam_select, beam_advance=self.do_beam_advance)[kind]
        return do(c, *args, illegal=what)

    def illegal_call_x(self, what, live, holds, ready, nolog, notok, fin, retired, full, srcs):
        c, m, rng = self.c, self.c.m, self.rng
        if what.startswith("splice"):
            r = int(self.pick(holds)) if holds else 0
            L = m.rows[r].length
            if what == "splice_gpt2":
                return "splice_row", (r, [(0, 1), (2, L - 2)])
            if what == "splice_retired":                                           # a retired row of the batch, or the first row beyond it
                return "splice_row", (int(self.pick(retired)) if retired and (m.batch >= m.max_batch or rng.random() < 0.5) else m.batch, [(0, 1)])
            if what == "splice_row_range":
                return "splice_row", (m.max_batch, [(0, 1)])
            ranges = dict(splice_empty=[(0, 1), (2, 0)], splice_unsorted=[(2, 1), (0, 1)], splice_overlap=[(0, 2), (1, 2)], splice_beyond=[(0, 1), (L - 1, 2)],
                          splice_n_keep=[(i, 1) for i in range(0, 2 * MAX_SPLICE_RANGES + 2, 2)])[what]
            return "splice_row", (r, ranges)
        if what.startswith("verify_rows"):
            good = [int(r) for r in ready[:2]]
            if what == "verify_rows_twice":
                return "verify_rows", (good + [good[0]], [self.ids(2) for _ in range(len(good) + 1)])
            if what == "verify_rows_positions":
                rows = [int(r) for r in ready[:5]]
                return "verify_rows", (rows, [self.ids(MAX_DRAFT) for r in rows])
            bad = dict(verify_rows_max_ctx=full, verify_rows_notok=notok, verify_rows_nolog=nolog, verify_rows_finished=fin)[what]
            b = int(self.pick(bad))
            rows = [r for r in good if r != b] + [b]
            return "verify_rows", (rows, [self.ids(1) for _ in rows[:-1]] + [self.ids(MAX_DRAFT if what == "verify_rows_max_ctx" else 1)])
        if what.startswith("advance"):
            good = [int(r) for r in ready[:2]]
            if what == "advance_kind":
                return "advance_rows", (good, [3] + [STEP] * (len(good) - 1), [self.ids(1) for _ in good])
            if what == "advance_twice":
                return "advance_rows", (good + [good[0]], [STEP] * len(good) + [FEED], [[] for _ in good] + [self.ids(2)])
            if what == "advance_step_positions":
                rows = [int(r) for r in ready[:5]]
                return "advance_rows", (rows, [STEP] * 5, [self.ids(MAX_DRAFT) for r in rows])
            if what in ("advance_step_nolog", "advance_step_notok"):
                b = int(self.pick(nolog if what == "advance_step_nolog" else notok))
                return "advance_rows", (good + [b], [STEP] * (len(good) + 1), [[] for _ in good] + [[]])
            if what == "advance_gap":
                return "advance_rows", ([m.batch + 1], [FEED], [self.ids(3)])
            if what == "advance_len0":
                return "advance_rows", ([int(self.pick(live))], [FEED], [[]])
            if what == "advance_neg_len":                                         # behind rows that are legal: nothing may change for them
                rows = good + [int(self.pick([r for r in live if r not in good] or live))]
                rows = rows if len(set(rows)) == len(rows) else rows[-1:]
                return "advance_rows", (rows, [STEP] * (len(rows) - 1) + [FEED], [[] for _ in rows], [0] * (len(rows) - 1) + [-1])
            n = m.max_batch                                                       # more than TGX_MAX_ADVANCE_POSITIONS ids in all: refused ahead of every row's own check
            return "advance_rows", (list(range(n)), [FEED] * n, [[0] * (MAX_ADVANCE_POSITIONS // n + 1) for _ in range(n)])
        two = [int(r) for r in srcs[:2]]
        spare = int(retired[0]) if retired else m.batch
        if what == "beam_select_twice":
            return "beam_select", (two + [two[0]], [0.0, -1.0, -2.0], 2, [])
        if what == "beam_select_nolog":
            return "beam_select", (two + [int(nolog[0])], [0.0, -1.0, -2.0], 2, [])
        if what == "beam_twice":
            return "beam_advance", (two + [two[0]], [0, 1], [1, 2])
        if what == "beam_token":
            return "beam_advance", (two, [0, 1], [1, m.vocab])
        if what == "beam_parent_is_spare":
            return "beam_advance", (two + [spare], [0, 2], [1, 2])
        if what == "beam_finished":
            return "beam_advance", (two + [int(fin[0])], [0, 1], [1, 2])
        return "beam_advance", ([two[0], m.batch + 1], [0, 0], [1, 2])          # beam_gap: the copied child would land in a new row that is not batch

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
                if saved[1].spliced and key == "restore_cross_layout":
                    self.mark("splice_then_restore_cross_layout")
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
            elif self.extended and self.rng.random() < 0.5:        # _x arms: half of the draws are the later row calls, three in ten of those illegal on purpose
                n_log = len(self.log)
                if i >= 1 and not self.drawn.get("beam_finished") and any(x.state == FINISHED for x in c.m.rows) and self.rng.random() < 0.6:
                    self.draw_illegal_x(force="beam_finished"); was_illegal = True      # (a finished row lives for an operation or two)
                elif i >= 1 and self.rng.random() < 0.3:
                    self.draw_illegal_x(); was_illegal = True
                else:
                    kinds = list(self.WEIGHTS_X); w = np.array([self.WEIGHTS_X[k] for k in kinds])
                    if self.stats.greedy < 2 * len(self.log):      # few tokens so far: towards the calls that produce them
                        w[kinds.index("verify_rows")] *= 3; w[kinds.index("advance_rows")] *= 2
                    if any(x.state == FINISHED for x in c.m.rows):  # a finished row lives for an operation or two: an admission over it next to a STEP of another row,
                        w[kinds.index("advance_rows")] *= 4; w[kinds.index("splice_row")] *= 3      # or a splice that clears its state
                    if c.m.pool and not c.m.pool.free and any(c.m.pool.shared(b) for x in c.m.rows for b in x.blocks):
                        w[kinds.index("splice_row")] *= 4           # an empty free list next to shared blocks: the copy on write that cannot be had
                    if c.m.pool and len(c.m.pool.free) <= 2:
                        w[kinds.index("beam")] *= 3                 # ... and the fresh tail blocks of a beam group's copies
                    self.draw_legal_x(kinds[int(self.rng.choice(len(kinds), p=w / w.sum()))]); was_illegal = False
                if len(self.log) == n_log:                          # the state offered that call nothing: one of the 16 instead
                    self.draw_legal(); was_illegal = False
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


def run_sequence(device, model, rng, n_ops, *, fam, dtype, bound, gap=4e-3, lp_tol=2e-5, aux=None, tag="", extended=False):
    """n_ops random operations on `device`, each predicted by `model` and checked; aux = (device, model) of the second context snapshots travel through"""
    main = Ctx(device, model, Mirror(fam, dtype, model.max_batch), "main")
    second = Ctx(aux[0], aux[1], Mirror(fam, dtype, aux[1].max_batch), "aux") if aux else None
    return Driver(main, second, rng, bound, gap, lp_tol, tag, extended).run(n_ops)
