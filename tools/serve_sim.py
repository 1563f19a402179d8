#!/usr/bin/env python3
"""serve_sim.py — the kernel contract of continuous batching (per-row lifecycle; paged KV, option kv.budget_tokens) driven the way a
serving loop would drive it, on the real kernels: a seeded stream of requests (prompt and output lengths uniform in given ranges) served on ONE context by

  continuous   every tick: retire the rows that reached their length (tgx_reset_row), admit waiting requests into idle rows while the token budget has room
               (tgx_forward_row + tgx_sample_row; with --joint all of the tick's admissions in ONE tgx_forward_rows call), then ONE tgx_decode call of n <= 16
               steps for all rows (n = the shortest remaining output)
  static       the reference worker's shape taken to a batch: B requests in, decode until the LONGEST is done (finished rows are retired, their slots stay empty),
               then the next B

With --mix every request draws its own sampler settings (greedy, T 0.8 / top-p 0.9, T 1.0 / top-k 50, T 0.7 / min-p 0.05) and seed, and the ticks run
tgx_decode_rows (per-row settings, include/tgx.h); with --device-stop as well, each request's output length is its max_new (tgx_set_row_stop) and every tick
is a full 16-step tgx_decode_rows call — the rows finish on the device, the host reads their counts back instead of limiting the call to the shortest output.  With --speculate N on top of the two, every tick is ONE
tgx_verify_rows call instead (per 64 positions): each live row with a prompt-lookup draft of up to N tokens from its own history, or with none.

With --chunk N (on --mix --device-stop) a waiting request is admitted in pieces of <= N prompt tokens, one piece per tick (chunked prefill, include/tgx.h
tgx_advance_rows): ONE call carries the tick's pieces (FEED_MORE, the last one FEED; at most --chunk-tick prompt tokens per tick, default N, in admission order) and
one step of every live row, so no live row waits for a whole prompt; ticks without a pending prompt stay full 16-step tgx_decode_rows calls.

Every mode also prints the median and the longest wall time between two consecutive tokens of a live row: a call that starts at t0, ends at t1 and gives a row k
tokens counts k gaps — the first from the row's previous token (the end of the call that produced it) to t0 + (t1 - t0) / k, the others (t1 - t0) / k each — so
the time the batch stood still for an admission shows up in the first gap.  --lib runs the tool on another build of the library (a baseline).

With --n-best K every request wants K samples of its prompt (T 0.8 / top-p 0.9, seeds s .. s + K - 1, all of the request's output length): the request is admitted into
K idle rows as ONE tgx_forward_row plus ONE tgx_fork_row (include/tgx.h; on a paged cache the prompt's full blocks are held once) — or, with --n-best-separate, as K
prompts in one tgx_forward_rows call — and the ticks run tgx_decode_rows.  The mode reports tokens per second and the peak of budget - kv.free_tokens.

The tool reports generated tokens per second, the mean number of live rows per step and what the cache held.  The reference has neither (its server runs one request at
a time, HttpServer.cpp:118-163; continuous batching and paged attention are README.md:32-34 TODOs): this is the measurement of the kernel half only — no queue, no
HTTP, synthetic weights; greedy unless --sampler.

    python tools/serve_sim.py [--model llama-3.2-1b] [--rows 32] [--requests 200] [--prompt 16,512] [--new 16,256] [--kv-budget 16384] [--policy continuous|static|both]
"""
import argparse, dataclasses, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tinygpt_amd import known_desc, synth
from tinygpt_amd.ffi import GREEDY, Model, product_backend

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama-3.2-1b")
ap.add_argument("--rows", type=int, default=32)
ap.add_argument("--requests", type=int, default=200)
ap.add_argument("--prompt", default="16,512")
ap.add_argument("--new", default="16,256")
ap.add_argument("--max-ctx", type=int, default=1024)
ap.add_argument("--kv-budget", type=int, default=0, help="paged KV: tokens of cache for all rows together (0 = one max_ctx slab per row)")
ap.add_argument("--policy", default="both", choices=["continuous", "static", "both"])
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--sampler", default="", help="e.g. 'temperature=0.8,top_p=0.9' (default: greedy)")
ap.add_argument("--mix", action="store_true", help="per-request sampler settings and seeds through tgx_decode_rows")
ap.add_argument("--device-stop", action="store_true", help="(with --mix) output lengths as max_new on the device, full 16-step calls")
ap.add_argument("--speculate", type=int, default=0, help="(with --mix --device-stop) prompt-lookup drafts of up to N tokens per row, one tgx_verify_rows call per tick in place of tgx_decode_rows")
ap.add_argument("--chunk", type=int, default=0, help="(with --mix --device-stop) admit prompts in pieces of <= N tokens through tgx_advance_rows, one piece per tick beside one step of every live row")
ap.add_argument("--chunk-tick", type=int, default=0, help="(with --chunk) prompt tokens per tick over all pending prompts (default: N)")
ap.add_argument("--lib", default="", help="the library to run on (default: this build's)")
ap.add_argument("--joint", action="store_true", help="admit every request that fits in a tick with ONE tgx_forward_rows call, then tgx_sample_row per row")
ap.add_argument("--n-best", type=int, default=0, help="K samples per request: one prefill + tgx_fork_row into K - 1 rows (paged KV: --kv-budget)")
ap.add_argument("--n-best-separate", action="store_true", help="(with --n-best) admit the K samples as K copies of the prompt in one tgx_forward_rows call instead")
args = ap.parse_args()
B = args.rows
CFG = GREEDY
if args.sampler:
    from tinygpt_amd.ffi import SamplerCfg
    CFG = SamplerCfg(**{k: (int(v) if k == "top_k" else float(v)) for k, v in (item.split("=") for item in args.sampler.split(","))})
plo, phi = (int(x) for x in args.prompt.split(","))
nlo, nhi = (int(x) for x in args.new.split(","))
assert phi + nhi <= args.max_ctx
desc = dataclasses.replace(known_desc(args.model), max_batch=B, max_ctx=args.max_ctx)
if args.lib:      # another build: bind what it exports
    import ctypes
    from tinygpt_amd.ffi import ABI, Backend
    probe = ctypes.CDLL(args.lib)
    backend = Backend(args.lib, "tgx_", required=[n for n in ABI if hasattr(probe, "tgx_" + n)])
else:
    backend = product_backend()
m = Model(desc, backend)
if args.kv_budget:
    m.set_option("kv.budget_tokens", args.kv_budget)
m.load_synthetic(1234, 0.02).finalize()
budget = args.kv_budget if args.kv_budget else B * args.max_ctx
blocks = (lambda n: (n + 127) // 128 * 128) if args.kv_budget else (lambda n: args.max_ctx)
rng = np.random.default_rng(args.seed)
reqs = [(int(rng.integers(plo, phi + 1)), int(rng.integers(nlo, nhi + 1))) for _ in range(args.requests)]
prompts = [synth.synth_prompt(desc.vocab, L, 1000 + i) for i, (L, _) in enumerate(reqs)]
if args.mix:
    from tinygpt_amd.ffi import SamplerCfg
    MIX = [GREEDY, SamplerCfg(0.8, 0, 0.9, 0.0), SamplerCfg(1.0, 50, 1.0, 0.0), SamplerCfg(0.7, 0, 1.0, 0.05)]
    req_cfg = [(MIX[int(rng.integers(0, len(MIX)))], int(rng.integers(1, 1 << 30))) for _ in reqs]
STOP = args.mix and args.device_stop
CHUNK = args.chunk if STOP else 0
if args.chunk and not STOP:
    raise SystemExit("--chunk needs --mix --device-stop")
SLACK = 16 if STOP else 0        # device stop: blocks are assigned up front for the whole 16-step call


def born():
    """a batch of B idle rows (tgx_forward creates the rows, tgx_reset_row retires each)"""
    m.reset_cache()
    m.forward(np.zeros((B, 1), dtype=np.int64)); m.sample(GREEDY)
    for r in range(B):
        m.reset_row(r)


def lookup(seq, cap):
    """prompt lookup: the tokens that followed the latest earlier occurrence of the sequence's last 3 / 2 / 1 tokens, at most cap of them"""
    for k in (3, 2, 1):
        if len(seq) <= k or cap < 1:
            continue
        tail = seq[-k:]
        for s0 in range(len(seq) - k - 1, -1, -1):
            if seq[s0:s0 + k] == tail:
                return seq[s0 + k:s0 + k + cap]
    return []


def serve(policy):
    born()
    waiting = list(range(len(reqs)))
    length, target = [0] * B, [0] * B
    produced = steps = live_steps = calls = 0
    peak_tokens = 0
    hist = [[] for _ in range(B)]      # --speculate: every row's tokens so far (prompt + produced), the drafter's input
    feeding = {}                       # --chunk: row -> [request, prompt tokens fed so far], in admission order
    last_tok, gaps = [0.0] * B, []     # the wall time of every live row's latest token; the gaps between consecutive tokens of a row (module docstring)

    def note(r, k, t_start, t_end):
        if k > 0:
            per = (t_end - t_start) / k
            gaps.append(t_start + per - last_tok[r]); gaps.extend([per] * (k - 1))
            last_tok[r] = t_end
    drafted = [0, 0]                   # draft tokens offered / accepted
    m.synchronize(); t0 = time.perf_counter()
    while waiting or any(length) or feeding:
        idle = [r for r in range(B) if not length[r] and r not in feeding]
        if policy == "continuous" or len(idle) == B:          # static: a new batch only when the whole previous one is done
            reserved = sum(blocks(t) for t in target if t)
            admit = []
            for r in idle:
                if not waiting:
                    break
                i = waiting[0]
                L, new = reqs[i]
                if reserved + blocks(L + new + SLACK) > budget:
                    break                                    # the head of the queue waits for room (FIFO)
                waiting.pop(0)
                if CHUNK:                                    # the prompt goes in piece by piece with the ticks below
                    feeding[r] = [i, 0]
                    target[r] = L + new + SLACK
                    reserved += blocks(L + new + SLACK)
                    continue
                if args.joint:                               # every admission of the tick in ONE tgx_forward_rows call below
                    admit.append((r, i))
                elif args.mix:
                    cfg, seed = req_cfg[i]
                    m.forward_row(r, prompts[i]); t = m.sample_row(r, cfg, seed=seed); m.set_row_sampler(r, cfg, seed)
                    hist[r] = [int(x) for x in prompts[i]] + [int(t)]
                    if STOP:
                        m.set_row_stop(r, max_new=new)
                else:
                    m.forward_row(r, prompts[i]); m.sample_row(r, CFG, seed=3)
                last_tok[r] = time.perf_counter()
                length[r], target[r] = L, L + new + SLACK
                reserved += blocks(L + new + SLACK)
                produced += 1                                 # the first token came from the prefill's logits
            if admit:
                m.forward_rows([r for r, _ in admit], [prompts[i] for _, i in admit])
                for r, i in admit:
                    if args.mix:
                        cfg, seed = req_cfg[i]
                        t = m.sample_row(r, cfg, seed=seed); m.set_row_sampler(r, cfg, seed)
                        hist[r] = [int(x) for x in prompts[i]] + [int(t)]
                        if STOP:
                            m.set_row_stop(r, max_new=reqs[i][1])
                    else:
                        m.sample_row(r, CFG, seed=3)
                    last_tok[r] = time.perf_counter()
        live = [r for r in range(B) if length[r]]
        if not live and not feeding:
            raise SystemExit("the budget admits no request")
        if feeding:                                            # one tgx_advance_rows: the tick's pieces and one step of every live row
            from tinygpt_amd.ffi import ADV_FEED, ADV_FEED_MORE, ADV_STEP
            assert len(live) <= 64, "one call steps at most 64 rows"
            rows_, kinds, ids_, room = list(live), [ADV_STEP] * len(live), [[] for _ in live], args.chunk_tick or CHUNK
            done = []
            for r, (i, off) in feeding.items():
                n_piece = min(CHUNK, len(prompts[i]) - off, room)
                if n_piece < 1:
                    break
                last = off + n_piece == len(prompts[i])
                rows_.append(r); kinds.append(ADV_FEED if last else ADV_FEED_MORE); ids_.append(prompts[i][off:off + n_piece])
                feeding[r][1] += n_piece; room -= n_piece
                if last:
                    done.append(r)
            ts = time.perf_counter()
            res = m.advance_rows(rows_, kinds, ids_)
            te = time.perf_counter()
            calls += 1; steps += 1
            for r, (ids, fin) in zip(live, res):
                length[r] += len(ids); produced += len(ids); live_steps += len(ids)
                note(r, len(ids), ts, te)
                if fin:
                    m.reset_row(r); length[r] = target[r] = 0
            for r in done:                                     # the prompt is in: the row's first token, its settings, its stop condition
                i = feeding.pop(r)[0]
                cfg, seed = req_cfg[i]
                m.sample_row(r, cfg, seed=seed); m.set_row_sampler(r, cfg, seed); m.set_row_stop(r, max_new=reqs[i][1])
                length[r] = reqs[i][0]; produced += 1
                last_tok[r] = time.perf_counter()
            peak_tokens = max(peak_tokens, sum(length))
            continue
        if STOP and args.speculate > 0:                        # one tgx_verify_rows per tick (per 64 positions): every live row with its prompt-lookup draft, or none
            group, pos = [], 0
            todo = []
            for r in live:
                d = lookup(hist[r], min(args.speculate, 15, args.max_ctx - length[r] - 1))
                if pos + len(d) + 1 > 64:
                    todo.append(group); group, pos = [], 0
                group.append((r, d)); pos += len(d) + 1
            todo.append(group)
            for group in todo:
                ts = time.perf_counter()
                res = m.verify_rows([r for r, _ in group], [d for _, d in group])
                te = time.perf_counter()
                calls += 1; steps += 1
                for (r, d), (ids, fin) in zip(group, res):
                    note(r, len(ids), ts, te)
                    hist[r].extend(int(t) for t in ids)
                    length[r] += len(ids); produced += len(ids); live_steps += len(ids)
                    peak_tokens = max(peak_tokens, sum(length))
                    drafted[0] += len(d); drafted[1] += len(ids) - 1 if d else 0
                    if fin:
                        m.reset_row(r); length[r] = target[r] = 0
            continue
        if STOP:                                               # full calls; the rows finish on the device
            n = 16
            ts = time.perf_counter()
            _, cnt, fin = m.decode_rows(n)
            te = time.perf_counter()
            calls += 1; steps += n
            for r in live:
                note(r, int(cnt[r]), ts, te)
                length[r] += int(cnt[r]); produced += int(cnt[r]); live_steps += int(cnt[r])
            peak_tokens = max(peak_tokens, sum(length))
            for r in live:
                if fin[r]:
                    m.reset_row(r); length[r] = target[r] = 0
            continue
        remaining = [target[r] - length[r] for r in live]
        n = min(16, min(remaining))
        ts = time.perf_counter()
        if args.mix:
            m.decode_rows(n)
        else:
            m.decode(n, CFG, seed=3, fetch=False)             # (not synchronised: this mode's gaps are those of the host's enqueue times)
        te = time.perf_counter()
        calls += 1; steps += n
        for r in live:
            note(r, n, ts, te)
            length[r] += n; produced += n; live_steps += n
        peak_tokens = max(peak_tokens, sum(length))
        for r in live:                                         # a finished row is retired at once under both policies (static: its slot stays empty until the batch is done)
            if length[r] >= target[r]:
                m.reset_row(r); length[r] = target[r] = 0
    m.synchronize(); dt = time.perf_counter() - t0
    print(f"{policy:10s} {len(reqs)} requests, {produced} tokens generated in {dt:.2f} s = {produced / dt:8.0f} tokens/s; {steps} steps in {calls} decode calls, "
          f"{live_steps / max(steps, 1):.1f} live rows per step of {B}; most tokens held at once {peak_tokens} (cache: {budget} tokens"
          f"{', paged' if args.kv_budget else ' as slabs'})", flush=True)
    if gaps:
        print(f"           between two consecutive tokens of a live row: median {np.median(gaps) * 1e3:.2f} ms, longest {max(gaps) * 1e3:.2f} ms ({len(gaps)} gaps)", flush=True)
    if STOP and args.speculate > 0:
        print(f"           --speculate {args.speculate}: {drafted[1]} of {drafted[0]} draft tokens accepted, one tgx_verify_rows call per tick and 64 positions", flush=True)


def serve_nbest(K, fork):
    """continuous policy over groups of K rows: a request takes K idle rows when the budget has room for its whole life (fork: the prompt's full blocks once)"""
    from tinygpt_amd.ffi import SamplerCfg
    warm = SamplerCfg(0.8, 0, 0.9, 0.0)
    born()
    nb = lambda n: (n + 127) // 128
    waiting = list(range(len(reqs)))
    groups = []                                   # [rows, length, target, reserved tokens, summed log-probability per sample]
    spreads = []                                  # per finished request: best - worst summed log-probability of its K samples
    idle = list(range(B))
    produced = steps = calls = peak_held = 0
    m.synchronize(); t0 = time.perf_counter()
    while waiting or groups:
        reserved = sum(g[3] for g in groups)
        while waiting and len(idle) >= K:
            i = waiting[0]
            L, new = reqs[i]
            if args.kv_budget:
                cost = (nb(L + new) * K if not fork else L // 128 + K * (nb(L + new) - L // 128)) * 128
            else:
                cost = K * args.max_ctx
            if reserved + cost > budget:
                break
            waiting.pop(0)
            rows, idle = idle[:K], idle[K:]
            if fork:
                m.forward_row(rows[0], prompts[i])
                if K > 1:
                    m.fork_row(rows[0], rows[1:])
            else:
                m.forward_rows(rows, [prompts[i]] * K)
            for k, r in enumerate(rows):
                seed = 1000 * i + k
                m.set_row_logprobs(r, 0)          # the samples are ranked by their summed log-probability (tgx_set_row_logprobs; tgx_reset_row switched it off)
                m.sample_row(r, warm, seed=seed); m.set_row_sampler(r, warm, seed)
            groups.append([rows, L, L + new, cost, [float(m.row_logprobs(r, 1)[0][0]) for r in rows]])
            reserved += cost
            produced += K
        if not groups:
            raise SystemExit("the budget admits no request")
        n = min(16, min(g[2] - g[1] for g in groups))
        m.decode_rows(n)
        calls += 1; steps += n
        if args.kv_budget:
            peak_held = max(peak_held, budget - m.get_option("kv.free_tokens"))
        for g in groups:
            g[1] += n; produced += n * K
            for k, r in enumerate(g[0]):          # drained every call: the ring holds 256 records, a call produces at most 16
                g[4][k] += float(m.row_logprobs(r, n)[0].sum())
        for g in [g for g in groups if g[1] >= g[2]]:
            spreads.append(max(g[4]) - min(g[4]))
            for r in g[0]:
                m.reset_row(r)
            idle += g[0]
            groups.remove(g)
    m.synchronize(); dt = time.perf_counter() - t0
    held = f"peak of budget - kv.free_tokens {peak_held} tokens = {peak_held // 128} blocks of {budget // 128}" if args.kv_budget else "unpaged"
    print(f"n-best {K} {'prefill + fork' if fork else 'K separate prompts'}: {len(reqs)} requests, {produced} tokens generated in {dt:.2f} s = {produced / dt:8.0f} tokens/s; "
          f"{steps} steps in {calls} decode calls; {held}; samples ranked by summed log-probability, best - worst of a request: mean {sum(spreads) / max(len(spreads), 1):.2f} nats", flush=True)


print(f"{desc.name}: {B} rows, max_ctx {args.max_ctx}, prompts {plo}..{phi}, outputs {nlo}..{nhi} tokens, "
      f"{'kv.budget_tokens ' + str(args.kv_budget) if args.kv_budget else 'unpaged'}{', mixed settings' if args.mix else ''}{', device stop' if STOP else ''}{', joint admission' if args.joint else ''}{', chunked prefill of ' + str(CHUNK) if CHUNK else ''}", flush=True)
if args.n_best:
    if args.mix or args.joint or args.device_stop or args.sampler or args.policy != "both":
        raise SystemExit("--n-best is a mode of its own (continuous policy, T 0.8 / top-p 0.9 per sample): it takes no --mix / --joint / --device-stop / --sampler / --policy")
    serve_nbest(args.n_best, not args.n_best_separate)
    sys.exit(0)
for pol in (["continuous", "static"] if args.policy == "both" else [args.policy]):
    serve(pol)
