#!/usr/bin/env python3
"""The corpus join against the way to the same answer without it -- the loop of query_packed_threshold_keys_device in groups
of eight over the packed rows that filled the corpus -- alternating in one process after warm-up:
    python3 tools/prof_join.py [reps] [--out DIR] [--trace] [--only self20k|self100k|self1m|cross|dense]
Legs (5 x 200 Booleans per entry, synthetic corpus with 300 planted near-copies of about 20 flipped Booleans):
    self20k, self100k, self1m   self-join at t = 0.7
    cross                       10 k rows of a second corpus against 1 M entries at t = 0.7
    dense                       self-join of 20 k at the median of the scores (about half of all pairs match)
The loop's capacity per row is min(the join's capacity, entries): a row has no more matches than the corpus has entries.
Where the whole loop would take longer than a few seconds (self1m, cross) it runs over the first `loop_groups` groups of eight
rows only and its time is scaled to all rows; the record says so ("loop_sampled").  Device time: hipEvents around the calls on
the current stream; medians and quartiles of `reps` (default 7) rounds in ms, one JSON line per leg, also appended to
DIR/join_prof.jsonl (default DIR: profiles).

--trace: two joins of the self20k, self100k and dense legs only, for a kernel trace in a run of its own (the scatter kernel's
share of the time is read from its statistics).  Every GPU step under its own time limit:
    timeout -k 10 900 python3 tools/prof_join.py 7 && \\
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d /tmp/join_trace -o join_trace --output-format csv -- \\
        python3 tools/prof_join.py --trace && \\
    cp /tmp/join_trace/*/join_trace_kernel_stats.csv profiles/"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lbaudiodetective_amd as lb  # noqa: E402
from oracle import oracle as O  # noqa: E402

SEED = 0x4C424145
PLANTS = 300
GROUP = 8


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


TRACE = "--trace" in sys.argv
OUT = _option("--out", os.path.join(ROOT, "profiles"))
ONLY = _option("--only")
_skip = {OUT, ONLY}
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in _skip]
REPS = 2 if TRACE else (int(args[0]) if args else 7)


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    return {"median": round(q[1], 4), "p25": round(q[0], 4), "p75": round(q[2], 4)}


def report(res):
    print(json.dumps(res), flush=True)
    if not TRACE:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "join_prof.jsonl"), "a") as f:
            f.write(json.dumps(res) + "\n")


def synth(seed, n):
    """packed rows [n, 5, 32] on the device with PLANTS near-copies: entry dst = entry src with about 20 Booleans flipped"""
    packed = lb.synth_corpus_device(seed, 0, n, 5, 200)
    g = torch.Generator().manual_seed(seed)
    at = torch.randperm(n, generator=g)[:2 * PLANTS]
    src, dst = at[:PLANTS].cuda(), at[PLANTS:].cuda()
    packed[dst] = packed[src]
    for _ in range(20):
        sub = torch.randint(0, 5, (PLANTS,), generator=g).cuda()
        bit = torch.randint(0, 200, (PLANTS,), generator=g).cuda()
        packed[dst, sub, bit // 8] ^= torch.bitwise_left_shift(torch.ones_like(bit), bit % 8).to(torch.uint8)
    return packed


def corpus_of(packed):
    c = lb.Corpus(200, 5, packed.shape[0])
    c.append_packed_device(packed)
    torch.cuda.synchronize()
    return c


def leg(name, corpus, rows_packed, queries, t, loop_groups=None):
    """the join of all rows of `queries` (None: a self-join) against `corpus`, and the loop over rows_packed"""
    n, rows = len(corpus), rows_packed.shape[0]
    # the total first (a call with one slot), then room for all of it
    _, off = corpus.join_threshold_keys_device(t, 1, queries=queries, skip_same_index=False)
    total = int(off[-1])
    capacity = total + 1024
    keys = torch.zeros(capacity, dtype=torch.int64, device="cuda")
    offsets = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    row_cap = min(capacity, n)
    lk = torch.zeros((GROUP, row_cap), dtype=torch.int64, device="cuda")
    lc = torch.zeros(GROUP, dtype=torch.int64, device="cuda")
    groups = (rows + GROUP - 1) // GROUP
    run_groups = groups if loop_groups is None or TRACE else min(groups, loop_groups)
    loop_total = torch.zeros((), dtype=torch.int64, device="cuda")

    def join():
        corpus.join_threshold_keys_device(t, capacity, queries=queries, skip_same_index=False, keys_out=keys, offsets_out=offsets)

    def loop():
        loop_total.zero_()
        for g in range(run_groups):
            r0 = g * GROUP
            q = min(GROUP, rows - r0)
            corpus.query_packed_threshold_keys_device(rows_packed[r0:r0 + q], q, 5, t, row_cap, keys_out=lk, counts_out=lc)
            loop_total.add_(lc[:q].sum())

    calls = {"join": join} if TRACE else {"join": join, "loop": loop}
    for f in calls.values():
        f()
        torch.cuda.synchronize()
    assert int(offsets[-1]) == total
    if not TRACE:
        assert int(loop_total) == int(offsets[run_groups * GROUP if run_groups < groups else rows]), "the loop and the join disagree"
    times = {k: [] for k in calls}
    reps = REPS if n * rows < 2e10 else max(2, REPS // 3)     # (a join of 10^12 pairs takes seconds)
    for _ in range(reps):
        for k, f in calls.items():
            times[k].append(device_ms(f))
    res = {"leg": name, "reps": reps, "entries": n, "rows": rows, "threshold": t, "matches": total, "capacity": capacity}
    res["join"] = _stats(times["join"])
    res["join_ns_per_pair"] = round(res["join"]["median"] * 1e6 / (n * rows), 5)
    if not TRACE:
        scale = groups / run_groups
        res["loop"] = {k: round(v * scale, 4) for k, v in _stats(times["loop"]).items()}
        res["loop_sampled"] = run_groups < groups
        res["loop_groups_run"] = run_groups
        res["loop_over_join"] = round(res["loop"]["median"] / res["join"]["median"], 3)
    report(res)


def median_score(n):
    """the median score of a few entries of the synthetic corpus against it: the dense leg's threshold"""
    c = corpus_of(lb.synth_corpus_device(SEED, 0, n, 5, 200))
    s = torch.cat([c.scores_device(lb.Fingerprint.from_bools(O.synth_entry(SEED, e, 5, 200))) for e in (3, 1000, n // 2, n - 7)])
    m = float(s.median())
    c.dispose()
    return m


def want(name):
    return (ONLY is None and (not TRACE or name in ("self20k", "self100k", "dense"))) or ONLY == name


def self_leg(name, n, groups):
    if want(name):
        packed = synth(SEED, n)
        c = corpus_of(packed)
        leg(f"self-join {n} x 5, t = 0.7", c, packed, None, 0.7, groups)
        c.dispose()
        del packed, c
        torch.cuda.empty_cache()


torch.cuda.set_device(0)
self_leg("self20k", 20_000, None)
self_leg("self100k", 100_000, None)

if want("cross"):
    packed = synth(SEED, 1_000_000)
    c = corpus_of(packed)
    rows = synth(SEED + 1, 10_000)
    rows[:PLANTS] = packed[5000:5000 + PLANTS]             # rows that exist in the corpus: the ingest check finds them
    q = corpus_of(rows)
    leg("cross-join 10 k rows x 1 M entries, t = 0.7", c, rows, q, 0.7, 250)
    c.dispose()
    q.dispose()
    del packed, rows, c, q
    torch.cuda.empty_cache()

if want("dense"):
    n = 20_000
    t = median_score(n)
    packed = synth(SEED, n)
    c = corpus_of(packed)
    leg(f"self-join {n} x 5, dense: t = the scores' median", c, packed, None, t, 250)
    c.dispose()
    del packed, c
    torch.cuda.empty_cache()

self_leg("self1m", 1_000_000, 2_000)                     # last: the one leg that takes seconds per join
