#!/usr/bin/env python3
"""The ragged corpus join against the way to the same answer without it -- a host loop over the distinct entry lengths of the
rows: gather the rows of one length, then query_packed_threshold_keys_device in groups of eight -- alternating in one process
after warm-up:
    python3 tools/prof_join_ragged.py [reps] [--out DIR] [--only self20k|self100k|cross]
Legs (200 Booleans per sub-fingerprint, lengths synth_ragged_counts(seed, 0, n, 20, 70), 300 planted near-copies of about 20
flipped Booleans among entries of equal length, t = 0.7):
    self20k, self100k   self-join
    cross               2 000 rows of a second corpus against 200 000 entries
The loop's keys of the rows (one list per length) are made before the clock starts; its gathers, scans and selections are
timed.  Its per-row totals are asserted equal to the join's offsets.  Where the whole loop would take many seconds (self100k)
it runs the first `loop_groups` groups of eight of every length only and its time is scaled to all groups; the record says so
("loop_sampled").  Device time: hipEvents around the calls on the current stream; medians and quartiles of `reps` (default 7,
at least 5 on the legs with a bar) rounds in ms, one JSON line per leg, also appended to DIR/join_ragged_prof.jsonl (default
DIR: profiles).  The bar of self20k and cross: the join's median is not above the loop's by more than the larger of the two
interquartile ranges ("bar_met"); the exit status is 1 when a leg misses it.
    timeout -k 10 900 python3 tools/prof_join_ragged.py 7"""
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
L = 200
T = 0.7


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
ONLY = _option("--only")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in {OUT, ONLY}]
REPS = int(args[0]) if args else 7


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
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "join_ragged_prof.jsonl"), "a") as f:
        f.write(json.dumps(res) + "\n")


def synth(seed, n):
    """(packed records [sum counts, 32] on the device, counts) with PLANTS near-copies: entry dst = an entry src of the same
    length with about 20 Booleans flipped"""
    counts = O.synth_ragged_counts(seed, 0, n, 20, 70)
    packed = lb.synth_ragged_corpus_device(seed, 0, counts, L)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    by_len = {}
    for e in order:
        by_len.setdefault(int(counts[e]), []).append(int(e))
    pairs = []
    while len(pairs) < PLANTS:
        for ids in by_len.values():
            if len(ids) >= 2 and len(pairs) < PLANTS:
                pairs.append((ids.pop(), ids.pop()))
    for src, dst in pairs:
        m = int(counts[src])
        packed[off[dst]:off[dst] + m] = packed[off[src]:off[src] + m]
        sub = torch.from_numpy(rng.integers(0, m, 20)).cuda() + int(off[dst])
        bit = torch.from_numpy(rng.integers(0, L, 20)).cuda()
        packed[sub, bit // 8] ^= torch.bitwise_left_shift(torch.ones_like(bit), bit % 8).to(torch.uint8)
    return packed, counts


def corpus_of(packed, counts):
    c = lb.Corpus.ragged(L, len(counts), int(counts.sum()))
    c.append_ragged_packed_device(packed, counts)
    torch.cuda.synchronize()
    return c


def _key(index):
    return (0x3F800000 << 32) | (0xFFFFFFFF - index)


def leg(name, corpus, rows_corpus, row_counts, barred, loop_groups=None):
    """the join of all entries of rows_corpus (None: a self-join) against `corpus`, and the per-length loop"""
    source = corpus if rows_corpus is None else rows_corpus
    n, rows = len(corpus), len(row_counts)
    _, _, off = corpus.join_ragged_threshold_keys_device(T, 1, queries=rows_corpus, skip_same_index=False, want_lags=False)
    total = int(off[-1])
    capacity = total + 1024
    keys = torch.zeros(capacity, dtype=torch.int64, device="cuda")
    lags = torch.zeros(capacity, dtype=torch.int32, device="cuda")
    offsets = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    row_cap = min(capacity, n)
    lk = torch.zeros((GROUP, row_cap), dtype=torch.int64, device="cuda")
    # the loop's plan, made before the clock starts: per length the rows (all, or the first loop_groups groups of eight)
    plan, groups, run_groups = [], 0, 0
    for m in sorted(set(int(x) for x in row_counts)):
        ids = np.nonzero(row_counts == m)[0]
        g = (len(ids) + GROUP - 1) // GROUP
        run = g if loop_groups is None else min(g, loop_groups)
        ids = ids[:run * GROUP]
        groups, run_groups = groups + g, run_groups + run
        plan.append((m, torch.from_numpy(ids).cuda(), torch.from_numpy(np.array([_key(int(e)) for e in ids], np.uint64).view(np.int64)).cuda(),
                     torch.empty((len(ids) * m, 32), dtype=torch.uint8, device="cuda"), torch.empty(len(ids) + 1, dtype=torch.int64, device="cuda")))

    def join():
        corpus.join_ragged_threshold_keys_device(T, capacity, queries=rows_corpus, skip_same_index=False, keys_out=keys, lags_out=lags,
                                                 offsets_out=offsets)

    # every group's counts go to a slot of their own: nothing but the route itself runs under the clock
    lc = torch.zeros((run_groups, GROUP), dtype=torch.int64, device="cuda")

    def loop():
        g = 0
        for m, ids, row_keys, packed, goff in plan:
            source.gather_keys_device(row_keys, packed_out=packed, offsets_out=goff, capacity=packed.shape[0])
            for r0 in range(0, len(ids), GROUP):
                q = min(GROUP, len(ids) - r0)
                corpus.query_packed_threshold_keys_device(packed[r0 * m:(r0 + q) * m], q, m, T, row_cap, keys_out=lk, counts_out=lc[g])
                g += 1

    calls = {"join": join, "loop": loop}
    for f in calls.values():
        f()
        torch.cuda.synchronize()
    assert int(offsets[-1]) == total
    per_row = offsets[1:] - offsets[:-1]
    g = 0
    for m, ids, _, _, _ in plan:                     # (after the clock: the loop's per-row totals are the join's)
        for r0 in range(0, len(ids), GROUP):
            q = min(GROUP, len(ids) - r0)
            assert torch.equal(lc[g, :q], per_row[ids[r0:r0 + q]]), "the loop and the join disagree"
            g += 1
    reps = max(5, REPS) if barred else max(3, REPS // 2)
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            times[k].append(device_ms(f))
    torch.cuda.synchronize()
    scale = groups / run_groups
    res = {"leg": name, "reps": reps, "entries": n, "rows": rows, "records": int(corpus.subfingerprint_total), "threshold": T,
           "matches": total, "capacity": capacity, "join": _stats(times["join"]),
           "loop": {k: round(v * scale, 4) for k, v in _stats(times["loop"]).items()}, "loop_sampled": run_groups < groups,
           "loop_groups": groups, "loop_groups_run": run_groups}
    res["loop_over_join"] = round(res["loop"]["median"] / res["join"]["median"], 3)
    if barred:
        iqr = max(res["join"]["p75"] - res["join"]["p25"], res["loop"]["p75"] - res["loop"]["p25"])
        res["bar_met"] = res["join"]["median"] <= res["loop"]["median"] + iqr
    report(res)
    return res.get("bar_met", True)


def want(name):
    return ONLY is None or ONLY == name


def self_leg(name, n, barred, groups):
    if not want(name):
        return True
    packed, counts = synth(SEED, n)
    c = corpus_of(packed, counts)
    ok = leg(f"ragged self-join {n} entries of 20 .. 70, t = {T}", c, None, counts, barred, groups)
    c.dispose()
    del packed, c
    torch.cuda.empty_cache()
    return ok


torch.cuda.set_device(0)
met = self_leg("self20k", 20_000, True, None)
if want("cross"):
    packed, counts = synth(SEED, 200_000)
    c = corpus_of(packed, counts)
    rows, row_counts = synth(SEED + 1, 2_000)
    q = corpus_of(rows, row_counts)
    met = leg(f"ragged cross-join 2 000 rows x 200 000 entries, t = {T}", c, q, row_counts, True, None) and met
    c.dispose()
    q.dispose()
    del packed, rows, c, q
    torch.cuda.empty_cache()
met = self_leg("self100k", 100_000, False, 1) and met
sys.exit(0 if met else 1)
