#!/usr/bin/env python3
"""What the host detour of a query costs: packed fingerprints on the device -> keys on the device, two routes on one commit.
    python3 tools/identify_pipeline.py [--reps N] [--uniform-queries Q] [--ragged-queries Q] [--trace] [--stats CSV]
Workloads: Q = 100 000 clips of the 44.1 kHz / 1024 configuration (one second each, 5 sub-fingerprints, fingerprinted on the
device) against the uniform corpus of 10 M x 5, and Q = 10 000 queries of 21 sub-fingerprints against the ragged corpus of 1 M
entries of 20..70.
Route (a): LBAudioDetectiveCorpusQueryPackedKeysDevice on the rows where they lie.
Route (b): what a caller had to do before: copy the rows to the host, unpack them, build a handle per query
(Fingerprint.from_bools, one call per sub-fingerprint), LBAudioDetectiveCorpusQueryBatchKeysDevice.
Per route and repetition: wall time (host clock around work that ends in a device synchronise) and the time between two
events on the stream around the whole route; for (b) also its three host stages.  After a warm-up call of each route the
routes alternate; every repetition is listed, with median, minimum and maximum.  The keys of both routes are compared.
--trace: a warm-up and two calls of route (a) only, for a `rocprofv3 --kernel-trace --stats` run of its own;
--stats CSV: no device work -- sums that run's kernel_stats CSV into the builders' / scans' share of the device time."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--uniform-queries", type=int, default=100_000)
ap.add_argument("--ragged-queries", type=int, default=10_000)
ap.add_argument("--uniform-entries", type=int, default=10_000_000)
ap.add_argument("--ragged-entries", type=int, default=1_000_000)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--stats")
args = ap.parse_args()

BUILDERS = ("build_plane_queries_kernel", "build_sliding_queries_kernel", "build_query_rows_kernel")


def summarize(path):
    """kernel_stats CSV of rocprofv3 (Name, Calls, TotalDurationNs, ...) -> the builders' share of the kernels' time"""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {"stats": os.path.basename(path), "kernel_ms": round(total / 1e6, 3), "kernels": []}
    built = 0.0
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"])
        name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        if any(b in name for b in BUILDERS):
            built += ns
        if ns / total > 0.002 or any(b in name for b in BUILDERS):
            out["kernels"].append({"name": name[-90:], "calls": int(r["Calls"]), "ms": round(ns / 1e6, 4), "share": round(ns / total, 5)})
    out["builders_ms"] = round(built / 1e6, 4)
    out["builders_share"] = round(built / total, 6)
    print(json.dumps(out), flush=True)


if args.stats:
    summarize(args.stats)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import lbaudiodetective_amd as lb  # noqa: E402
from oracle import oracle as O  # noqa: E402

SEED = 0x4C424147
if not torch.cuda.is_available():
    sys.exit("identify_pipeline.py measures on a GPU; none is visible")
torch.cuda.set_device(0)


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def timed(fn):
    """(wall ms, ms between two events on the stream around fn)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


def workload(name, corpus, packed, n, per):
    keys_a = torch.zeros(n, dtype=torch.int64, device="cuda")
    keys_b = torch.zeros(n, dtype=torch.int64, device="cuda")
    stages = {"to_host_and_unpack": [], "handles": [], "query_call": []}

    def route_a():
        corpus.query_packed_keys_device(packed, n, per, keys_out=keys_a)

    def route_b():
        t0 = time.perf_counter()
        bools = lb.unpack_packed(packed.cpu().numpy().reshape(-1, 32), 200).reshape(n, per, 200)
        t1 = time.perf_counter()
        fps = [lb.Fingerprint.from_bools(b) for b in bools]
        t2 = time.perf_counter()
        corpus.query_batch_keys_device(fps, keys_b)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        for key, dt in zip(stages, (t1 - t0, t2 - t1, t3 - t2)):
            stages[key].append(dt * 1e3)
        for f in fps:
            f.dispose()

    if args.trace:
        for _ in range(3):
            route_a()
        torch.cuda.synchronize()
        return
    route_a()
    route_b()                                       # warm-up: allocations, plans, code objects
    for v in stages.values():
        v.clear()
    t = {"a_wall": [], "a_events": [], "b_wall": [], "b_events": []}
    for _ in range(args.reps):
        w, e = timed(route_a)
        t["a_wall"].append(w)
        t["a_events"].append(e)
        w, e = timed(route_b)
        t["b_wall"].append(w)
        t["b_events"].append(e)
    same = bool(torch.equal(keys_a, keys_b))
    res = {"workload": name, "queries": n, "subfingerprints_per_query": per, "entries": len(corpus), "reps": args.reps, "keys_equal": same,
           "unit": "ms", **{k: spread(v) for k, v in t.items()}, "b_stages": {k: spread(v) for k, v in stages.items()}}
    res["wall_ratio_b_over_a"] = round(res["b_wall"]["median"] / res["a_wall"]["median"], 3)
    print(json.dumps(res), flush=True)
    if not same:
        sys.exit("the two routes disagree")


# ---- uniform: clips of the 44.1 kHz / 1024 configuration against 10 M x 5 -------------------------------------------------------
rate, window = 44100, 1024
det = lb.Detective().configure(sample_rate=rate, window=window)
per = det.subfingerprint_count(rate)
nq = args.uniform_queries
packed = torch.empty((nq, per, 32), dtype=torch.uint8, device="cuda")
chunk = 8192
for at in range(0, nq, chunk):                      # the clips themselves are not kept: 100 000 seconds of PCM are 17.6 GB
    m = min(chunk, nq - at)
    det.fingerprint_clips_device(lb.synth_clips_device(SEED, at, m, rate, rate), out=packed[at:at + m])
ne = args.uniform_entries
uni = lb.Corpus(200, per, ne)
uni.append_packed_device(lb.synth_corpus_device(SEED, 0, ne, per, 200))
torch.cuda.synchronize()
workload(f"uniform {ne} x {per}, clips at 44.1 kHz / 1024", uni, packed, nq, per)
del uni, packed
torch.cuda.empty_cache()

# ---- ragged: queries of 21 against 1 M entries of 20..70 ---------------------------------------------------------------------
nr, nq, per = args.ragged_entries, args.ragged_queries, 21
counts = O.synth_ragged_counts(SEED, 0, nr, 20, 70)
records = lb.synth_ragged_corpus_device(SEED, 0, counts, 200)
rag = lb.Corpus.ragged(200, nr, int(counts.sum()))
rag.append_ragged_packed_device(records, counts)
off = np.concatenate([[0], np.cumsum(counts)])
rng = np.random.default_rng(3)
picks = rng.integers(0, nr, nq)
# a window of 21 records that starts inside entry picks[i] (and stays inside it where the entry has 21 or more)
starts = off[picks] + rng.integers(0, np.maximum(counts[picks].astype(np.int64) - per + 1, 1))
starts = np.minimum(starts, off[-1] - per)
idx = torch.from_numpy(starts[:, None] + np.arange(per)[None, :]).cuda()
packed = records[idx].contiguous()                  # [nq, 21, 32]
torch.cuda.synchronize()
workload(f"ragged {nr} of 20..70, queries of {per}", rag, packed, nq, per)
