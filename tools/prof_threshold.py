#!/usr/bin/env python3
"""Threshold queries against the top-1 and top-K (K = 10) calls of the same build, alternating in one process after warm-up:
    python3 tools/prof_threshold.py [reps] [--out DIR] [--trace] [--only uniform|ragged]
Legs: the uniform corpus of 10 M x 5 sub-fingerprints (one query and a batch of 8) and the ragged corpus of 1 M entries of
20..70 against a query of 21, each at a selective threshold (0.7: the query's own entry and four planted copies) and at a dense
one (the median of the query's scores: about half the corpus, capacity >= count); and the aligned (packed) form at the
selective threshold with capacity 1024 and 2^20, which shows what aligning empty slots costs.  Device time: hipEvents around
the KeysDevice forms on the current stream; medians and quartiles of `reps` (default 30) calls in ms, one JSON line per leg,
also appended to DIR/threshold_prof.jsonl (default DIR: profiles).

--trace: three calls of each leg only, for a kernel trace in a run of its own.  Every GPU step under its own time limit:
    timeout -k 10 600 python3 tools/prof_threshold.py 30 && \\
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d /tmp/threshold_trace -o threshold_trace --output-format csv -- \\
        python3 tools/prof_threshold.py --trace && \\
    cp /tmp/threshold_trace/*/threshold_trace_kernel_stats.csv profiles/"""
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


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


TRACE = "--trace" in sys.argv
OUT = _option("--out", os.path.join(ROOT, "profiles"))
ONLY = _option("--only")
_skip = {OUT, ONLY}
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in _skip]
REPS = 3 if TRACE else (int(args[0]) if args else 30)


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _packed(bools):
    return np.ascontiguousarray(O.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _stats(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    return {"median": round(q[1], 4), "p25": round(q[0], 4), "p75": round(q[2], 4)}


def report(res):
    print(json.dumps(res), flush=True)
    if not TRACE:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "threshold_prof.jsonl"), "a") as f:
            f.write(json.dumps(res) + "\n")


def alternate(name, calls, extra):
    """calls: {label: function}; warm-up, then REPS rounds of every call in turn"""
    for f in calls.values():
        f()
        f()
        torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(REPS):
        for k, f in calls.items():
            t[k].append(device_ms(f))
    res = {"leg": name, "reps": REPS, **extra}
    for k, v in t.items():
        res[k] = _stats(v)
    return res


def leg(name, corpus, fps, qbools):
    q = len(fps)
    k1 = torch.zeros(q, dtype=torch.int64, device="cuda")
    kk = torch.zeros((q, 10), dtype=torch.int64, device="cuda")
    scores = torch.stack([corpus.scores_device(f) for f in fps])
    median = float(scores.median(dim=1).values.max())
    dense_count = int((scores >= median).sum(dim=1).max())
    sel_count = (scores >= 0.7).sum(dim=1).tolist()
    del scores
    torch.cuda.empty_cache()
    sel = (torch.zeros((q, 1024), dtype=torch.int64, device="cuda"), torch.zeros(q, dtype=torch.int64, device="cuda"))
    dense = (torch.zeros((q, dense_count + 1024), dtype=torch.int64, device="cuda"), torch.zeros(q, dtype=torch.int64, device="cuda"))
    calls = {
        "top1": lambda: corpus.query_batch_keys_device(fps, k1),
        "topk10": lambda: corpus.query_batch_topk_keys_device(fps, 10, kk),
        "threshold_selective": lambda: corpus.query_batch_threshold_keys_device(fps, 0.7, 1024, *sel),
        "threshold_dense": lambda: corpus.query_batch_threshold_keys_device(fps, median, dense_count + 1024, *dense),
    }
    res = alternate(name, calls, {"queries": q, "selective_counts": sel_count, "dense_threshold": median, "dense_count": dense_count})
    assert sel[1].tolist() == sel_count and int(dense[1].max()) == dense_count
    res["selective_minus_topk10"] = round(res["threshold_selective"]["median"] - res["topk10"]["median"], 4)
    report(res)
    if q != 1:
        return
    # the aligned (packed) form at the selective threshold: capacity 1024 and 2^20
    d_rows = torch.from_numpy(_packed(qbools[0][None])).cuda()
    per = qbools[0].shape[0]
    calls = {"topk10_aligned": lambda: corpus.query_packed_topk_keys_device(d_rows, 1, per, 10, aligned=True)}
    for cap in (1024, 1 << 20):
        out = (torch.zeros((1, cap), dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"),
               torch.zeros((1, cap), dtype=torch.int32, device="cuda"))
        calls[f"threshold_aligned_cap{cap}"] = aligned_call(corpus, d_rows, per, out)
    report(alternate(name + ", aligned (packed form), t = 0.7", calls, {"queries": 1, "selective_counts": sel_count}))


def aligned_call(corpus, d_rows, per, out):
    return lambda: corpus.query_packed_threshold_keys_device(d_rows, 1, per, 0.7, out[0].shape[1], *out)


torch.cuda.set_device(0)
if ONLY in (None, "uniform"):
    n = 10_000_000
    qbools = [O.synth_entry(SEED, 1_000_003 * (i + 1), 5, 200) for i in range(8)]
    packed = lb.synth_corpus_device(SEED, 0, n, 5, 200)
    for i, b in enumerate(qbools):                          # four planted copies of every query beside its own entry
        row = torch.from_numpy(_packed(b)).cuda()
        for at in (17 + i, 2_500_000 + i, 6_000_001 + i, n - 1 - i):
            packed[at] = row
    uni = lb.Corpus(200, 5, n)
    uni.append_packed_device(packed)
    qs = [lb.Fingerprint.from_bools(b) for b in qbools]
    torch.cuda.synchronize()
    del packed
    leg("uniform 10M x 5, one query", uni, qs[:1], qbools[:1])
    leg("uniform 10M x 5, batch of 8", uni, qs, qbools)
    uni.dispose()
    torch.cuda.empty_cache()

if ONLY in (None, "ragged"):
    nr = 1_000_000
    counts = O.synth_ragged_counts(SEED, 0, nr, 20, 70)
    flat = lb.synth_ragged_corpus_device(SEED, 0, counts, 200)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    e = 500_001
    qb = O.synth_entry(SEED, e, int(counts[e]), 200)[:21]
    row = torch.from_numpy(_packed(qb)).cuda()
    for at in (11, 250_000, 750_003, nr - 2):               # planted: the query at the head of four more entries
        m = min(21, int(counts[at]))
        flat[off[at]:off[at] + m] = row[:m]
    rag = lb.Corpus.ragged(200, nr, int(counts.sum()))
    rag.append_ragged_packed_device(flat, counts)
    torch.cuda.synchronize()
    del flat
    leg("ragged 1M of 20..70, query of 21", rag, [lb.Fingerprint.from_bools(qb)], [qb])
    rag.dispose()
