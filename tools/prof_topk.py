#!/usr/bin/env python3
"""Top-K queries against their top-1 counterparts, alternating in one process after warm-up:
    python3 tools/prof_topk.py [reps] [--trace]
Legs: the uniform corpus of 10 M x 5 sub-fingerprints (K = 10 and K = 1024, one query and a batch of 8) and the ragged corpus of
1 M entries of 20..70 against a query of 21.  Device time: hipEvents around the KeysDevice forms on the current stream (top-1:
LBAudioDetectiveCorpusQueryBatchKeysDevice, top-K: LBAudioDetectiveCorpusQueryBatchTopKKeysDevice); host time: wall clock
of the host-returning calls (LBAudioDetectiveCorpusQuery / QueryBatch against QueryTopK / QueryBatchTopK).  Medians in ms.
--trace: a few calls of each leg only (for a rocprofv3 --kernel-trace --stats pass)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import lbaudiodetective_amd as lb  # noqa: E402
from oracle import oracle as O  # noqa: E402

SEED = 0x4C424145
args = [a for a in sys.argv[1:] if not a.startswith("--")]
TRACE = "--trace" in sys.argv
REPS = 3 if TRACE else (int(args[0]) if args else 30)


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def leg(name, corpus, fps, k):
    q = len(fps)
    k1 = torch.zeros(q, dtype=torch.int64, device="cuda")
    kk = torch.zeros((q, k), dtype=torch.int64, device="cuda")
    top1_dev = lambda: corpus.query_batch_keys_device(fps, k1)  # noqa: E731
    topk_dev = lambda: corpus.query_batch_topk_keys_device(fps, k, kk)  # noqa: E731
    if q == 1:
        top1_host = lambda: corpus.query(fps[0])  # noqa: E731
        topk_host = lambda: corpus.query_topk(fps[0], k)  # noqa: E731
    else:
        top1_host = lambda: corpus.query_batch(fps)  # noqa: E731
        topk_host = lambda: corpus.query_batch_topk(fps, k)  # noqa: E731
    for f in (top1_dev, topk_dev, top1_host, topk_host):        # warm-up: allocations, plans, code objects
        f()
        f()
        torch.cuda.synchronize()                                  # (the polled top-1 query runs on the corpus' own stream)
    t = {"top1_device": [], "topk_device": [], "top1_host": [], "topk_host": []}
    for _ in range(REPS):
        t["top1_device"].append(device_ms(top1_dev))
        t["topk_device"].append(device_ms(topk_dev))
        t["top1_host"].append(wall_ms(top1_host))
        t["topk_host"].append(wall_ms(topk_host))
    res = {"leg": name, "queries": q, "k": k, **{key: round(statistics.median(v), 4) for key, v in t.items()}}
    res["ratio_device"] = round(res["topk_device"] / res["top1_device"], 3)
    res["ratio_host"] = round(res["topk_host"] / res["top1_host"], 3)
    print(json.dumps(res), flush=True)
    return res


torch.cuda.set_device(0)
n = 10_000_000
uni = lb.Corpus(200, 5, n)
uni.append_packed_device(lb.synth_corpus_device(SEED, 0, n, 5, 200))
qs = [lb.Fingerprint.from_bools(O.synth_entry(SEED, 1_000_003 * (i + 1), 5, 200)) for i in range(8)]
torch.cuda.synchronize()
for k in (10, 1024):
    leg("uniform 10M x 5, one query", uni, qs[:1], k)
    leg("uniform 10M x 5, batch of 8", uni, qs, k)
del uni
torch.cuda.empty_cache()

nr = 1_000_000
counts = O.synth_ragged_counts(SEED, 0, nr, 20, 70)
rag = lb.Corpus.ragged(200, nr, int(counts.sum()))
rag.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, 0, counts, 200), counts)
e = 500_001
rq = [lb.Fingerprint.from_bools(O.synth_entry(SEED, e, int(counts[e]), 200)[:21])]
torch.cuda.synchronize()
for k in (10, 1024):
    leg("ragged 1M of 20..70, query of 21", rag, rq, k)
