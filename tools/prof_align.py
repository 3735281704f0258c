#!/usr/bin/env python3
"""Aligned corpus queries against their plain counterparts, alternating in one process after warm-up:
    python3 tools/prof_align.py [reps] [--trace]
Legs: top-10 of a batch of 8 against the uniform corpus of 10 M x 5 sub-fingerprints and against the ragged corpus of 1 M entries
of 20..70 (queries of 21), the top-1 query on both, and the match profile of a query of 48 against one entry of 200 000
sub-fingerprints.  Device time: hipEvents on the current stream around the KeysDevice forms (plain: QueryBatchTopKKeysDevice;
aligned: the same plus CorpusAlignKeysDevice on its keys) and around the profile call; host time: wall clock of the
host-returning calls (QueryBatchTopK / Query against QueryBatchTopKAligned / QueryAligned).  Medians in ms.
--trace: a few calls of each leg only (for a rocprofv3 --kernel-trace --stats pass)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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


def run(name, fns, **extra):
    """fns: {label: (timer, callable)}; warm-up twice each, then REPS rounds in turn."""
    for _, f in fns.values():
        f()
        f()
        torch.cuda.synchronize()
    t = {key: [] for key in fns}
    for _ in range(REPS):
        for key, (timer, f) in fns.items():
            t[key].append(timer(f))
    res = {"leg": name, **extra, **{key: round(statistics.median(v), 4) for key, v in t.items()}}
    if "plain_device" in res:
        res["added_device"] = round(res["aligned_device"] - res["plain_device"], 4)
        res["added_host"] = round(res["aligned_host"] - res["plain_host"], 4)
    print(json.dumps(res), flush=True)
    return res


def topk_leg(name, corpus, fps, k):
    q = len(fps)
    kk = torch.zeros((q, k), dtype=torch.int64, device="cuda")
    plain_dev = lambda: corpus.query_batch_topk_keys_device(fps, k, kk)  # noqa: E731

    def aligned_dev():
        corpus.query_batch_topk_keys_device(fps, k, kk)
        corpus.align_keys_device(fps, kk, k)

    align_only = lambda: corpus.align_keys_device(fps, kk, k)  # noqa: E731
    run(name, {"plain_device": (device_ms, plain_dev), "aligned_device": (device_ms, aligned_dev),
               "align_only_device": (device_ms, align_only),
               "plain_host": (wall_ms, lambda: corpus.query_batch_topk(fps, k)),
               "aligned_host": (wall_ms, lambda: corpus.query_batch_topk_aligned(fps, k))}, queries=q, k=k)


def top1_leg(name, corpus, fp):
    run(name, {"plain_host": (wall_ms, lambda: corpus.query(fp)), "aligned_host": (wall_ms, lambda: corpus.query_aligned(fp))})


torch.cuda.set_device(0)
n = 10_000_000
uni = lb.Corpus(200, 5, n)
uni.append_packed_device(lb.synth_corpus_device(SEED, 0, n, 5, 200))
qs = [lb.Fingerprint.from_bools(O.synth_entry(SEED, 1_000_003 * (i + 1), 5, 200)) for i in range(8)]
torch.cuda.synchronize()
topk_leg("uniform 10M x 5, batch of 8", uni, qs, 10)
top1_leg("uniform 10M x 5, top-1", uni, qs[0])
del uni
torch.cuda.empty_cache()

nr = 1_000_000
counts = O.synth_ragged_counts(SEED, 0, nr, 20, 70)
rag = lb.Corpus.ragged(200, nr, int(counts.sum()))
rag.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, 0, counts, 200), counts)
rq = [lb.Fingerprint.from_bools(O.synth_entry(SEED, e, int(counts[e]), 200)[:21]) for e in range(500_001, 500_009)]
torch.cuda.synchronize()
topk_leg("ragged 1M of 20..70, batch of 8 queries of 21", rag, rq, 10)
top1_leg("ragged 1M of 20..70, top-1 of a query of 21", rag, rq[0])
del rag
torch.cuda.empty_cache()

rng = np.random.default_rng(1)
long = (rng.random((200_000, 200)) < 0.5).astype(np.uint8)
one = lb.Corpus.ragged(200, 1, 200_000)
one.append_fingerprint(lb.Fingerprint.from_bools(long))
pq = lb.Fingerprint.from_bools(long[77_777:77_825])
torch.cuda.synchronize()
L = lb.lib()
count, first = lb._native.UInt64(0), lb._native.SInt32(0)
buf = np.zeros(200_000 - 48 + 1, np.float32)
ptr = buf.ctypes.data_as(lb._native.C.POINTER(lb._native.Float32))
profile = lambda: L.LBAudioDetectiveCorpusMatchProfile(one._ref, pq._ref, 0, 0, ptr, buf.size,  # noqa: E731
                                                       lb._native.C.byref(count), lb._native.C.byref(first))
run("match profile, query of 48 against 200 000", {"profile_device": (device_ms, profile), "profile_host": (wall_ms, profile)},
    offsets=int(buf.size))
assert int(np.argmax(buf)) == 77_777
