#!/usr/bin/env python3
"""The gather of corpus entries against the yardstick a memory-bound copy cannot beat -- a device-to-device hipMemcpyAsync of
the same number of OUTPUT bytes -- alternating in one process after warm-up:
    python3 tools/prof_gather.py [reps] [--out DIR] [--only urandom|uall|rrandom|rall]
Legs:
    urandom   1 M random entries of a 10 M-entry 5 x 200 uniform corpus
    uall      all 10 M entries of it, in order
    rrandom   100 k random entries of a 1 M-entry ragged corpus of 20 .. 70 sub-fingerprints (length 200)
    rall      all 1 M entries of it, in order
Every call is the whole gather: lengths, the two scans and the copy, with the capacity at the true total.  Device time:
hipEvents around the calls on the current stream; medians and quartiles of `reps` (default 9) rounds in ms, one JSON line per
leg, also appended to DIR/gather_prof.jsonl (default DIR: profiles).  Every GPU step under its own time limit:
    timeout -k 10 600 python3 tools/prof_gather.py 9 --only urandom && timeout -k 10 600 python3 tools/prof_gather.py 9 --only uall && \\
    timeout -k 10 600 python3 tools/prof_gather.py 9 --only rrandom && timeout -k 10 600 python3 tools/prof_gather.py 9 --only rall"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lbaudiodetective_amd as lb  # noqa: E402

SEED = 0x47415448


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
ONLY = _option("--only")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in {OUT, ONLY}]
REPS = int(args[0]) if args else 9


def _hip():
    """the HIP runtime this process has loaded already (torch's), by its path: no second runtime comes in"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime is loaded"
    h = C.CDLL(sorted(paths)[0])
    h.hipMemcpyAsync.restype = C.c_int
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return h


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
    with open(os.path.join(OUT, "gather_prof.jsonl"), "a") as f:
        f.write(json.dumps(res) + "\n")


def leg(name, corpus, indices):
    """the gather of `indices` (numpy) out of `corpus`, and the copy of as many bytes as it writes"""
    hip = _hip()
    keys = torch.from_numpy((np.uint64(0xFFFFFFFF) - indices.astype(np.uint64)).view(np.int64)).cuda()
    packed, offsets = corpus.gather_keys_device(keys)                     # (sizes itself: the true total)
    total = packed.shape[0]
    src = torch.empty_like(packed).copy_(packed)
    dst = torch.empty_like(packed)
    nbytes = packed.numel()
    stream = torch.cuda.current_stream().cuda_stream

    def gather():
        corpus.gather_keys_device(keys, packed_out=packed, offsets_out=offsets, capacity=total)

    def copy():
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream) == 0      # 3: hipMemcpyDeviceToDevice

    calls = {"gather": gather, "memcpy": copy}
    for f in calls.values():
        for _ in range(2):
            f()
        torch.cuda.synchronize()
    assert int(offsets[-1]) == total and torch.equal(dst, src)
    times = {k: [] for k in calls}
    for _ in range(REPS):
        for k, f in calls.items():
            times[k].append(device_ms(f))
    res = {"leg": name, "reps": REPS, "entries": len(corpus), "keys": len(indices), "subfingerprints": total, "output_bytes": nbytes}
    for k in calls:
        res[k] = _stats(times[k])
        res[k + "_gb_per_s"] = round(nbytes / res[k]["median"] / 1e6, 1)
    res["gather_over_memcpy"] = round(res["gather"]["median"] / res["memcpy"]["median"], 3)
    report(res)


def want(*names):
    return ONLY is None or ONLY in names


torch.cuda.set_device(0)
rng = np.random.default_rng(SEED)

if want("urandom", "uall"):
    n = 10_000_000
    c = lb.Corpus(200, 5, n)
    step = 1_000_000
    for first in range(0, n, step):                                       # (the synthetic rows a block at a time)
        c.append_packed_device(lb.synth_corpus_device(SEED, first, step, 5, 200))
        torch.cuda.synchronize()
    torch.cuda.empty_cache()
    if want("urandom"):
        leg("uniform 10 M x 5 x 200: 1 M random entries", c, rng.integers(0, n, 1_000_000))
    if want("uall"):
        leg("uniform 10 M x 5 x 200: all entries in order", c, np.arange(n))
    c.dispose()
    del c
    torch.cuda.empty_cache()

if want("rrandom", "rall"):
    n = 1_000_000
    counts = np.random.default_rng(SEED + 1).integers(20, 71, n).astype(np.uint32)
    c = lb.Corpus.ragged(200, n, int(counts.sum()))
    step = 100_000
    for first in range(0, n, step):
        c.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, first, counts[first:first + step], 200), counts[first:first + step])
        torch.cuda.synchronize()
    torch.cuda.empty_cache()
    if want("rrandom"):
        leg("ragged 1 M entries of 20 .. 70 x 200: 100 k random entries", c, rng.integers(0, n, 100_000))
    if want("rall"):
        leg("ragged 1 M entries of 20 .. 70 x 200: all entries in order", c, np.arange(n))
    c.dispose()
