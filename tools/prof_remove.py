#!/usr/bin/env python3
"""The removal of corpus entries against two yardsticks, alternating in one process after warm-up:
    python3 tools/prof_remove.py [reps] [--out DIR] [--only u1|u50|utail|r1] [--entries N] [--ragged-entries N]
Legs:
    u1, u50   uniform 10 M entries x 5 x 200 Booleans, a random 1 % / 50 % of the entries removed
    utail     the same corpus, the last 1 % removed (nothing is moved)
    r1        ragged, 1 M entries of 20 .. 70 sub-fingerprints, a random 1 % removed
Per round: the corpus is refilled (untimed), then timed
    remove    remove_keys_device with the keys of the entries on the device
    copy      (a) one device-to-device hipMemcpyAsync of the stored bytes that lie above the first removed entry: the read-once /
              write-once floor (the bounce scheme moves the data twice)
    rebuild   (b) what the removal replaces: append_packed_device / append_ragged_packed_device of the kept rows into a second,
              empty corpus (the kept rows are gathered beforehand, untimed: a service would not even have them on the device)
Device time: hipEvents around the calls on the current stream (a removal reads its index back in the middle: the gap is part of
it); medians and quartiles of `reps` (default 5) rounds in ms, one JSON line per leg, also appended to DIR/remove_prof.jsonl
(default DIR: profiles).  Under its own time limit:
    timeout -k 10 600 python3 tools/prof_remove.py 5"""
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
from oracle import oracle as O  # noqa: E402

SEED = 0x4C424146


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
ONLY = _option("--only")
N_UNIFORM = int(_option("--entries", 10_000_000))
N_RAGGED = int(_option("--ragged-entries", 1_000_000))
_skip = {OUT, ONLY, _option("--entries"), _option("--ragged-entries")}
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in _skip]
REPS = int(args[0]) if args else 5

# the HIP runtime the library itself is linked against (one runtime in the process: torch's)
lb.lib()
_hip = C.CDLL(lb.LIB_PATH)
_hip.hipMemcpyAsync.restype = C.c_int
_hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
HIP_D2D = 3


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
    with open(os.path.join(OUT, "remove_prof.jsonl"), "a") as f:
        f.write(json.dumps(res) + "\n")


def keys_of(indices):
    """64-bit keys as the query calls write them (score word: 1.0), on the device"""
    idx = np.asarray(indices, np.uint64)
    return torch.from_numpy(((np.uint64(0x3F800000) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)).view(np.int64)).cuda()


def leg(name, corpus, second, fill, fill_kept, n, indices, floor_bytes):
    """fill(corpus): all entries appended; fill_kept(second): the kept rows appended (the rebuild)"""
    keys = keys_of(indices)
    removed_want = len(np.unique(indices))
    src = torch.empty(max(1, floor_bytes), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    stream = torch.cuda.current_stream().cuda_stream

    def copy():
        if floor_bytes:
            assert _hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), floor_bytes, HIP_D2D, stream) == 0

    times = {"remove": [], "copy": [], "rebuild": []}
    for rep in range(REPS + 1):                                   # (round 0 warms up: the scratch grows there)
        if len(corpus):
            corpus.remove_keys_device(keys_of(np.arange(len(corpus))))     # empty it: a removal of everything moves nothing
        fill(corpus)
        if len(second):
            second.remove_keys_device(keys_of(np.arange(len(second))))
        torch.cuda.synchronize()
        got = []
        t_remove = device_ms(lambda: got.append(corpus.remove_keys_device(keys)))
        t_copy = device_ms(copy)
        t_rebuild = device_ms(lambda: fill_kept(second))
        assert got[0] == removed_want and len(corpus) == n - removed_want == len(second)
        if rep:
            times["remove"].append(t_remove)
            times["copy"].append(t_copy)
            times["rebuild"].append(t_rebuild)
    res = {"leg": name, "reps": REPS, "entries": n, "removed": removed_want, "bytes_above_first_removed": floor_bytes}
    for k, v in times.items():
        res[k] = _stats(v)
    res["remove_over_copy"] = round(res["remove"]["median"] / res["copy"]["median"], 3) if res["copy"]["median"] > 0 else None
    res["rebuild_over_remove"] = round(res["rebuild"]["median"] / res["remove"]["median"], 3)
    report(res)


def want(name):
    return ONLY is None or ONLY == name


torch.cuda.set_device(0)
rng = np.random.default_rng(SEED)

if any(want(x) for x in ("u1", "u50", "utail")):
    n = N_UNIFORM
    packed = lb.synth_corpus_device(SEED, 0, n, 5, 200)
    c, second = lb.Corpus(200, 5, n), lb.Corpus(200, 5, n)
    stride = c.entry_stride_bytes
    for name, indices in (("u1", rng.choice(n, n // 100, replace=False)), ("u50", rng.choice(n, n // 2, replace=False)),
                          ("utail", np.arange(n - n // 100, n))):
        if not want(name):
            continue
        keep = np.ones(n, bool)
        keep[indices] = False
        kept_rows = packed[torch.from_numpy(np.nonzero(keep)[0]).cuda()].contiguous()
        leg(f"uniform {n} x 5 x 200, {name}", c, second, lambda x: x.append_packed_device(packed),
            lambda x: x.append_packed_device(kept_rows), n, indices, (n - int(indices.min())) * stride)
        del kept_rows
        torch.cuda.empty_cache()
    c.dispose()
    second.dispose()
    del packed
    torch.cuda.empty_cache()

if want("r1"):
    n = N_RAGGED
    counts = O.synth_ragged_counts(SEED, 0, n, 20, 70)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(off[-1])
    packed = lb.synth_ragged_corpus_device(SEED, 0, counts, 200)
    c, second = lb.Corpus.ragged(200, n, total), lb.Corpus.ragged(200, n, total)
    indices = rng.choice(n, n // 100, replace=False)
    keep = np.ones(n, bool)
    keep[indices] = False
    kept_counts = counts[keep]
    kept_rows = packed[torch.from_numpy(np.nonzero(np.repeat(keep, counts))[0]).cuda()].contiguous()
    leg(f"ragged {n} entries of 20..70, r1", c, second, lambda x: x.append_ragged_packed_device(packed, counts),
        lambda x: x.append_ragged_packed_device(kept_rows, kept_counts), n, indices, (total - int(off[indices.min()])) * 32)
    c.dispose()
    second.dispose()
