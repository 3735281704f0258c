#!/usr/bin/env python3
"""The batch recording timeline against the two things it stands beside, alternating in one process per shape after warm-up:
    python3 tools/prof_timeline_batch.py [reps] [--out DIR] [--shape NAME]
Shapes (synthetic ragged corpora of entries of 20 .. 70 sub-fingerprints of 200 Booleans, random recordings):
    small    1 024 channels x 256 sub-fingerprints against 2 000 entries -- a broadcast monitor's
    large    1 024 x 256 against 100 000 entries
    long     8 x 2 400 against 100 000 entries: form S is the only one
Legs:
    batch    Corpus.recording_timeline_batch_keys_device as the plan takes it (form W at 1 024 x 256)
    batch_s  the same with form S forced (LBAudioDetectiveDebugSetTimelineBatchForm), where the plan takes form W
    loop     the loop of single calls, one Corpus.recording_timeline_keys_device per recording: the only way to these results
             without the batch call
    scan     Corpus.query_packed_topk_keys_device(packed, recordings, per, k=1, aligned=True): what StreamBank.identify costs
             (another question: one entry per recording, not one per offset)
Without --shape the tool runs every shape in a CHILD process of its own under its own time limit, one after the other, and stops
at the first that fails; with --shape it is that child.  Times: a host clock around the calls and the synchronise that ends them,
and device events; medians and quartiles of `reps` rounds (default 7, at least 5) in ms, one warm-up round in front.  After the
clock stops the batch legs' keys and lengths must equal the loop's bit for bit.  One JSON object per shape, printed and merged into
DIR/timeline_batch.json (default DIR: profiles).  No bar: nothing here decides acceptance.
    timeout -k 10 900 python3 tools/prof_timeline_batch.py 7"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x544C4241
L = 200
THRESHOLD = 0.7
# name: (recordings, sub-fingerprints each, entries, seconds the child may take)
SHAPES = {"small": (1024, 256, 2000, 240), "large": (1024, 256, 100000, 420), "long": (8, 2400, 100000, 240)}


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
SHAPE = _option("--shape")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in {OUT, SHAPE}]
REPS = max(5, int(args[0]) if args else 7)


def _stats(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    return {"median": round(q[1], 4), "p25": round(q[0], 4), "p75": round(q[2], 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def parent():
    """every shape in a fresh child under its own time limit; this process never opens the device"""
    os.makedirs(OUT, exist_ok=True)
    merged = {}
    for name, (_r, _p, _e, limit) in SHAPES.items():
        cmd = [sys.executable, os.path.abspath(__file__), str(REPS), "--out", OUT, "--shape", name]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {limit} s; stopping", flush=True)
            return 124
        if run.returncode != 0:
            print(f"{name}: exit status {run.returncode}; stopping\n{run.stderr[-3000:]}", flush=True)
            return run.returncode
        merged[name] = json.loads(run.stdout.strip().splitlines()[-1])
        print(json.dumps({name: merged[name]}), flush=True)
        with open(os.path.join(OUT, "timeline_batch.json"), "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")
    return 0


def child(name):
    import numpy as np
    import torch
    import lbaudiodetective_amd as lb

    R, per, entries, _limit = SHAPES[name]
    torch.cuda.set_device(0)
    counts = np.random.default_rng(SEED).integers(20, 71, entries).astype(np.uint32)
    counts[0], counts[1] = 20, 70
    corpus = lb.Corpus.ragged(L, entries, int(counts.sum()))
    corpus.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, 0, counts, L), counts)
    packed = lb.synth_ragged_corpus_device(SEED + 1, 0, np.array([R * per], np.uint32), L).reshape(R, per, 32).contiguous()
    rows = [packed[r] for r in range(R)]
    # a piece of an entry in every recording, so that the keys are not all noise
    src = lb.synth_ragged_corpus_device(SEED, 0, counts[:64], L)
    off = np.concatenate([[0], np.cumsum(counts[:64])])
    for r in range(R):
        j = r % 64
        packed[r, 5:5 + int(counts[j])] = src[int(off[j]):int(off[j + 1])]
    plan = lb.debug_timeline_batch_plan(R, per, 20, 70, entries)
    out = {k: (torch.zeros((R, per), dtype=torch.int64, device="cuda"), torch.zeros((R, per), dtype=torch.int32, device="cuda"))
           for k in ("batch", "batch_s", "loop")}
    scan_keys = torch.zeros((R, 1), dtype=torch.int64, device="cuda")
    scan_lags = torch.zeros((R, 1), dtype=torch.int32, device="cuda")

    def leg_batch(which):
        lb.debug_set_timeline_batch_form(which == "batch_s")
        try:
            corpus.recording_timeline_batch_keys_device(packed, R, per, THRESHOLD, keys_out=out[which][0], lengths_out=out[which][1])
        finally:
            lb.debug_set_timeline_batch_form(False)

    def leg_loop():
        keys, lengths = out["loop"]
        for r in range(R):
            corpus.recording_timeline_keys_device(packed=rows[r], per_query=per, threshold=THRESHOLD, keys_out=keys[r], lengths_out=lengths[r])

    def leg_scan():
        corpus.query_packed_topk_keys_device(packed, R, per, 1, keys_out=scan_keys, lags_out=scan_lags, aligned=True)

    legs = {"batch": lambda: leg_batch("batch")}
    if plan["form"] == 1:
        legs["batch_s"] = lambda: leg_batch("batch_s")
    legs["loop"] = leg_loop
    legs["scan"] = leg_scan

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)

    host = {k: [] for k in legs}
    device = {k: [] for k in legs}
    for rep in range(REPS + 1):                                       # (the first round warms every leg up)
        for k, f in legs.items():
            h, d = timed(f)
            if rep:
                host[k].append(h)
                device[k].append(d)
    torch.cuda.synchronize()
    for k in legs:
        if k.startswith("batch"):
            assert torch.equal(out[k][0], out["loop"][0]) and torch.equal(out[k][1], out["loop"][1]), f"{k} differs from the loop of single calls"
    winners = int((out["batch"][0] != 0).sum())
    ones = int(((out["batch"][0] >> 32) == 0x3F800000).sum())
    assert ones >= R, "every recording holds a piece of an entry"
    res = {"recordings": R, "per": per, "entries": entries, "entry_lengths": [20, 70], "threshold": THRESHOLD, "reps": REPS, "plan": plan,
           "offsets_with_a_winner": winners, "cells_of_one": ones, "host_ms": {k: _stats(v) for k, v in host.items()},
           "device_ms": {k: _stats(v) for k, v in device.items()}}
    for k in legs:
        if k != "batch":
            res[k + "_over_batch_host"] = round(res["host_ms"][k]["median"] / res["host_ms"]["batch"]["median"], 3)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(child(SHAPE) if SHAPE else parent())
