#!/usr/bin/env python3
"""The batch recording top-K against the two ways to its results that existed before it, alternating in one process per shape
after warm-up:
    python3 tools/prof_recording_batch.py [reps] [--out DIR] [--shape NAME]
Shapes (synthetic ragged corpora of entries of 20 .. 70 sub-fingerprints of 200 Booleans, random recordings with a piece of an
entry in each), every one at k = 1 and k = 10, keys and aligned lags:
    small    1 024 channels x 256 sub-fingerprints against 2 000 entries -- a broadcast monitor's
    large    1 024 x 256 against 100 000 entries
    long     8 x 2 400 against 100 000 entries: form S is the only one
Legs:
    batch    (a) Corpus.query_packed_recording_topk_batch_keys_device as the plan takes it (form W at 1 024 x 256)
    batch_s  (b) the same with form S forced (LBAudioDetectiveDebugSetRecordingBatchForm), where the plan takes form W
    loop     (c) the loop of single calls, one Corpus.query_packed_recording_topk_keys_device per recording
    scan     (d) Corpus.query_packed_topk_keys_device(packed, recordings, per, k, aligned=True): the scan behind StreamBank.identify
Without --shape the tool runs every shape in a CHILD process of its own under its own time limit, one after the other, and stops
at the first that fails; with --shape it is that child.  Times: a host clock around the calls and the synchronise that ends them,
and device events; the median of `reps` rounds (default 7, at least 5) with [min, max] in ms, one warm-up round in front.  After
the clock stops the batch legs' keys and lags must equal the loop's AND the scan's bit for bit.
The bar, at `small` only and against code that existed before the batch call: the maximum of (a) lies below the minimum of (c)
and below the minimum of (d), on both clocks, at both k; the tool fails otherwise.  keep_form_w records whether (a)'s maximum lies
below (b)'s minimum there.  One JSON object per shape, printed and merged into DIR/recording_batch.json (default DIR: profiles).
    timeout -k 10 1100 python3 tools/prof_recording_batch.py 7"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x52424154
L = 200
KS = (1, 10)
# name: (recordings, sub-fingerprints each, entries, seconds the child may take)
SHAPES = {"small": (1024, 256, 2000, 240), "large": (1024, 256, 100000, 540), "long": (8, 2400, 100000, 240)}


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
SHAPE = _option("--shape")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in {OUT, SHAPE}]
REPS = max(5, int(args[0]) if args else 7)


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def parent():
    """every shape in a fresh child under its own time limit; this process never opens the device"""
    os.makedirs(OUT, exist_ok=True)
    merged, missed = {}, 0
    for name, (_r, _p, _e, limit) in SHAPES.items():
        cmd = [sys.executable, os.path.abspath(__file__), str(REPS), "--out", OUT, "--shape", name]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {limit} s; stopping", flush=True)
            return 124
        last = run.stdout.strip().splitlines()[-1:] or [""]
        if run.returncode != 0 and not (run.returncode == 1 and last[0].startswith("{")):
            print(f"{name}: exit status {run.returncode}; stopping\n{run.stdout[-3000:]}\n{run.stderr[-3000:]}", flush=True)
            return run.returncode
        missed = missed or run.returncode                             # (a missed bar is recorded with its figures)
        merged[name] = json.loads(last[0])
        print(json.dumps({name: merged[name]}), flush=True)
        with open(os.path.join(OUT, "recording_batch.json"), "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")
    return missed


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
    # a piece of an entry in every recording, so that the best key is not noise
    src = lb.synth_ragged_corpus_device(SEED, 0, counts[:64], L)
    off = np.concatenate([[0], np.cumsum(counts[:64])])
    for r in range(R):
        j = r % 64
        packed[r, 5:5 + int(counts[j])] = src[int(off[j]):int(off[j + 1])]
    plan = lb.debug_recording_batch_plan(R, per, 20, 70, entries, 0, True)
    res = {"recordings": R, "per": per, "entries": entries, "entry_lengths": [20, 70], "reps": REPS, "plan": plan}
    failed = []
    for k in KS:
        out = {leg: (torch.zeros((R, k), dtype=torch.int64, device="cuda"), torch.zeros((R, k), dtype=torch.int32, device="cuda"))
               for leg in ("batch", "batch_s", "loop", "scan")}

        def leg_batch(which):
            lb.debug_set_recording_batch_form(which == "batch_s")
            try:
                corpus.query_packed_recording_topk_batch_keys_device(packed, R, per, k, keys_out=out[which][0], lags_out=out[which][1])
            finally:
                lb.debug_set_recording_batch_form(False)

        def leg_loop():
            keys, lags = out["loop"]
            for r in range(R):
                corpus.query_packed_recording_topk_keys_device(rows[r], per, k, keys_out=keys[r], lags_out=lags[r])

        def leg_scan():
            corpus.query_packed_topk_keys_device(packed, R, per, k, keys_out=out["scan"][0], lags_out=out["scan"][1], aligned=True)

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

        host = {leg: [] for leg in legs}
        device = {leg: [] for leg in legs}
        for rep in range(REPS + 1):                                   # (the first round warms every leg up)
            for leg, f in legs.items():
                h, d = timed(f)
                if rep:
                    host[leg].append(h)
                    device[leg].append(d)
        torch.cuda.synchronize()
        for leg in legs:
            if leg.startswith("batch"):
                for base in ("loop", "scan"):
                    assert torch.equal(out[leg][0], out[base][0]) and torch.equal(out[leg][1], out[base][1]), f"k={k}: {leg} differs from {base}"
        ones = int(((out["batch"][0][:, 0] >> 32) == 0x3F800000).sum())
        assert ones == R and bool((out["batch"][1][:, 0] == -5).all()), "every recording holds a piece of an entry at offset 5"
        one = {"host_ms": {leg: _stats(v) for leg, v in host.items()}, "device_ms": {leg: _stats(v) for leg, v in device.items()}}
        for clock in ("host_ms", "device_ms"):
            t = one[clock]
            for leg in legs:
                if leg != "batch":
                    one[f"{leg}_over_batch_{clock[:-3]}"] = round(t[leg]["median"] / t["batch"]["median"], 3)
            if name == "small":
                if not (t["batch"]["max"] < t["loop"]["min"] and t["batch"]["max"] < t["scan"]["min"]):
                    failed.append(f"k={k} {clock}: batch max {t['batch']['max']} is not below loop min {t['loop']['min']} and scan min {t['scan']['min']}")
                if "batch_s" in t:
                    one[f"keep_form_w_{clock[:-3]}"] = t["batch"]["max"] < t["batch_s"]["min"]
        res[f"k{k}"] = one
    res["bar"] = "missed: " + "; ".join(failed) if failed else ("met" if name == "small" else "none at this shape")
    print(json.dumps(res), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(child(SHAPE) if SHAPE else parent())
