#!/usr/bin/env python3
"""The recording segments call against the step in front of it and the host path it replaces, in one process per shape:
    python3 tools/prof_segments.py [reps] [--out DIR] [--shape NAME]
Shapes (synthetic ragged corpora of entries of 20 .. 70 sub-fingerprints of 200 Booleans, random recordings with a piece of an
entry planted in each):
    monitor  1 024 channels x 256 sub-fingerprints against 2 000 entries -- a broadcast monitor's
    long     8 x 2 400 against 100 000 entries
Each at two thresholds: 0.7 (the planted pieces and little else are candidates) and 0.3 (noise winners at many offsets).
Legs:
    segments  timeline_segments_device alone on the timeline's keys and lengths, by device events (and a host clock around the call
              and the synchronise that ends it)
    timeline  Corpus.recording_timeline_batch_keys_device alone -- what StreamBank.timeline costs behind its window -- by device
              events
    host      the path the call replaces: keys and lengths read back, decode_timeline_batch_keys, timeline_segments per row, by
              host clock (nothing is uploaded again, which a caller who goes on with the ids or the gather would also pay)
Without --shape the tool runs every shape in a CHILD process of its own under its own time limit, one after the other, and stops
at the first that fails; with --shape it is that child.  Median, min and max of `reps` rounds (default 7) in ms, one warm-up round
in front.  After the clock stops the device rows must equal the host path's, every word.  One JSON object per shape, printed and
merged into DIR/segments.json (default DIR: profiles).
    timeout -k 10 600 python3 tools/prof_segments.py 7"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5345474D
L = 200
THRESHOLDS = (0.7, 0.3)
# name: (recordings, sub-fingerprints each, entries, slots per row, seconds the child may take)
SHAPES = {"monitor": (1024, 256, 2000, 16, 240), "long": (8, 2400, 100000, 128, 240)}


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
SHAPE = _option("--shape")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in {OUT, SHAPE}]
REPS = max(3, int(args[0]) if args else 7)


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def parent():
    """every shape in a fresh child under its own time limit; this process never opens the device"""
    os.makedirs(OUT, exist_ok=True)
    merged = {}
    for name, shape in SHAPES.items():
        cmd = [sys.executable, os.path.abspath(__file__), str(REPS), "--out", OUT, "--shape", name]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=shape[-1])
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {shape[-1]} s; stopping", flush=True)
            return 124
        if run.returncode != 0:
            print(f"{name}: exit status {run.returncode}; stopping\n{run.stderr[-3000:]}", flush=True)
            return run.returncode
        merged[name] = json.loads(run.stdout.strip().splitlines()[-1])
        print(json.dumps({name: merged[name]}), flush=True)
        with open(os.path.join(OUT, "segments.json"), "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")
    return 0


def child(name):
    import numpy as np
    import torch
    import lbaudiodetective_amd as lb

    R, per, entries, cap, _limit = SHAPES[name]
    torch.cuda.set_device(0)
    counts = np.random.default_rng(SEED).integers(20, 71, entries).astype(np.uint32)
    counts[0], counts[1] = 20, 70
    corpus = lb.Corpus.ragged(L, entries, int(counts.sum()))
    corpus.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, 0, counts, L), counts)
    packed = lb.synth_ragged_corpus_device(SEED + 1, 0, np.array([R * per], np.uint32), L).reshape(R, per, 32).contiguous()
    src = lb.synth_ragged_corpus_device(SEED, 0, counts[:64], L)
    off = np.concatenate([[0], np.cumsum(counts[:64])])
    for r in range(R):
        j = r % 64
        packed[r, 5:5 + int(counts[j])] = src[int(off[j]):int(off[j + 1])]
    keys = torch.zeros((R, per), dtype=torch.int64, device="cuda")
    lengths = torch.zeros((R, per), dtype=torch.int32, device="cuda")
    outs = (torch.zeros((R, cap), dtype=torch.int32, device="cuda"), torch.zeros((R, cap), dtype=torch.int64, device="cuda"),
            torch.zeros((R, cap), dtype=torch.int32, device="cuda"), torch.zeros(R, dtype=torch.int32, device="cuda"))
    host_rows = []

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)

    res = {"recordings": R, "per": per, "entries": entries, "entry_lengths": [20, 70], "capacity": cap, "reps": REPS, "thresholds": {}}
    for threshold in THRESHOLDS:
        def leg_timeline():
            corpus.recording_timeline_batch_keys_device(packed, R, per, threshold, keys_out=keys, lengths_out=lengths)

        def leg_segments():
            lb.timeline_segments_device(keys, lengths, cap, starts_out=outs[0], keys_out=outs[1], lengths_out=outs[2], counts_out=outs[3])

        def leg_host():
            idx, sc, ln = lb.decode_timeline_batch_keys(keys, lengths)
            host_rows[:] = [lb.timeline_segments(idx[r], sc[r], ln[r]) for r in range(R)]

        legs = {"timeline": leg_timeline, "segments": leg_segments, "host": leg_host}
        host = {k: [] for k in legs}
        device = {k: [] for k in legs}
        for rep in range(REPS + 1):                                   # (the first round warms every leg up)
            for k, f in legs.items():
                h, d = timed(f)
                if rep:
                    host[k].append(h)
                    device[k].append(d)
        torch.cuda.synchronize()
        # after the clock: the device rows are the host path's, every word
        st, ks, ln, cn = (x.cpu().numpy() for x in outs)
        hk = keys.cpu().numpy()
        spans = 0
        for r in range(R):
            kept = host_rows[r][0]
            m = min(len(kept), cap)
            assert cn[r] == len(kept), f"recording {r}: {cn[r]} spans, the host path has {len(kept)}"
            assert np.array_equal(st[r, :m], kept[:m]) and np.array_equal(ks[r, :m], hk[r][kept[:m]]), f"recording {r} differs"
            assert np.array_equal(ln[r, :m].view(np.uint32), host_rows[r][3][:m]), f"recording {r}: lengths differ"
            assert not st[r, m:].any() and not ks[r, m:].any() and not ln[r, m:].any(), f"recording {r}: no zeros behind the spans"
            spans += len(kept)
        one = {"candidates": int(((keys != 0) & (lengths != 0)).sum()), "spans": spans, "largest_count": int(cn.max()),
               "segments_device_ms": _stats(device["segments"]), "segments_host_clock_ms": _stats(host["segments"]),
               "timeline_device_ms": _stats(device["timeline"]), "host_path_ms": _stats(host["host"])}
        one["host_path_over_segments"] = round(one["host_path_ms"]["median"] / one["segments_host_clock_ms"]["median"], 1)
        one["segments_below_host_path"] = one["segments_host_clock_ms"]["median"] < one["host_path_ms"]["median"]
        res["thresholds"][str(threshold)] = one
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(child(SHAPE) if SHAPE else parent())
