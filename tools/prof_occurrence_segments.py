#!/usr/bin/env python3
"""The occurrence segments call against the steps in front of it and the host path it replaces, in one process per shape:
    python3 tools/prof_occurrence_segments.py [reps] [--out DIR] [--shape NAME]
Shape (a synthetic ragged corpus of entries of 20 .. 70 sub-fingerprints of 200 Booleans, random windows with a piece of an entry
planted in each):
    monitor  1 024 windows x 256 sub-fingerprints against 2 000 entries -- a broadcast monitor's
At the two thresholds of tools/prof_occurrences_batch.py, peaks on, rows of 8 192 slots:
    planted  1.0: only the planted pieces reach it
    dense    the 99th percentile of the cells of one window against 500 entries: about 1 % of all cells reach it
Legs:
    segments     occurrence_segments_device alone on the occurrences' keys, lags, counts and the lengths, by device events (and a
                 host clock around the call and the synchronise that ends it)
    lengths      Corpus.entry_lengths_from_keys_device alone on the occurrences' key block, by device events
    occurrences  Corpus.query_packed_occurrences_batch_keys_device alone -- what StreamBank.occurrences costs behind its window
    composite    Corpus.recording_occurrence_segments_batch_keys_device: the three on one stream, its own blocks included
    host         the path the call replaces: keys, lags, lengths and counts read back, decode_occurrence_keys and
                 occurrence_segments per row, by host clock, in 2 rounds (nothing is uploaded again)
Without --shape the tool runs every shape in a CHILD process of its own under its own time limit and stops at the first that
fails; with --shape it is that child.  Median, min and max of `reps` rounds (default 7) in ms, one warm-up round in front.  After
the clock stops the device rows must equal the host path's, every word.  One JSON object per shape, printed and merged into
DIR/occurrence_segments.json (default DIR: profiles) beside the commit the library was built from.
    timeout -k 10 600 python3 tools/prof_occurrence_segments.py 7"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x4F424154
L = 200
CAPACITY = 8192
COMMIT = "c439f6e plus this change"
# name: (windows, sub-fingerprints each, entries, slots per output row, seconds the child may take)
SHAPES = {"monitor": (1024, 256, 2000, 32, 500)}


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
    merged = {"commit": COMMIT}
    for name, shape in SHAPES.items():
        cmd = [sys.executable, os.path.abspath(__file__), str(REPS), "--out", OUT, "--shape", name]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=shape[-1])
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {shape[-1]} s; stopping", flush=True)
            return 124
        if run.returncode != 0:
            print(f"{name}: exit status {run.returncode}; stopping\n{run.stdout[-2000:]}\n{run.stderr[-3000:]}", flush=True)
            return run.returncode
        merged[name] = json.loads(run.stdout.strip().splitlines()[-1])
        print(json.dumps({name: merged[name]}), flush=True)
        with open(os.path.join(OUT, "occurrence_segments.json"), "w") as f:
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
    # the dense threshold: the 99th percentile of one window's cells against the first 500 entries
    sample = lb.Corpus.ragged(L, 500, int(counts[:500].sum()))
    sample.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, 0, counts[:500], L), counts[:500])
    k, _g, c = sample.query_packed_occurrences_keys_device(packed[1], per, 1e-6, 1 << 18, want_lags=False)
    torch.cuda.synchronize()
    cells = np.sort(lb.decode_occurrence_keys(k, None, int(c[0]))[1])
    assert int(c[0]) <= 1 << 18 and len(cells) > 50000
    thresholds = {"planted": 1.0, "dense": float(cells[int(len(cells) * 0.99)])}

    keys = torch.zeros((R, CAPACITY), dtype=torch.int64, device="cuda")
    lags = torch.zeros((R, CAPACITY), dtype=torch.int32, device="cuda")
    occ = torch.zeros(R, dtype=torch.int64, device="cuda")
    lengths = torch.zeros((R, CAPACITY), dtype=torch.int32, device="cuda")
    outs = (torch.zeros((R, cap), dtype=torch.int32, device="cuda"), torch.zeros((R, cap), dtype=torch.int64, device="cuda"),
            torch.zeros((R, cap), dtype=torch.int32, device="cuda"), torch.zeros((R, cap), dtype=torch.int32, device="cuda"),
            torch.zeros(R, dtype=torch.int32, device="cuda"))
    host_rows, composite = [], []

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)

    res = {"recordings": R, "per": per, "entries": entries, "entry_lengths": [20, 70], "capacity": CAPACITY, "out_capacity": cap,
           "peaks": True, "reps": REPS, "thresholds": {}}
    for what, threshold in thresholds.items():
        def leg_occurrences():
            corpus.query_packed_occurrences_batch_keys_device(packed, R, per, threshold, CAPACITY, peaks=True, keys_out=keys, lags_out=lags,
                                                              counts_out=occ)

        def leg_lengths():
            corpus.entry_lengths_from_keys_device(keys, out=lengths)

        def leg_segments():
            lb.occurrence_segments_device(keys, lags, lengths, occ, per, cap, starts_out=outs[0], keys_out=outs[1], lags_out=outs[2],
                                          lengths_out=outs[3], counts_out=outs[4])

        def leg_composite():
            composite[:] = corpus.recording_occurrence_segments_batch_keys_device(packed, R, per, threshold, CAPACITY, cap, peaks=True)

        def leg_host():
            hk, hg, hn, hc = keys.cpu().numpy(), lags.cpu().numpy(), lengths.cpu().numpy(), occ.cpu().numpy()
            host_rows.clear()
            for r in range(R):
                m = min(int(hc[r]), CAPACITY)
                idx, sc, lg = lb.decode_occurrence_keys(hk[r], hg[r], m)
                host_rows.append(lb.occurrence_segments(idx, sc, lg, hn[r, :m], per))

        legs = {"occurrences": leg_occurrences, "lengths": leg_lengths, "segments": leg_segments, "composite": leg_composite,
                "host": leg_host}
        host = {k: [] for k in legs}
        device = {k: [] for k in legs}
        for rep in range(REPS + 1):                                   # (the first round warms every leg up)
            for k, f in legs.items():
                if k == "host" and rep not in (1, 2):           # (seconds a round where the rows are dense; it needs no warm-up)
                    continue
                h, d = timed(f)
                if rep:
                    host[k].append(h)
                    device[k].append(d)
        torch.cuda.synchronize()
        # after the clock: the device rows, the call's and the composite's, are the host path's, every word
        assert all(torch.equal(a, b) for a, b in zip(outs, composite[:5])) and torch.equal(composite[5], occ), "the composite differs"
        st, ks, lg, ln, cn = (x.cpu().numpy() for x in outs)
        hc = occ.cpu().numpy()
        spans = 0
        for r in range(R):
            start, idx, sc, lag, length = host_rows[r]
            m = min(len(start), cap)
            assert cn[r] == len(start), f"window {r}: {cn[r]} spans, the host path has {len(start)}"
            got_idx = 0xFFFFFFFF - (ks[r, :m].view(np.uint64) & np.uint64(0xFFFFFFFF))
            got_sc = (ks[r, :m].view(np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)
            assert np.array_equal(st[r, :m], start[:m]) and np.array_equal(got_idx, idx[:m].astype(np.uint64)), f"window {r} differs"
            assert np.array_equal(got_sc.view(np.uint32), sc[:m].view(np.uint32)) and np.array_equal(lg[r, :m], lag[:m]), f"window {r} differs"
            assert np.array_equal(ln[r, :m].view(np.uint32), length[:m]), f"window {r}: lengths differ"
            assert not st[r, m:].any() and not ks[r, m:].any() and not lg[r, m:].any() and not ln[r, m:].any(), f"window {r}: no zeros"
            spans += len(start)
        one = {"threshold": threshold, "cells": int(np.minimum(hc, CAPACITY).sum()), "largest_row": int(hc.max()),
               "rows_cut": int((hc > CAPACITY).sum()), "spans": spans, "largest_count": int(cn.max()),
               "segments_device_ms": _stats(device["segments"]), "segments_host_clock_ms": _stats(host["segments"]),
               "lengths_device_ms": _stats(device["lengths"]), "occurrences_device_ms": _stats(device["occurrences"]),
               "composite_device_ms": _stats(device["composite"]), "composite_host_clock_ms": _stats(host["composite"]),
               "host_path_ms": _stats(host["host"])}
        one["composite_over_occurrences"] = round(one["composite_device_ms"]["median"] / one["occurrences_device_ms"]["median"], 3)
        one["host_path_over_segments"] = round(one["host_path_ms"]["median"] / one["segments_host_clock_ms"]["median"], 1)
        res["thresholds"][what] = one
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(child(SHAPE) if SHAPE else parent())
