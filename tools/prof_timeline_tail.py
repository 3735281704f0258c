#!/usr/bin/env python3
"""The timeline tail (every channel's timeline kept current from a push) against what a caller runs today, alternating in one
process per shape after warm-up:
    python3 tools/prof_timeline_tail.py [reps] [--out DIR] [--shape NAME]
Shapes (prof_occurrences_tail.py's: synthetic ragged corpora of entries of 20 .. 70 sub-fingerprints of 200 Booleans, random windows
with an entry that ends at the newest sub-fingerprint of each), every window with NEW = 5 new sub-fingerprints:
    small    1 024 windows x 256 sub-fingerprints against 2 000 entries -- a broadcast monitor's, one push a second
    large    1 024 x 256 against 100 000 entries
Thresholds: `planted` (1.0, the planted entries alone) and `dense` (the 99th percentile of the cells of one window against 500
entries, taken from a single occurrences call: about 1 % of the cells count).
Legs (keys and lengths; new counts on the device, max_new = NEW):
    timeline   (a)  Corpus.recording_timeline_batch_keys_device on the windows after the push: what StreamBank.timeline runs behind
                    window_device, every cell of every window again
    best       (b)  Corpus.query_packed_recording_topk_tail_batch_keys_device, K = 1 (StreamBank.new_best): the same new cells without
                    the fold per offset (no threshold: measured once per shape)
    tail_prev  (c)  Corpus.recording_timeline_tail_batch_keys_device with the previous windows' timeline as inPrevKeys
    tail_bare  (c') the same without inPrevKeys
Without --shape the tool runs every shape in a CHILD process of its own under its own time limit, one after the other, and stops
at the first that fails; with --shape it is that child.  Times: device events around each call (and a host clock around the call
and the synchronise that ends it); the median of `reps` rounds (default 5, at least 5) with [min, max] in ms, one warm-up round in
front.  After the clock stops (c)'s keys and lengths must equal (a)'s, bit for bit -- the windows before the push are the windows
after it moved by NEW, and (c)'s previous state is (a) on those --, and (c') must equal (a) wherever (c') holds a key that the
shifted previous state does not beat.
The condition, at both shapes and thresholds: in device time the maximum of (c) lies below the minimum of (a).  The verdict and
the figures are recorded either way; the tool's status is 1 where the condition is missed.  One JSON object per shape, printed and
merged into DIR/timeline_tail.json (default DIR: profiles).
    timeout -k 10 900 python3 tools/prof_timeline_tail.py 5"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x4F544149
L = 200
NEW = 5
LONGEST = 70
# name: (windows, sub-fingerprints each, entries, seconds the child may take)
SHAPES = {"small": (1024, 256, 2000, 300), "large": (1024, 256, 100000, 500)}


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
SHAPE = _option("--shape")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in {OUT, SHAPE}]
REPS = max(5, int(args[0]) if args else 5)


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
        missed = missed or run.returncode                             # (a missed condition is recorded with its figures)
        merged[name] = json.loads(last[0])
        print(json.dumps({name: merged[name]}), flush=True)
        with open(os.path.join(OUT, "timeline_tail.json"), "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")
    return missed


def child(name):
    import numpy as np
    import torch
    import lbaudiodetective_amd as lb

    R, per, entries, _limit = SHAPES[name]
    torch.cuda.set_device(0)
    counts = np.random.default_rng(SEED).integers(20, LONGEST + 1, entries).astype(np.uint32)
    counts[0], counts[1] = 20, LONGEST
    corpus = lb.Corpus.ragged(L, entries, int(counts.sum()))
    corpus.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, 0, counts, L), counts)
    # NEW sub-fingerprints in front of every window: the windows before the push
    long = lb.synth_ragged_corpus_device(SEED + 1, 0, np.array([R * (per + NEW)], np.uint32), L).reshape(R, per + NEW, 32).contiguous()
    # an entry that ends at the newest sub-fingerprint of every window, so that the planted threshold has its matches
    src = lb.synth_ragged_corpus_device(SEED, 0, counts[:64], L)
    off = np.concatenate([[0], np.cumsum(counts[:64])])
    for r in range(R):
        j = r % 64
        long[r, per + NEW - int(counts[j]):] = src[int(off[j]):int(off[j + 1])]
    before = long[:, :per].contiguous()
    packed = long[:, NEW:].contiguous()
    d_new = torch.full((R,), NEW, dtype=torch.int32, device="cuda")
    # the dense threshold: the 99th percentile of one window's cells against the first 500 entries
    sample = lb.Corpus.ragged(L, 500, int(counts[:500].sum()))
    sample.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, 0, counts[:500], L), counts[:500])
    keys, _lags, count = sample.query_packed_occurrences_keys_device(packed[1], per, 1e-6, 1 << 18, want_lags=False)
    torch.cuda.synchronize()
    cells = np.sort(lb.decode_occurrence_keys(keys, None, int(count[0]))[1])
    assert int(count[0]) <= 1 << 18 and len(cells) > 50000
    thresholds = {"planted": 1.0, "dense": float(cells[int(len(cells) * 0.99)])}
    steps = int(counts.astype(np.int64).sum())
    res = {"windows": R, "per": per, "entries": entries, "entry_lengths": [20, LONGEST], "new": NEW, "reps": REPS,
           "plan": lb.debug_timeline_tail_plan(R, per, 20, LONGEST, entries, NEW, 0),
           "best_plan": lb.debug_recording_tail_plan(R, per, LONGEST, entries, NEW, 0, True),
           "timeline_plan": lb.debug_timeline_batch_plan(R, per, 20, LONGEST, entries, 0),
           # cell steps per window, by arithmetic: every offset of every entry, against the NEW newest
           "cell_steps_per_window": {"timeline": int(((per - counts.astype(np.int64) + 1) * counts).sum()), "tail": NEW * steps},
           "thresholds": thresholds, "by_threshold": {}}
    res["cell_steps_ratio"] = round(res["cell_steps_per_window"]["timeline"] / res["cell_steps_per_window"]["tail"], 2)

    def pair():
        return (torch.zeros((R, per), dtype=torch.int64, device="cuda"), torch.zeros((R, per), dtype=torch.int32, device="cuda"))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)

    def measure(legs):
        host = {leg: [] for leg in legs}
        device = {leg: [] for leg in legs}
        for rep in range(REPS + 1):                                   # (the first round warms every leg up)
            for leg, f in legs.items():
                h, d = timed(f)
                if rep:
                    host[leg].append(h)
                    device[leg].append(d)
        torch.cuda.synchronize()
        return {leg: _stats(v) for leg, v in host.items()}, {leg: _stats(v) for leg, v in device.items()}

    best_out = (torch.zeros((R, 1), dtype=torch.int64, device="cuda"), torch.zeros((R, 1), dtype=torch.int32, device="cuda"))
    _h, best = measure({"best": lambda: corpus.query_packed_recording_topk_tail_batch_keys_device(
        packed, R, per, d_new, 1, max_new=NEW, keys_out=best_out[0], lags_out=best_out[1])})
    res["best_device_ms"] = best["best"]
    failed = []
    for what, t in thresholds.items():
        seed, full, rolled, bare = pair(), pair(), pair(), pair()
        corpus.recording_timeline_batch_keys_device(before, R, per, t, keys_out=seed[0], lengths_out=seed[1])
        legs = {
            "timeline": lambda: corpus.recording_timeline_batch_keys_device(packed, R, per, t, keys_out=full[0], lengths_out=full[1]),
            "tail_prev": lambda: corpus.recording_timeline_tail_batch_keys_device(packed, R, per, d_new, t, max_new=NEW, prev_keys=seed[0],
                                                                                  keys_out=rolled[0], lengths_out=rolled[1]),
            "tail_bare": lambda: corpus.recording_timeline_tail_batch_keys_device(packed, R, per, d_new, t, max_new=NEW,
                                                                                  keys_out=bare[0], lengths_out=bare[1]),
        }
        host, device = measure(legs)
        # after the clock: the invariant, bit for bit, and the bare strip inside it
        assert torch.equal(rolled[0], full[0]) and torch.equal(rolled[1], full[1]), f"{what}: the rolled timeline differs from the batch timeline"
        held = bare[0] != 0
        assert bool(held.any()) and bool((bare[0][held] <= full[0][held]).all()), f"{what}: the bare strip is not inside the timeline"
        moved = torch.zeros_like(seed[0])
        moved[:, :per - NEW] = seed[0][:, NEW:]
        assert torch.equal(torch.maximum(moved, bare[0]), full[0]), f"{what}: strip and shifted state do not merge to the timeline"
        row = {"threshold": t, "host_ms": host, "device_ms": device,
               "offsets_with_a_key": int((full[0] != 0).sum()), "offsets_with_a_new_key": int(held.sum()),
               "timeline_over_tail_prev_device": round(device["timeline"]["median"] / device["tail_prev"]["median"], 2),
               "tail_prev_over_best_device": round(device["tail_prev"]["median"] / best["best"]["median"], 3),
               "tail_prev_below_timeline_device": device["tail_prev"]["max"] < device["timeline"]["min"]}
        if not row["tail_prev_below_timeline_device"]:
            failed.append(f"{what}: tail_prev max {device['tail_prev']['max']} is not below timeline min {device['timeline']['min']}")
        res["by_threshold"][what] = row
    res["condition"] = "missed: " + "; ".join(failed) if failed else "met"
    print(json.dumps(res), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(child(SHAPE) if SHAPE else parent())
