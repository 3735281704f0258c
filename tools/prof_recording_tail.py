#!/usr/bin/env python3
"""The recording tail (which entries a push completed, one value per entry) against what a caller runs today, alternating in one
process per shape after warm-up:
    python3 tools/prof_recording_tail.py [reps] [--out DIR] [--shape NAME]
Shapes (prof_occurrences_tail.py's: synthetic ragged corpora of entries of 20 .. 70 sub-fingerprints of 200 Booleans, random windows
with an entry that ends at the newest sub-fingerprint of each), every window with NEW = 5 new sub-fingerprints:
    small    1 024 windows x 256 sub-fingerprints against 2 000 entries -- a broadcast monitor's, one push a second
    large    1 024 x 256 against 100 000 entries
Legs (keys and lags; the threshold is the planted 1.0, rows of CAPACITY = 64 slots):
    topk       (a)  Corpus.query_packed_recording_topk_tail_batch_keys_device, K = 1, new counts on the device, max_new = NEW
    threshold  (a') Corpus.query_packed_recording_threshold_tail_batch_keys_device at 1.0
    tail       (b)  Corpus.query_packed_occurrences_tail_batch_keys_device on the same windows at 1.0: today's cheapest way to learn
                    what a push completed
    short      (c)  Corpus.query_packed_recording_topk_batch_keys_device, K = 1, on the windows cut to 70 + NEW - 1: today's cheapest
                    fixed-size answer
Without --shape the tool runs every shape in a CHILD process of its own under its own time limit, one after the other, and stops
at the first that fails; with --shape it is that child.  Times: device events around each call (and a host clock around the call
and the synchronise that ends it); the median of `reps` rounds (default 5, at least 5) with [min, max] in ms, one warm-up round in
front.  After the clock stops (a')'s rows must equal (b)'s rows folded on the host -- per distinct entry the key of its largest
cell and the lag of the lowest offset that reaches it -- and (a)'s key must be the largest of them.
The condition, at `small` only: in device time the maximum of (a) and of (a') each lie below the minimum of (b) -- less, beyond the
spread of the repeated runs of both legs.  The verdict and the figures are recorded either way; the tool's status is 1 where the
condition is missed.  One JSON object per shape, printed and merged into DIR/recording_tail.json (default DIR: profiles).
    timeout -k 10 900 python3 tools/prof_recording_tail.py 5"""
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
CAPACITY = 64
NEW = 5
LONGEST = 70
THRESHOLD = 1.0
# name: (windows, sub-fingerprints each, entries, seconds the child may take)
SHAPES = {"small": (1024, 256, 2000, 300), "large": (1024, 256, 100000, 400)}


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
        with open(os.path.join(OUT, "recording_tail.json"), "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")
    return missed


def _check_rows(np, topk, threshold, tail):
    """(a')'s rows against (b)'s folded on the host, (a)'s key against the largest of them; returns the entries named per window"""
    ak, al = (x.cpu().numpy() for x in topk)
    tk, tl, tc = (x.cpu().numpy() for x in threshold)
    bk, bl, bc = (x.cpu().numpy() for x in tail)
    assert int(bc.max()) <= CAPACITY and int(tc.max()) <= CAPACITY, "a row is cut: the fold on the host would not be exact"
    named = []
    for r in range(len(tc)):
        best = {}
        for key, lag in zip(bk[r, :int(bc[r])].view(np.uint64).tolist(), bl[r, :int(bc[r])].tolist()):
            j = 0xFFFFFFFF - (key & 0xFFFFFFFF)
            if j not in best or key > best[j][0]:                     # (entry, then offset ascending: the first of equals is the lowest)
                best[j] = (key, lag)
        order = sorted(best)
        m = len(order)
        assert int(tc[r]) == m and tk[r, :m].view(np.uint64).tolist() == [best[j][0] for j in order], f"row {r}: the keys differ"
        assert tl[r, :m].tolist() == [best[j][1] for j in order] and not tk[r, m:].any() and not tl[r, m:].any(), f"row {r}: the lags differ"
        if m:
            top = max(best.values())                                  # the largest key: the highest score, then the lowest index
            assert int(ak[r, 0].view(np.uint64)) == top[0] and int(al[r, 0]) == top[1], f"row {r}: the best entry differs"
        named.append(m)
    return named


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
    packed = lb.synth_ragged_corpus_device(SEED + 1, 0, np.array([R * per], np.uint32), L).reshape(R, per, 32).contiguous()
    # an entry that ends at the newest sub-fingerprint of every window, so that the planted threshold has its matches
    src = lb.synth_ragged_corpus_device(SEED, 0, counts[:64], L)
    off = np.concatenate([[0], np.cumsum(counts[:64])])
    for r in range(R):
        j = r % 64
        packed[r, per - int(counts[j]):] = src[int(off[j]):int(off[j + 1])]
    short_per = LONGEST + NEW - 1
    short = packed[:, per - short_per:].contiguous()
    d_new = torch.full((R,), NEW, dtype=torch.int32, device="cuda")
    res = {"windows": R, "per": per, "entries": entries, "entry_lengths": [20, LONGEST], "new": NEW, "reps": REPS, "capacity": CAPACITY,
           "threshold": THRESHOLD, "k": 1,
           "plan": lb.debug_recording_tail_plan(R, per, LONGEST, entries, NEW, 0, True),
           "tail_plan": lb.debug_occurrences_tail_plan(R, per, 20, LONGEST, entries, NEW, 0),
           "short_plan": lb.debug_recording_batch_plan(R, short_per, 20, LONGEST, entries, 0, True)}

    def keyed(slots, with_counts):
        out = (torch.zeros((R, slots), dtype=torch.int64, device="cuda"), torch.zeros((R, slots), dtype=torch.int32, device="cuda"))
        return out + ((torch.zeros(R, dtype=torch.int64, device="cuda"),) if with_counts else ())

    out = {"topk": keyed(1, False), "threshold": keyed(CAPACITY, True), "tail": keyed(CAPACITY, True), "short": keyed(1, False)}

    def leg_topk():
        k, g = out["topk"]
        corpus.query_packed_recording_topk_tail_batch_keys_device(packed, R, per, d_new, 1, max_new=NEW, keys_out=k, lags_out=g)

    def leg_threshold():
        k, g, c = out["threshold"]
        corpus.query_packed_recording_threshold_tail_batch_keys_device(packed, R, per, d_new, THRESHOLD, CAPACITY, max_new=NEW, keys_out=k,
                                                                       lags_out=g, counts_out=c)

    def leg_tail():
        k, g, c = out["tail"]
        corpus.query_packed_occurrences_tail_batch_keys_device(packed, R, per, d_new, THRESHOLD, CAPACITY, max_new=NEW, keys_out=k, lags_out=g,
                                                               counts_out=c)

    def leg_short():
        k, g = out["short"]
        corpus.query_packed_recording_topk_batch_keys_device(short, R, short_per, 1, keys_out=k, lags_out=g)

    legs = {"topk": leg_topk, "threshold": leg_threshold, "tail": leg_tail, "short": leg_short}

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
    for rep in range(REPS + 1):                                       # (the first round warms every leg up)
        for leg, f in legs.items():
            h, d = timed(f)
            if rep:
                host[leg].append(h)
                device[leg].append(d)
    torch.cuda.synchronize()
    named = _check_rows(np, out["topk"], out["threshold"], out["tail"])
    assert min(named) >= 1, "every window holds an entry that ends at its newest sub-fingerprint"
    # (recorded, not required) the planted entry is the best of the shortened window too: the same key, the lag moved by the cut
    ak, al = (x.cpu().numpy() for x in out["topk"])
    sk, sl = (x.cpu().numpy() for x in out["short"])
    res["short_names_the_same_entry"] = bool(np.array_equal(ak, sk) and np.array_equal(al + (per - short_per), sl))
    res["entries_named_per_window"] = {"min": int(min(named)), "median": float(np.median(named)), "max": int(max(named))}
    res["host_ms"] = {leg: _stats(v) for leg, v in host.items()}
    res["device_ms"] = {leg: _stats(v) for leg, v in device.items()}
    tm = res["device_ms"]
    for leg in ("topk", "threshold"):
        res[f"tail_over_{leg}_device"] = round(tm["tail"]["median"] / tm[leg]["median"], 3)
        res[f"short_over_{leg}_device"] = round(tm["short"]["median"] / tm[leg]["median"], 3)
        res[f"{leg}_below_tail_device"] = tm[leg]["max"] < tm["tail"]["min"]
        res[f"{leg}_below_short_device"] = tm[leg]["max"] < tm["short"]["min"]
    failed = []
    if name == "small":
        failed = [f"{leg} max {tm[leg]['max']} is not below tail min {tm['tail']['min']}" for leg in ("topk", "threshold")
                  if not res[f"{leg}_below_tail_device"]]
    res["condition"] = "missed: " + "; ".join(failed) if failed else ("met" if name == "small" else "none at this shape")
    print(json.dumps(res), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(child(SHAPE) if SHAPE else parent())
