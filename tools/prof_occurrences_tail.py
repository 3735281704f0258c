#!/usr/bin/env python3
"""The tail occurrences (the cells a push completed) against what a caller runs today, alternating in one process per shape after
warm-up:
    python3 tools/prof_occurrences_tail.py [reps] [--out DIR] [--shape NAME]
Shapes (synthetic ragged corpora of entries of 20 .. 70 sub-fingerprints of 200 Booleans, random windows with an entry that ends at
the newest sub-fingerprint of each), every window with NEW = 5 new sub-fingerprints:
    small    1 024 windows x 256 sub-fingerprints against 2 000 entries -- a broadcast monitor's, one push a second
    large    1 024 x 256 against 100 000 entries
Thresholds, at every shape:
    planted  1.0: only the planted entries reach it
    dense    the 99th percentile of the cells of one window against 500 entries, taken from a single occurrences call: about 1 % of
             all cells reach it; the rows of CAPACITY slots are cut where a window has more, the counts stay true
Legs (keys, lags and counts, no peaks):
    tail     (a) Corpus.query_packed_occurrences_tail_batch_keys_device, new counts on the device, max_new = NEW
    batch    (b) Corpus.query_packed_occurrences_batch_keys_device on the same windows: what a caller must run today
    short    (c) the same call on the windows shortened to 70 + NEW - 1 sub-fingerprints: today's best workaround, which still
             computes 70 - n_j + NEW offsets for an entry of n_j and reports the older ones of them again
Without --shape the tool runs every shape in a CHILD process of its own under its own time limit, one after the other, and stops
at the first that fails; with --shape it is that child.  Times: a host clock around the call and the synchronise that ends it, and
device events; the median of `reps` rounds (default 5, at least 5) with [min, max] in ms, one warm-up round in front.  After the
clock stops (a)'s rows must equal (b)'s rows with only the tail cells kept: where (b)'s row holds every match the whole row and the
count, where it was cut at CAPACITY the part that its kept cells determine.
The bar, at `small` only: in device time the maximum of (a) lies below the minimum of (b) at both thresholds -- less, beyond the
spread of the repeated runs; the tool fails otherwise.  tail_below_short records whether (a)'s maximum lies below (c)'s minimum;
it is reported, not required.  One JSON object per shape, printed and merged into DIR/occurrences_tail.json (default DIR:
profiles).
    timeout -k 10 900 python3 tools/prof_occurrences_tail.py 5"""
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
CAPACITY = 8192
NEW = 5
LONGEST = 70
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
        missed = missed or run.returncode                             # (a missed bar is recorded with its figures)
        merged[name] = json.loads(last[0])
        print(json.dumps({name: merged[name]}), flush=True)
        with open(os.path.join(OUT, "occurrences_tail.json"), "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")
    return missed


def _check_rows(np, tail, batch, lengths, per, what):
    """(a)'s rows against (b)'s with only the tail cells kept; returns the rows of (b) that held every match"""
    tk, tl, tc = (x.cpu().numpy() for x in tail)
    bk, bl, bc = (x.cpu().numpy() for x in batch)
    whole = 0
    for r in range(len(tc)):
        m = min(int(bc[r]), CAPACITY)
        k, lag = bk[r, :m].view(np.uint64), bl[r, :m].astype(np.int64)
        n_j = lengths[(0xFFFFFFFF - (k & np.uint64(0xFFFFFFFF))).astype(np.int64)]
        keep = (lag <= 0) & (n_j <= per) & (-lag >= per - n_j - NEW + 1)
        k, lag = k[keep][:CAPACITY], lag[keep][:CAPACITY]
        assert np.array_equal(tk[r, :len(k)].view(np.uint64), k) and np.array_equal(tl[r, :len(k)], lag), f"{what}: row {r} differs"
        if int(bc[r]) <= CAPACITY:                                    # (b) holds every match: the whole row and the count
            whole += 1
            assert int(tc[r]) == int(keep.sum()) and not tk[r, len(k):].any() and not tl[r, len(k):].any(), f"{what}: row {r} differs"
        else:
            assert int(tc[r]) >= len(k), f"{what}: row {r} differs"
    return whole


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
    # the dense threshold: the 99th percentile of one window's cells against the first 500 entries
    sample = lb.Corpus.ragged(L, 500, int(counts[:500].sum()))
    sample.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, 0, counts[:500], L), counts[:500])
    keys, _lags, count = sample.query_packed_occurrences_keys_device(packed[1], per, 1e-6, 1 << 18, want_lags=False)
    torch.cuda.synchronize()
    cells = np.sort(lb.decode_occurrence_keys(keys, None, int(count[0]))[1])
    assert int(count[0]) <= 1 << 18 and len(cells) > 50000
    thresholds = {"planted": 1.0, "dense": float(cells[int(len(cells) * 0.99)])}
    lengths = counts.astype(np.int64)
    steps = int(lengths.sum())
    res = {"windows": R, "per": per, "entries": entries, "entry_lengths": [20, LONGEST], "new": NEW, "reps": REPS, "capacity": CAPACITY,
           "plan": lb.debug_occurrences_tail_plan(R, per, 20, LONGEST, entries, NEW, 0),
           "batch_plan": lb.debug_occurrences_batch_plan(R, per, 20, LONGEST, entries, 0),
           "short_plan": lb.debug_occurrences_batch_plan(R, short_per, 20, LONGEST, entries, 0),
           # cell steps per window, by arithmetic: every offset of every entry, against the NEW newest
           "cell_steps_per_window": {"tail": NEW * steps, "batch": int(((per - lengths + 1) * lengths).sum()),
                                     "short": int(((short_per - lengths + 1) * lengths).sum())}}
    failed = []
    for what, t in thresholds.items():
        out = {leg: (torch.zeros((R, CAPACITY), dtype=torch.int64, device="cuda"), torch.zeros((R, CAPACITY), dtype=torch.int32, device="cuda"),
                     torch.zeros(R, dtype=torch.int64, device="cuda")) for leg in ("tail", "batch", "short")}

        def leg_tail():
            k, g, c = out["tail"]
            corpus.query_packed_occurrences_tail_batch_keys_device(packed, R, per, d_new, t, CAPACITY, max_new=NEW, keys_out=k, lags_out=g,
                                                                   counts_out=c)

        def leg_batch():
            k, g, c = out["batch"]
            corpus.query_packed_occurrences_batch_keys_device(packed, R, per, t, CAPACITY, peaks=False, keys_out=k, lags_out=g, counts_out=c)

        def leg_short():
            k, g, c = out["short"]
            corpus.query_packed_occurrences_batch_keys_device(short, R, short_per, t, CAPACITY, peaks=False, keys_out=k, lags_out=g,
                                                              counts_out=c)

        legs = {"tail": leg_tail, "batch": leg_batch, "short": leg_short}

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
        whole = _check_rows(np, out["tail"], out["batch"], lengths, per, what)
        matches = {leg: out[leg][2].cpu().numpy() for leg in legs}
        if what == "planted":
            assert int(matches["tail"].min()) >= 1, "every window holds an entry that ends at its newest sub-fingerprint"
        one = {"threshold": t, "batch_rows_uncut": whole,
               "matches_per_window": {leg: {"min": int(m.min()), "median": float(np.median(m)), "max": int(m.max())} for leg, m in matches.items()},
               "host_ms": {leg: _stats(v) for leg, v in host.items()}, "device_ms": {leg: _stats(v) for leg, v in device.items()}}
        for clock in ("host_ms", "device_ms"):
            tm = one[clock]
            one[f"batch_over_tail_{clock[:-3]}"] = round(tm["batch"]["median"] / tm["tail"]["median"], 3)
            one[f"short_over_tail_{clock[:-3]}"] = round(tm["short"]["median"] / tm["tail"]["median"], 3)
            one[f"tail_below_short_{clock[:-3]}"] = tm["tail"]["max"] < tm["short"]["min"]
        if name == "small":
            tm = one["device_ms"]
            if not tm["tail"]["max"] < tm["batch"]["min"]:
                failed.append(f"{what}: tail max {tm['tail']['max']} is not below batch min {tm['batch']['min']}")
        res[what] = one
    res["bar"] = "missed: " + "; ".join(failed) if failed else ("met" if name == "small" else "none at this shape")
    print(json.dumps(res), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(child(SHAPE) if SHAPE else parent())
