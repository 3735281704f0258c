#!/usr/bin/env python3
"""The tail peaks (the peak rule for the cells a push made judgeable) against the live occurrences without peaks and against what a
caller who wants one event per airing runs today, alternating in one process per shape after warm-up:
    python3 tools/prof_occurrences_tail_peaks.py [reps] [--out DIR] [--shape NAME]
Shapes (prof_occurrences_tail.py's: synthetic ragged corpora of entries of 20 .. 70 sub-fingerprints of 200 Booleans, random windows,
here with an entry that ends ONE BEFORE the newest sub-fingerprint of each), every window with NEW = 5 new sub-fingerprints:
    small    1 024 windows x 256 sub-fingerprints against 2 000 entries -- a broadcast monitor's, one push a second
    large    1 024 x 256 against 100 000 entries
Thresholds, at every shape:
    planted  1.0: only the planted entries reach it
    dense    the 99th percentile of the cells of one window against 500 entries: about 1 % of all cells reach it
Legs (keys, lags and counts):
    peaks    (a) Corpus.query_packed_occurrences_tail_peaks_batch_keys_device, final off, new counts on the device, max_new = NEW
             (D = 8 lanes a recording, NEW + 2 cells a pair)
    tail     (b) Corpus.query_packed_occurrences_tail_batch_keys_device on the same windows: the live list WITHOUT the peak rule
    batch    (c) Corpus.query_packed_occurrences_batch_keys_device, peaks on, on the same windows: every older peak again
    short    (d) the same call on the windows cut to 70 + NEW + 1 = 76 sub-fingerprints: today's best workaround
and at `small`, the planted threshold: (a) under max_new = 6 (D = 8) against max_new = 7 (D = 16) with the same new counts -- what
a doubled D costs.
Times: a host clock around the call and the synchronise that ends it, and device events; the median of `reps` rounds (default 5,
at least 5) with [min, max] in ms, one warm-up round in front.  After the clock stops (a)'s rows must equal (c)'s rows with only the
judged cells kept, wherever (c)'s row holds every peak.  No ratio is required: peaks_below_batch / peaks_below_short record whether
(a)'s maximum lies below the other leg's minimum in device time.  One JSON object per shape, printed and merged into
DIR/occurrences_tail_peaks.json (default DIR: profiles); with --shape that one shape runs in this process and is only printed.
Legs (a) and (b) are the two instances of ONE kernel pair (k_occurrences_tail.hip, PEAKS on and off).
    timeout -k 10 900 python3 tools/prof_occurrences_tail_peaks.py 5"""
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
COMMIT = "b2ef2dd plus this change"
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
    merged = {"commit": COMMIT}
    for name, (_r, _p, _e, limit) in SHAPES.items():
        cmd = [sys.executable, os.path.abspath(__file__), str(REPS), "--out", OUT, "--shape", name]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {limit} s; stopping", flush=True)
            return 124
        last = run.stdout.strip().splitlines()[-1:] or [""]
        if run.returncode != 0:
            print(f"{name}: exit status {run.returncode}; stopping\n{run.stdout[-3000:]}\n{run.stderr[-3000:]}", flush=True)
            return run.returncode
        merged[name] = json.loads(last[0])
        print(json.dumps({name: merged[name]}), flush=True)
        with open(os.path.join(OUT, "occurrences_tail_peaks.json"), "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")
    return 0


def _check_rows(np, peaks, batch, lengths, per, what):
    """(a)'s rows against (c)'s with only the judged cells kept, where (c)'s row holds every peak; returns the number of such rows"""
    pk, pl, pc = (x.cpu().numpy() for x in peaks)
    bk, bl, bc = (x.cpu().numpy() for x in batch)
    whole = 0
    for r in range(len(pc)):
        if int(bc[r]) > CAPACITY:
            continue
        whole += 1
        m = int(bc[r])
        k, lag = bk[r, :m].view(np.uint64), bl[r, :m].astype(np.int64)
        last = per - lengths[(0xFFFFFFFF - (k & np.uint64(0xFFFFFFFF))).astype(np.int64)]
        keep = (lag <= 0) & (last >= 0) & (-lag >= last - NEW) & (-lag <= last - 1)
        k, lag = k[keep], lag[keep]
        assert int(pc[r]) == len(k) <= CAPACITY, f"{what}: the count of row {r} differs"
        assert np.array_equal(pk[r, :len(k)].view(np.uint64), k) and np.array_equal(pl[r, :len(k)], lag), f"{what}: row {r} differs"
        assert not pk[r, len(k):].any() and not pl[r, len(k):].any(), f"{what}: row {r} differs"
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
    # an entry that ends one before the newest sub-fingerprint of every window: the newest JUDGED cell, so that the planted
    # threshold has its matches
    src = lb.synth_ragged_corpus_device(SEED, 0, counts[:64], L)
    off = np.concatenate([[0], np.cumsum(counts[:64])])
    for r in range(R):
        j = r % 64
        packed[r, per - 1 - int(counts[j]):per - 1] = src[int(off[j]):int(off[j + 1])]
    short_per = LONGEST + NEW + 1
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
           "short_per": short_per,
           "plan": lb.debug_occurrences_tail_peaks_plan(R, per, 20, LONGEST, entries, NEW, 0),
           "tail_plan": lb.debug_occurrences_tail_plan(R, per, 20, LONGEST, entries, NEW, 0),
           "batch_plan": lb.debug_occurrences_batch_plan(R, per, 20, LONGEST, entries, 0),
           "short_plan": lb.debug_occurrences_batch_plan(R, short_per, 20, LONGEST, entries, 0),
           # cell steps per window, by arithmetic
           "cell_steps_per_window": {"peaks": (NEW + 2) * steps, "tail": NEW * steps, "batch": int(((per - lengths + 1) * lengths).sum()),
                                     "short": int(((short_per - lengths + 1) * lengths).sum())}}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)

    def rounds(legs):
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

    def buffers():
        return (torch.zeros((R, CAPACITY), dtype=torch.int64, device="cuda"), torch.zeros((R, CAPACITY), dtype=torch.int32, device="cuda"),
                torch.zeros(R, dtype=torch.int64, device="cuda"))

    for what, t in thresholds.items():
        out = {leg: buffers() for leg in ("peaks", "tail", "batch", "short")}

        def leg_peaks(max_new=NEW, into="peaks"):
            k, g, c = out[into]
            corpus.query_packed_occurrences_tail_peaks_batch_keys_device(packed, R, per, d_new, t, CAPACITY, max_new=max_new, keys_out=k,
                                                                         lags_out=g, counts_out=c)

        def leg_tail():
            k, g, c = out["tail"]
            corpus.query_packed_occurrences_tail_batch_keys_device(packed, R, per, d_new, t, CAPACITY, max_new=NEW, keys_out=k, lags_out=g,
                                                                   counts_out=c)

        def leg_batch():
            k, g, c = out["batch"]
            corpus.query_packed_occurrences_batch_keys_device(packed, R, per, t, CAPACITY, peaks=True, keys_out=k, lags_out=g, counts_out=c)

        def leg_short():
            k, g, c = out["short"]
            corpus.query_packed_occurrences_batch_keys_device(short, R, short_per, t, CAPACITY, peaks=True, keys_out=k, lags_out=g,
                                                              counts_out=c)

        legs = {"peaks": leg_peaks, "tail": leg_tail, "batch": leg_batch, "short": leg_short}
        host, device = rounds(legs)
        whole = _check_rows(np, out["peaks"], out["batch"], lengths, per, what)
        matches = {leg: out[leg][2].cpu().numpy() for leg in legs}
        if what == "planted":
            assert int(matches["peaks"].min()) >= 1, "every window holds an entry that ends one before its newest sub-fingerprint"
            assert whole == R
        one = {"threshold": t, "batch_rows_uncut": whole,
               "matches_per_window": {leg: {"min": int(m.min()), "median": float(np.median(m)), "max": int(m.max())} for leg, m in matches.items()},
               "host_ms": host, "device_ms": device}
        for clock in ("host_ms", "device_ms"):
            tm = one[clock]
            for leg in ("tail", "batch", "short"):
                one[f"{leg}_over_peaks_{clock[:-3]}"] = round(tm[leg]["median"] / tm["peaks"]["median"], 3)
        tm = one["device_ms"]
        one["peaks_below_batch_device"] = tm["peaks"]["max"] < tm["batch"]["min"]
        one["peaks_below_short_device"] = tm["peaks"]["max"] < tm["short"]["min"]
        if name == "small" and what == "planted":
            # the same new counts under max_new 6 (D = 8) and 7 (D = 16): equal rows, the cost of the doubled D
            out["d8"], out["d16"] = buffers(), buffers()
            h2, d2 = rounds({"d8": lambda: leg_peaks(6, "d8"), "d16": lambda: leg_peaks(7, "d16")})
            for x, y, z in zip(out["d8"], out["d16"], out["peaks"]):
                assert torch.equal(x, y) and torch.equal(x, z), "max_new beyond the clamp changed a row"
            one["doubled_lanes"] = {"lanes": {"max_new_6": lb.debug_occurrences_tail_peaks_plan(R, per, 20, LONGEST, entries, 6, 0)["lanes"],
                                              "max_new_7": lb.debug_occurrences_tail_peaks_plan(R, per, 20, LONGEST, entries, 7, 0)["lanes"]},
                                    "host_ms": h2, "device_ms": d2,
                                    "d16_over_d8_device": round(d2["d16"]["median"] / d2["d8"]["median"], 3)}
        res[what] = one
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(child(SHAPE) if SHAPE else parent())
