#!/usr/bin/env python3
"""The batch occurrences and the batch recording threshold against the loops of single calls they replace, alternating in one
process per shape after warm-up:
    python3 tools/prof_occurrences_batch.py [reps] [--out DIR] [--shape NAME]
Shapes (synthetic ragged corpora of entries of 20 .. 70 sub-fingerprints of 200 Booleans, random recordings with a piece of an
entry in each):
    small    1 024 channels x 256 sub-fingerprints against 2 000 entries -- a broadcast monitor's
    large    1 024 x 256 against 100 000 entries
Thresholds, at every shape:
    planted  1.0: only the planted pieces reach it -- one match per recording and planted entry
    dense    the 99th percentile of the cells of one recording against 500 entries, taken from a single occurrences call: about
             1 % of all cells reach it; the rows of CAPACITY slots are cut where a recording has more, the counts stay true
Legs of the occurrences (peaks only, keys, lags and counts):
    batch    (a) Corpus.query_packed_occurrences_batch_keys_device as the plan takes it (form W at 1 024 x 256)
    batch_s  (b) the same with form S forced (LBAudioDetectiveDebugSetOccurrencesBatchForm), where the plan takes form W
    loop     (c) the loop of single calls, one Corpus.query_packed_occurrences_keys_device per recording
Legs of the recording threshold (keys, counts and aligned lags):
    tbatch   (d) Corpus.query_packed_recording_threshold_batch_keys_device
    tloop    (e) the loop of single calls, one Corpus.query_packed_recording_threshold_keys_device per recording
Without --shape the tool runs every shape in a CHILD process of its own under its own time limit, one after the other, and stops
at the first that fails; with --shape it is that child.  Times: a host clock around the calls and the synchronise that ends them,
and device events; the median of `reps` rounds (default 7, at least 5) with [min, max] in ms, one warm-up round in front.  After
the clock stops every batch leg's keys, lags and counts must equal its loop's bit for bit.
The bar, at `small` only: in device time the maximum of (a) lies below the minimum of (c), and the maximum of (d) below the
minimum of (e), at both thresholds -- less, beyond the spread of the repeated runs; the tool fails otherwise.  keep_form_w records
whether (a)'s maximum lies below (b)'s minimum.  One JSON object per shape, printed and merged into DIR/occurrences_batch.json
(default DIR: profiles).
    timeout -k 10 1100 python3 tools/prof_occurrences_batch.py 7"""
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
# name: (recordings, sub-fingerprints each, entries, seconds the child may take)
SHAPES = {"small": (1024, 256, 2000, 300), "large": (1024, 256, 100000, 700)}


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
        with open(os.path.join(OUT, "occurrences_batch.json"), "w") as f:
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
    # a piece of an entry in every recording, so that the planted threshold has its matches
    src = lb.synth_ragged_corpus_device(SEED, 0, counts[:64], L)
    off = np.concatenate([[0], np.cumsum(counts[:64])])
    for r in range(R):
        j = r % 64
        packed[r, 5:5 + int(counts[j])] = src[int(off[j]):int(off[j + 1])]
    # the dense threshold: the 99th percentile of one recording's cells against the first 500 entries
    sample = lb.Corpus.ragged(L, 500, int(counts[:500].sum()))
    sample.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, 0, counts[:500], L), counts[:500])
    keys, _lags, count = sample.query_packed_occurrences_keys_device(rows[1], per, 1e-6, 1 << 18, want_lags=False)
    torch.cuda.synchronize()
    cells = np.sort(lb.decode_occurrence_keys(keys, None, int(count[0]))[1])
    assert int(count[0]) <= 1 << 18 and len(cells) > 50000
    thresholds = {"planted": 1.0, "dense": float(cells[int(len(cells) * 0.99)])}
    plan = lb.debug_occurrences_batch_plan(R, per, 20, 70, entries, 0)
    res = {"recordings": R, "per": per, "entries": entries, "entry_lengths": [20, 70], "reps": REPS, "capacity": CAPACITY, "peaks": True,
           "plan": plan, "threshold_plan": lb.debug_recording_batch_plan(R, per, 20, 70, entries, 0, True)}
    failed = []
    for what, t in thresholds.items():
        out = {leg: (torch.zeros((R, CAPACITY), dtype=torch.int64, device="cuda"), torch.zeros((R, CAPACITY), dtype=torch.int32, device="cuda"),
                     torch.zeros(R, dtype=torch.int64, device="cuda")) for leg in ("batch", "batch_s", "loop", "tbatch", "tloop")}

        def leg_batch(which):
            lb.debug_set_occurrences_batch_form(which == "batch_s")
            try:
                corpus.query_packed_occurrences_batch_keys_device(packed, R, per, t, CAPACITY, peaks=True, keys_out=out[which][0],
                                                                  lags_out=out[which][1], counts_out=out[which][2])
            finally:
                lb.debug_set_occurrences_batch_form(False)

        def leg_loop():
            k, g, c = out["loop"]
            for r in range(R):
                corpus.query_packed_occurrences_keys_device(rows[r], per, t, CAPACITY, peaks=True, keys_out=k[r], lags_out=g[r],
                                                            count_out=c[r:r + 1])

        def leg_tbatch():
            k, g, c = out["tbatch"]
            corpus.query_packed_recording_threshold_batch_keys_device(packed, R, per, t, CAPACITY, keys_out=k, lags_out=g, counts_out=c)

        def leg_tloop():
            k, g, c = out["tloop"]
            for r in range(R):
                corpus.query_packed_recording_threshold_keys_device(rows[r], per, t, CAPACITY, keys_out=k[r], lags_out=g[r],
                                                                    count_out=c[r:r + 1])

        legs = {"batch": lambda: leg_batch("batch")}
        if plan["form"] == 1:
            legs["batch_s"] = lambda: leg_batch("batch_s")
        legs["loop"] = leg_loop
        legs["tbatch"] = leg_tbatch
        legs["tloop"] = leg_tloop

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
        for leg, base in (("batch", "loop"), ("batch_s", "loop"), ("tbatch", "tloop")):
            if leg in legs:
                assert all(torch.equal(out[leg][i], out[base][i]) for i in range(3)), f"{what}: {leg} differs from {base}"
        matches = out["batch"][2].cpu().numpy()
        entries_above = out["tbatch"][2].cpu().numpy()
        if what == "planted":
            want = 1                                                  # the planted entry of every recording, at offset 5
            assert int(matches.min()) >= want and bool((out["batch"][1][:, 0] == -5).all()), "every recording holds a piece at offset 5"
        one = {"threshold": t, "matches_per_recording": {"min": int(matches.min()), "median": float(np.median(matches)), "max": int(matches.max())},
               "entries_per_recording": {"min": int(entries_above.min()), "median": float(np.median(entries_above)), "max": int(entries_above.max())},
               "host_ms": {leg: _stats(v) for leg, v in host.items()}, "device_ms": {leg: _stats(v) for leg, v in device.items()}}
        for clock in ("host_ms", "device_ms"):
            tm = one[clock]
            one[f"loop_over_batch_{clock[:-3]}"] = round(tm["loop"]["median"] / tm["batch"]["median"], 3)
            one[f"tloop_over_tbatch_{clock[:-3]}"] = round(tm["tloop"]["median"] / tm["tbatch"]["median"], 3)
            if "batch_s" in tm:
                one[f"batch_s_over_batch_{clock[:-3]}"] = round(tm["batch_s"]["median"] / tm["batch"]["median"], 3)
                one[f"keep_form_w_{clock[:-3]}"] = tm["batch"]["max"] < tm["batch_s"]["min"]
        if name == "small":
            tm = one["device_ms"]
            for a, c in (("batch", "loop"), ("tbatch", "tloop")):
                if not tm[a]["max"] < tm[c]["min"]:
                    failed.append(f"{what}: {a} max {tm[a]['max']} is not below {c} min {tm[c]['min']}")
        res[what] = one
    res["bar"] = "missed: " + "; ".join(failed) if failed else ("met" if name == "small" else "none at this shape")
    print(json.dumps(res), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(child(SHAPE) if SHAPE else parent())
