#!/usr/bin/env python3
"""Randomized GPU-vs-numpy sweep of the recording family: tools/fuzz_recording.py [trials] [seed] [--plan-only] [--only T].
The seven kernel files on occurrences_common.hpp's pair loop (k_occurrences, k_recording, k_timeline, their three batch forms and
k_segments) and the three host plans behind them, every output word against tests/recording_ref.py -- folds of align_ref.profile's
cells, never another device call.  A trial draws SEVERAL axes at once: sub-fingerprint lengths 1..200 (odd ones, both sides of the
word edges), every kind of range, corpora of 1..200 entries on both sides of 64 and 128 (fuzz_ragged.py's length distributions, a
rare entry of 300 and of exactly the cap of 1024; appended in two pieces; duplicated entries, an all-zero entry, an entry of one
repeated sub-fingerprint, empty sub-fingerprints, 11 pairs), 1..9 recordings of one length from 1 to 1 100 (one, two to three,
exactly four, five and more tiles of 126 offsets; 378 | 379 where form W ends, 504 | 505 where the second tile group begins; some
recordings equal, one all zero), entries planted into recordings (verbatim and noisy, twice back to back, at two offsets, at the
first and last offset of a tile and of the recording, runs of the repeated sub-fingerprint) and a recording planted into a longer
entry (case A), thresholds that are values of the reference's own cells (so ties at the threshold are exact), capacities of 1,
count - 1, count, count + 1 and more, k of 1 .. 1024, an index base of 0, below 2^20 or the largest legal, a grid ceiling of 0..3,
form S forced per batch family, and a join scratch limit that makes one recording take two entry chunks or a batch two passes.
The recordings of a batch, then the entries, are cut back where the numpy reference of a trial would take more than BUDGET steps.
Every trial makes all of these calls: the packed occurrences (all cells, peaks), the recording scores, top-K and threshold, the
timeline, the segments of that timeline, and the batch form of each; every third trial also the fingerprint-handle forms.  Keys
as 64-bit integers, lags, lengths, starts and counts exactly, scores as float bit patterns; every output buffer is poison-filled
and carries slack words behind it that must stay poison.  A library or HIP error ends the run.  Every trial has a generator of
its own (seed, trial), so --only T replays trial T alone; --plan-only runs the generator and the reference without a device
and prints how many trials land in each path bucket (tests/test_fuzz_recording_cpu.py holds those counts up).
Every trial also makes the LIVE PEAKS call (k_occurrences_tail.hip's PEAKS instances) on its batch of recordings: new counts of
0 .. above the bound, a bound of 1 .. 62 (every width D of 4 .. 64 lanes), final on or off, the batch occurrences' threshold, a
capacity around the reference's counts -- against recording_ref's peaks-on list with only the judged cells kept (expected_live).  Its axes are
drawn LAST from the trial's generator, so every other draw of a trial is what it was before the call existed.

The suite runs 200 trials with seed 20261002 (tests/test_gpu_parity.py).  Wall times on an MI355X machine, process start to exit:
fuzz_ragged.py 400 20261002 takes 21.1 s (21.09 and 21.18 in two runs); this tool takes 6.3 s for 50 trials, 9.9 s for 100, 17.7 s
for 200, 21.3 s for 250 and 26.0 s for 300 -- about 0.07 s a trial, five sixths of it the numpy reference -- so 200 is the largest
multiple of 50 that stays below the ragged sweep (measured before the live peaks call joined the trials; it adds one call and one
filter of a list the reference has already made).  The long runs are recorded in profiles/fuzz_recording.txt and, with the live
peaks call, profiles/fuzz_recording_live_peaks.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import lbaudiodetective_amd as lb
import recording_ref as ref

TILE, BLOCK = 126, 64                            # kOcTile, kOcEntries
ENTRY_CAP = 1024                                 # LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS
L_VALUES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 199, 200)    # (a ragged corpus takes no length above 200)
PER_VALUES = (1, 1, 2, 17, 60, 100, 125, 126, 127, 200, 251, 252, 253, 300, 378, 379, 380, 440, 503, 504, 505, 506, 630, 700, 1100)
BUDGET = 10000                                   # profile steps, weighted by the recording's length, a trial's reference may take
FAMILIES = ("occurrences", "recording", "timeline")
POISON, POISON32, SLACK = -0x0123456789ABCDEF, 0x5A5A5A5A, 5
LIVE_MAX_NEW = (1, 2, 5, 6, 7, 8, 14, 30, 31, 62)   # the live peaks' bound: 4, 4, 8, 8, 16, 16, 16, 32, 64 and 64 lanes a recording


def rand_fp(rng, n, L, p_zero, p_both):
    pairs = (L + 1) // 2
    pos = rng.random((n, pairs)) < 0.5
    zero = rng.random((n, pairs)) < p_zero
    both = rng.random((n, pairs)) < p_both
    f = np.zeros((n, 2 * pairs), np.uint8)
    f[:, 0::2] = (pos & ~zero) | both
    f[:, 1::2] = (~pos & ~zero) | both
    return np.ascontiguousarray(f[:, :L])


def pack(bools):
    """[n, L] Booleans -> [n, 32] bytes, Boolean i at bit i & 7 of byte i >> 3 (lb.pack_subfingerprint's layout)"""
    b = np.asarray(bools, np.uint8)
    full = np.zeros((b.shape[0], 256), np.uint8)
    full[:, :b.shape[1]] = b
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little"))


def _lengths(rng, n):
    shape = int(rng.integers(0, 5))
    if shape == 0:
        lens = rng.integers(1, 12, n)
    elif shape == 1:
        lens = rng.integers(40, 91, n)
    elif shape == 2:
        lens = rng.integers(1, 91, n)
    elif shape == 3:
        lens = np.full(n, int(rng.integers(1, 40)))
    else:
        lens = rng.integers(1, 30, n)
        lens[rng.integers(0, n)] = 300
    if rng.integers(0, 12) == 0:
        lens[rng.integers(0, n)] = ENTRY_CAP
    return lens.astype(np.int64)


def _weight(lens, per):
    return int(np.minimum(lens, per).sum() * (1.0 + per / 500.0))


def _plant(rng, rec, entries, constant):
    """entries planted into one recording (in place)"""
    per = len(rec)
    fits = [j for j, e in enumerate(entries) if len(e) <= per]
    for _ in range(int(rng.integers(0, 4))):
        if not fits:
            return
        j = constant if (constant in fits and rng.integers(0, 3) == 0) else fits[int(rng.integers(0, len(fits)))]
        e = entries[j]
        m = len(e)
        edges = [o for o in (0, per - m, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 3 * TILE - 1, 3 * TILE, 4 * TILE - 1, 4 * TILE)
                 if 0 <= o <= per - m]
        o = edges[int(rng.integers(0, len(edges)))] if rng.integers(0, 2) else int(rng.integers(0, per - m + 1))
        src = e.copy()
        if rng.integers(0, 3) == 0:                                          # a noisy copy
            src ^= (rng.random(src.shape) < 0.03).astype(np.uint8)
        kind = int(rng.integers(0, 4))
        if j == constant and per >= m + 1:                                   # a run of the repeated sub-fingerprint: overlapping 1.0s
            run = min(per, m + int(rng.integers(1, 4)))
            o = min(o, per - run)
            rec[o:o + run] = e[0]
        elif kind == 0 and o + 2 * m <= per:                                 # twice back to back: plateaus, adjacent peaks
            rec[o:o + m] = src
            rec[o + m:o + 2 * m] = src
        elif kind == 1 and 2 * m <= per:                                     # at two offsets: a tie for the lag
            rec[o:o + m] = src
            o2 = int(rng.integers(0, per - m + 1))
            if abs(o2 - o) >= m:
                rec[o2:o2 + m] = src
        else:
            rec[o:o + m] = src


def _threshold(rng, values):
    """a value of the reference's own cells (> 0, as the calls demand), or the next float above the largest"""
    v = np.sort(np.asarray(values, np.float32).reshape(-1))
    v = v[v > 0]
    if len(v) == 0:
        return np.float32(0.5)
    distinct = np.unique(v)
    kind = rng.choice(5, p=[0.2, 0.08, 0.27, 0.25, 0.2])
    if kind == 0:
        t = v[-1]
    elif kind == 1:
        t = np.nextafter(v[-1], np.float32(np.inf))
    elif kind == 2:
        t = distinct[-min(len(distinct), int(rng.integers(2, 6)))]
    elif kind == 3:
        t = v[len(v) // 2]
    else:
        t = v[len(v) // 10]
    return np.float32(t)


def _capacity(rng, lo, hi):
    return max(1, int(rng.choice([1, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, hi + 100])))


def _plans(R, per, lens, limit):
    """family -> (batch plan, single plan); None where the call takes none (the timeline with no entry inside the recording)"""
    lo, hi, n = int(lens.min()), int(lens.max()), len(lens)
    out = {}
    for R_ in (R, 1):
        out.setdefault("occurrences", []).append(lb.debug_occurrences_batch_plan(R_, per, lo, hi, n, limit["occurrences"]))
        out.setdefault("recording", []).append(lb.debug_recording_batch_plan(R_, per, lo, hi, n, limit["recording"]))
        lb.debug_recording_batch_plan(R_, per, lo, hi, n, limit["recording"], key_form=True)       # (raises where refused)
        lb.debug_recording_batch_plan(R_, per, lo, hi, n, limit["occurrences"], key_form=True)     # (the batch threshold's)
        out.setdefault("timeline", []).append(lb.debug_timeline_batch_plan(R_, per, lo, hi, n, limit["timeline"]) if lo <= per else None)
    return out


def _limits(rng, R, per, lens):
    """the join scratch limit per family: 0, or one the plan accepts under which ONE recording takes at least two entry chunks,
    or a batch at least two passes -- taken from the plan at the default"""
    n = len(lens)
    zero = {f: 0 for f in FAMILIES}
    mode = int(rng.choice(3, p=[0.4, 0.35, 0.25]))                           # 0: the default; 1: chunks; 2: passes
    if mode == 0:
        return zero
    chunks = mode == 1 and n > BLOCK                                         # (a corpus of one block has no second chunk: passes)
    default = _plans(R, per, lens, zero)
    out = dict(zero)
    for fam in FAMILIES:
        d = default[fam][0]
        if d is None or d["recordings_per_pass"] == 0:
            continue
        one = d["scratch_bytes"] // d["recordings_per_pass"]
        tries = [int(one * f) for f in (0.6, 0.4, 0.8, 0.25)] if chunks else [one * max(1, R // 2)] if R >= 2 else []
        for limit in tries:
            trial = dict(zero)
            trial[fam] = limit
            try:
                p = _plans(R, per, lens, trial)[fam]
            except lb.LBAudioDetectiveError:
                continue
            if p[1]["entries_per_chunk"] < n if chunks else p[0]["recordings_per_pass"] < R:
                out[fam] = limit
                break
    return out


def make_trial(rng):
    """one trial as a plain dict: the inputs, every call's arguments, the reference's cells (`cells`: per recording, equal
    recordings share one list) and the path buckets the trial lands in (`paths`).  Needs no GPU."""
    L = int(rng.choice(L_VALUES))
    if rng.integers(0, 3) == 0:
        n = int(rng.choice([1, 2, 63, 64, 65, 127, 128, 129, 200]))
    else:
        lo, hi = ((1, 65), (65, 129), (129, 201))[int(rng.integers(0, 3))]
        n = int(rng.integers(lo, hi))
    lens = _lengths(rng, n)
    per = int(rng.choice(PER_VALUES))
    if rng.integers(0, 7) == 0:
        per = int(min(lens[rng.integers(0, n)], 1100))                       # an entry of exactly the recording's length
    R = int(rng.integers(1, 10))
    R = max(1, min(R, BUDGET // max(1, _weight(lens, per))))
    while _weight(lens, per) > BUDGET and n > 1:                             # (one recording alone is too much: fewer entries)
        n = n * 3 // 4
        lens = lens[:n]
    p_zero, p_both = float(rng.choice([0.0, 0.02, 0.3])), float(rng.choice([0.0, 0.0, 0.05]))
    entries = [rand_fp(rng, int(k), L, p_zero, p_both) for k in lens]
    for _ in range(int(rng.integers(0, 4))):                                 # duplicates: ties between entries
        i, j = int(rng.integers(0, n)), int(rng.integers(0, n))
        entries[j] = entries[i].copy()
    if rng.integers(0, 4) == 0:
        entries[int(rng.integers(0, n))][:] = 0
    constant = -1
    if rng.integers(0, 2) == 0:                                              # one sub-fingerprint repeated
        constant = int(rng.integers(0, n))
        entries[constant][:] = rand_fp(rng, 1, L, 0.0, 0.0)[0]
    recordings = [rand_fp(rng, per, L, p_zero, p_both) for _ in range(R)]
    for rec in recordings:
        _plant(rng, rec, entries, constant)
    single = int(rng.integers(0, R))
    if R >= 2 and rng.integers(0, 3) == 0:                                   # two equal recordings
        i, j = (int(x) for x in rng.choice(R, 2, replace=False))
        recordings[j] = recordings[i].copy()
    if R >= 2 and rng.integers(0, 3) == 0:                                   # one all zero (not the single calls' one)
        recordings[(single + 1 + int(rng.integers(0, R - 1))) % R][:] = 0
    longer = [j for j, e in enumerate(entries) if len(e) > per]
    if longer and rng.integers(0, 2) == 0:                                   # case A: a recording inside a longer entry
        e = entries[longer[int(rng.integers(0, len(longer)))]]
        at = int(rng.choice([0, len(e) - per, int(rng.integers(0, len(e) - per + 1))]))
        e[at:at + per] = recordings[single]
        if len(e) >= 2 * per and rng.integers(0, 2) == 0:                    # ... twice: a tie for the lag in case A
            at2 = at + per if at + 2 * per <= len(e) else at - per
            if at2 >= 0:
                e[at2:at2 + per] = recordings[single]
    lens = np.array([len(e) for e in entries], np.int64)
    range_ = int(rng.choice([0, 1, 2, L // 2 + 1, L - 1, L, L + 7]))

    made, cells = {}, []
    for rec in recordings:                                                   # the costly half, once per distinct recording
        key = rec.tobytes()
        if key not in made:
            made[key] = ref.cells(rec, entries, range_)
        cells.append(made[key])

    rows, one = range(R), cells[single]
    inside = lambda cs: [q for q, entry_long in cs if not entry_long] or [np.zeros(1, np.float32)]
    thresholds = {
        "occurrences": _threshold(rng, np.concatenate([q for q, _ in one])),
        "occurrences_batch": _threshold(rng, np.concatenate([q for r in rows for q, _ in cells[r]])),
        "threshold": _threshold(rng, ref.scores(one)[0]),
        "threshold_batch": _threshold(rng, np.concatenate([ref.scores(cells[r])[0] for r in rows])),
        "timeline": _threshold(rng, np.concatenate(inside(one))),
        "timeline_batch": _threshold(rng, np.concatenate([q for r in rows for q in inside(cells[r])])),
    }
    index_base = int(rng.choice([0, int(rng.integers(1, 1 << 20)), (1 << 32) - n]))
    counts = {
        "occurrences": [len(ref.occurrences_all(one, thresholds["occurrences"], False)[0])],
        "occurrences_peaks": [len(ref.occurrences_all(one, thresholds["occurrences"], True)[0])],
        "threshold": [ref.threshold(one, thresholds["threshold"], 1)[2]],
        "segments": [ref.segments(*ref.timeline(one, per, thresholds["timeline"]), 1)[3]],
        "occurrences_batch": [len(ref.occurrences_all(cells[r], thresholds["occurrences_batch"], False)[0]) for r in rows],
        "occurrences_peaks_batch": [len(ref.occurrences_all(cells[r], thresholds["occurrences_batch"], True)[0]) for r in rows],
        "threshold_batch": [ref.threshold(cells[r], thresholds["threshold_batch"], 1)[2] for r in rows],
        "segments_batch": [ref.segments(*ref.timeline(cells[r], per, thresholds["timeline_batch"]), 1)[3] for r in rows],
    }
    capacities = {name: _capacity(rng, min(c), max(c)) for name, c in counts.items()}
    k = int(rng.choice([1, 2, 10, n, n + 3, 1024]))
    grid_ceiling = int(rng.choice([0, 1, 2, 3]))
    force_shared = {fam: bool(rng.integers(0, 3) == 0) for fam in FAMILIES}
    scratch_limit = _limits(rng, R, per, lens)

    paths = set()
    for fam, (b, s) in _plans(R, per, lens, scratch_limit).items():
        if b is None:
            continue
        paths.add(f"{fam}:form_s" if b["form"] == 0 else f"{fam}:form_s_forced" if force_shared[fam] else f"{fam}:form_w")
        if b["recordings_per_pass"] < R:
            paths.add(f"{fam}:passes")
        if s["entries_per_chunk"] < n:
            paths.add(f"{fam}:chunks")
        t = b["tiles"]
        paths.add(f"{fam}:tiles_" + ("1" if t == 1 else "2_3" if t < 4 else "4" if t == 4 else "5_up"))
    paths.add("entries_to_64" if n <= 64 else "entries_65_128" if n <= 128 else "entries_above_128")
    positive = [int((ref.scores(cells[r])[0] > 0).sum()) for r in rows]
    timeline_counts = [int(np.count_nonzero(ref.timeline(one, per, thresholds["timeline"])[0]))] + \
        [int(np.count_nonzero(ref.timeline(cells[r], per, thresholds["timeline_batch"])[0])) for r in rows]
    for name, hit in (("case_a", bool((lens > per).any())), ("equal_length", bool((lens == per).any())), ("per_1", per == 1),
                      ("odd_L", L % 2 == 1), ("range_below_L", 0 < range_ < L), ("range_at_or_above_L", range_ >= L),
                      ("grid_ceiling_1", grid_ceiling == 1), ("index_base", index_base != 0),
                      ("capacity_cuts", any(capacities[x] < max(c) for x, c in counts.items())),
                      ("capacity_exact", any(capacities[x] in c and capacities[x] > 0 for x, c in counts.items())),
                      ("batch_empty_row", any(min(counts[x]) == 0 < max(counts[x]) for x in counts if x.endswith("_batch"))),
                      ("k_above_positive", k > min(positive)),
                      ("all_empty", not any(max(c) for c in counts.values()) and not any(timeline_counts))):
        if hit:
            paths.add(name)
    # the live peaks call, drawn last: per recording a new count (0, 1, the bound, above it, anything up to it), final or not
    max_new = int(rng.choice(LIVE_MAX_NEW))
    live = {"max_new": max_new, "final": bool(rng.integers(0, 2)),
            "new": [int(rng.choice([0, 1, max_new, max_new + 3, int(rng.integers(0, max_new + 1))])) for _ in rows]}
    found = [live_peaks(cells[r], lens, per, min(live["new"][r], max_new, per), live["final"], thresholds["occurrences_batch"], None, 0)[2]
             for r in rows]
    live["capacity"] = _capacity(rng, min(found), max(found))
    return {"live": live, "L": L, "entries": entries, "recordings": recordings, "single": single, "cut": int(rng.integers(0, n + 1)), "range": range_,
            "thresholds": thresholds, "capacities": capacities, "k": k, "index_base": index_base, "peaks": (False, True),
            "scratch_limit": scratch_limit, "grid_ceiling": grid_ceiling, "force_shared": force_shared, "handles": False,
            "cells": cells, "paths": sorted(paths)}


def expected(trial, only=None):
    """name -> tuple of arrays: what every call of the trial must write, from recording_ref alone"""
    cells, one = trial["cells"], trial["cells"][trial["single"]]
    per, k, base = len(trial["recordings"][0]), trial["k"], trial["index_base"]
    ts, cap = trial["thresholds"], trial["capacities"]

    def timeline(cs, t):
        return ref.timeline(cs, per, t, base)

    makers = {
        "occurrences": lambda cs, b: ref.occurrences(cs, ts["occurrences" + b], False, cap["occurrences" + b], base),
        "occurrences_peaks": lambda cs, b: ref.occurrences(cs, ts["occurrences" + b], True, cap["occurrences_peaks" + b], base),
        "scores": lambda cs, b: ref.scores(cs),
        "topk": lambda cs, b: ref.topk(cs, k, base),
        "threshold": lambda cs, b: ref.threshold(cs, ts["threshold" + b], cap["threshold" + b], base),
        "timeline": lambda cs, b: timeline(cs, ts["timeline" + b]),
        "segments": lambda cs, b: ref.segments(*timeline(cs, ts["timeline" + b]), cap["segments" + b]),
    }
    out = {}
    for name, make in makers.items():
        if only is None or name in only:
            out[name] = tuple(np.asarray(x) for x in make(one, ""))
            out[name + "_batch"] = ref.batch([make(cs, "_batch") for cs in cells])
    return out


def live_peaks(cs, lens, per, d, final, t, capacity, base):
    """one row of the live peaks call: recording_ref's peaks-on list with only the judged cells kept -- the entries not longer
    than the recording, the offsets max(0, last - d) .. last - 1, with `final` .. last, last = per - the entry's length -- as
    (keys, lags, true count), cut at `capacity` (None: the whole list)"""
    keys, lags = ref.occurrences_all(cs, t, True, base)
    n_j = np.asarray(lens, np.int64)[(ref.LOW - (keys & np.uint64(ref.LOW))).astype(np.int64) - base]
    last, o = per - n_j, -lags.astype(np.int64)
    keep = (n_j <= per) & (lags <= 0) & (o >= last - d) & (o <= (last if final else last - 1))
    keys, lags = keys[keep], lags[keep]
    if capacity is None:
        return keys, lags, len(keys)
    return (*ref._cut(capacity, keys, lags), len(keys))


def expected_live(trial):
    """name -> tuple of arrays: what the live peaks call of the trial must write, from recording_ref alone"""
    per, lv = len(trial["recordings"][0]), trial["live"]
    lens = [len(e) for e in trial["entries"]]
    return {"live_peaks_batch": ref.batch([live_peaks(cs, lens, per, min(d, lv["max_new"], per), lv["final"],
                                                      trial["thresholds"]["occurrences_batch"], lv["capacity"], trial["index_base"])
                                           for cs, d in zip(trial["cells"], lv["new"])])}


def describe(trial):
    lens = [len(e) for e in trial["entries"]]
    return (f"L {trial['L']} range {trial['range']} entries {len(lens)} of {min(lens)}..{max(lens)} recordings {len(trial['recordings'])} x "
            f"{len(trial['recordings'][0])} single {trial['single']} base {trial['index_base']} k {trial['k']} grid {trial['grid_ceiling']} "
            f"force {trial['force_shared']} limit {trial['scratch_limit']} thresholds { {a: float(b) for a, b in trial['thresholds'].items()} } "
            f"capacities {trial['capacities']} live {trial['live']} paths {trial['paths']}")


# ---- the device half ---------------------------------------------------------------------------------------------------------------
class _Outputs:
    """poison-filled device buffers with slack behind them"""

    def __init__(self, torch):
        self.torch, self.made = torch, []

    def new(self, n, kind):
        dtype, poison = (self.torch.int64, POISON) if kind == "i64" else (self.torch.int32, POISON32)
        t = self.torch.full((n + SLACK,), poison, dtype=dtype, device="cuda")
        self.made.append((t, n, poison))
        return t.view(self.torch.float32) if kind == "f32" else t

    def slack_intact(self):
        return all(bool((t[n:] == poison).all()) for t, n, poison in self.made)


def _host(x, n, shape, view):
    return x.cpu().numpy().reshape(-1)[:n].view(view).reshape(shape)


def run_trial(torch, trial, want):
    """every call of the trial on the device -> the names of the calls whose output differs from `want`.  Errors propagate."""
    entries, recs, L = trial["entries"], trial["recordings"], trial["L"]
    n, R, per, s = len(entries), len(recs), len(recs[0]), trial["single"]
    rg, base, k, ts, cap, limit = trial["range"], trial["index_base"], trial["k"], trial["thresholds"], trial["capacities"], trial["scratch_limit"]
    counts = np.array([len(e) for e in entries], np.uint32)
    corpus = lb.Corpus.ragged(L, n + 1, int(counts.sum()) + 8)
    dev = torch.from_numpy(pack(np.concatenate(entries))).cuda()
    cut, at = trial["cut"], int(counts[:trial["cut"]].sum())
    if cut:
        corpus.append_ragged_packed_device(dev[:at], counts[:cut])
    if cut < n:
        corpus.append_ragged_packed_device(dev[at:], counts[cut:])
    block = torch.from_numpy(pack(np.concatenate(recs))).cuda()
    one = block.reshape(R, per, 32)[s].contiguous()
    fp = lb.Fingerprint.from_bools(recs[s]) if trial["handles"] else None
    bad = []
    u64, i32, u32, f32, i64 = np.uint64, np.int32, np.uint32, np.float32, np.int64

    def check(name, got):
        same = same_values(got, want[name])                                  # (scores as bit patterns)
        if not same or not o.slack_intact():
            bad.append(name + ("" if same else " (values)") + ("" if o.slack_intact() else " (slack overwritten)"))

    lb.debug_set_grid_ceiling(trial["grid_ceiling"])
    lb.debug_set_occurrences_batch_form(trial["force_shared"]["occurrences"])
    lb.debug_set_recording_batch_form(trial["force_shared"]["recording"])
    lb.debug_set_timeline_batch_form(trial["force_shared"]["timeline"])
    # -- occurrences
    corpus.set_join_scratch_limit(limit["occurrences"])
    for peaks, name in ((False, "occurrences"), (True, "occurrences_peaks")):
        c = cap[name]
        for form in ("packed", "handle") if fp is not None else ("packed",):
            o = _Outputs(torch)
            keys, lags, count = o.new(c, "i64"), o.new(c, "i32"), o.new(1, "i64")
            if form == "packed":
                corpus.query_packed_occurrences_keys_device(one, per, float(ts["occurrences"]), c, peaks=peaks, range_=rg, index_base=base,
                                                            keys_out=keys, lags_out=lags, count_out=count)
            else:
                corpus.query_occurrences_keys_device(fp, float(ts["occurrences"]), c, peaks=peaks, range_=rg, index_base=base, keys_out=keys,
                                                     lags_out=lags, count_out=count)
            check(name, (_host(keys, c, (c,), u64), _host(lags, c, (c,), i32), _host(count, 1, (), i64)))
        c = cap[name + "_batch"]
        o = _Outputs(torch)
        keys, lags, count = o.new(R * c, "i64"), o.new(R * c, "i32"), o.new(R, "i64")
        corpus.query_packed_occurrences_batch_keys_device(block, R, per, float(ts["occurrences_batch"]), c, peaks=peaks, range_=rg,
                                                          index_base=base, keys_out=keys, lags_out=lags, counts_out=count)
        check(name + "_batch", (_host(keys, R * c, (R, c), u64), _host(lags, R * c, (R, c), i32), _host(count, R, (R,), i64)))
    lv = trial["live"]                                                       # (the live peaks: the occurrences' limit)
    c = lv["capacity"]
    o = _Outputs(torch)
    keys, lags, count = o.new(R * c, "i64"), o.new(R * c, "i32"), o.new(R, "i64")
    corpus.query_packed_occurrences_tail_peaks_batch_keys_device(block, R, per, lv["new"], float(ts["occurrences_batch"]), c,
                                                                 max_new=lv["max_new"], final=lv["final"], range_=rg, index_base=base,
                                                                 keys_out=keys, lags_out=lags, counts_out=count)
    check("live_peaks_batch", (_host(keys, R * c, (R, c), u64), _host(lags, R * c, (R, c), i32), _host(count, R, (R,), i64)))
    c = cap["threshold_batch"]                                               # (the batch threshold: the occurrences' switch and limit)
    o = _Outputs(torch)
    keys, lags, count = o.new(R * c, "i64"), o.new(R * c, "i32"), o.new(R, "i64")
    corpus.query_packed_recording_threshold_batch_keys_device(block, R, per, float(ts["threshold_batch"]), c, range_=rg, index_base=base,
                                                              keys_out=keys, lags_out=lags, counts_out=count)
    check("threshold_batch", (_host(keys, R * c, (R, c), u64), _host(lags, R * c, (R, c), i32), _host(count, R, (R,), i64)))
    # -- recording scores, top-K, threshold
    corpus.set_join_scratch_limit(limit["recording"])
    for form in ("packed", "handle") if fp is not None else ("packed",):
        o = _Outputs(torch)
        sc, lags = o.new(n, "f32"), o.new(n, "i32")
        if form == "packed":
            corpus.recording_scores_device(packed=one, per_query=per, range_=rg, scores_out=sc, lags_out=lags)
        else:
            corpus.recording_scores_device(fp=fp, range_=rg, scores_out=sc, lags_out=lags)
        check("scores", (_host(sc, n, (n,), f32), _host(lags, n, (n,), i32)))
    o = _Outputs(torch)
    sc, lags = o.new(R * n, "f32"), o.new(R * n, "i32")
    corpus.recording_scores_batch_device(block, R, per, range_=rg, scores_out=sc, lags_out=lags)
    check("scores_batch", (_host(sc, R * n, (R, n), f32), _host(lags, R * n, (R, n), i32)))
    o = _Outputs(torch)
    keys, lags = o.new(k, "i64"), o.new(k, "i32")
    corpus.query_packed_recording_topk_keys_device(one, per, k, range_=rg, index_base=base, keys_out=keys, lags_out=lags)
    check("topk", (_host(keys, k, (k,), u64), _host(lags, k, (k,), i32)))
    o = _Outputs(torch)
    keys, lags = o.new(R * k, "i64"), o.new(R * k, "i32")
    corpus.query_packed_recording_topk_batch_keys_device(block, R, per, k, range_=rg, index_base=base, keys_out=keys, lags_out=lags)
    check("topk_batch", (_host(keys, R * k, (R, k), u64), _host(lags, R * k, (R, k), i32)))
    c = cap["threshold"]
    o = _Outputs(torch)
    keys, lags, count = o.new(c, "i64"), o.new(c, "i32"), o.new(1, "i64")
    corpus.query_packed_recording_threshold_keys_device(one, per, float(ts["threshold"]), c, range_=rg, index_base=base, keys_out=keys,
                                                        lags_out=lags, count_out=count)
    check("threshold", (_host(keys, c, (c,), u64), _host(lags, c, (c,), i32), _host(count, 1, (), i64)))
    # -- timeline and segments
    corpus.set_join_scratch_limit(limit["timeline"])
    c = cap["segments"]
    for form in ("packed", "handle") if fp is not None else ("packed",):
        o = _Outputs(torch)
        keys, lens = o.new(per, "i64"), o.new(per, "i32")
        if form == "packed":
            corpus.recording_timeline_keys_device(packed=one, per_query=per, threshold=float(ts["timeline"]), range_=rg, index_base=base,
                                                  keys_out=keys, lengths_out=lens)
        else:
            corpus.recording_timeline_keys_device(fp=fp, threshold=float(ts["timeline"]), range_=rg, index_base=base, keys_out=keys,
                                                  lengths_out=lens)
        check("timeline", (_host(keys, per, (per,), u64), _host(lens, per, (per,), u32)))
    o = _Outputs(torch)
    st, sk, sl, sn = o.new(c, "i32"), o.new(c, "i64"), o.new(c, "i32"), o.new(1, "i32")
    lb.timeline_segments_device(keys[:per], lens[:per], c, starts_out=st, keys_out=sk, lengths_out=sl, counts_out=sn)
    check("segments", (_host(st, c, (c,), i32), _host(sk, c, (c,), u64), _host(sl, c, (c,), u32), _host(sn, 1, (), i32)))
    c = cap["segments_batch"]
    o = _Outputs(torch)
    keys, lens = o.new(R * per, "i64"), o.new(R * per, "i32")
    corpus.recording_timeline_batch_keys_device(block, R, per, float(ts["timeline_batch"]), range_=rg, index_base=base, keys_out=keys,
                                                lengths_out=lens)
    check("timeline_batch", (_host(keys, R * per, (R, per), u64), _host(lens, R * per, (R, per), u32)))
    o = _Outputs(torch)
    got = corpus.recording_segments_batch_keys_device(block, R, per, float(ts["timeline_batch"]), c, range_=rg, index_base=base)
    check("segments_batch", (_host(got[0], R * c, (R, c), i32), _host(got[1], R * c, (R, c), u64), _host(got[2], R * c, (R, c), u32),
                             _host(got[3], R, (R,), i32)))
    torch.cuda.synchronize()
    return bad


def same_values(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else np.asarray(x),
                                                   np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else np.asarray(y))
                                    for x, y in zip(a, b))


def trial_rng(seed, t):
    """the generator of trial t alone"""
    return np.random.default_rng([int(seed), int(t)])


def main(argv):
    argv = list(argv)
    only = None
    if "--only" in argv:
        at = argv.index("--only")
        only = int(argv[at + 1])
        del argv[at:at + 2]
    flags = [a for a in argv if a.startswith("--")]
    args = [a for a in argv if not a.startswith("--")]
    trials = int(args[0]) if len(args) > 0 else 200
    seed = int(args[1]) if len(args) > 1 else 1
    plan_only = "--plan-only" in flags
    torch = None
    if not plan_only:
        import torch
    bad, t0, t_ref = 0, time.time(), 0.0
    buckets, empty = {}, 0
    for t in range(trials) if only is None else [only]:
        t1 = time.time()
        trial = make_trial(trial_rng(seed, t))
        trial["handles"] = t % 3 == 0
        want = expected(trial)
        want.update(expected_live(trial))
        t_ref += time.time() - t1
        for p in trial["paths"]:
            buckets[p] = buckets.get(p, 0) + 1
        empty += "all_empty" in trial["paths"]
        if plan_only:
            continue
        try:
            wrong = run_trial(torch, trial, want)
        finally:
            lb.debug_set_grid_ceiling(0)
            lb.debug_set_occurrences_batch_form(False)
            lb.debug_set_recording_batch_form(False)
            lb.debug_set_timeline_batch_form(False)
        if wrong:
            bad += 1
            print("RECORDING MISMATCH seed", seed, "trial", t, "calls", wrong, describe(trial), flush=True)
    done = trials if only is None else 1
    if plan_only:
        for name in sorted(buckets):
            print(f"{name:32s} {buckets[name]}")
        print(f"{done} trials planned, {done - empty} of them ({100.0 * (done - empty) / max(1, done):.0f} %) with a non-empty list, "
              f"{time.time() - t0:.1f} s")
        return 0
    print(f"{done} trials, {bad} mismatches, {time.time() - t0:.1f} s ({t_ref:.1f} s of it the numpy reference); seed {seed}; "
          f"{done - empty} trials with a non-empty list; paths {dict(sorted(buckets.items()))}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
