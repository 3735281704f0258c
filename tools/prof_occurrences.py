#!/usr/bin/env python3
"""The occurrences call against what it is built from and what it replaces, alternating in one process after warm-up:
    python3 tools/prof_occurrences.py [reps] [--out DIR] [--only 100k|1m]
Corpus: synth_ragged_corpus_device, lengths synth_ragged_counts(seed, 0, n, 20, 70), 200 Booleans per sub-fingerprint, at
100 000 and 1 000 000 entries.  Recording: 2 400 synthetic sub-fingerprints (about an hour at the default settings); 300
entries of the corpus are made verbatim pieces of it (entry e = recording[o_e : o_e + n_e]), so each of them occurs in the
recording with a cell of 1.0.  t = 0.7.  Legs:
    a        Corpus.query_occurrences_keys_device, peaks off ("a") and on ("a_peaks")
    b        Corpus.scores_device with the same query on the same corpus: the same sub-fingerprint compares, folded to the
             maximum per entry by the scan that exists
    c        the match_profile loop plus a host filter that (a) replaces, on a sample of `C_SAMPLE` entries, host wall time,
             scaled to all entries ("c_sampled")
Device time of a and b: hipEvents around the calls on the current stream; medians and quartiles of `reps` (default 7, at least
5) rounds in ms.  After the clock stops: the entries with a cell in (a) are the entries whose score in (b) is >= t, every
planted entry among them, and the sampled entries' cells of (a) are the filter of (c).  One JSON line per corpus size, also
appended to DIR/occurrences_prof.jsonl (default DIR: profiles).  The bar: the median of a is not above the median of b by more
than the larger of the two interquartile ranges ("bar_met"); the exit status is 1 when a size misses it.
    timeout -k 10 600 python3 tools/prof_occurrences.py 7"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lbaudiodetective_amd as lb  # noqa: E402
from oracle import oracle as O  # noqa: E402

SEED = 0x4C424146
PLANTS = 300
N_QUERY = 2400
L = 200
T = 0.7
C_SAMPLE = 64
TILE, WAVES, LDS_RECORD, LDS_TABLE, LDS_CU = 126, 4, 36, 5151 * 4, 160 * 1024     # k_occurrences.hip's constants


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
ONLY = _option("--only")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in {OUT, ONLY}]
REPS = max(5, int(args[0]) if args else 7)


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    return {"median": round(q[1], 4), "p25": round(q[0], 4), "p75": round(q[2], 4)}


def lds_bytes(ne_max):
    return (WAVES * TILE + 2 + min(ne_max, N_QUERY)) * LDS_RECORD + LDS_TABLE


def run(name, n):
    counts = O.synth_ragged_counts(SEED, 0, n, 20, 70)
    packed = lb.synth_ragged_corpus_device(SEED, 0, counts, L)
    recording = lb.synth_ragged_corpus_device(SEED + 7, 0, np.array([N_QUERY], np.uint32), L)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rng = np.random.default_rng(SEED)
    planted = np.sort(rng.choice(n, PLANTS, replace=False))
    for e in planted:
        m = int(counts[e])
        o = int(rng.integers(0, N_QUERY - m + 1))
        packed[off[e]:off[e] + m] = recording[o:o + m]
    corpus = lb.Corpus.ragged(L, n, int(counts.sum()))
    corpus.append_ragged_packed_device(packed, counts)
    fp = lb.Fingerprint.from_bools(lb.unpack_packed(recording.cpu().numpy(), L).reshape(N_QUERY, L))
    torch.cuda.synchronize()

    totals = {}
    for peaks in (False, True):
        _, _, count = corpus.query_occurrences_keys_device(fp, T, 1, peaks=peaks, want_lags=False)
        totals[peaks] = int(count[0])
    capacity = max(totals.values()) + 1024
    keys = {p: torch.zeros(capacity, dtype=torch.int64, device="cuda") for p in (False, True)}
    lags = {p: torch.zeros(capacity, dtype=torch.int32, device="cuda") for p in (False, True)}
    count = {p: torch.zeros(1, dtype=torch.int64, device="cuda") for p in (False, True)}
    scores = [None]

    def occurrences(peaks):
        corpus.query_occurrences_keys_device(fp, T, capacity, peaks=peaks, keys_out=keys[peaks], lags_out=lags[peaks],
                                             count_out=count[peaks])

    def scan():
        scores[0] = corpus.scores_device(fp)

    calls = {"a": lambda: occurrences(False), "b": scan, "a_peaks": lambda: occurrences(True)}
    for f in calls.values():
        f()
        torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(REPS):
        for k, f in calls.items():
            times[k].append(device_ms(f))
    torch.cuda.synchronize()
    # (c) the loop that (a) replaces: one synchronous call per entry and a filter on the host
    sample = np.unique(np.concatenate([planted[:C_SAMPLE // 2], rng.choice(n, C_SAMPLE // 2, replace=False)]))
    loop_cells = {}
    c_times = []
    for _ in range(3):
        t0 = time.perf_counter()
        for e in sample:
            p, _first = corpus.match_profile(fp, int(e))
            o = np.flatnonzero(p >= np.float32(T))
            loop_cells[int(e)] = (o, p[o])
        c_times.append((time.perf_counter() - t0) * 1e3 * n / len(sample))
    # after the clock: the three routes agree
    idx, sc, lg = lb.decode_occurrence_keys(keys[False], lags[False], int(count[False][0]))
    assert int(count[False][0]) == totals[False] and int(count[True][0]) == totals[True]
    s = scores[0].cpu().numpy()
    assert np.array_equal(np.unique(idx), np.flatnonzero(s >= np.float32(T))), "occurrences and the scan disagree"
    assert np.isin(planted, idx).all(), "a planted entry was not found"
    for e, (o, cells) in loop_cells.items():
        mine = idx == e
        assert np.array_equal(-lg[mine], o) and np.array_equal(sc[mine].view(np.uint32), cells.view(np.uint32)), "occurrences and the loop disagree"
    compares = int(((N_QUERY - counts.astype(np.int64) + 1) * counts).sum())
    ne_max = int(counts.max())
    res = {"leg": name, "reps": REPS, "entries": n, "records": int(counts.sum()), "n_query": N_QUERY, "threshold": T,
           "plants": PLANTS, "matches": totals[False], "matches_peaks": totals[True], "compares": compares,
           "a": _stats(times["a"]), "a_peaks": _stats(times["a_peaks"]), "b": _stats(times["b"]), "c": _stats(c_times),
           "c_sampled": len(sample), "lds_bytes": lds_bytes(ne_max), "lds_bytes_at_1024": lds_bytes(1024),
           "workgroups_per_cu_by_lds": LDS_CU // lds_bytes(ne_max), "workgroups_per_cu_by_lds_at_1024": LDS_CU // lds_bytes(1024)}
    res["a_over_b"] = round(res["a"]["median"] / res["b"]["median"], 3)
    res["c_over_a"] = round(res["c"]["median"] / res["a"]["median"], 1)
    res["peaks_over_all"] = round(res["a_peaks"]["median"] / res["a"]["median"], 3)
    res["ps_per_compare"] = {k: round(res[k]["median"] * 1e9 / compares, 3) for k in ("a", "a_peaks", "b")}
    iqr = max(res["a"]["p75"] - res["a"]["p25"], res["b"]["p75"] - res["b"]["p25"])
    res["bar_met"] = res["a"]["median"] <= res["b"]["median"] + iqr
    print(json.dumps(res), flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "occurrences_prof.jsonl"), "a") as f:
        f.write(json.dumps(res) + "\n")
    corpus.dispose()
    del packed, corpus
    torch.cuda.empty_cache()
    return res["bar_met"]


torch.cuda.set_device(0)
met = True
for name, n in (("100k", 100_000), ("1m", 1_000_000)):
    if ONLY is None or ONLY == name:
        met = run(f"{n} entries of 20 .. 70, recording of {N_QUERY}, t = {T}", n) and met
sys.exit(0 if met else 1)
