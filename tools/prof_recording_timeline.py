#!/usr/bin/env python3
"""The recording-timeline call against the two calls it stands beside, alternating in one process after warm-up:
    python3 tools/prof_recording_timeline.py [reps] [--out DIR] [--only 100k|1m]
Corpus: tools/prof_occurrences.py's -- synth_ragged_corpus_device, lengths synth_ragged_counts(seed, 0, n, 20, 70), 200 Booleans
per sub-fingerprint, at 100 000 and 1 000 000 entries.  Recording: 2 400 synthetic sub-fingerprints (about an hour at the default
settings); 300 entries of the corpus are made verbatim pieces of it (entry e = recording[o_e : o_e + n_e]), so each of them scores
1.0 at offset o_e.  t = 0.7.  Legs:
    a        Corpus.recording_timeline_keys_device with lengths
    b        Corpus.recording_scores_device with lags: the same pair loop folded per entry, untouched
    c        Corpus.query_occurrences_keys_device, peaks off: the cells as a list, untouched
Device time: hipEvents around the calls on the current stream; medians and quartiles of `reps` (default 7, at least 5) rounds in
ms.  After the clock stops: every planted offset of (a) names its planted entry (the lowest planted there) with score 1.0 and its
length, and (a) equals the per-offset fold of (c)'s list.  One JSON line per corpus size, also appended to
DIR/recording_timeline_prof.jsonl (default DIR: profiles).  The bar is stated against (b), code this call does not touch: the
median of a is at most 1.10 x the median of b ("bar_met"); the exit status is 1 when a size misses it.
    timeout -k 10 900 python3 tools/prof_recording_timeline.py 7"""
import json
import os
import re
import statistics
import sys

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
BAR = 1.10
WALK = int(re.search(r"constexpr\s+uint32_t\s+kTlEntries\s*=\s*(\d+)\s*;",
                     open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_timeline.hip")).read()).group(1))


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


def alternate(calls):
    """warm-up, then REPS rounds of every call in turn -> name -> device ms"""
    for f in calls.values():
        f()
        torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(REPS):
        for k, f in calls.items():
            times[k].append(device_ms(f))
    torch.cuda.synchronize()
    return times


def run(name, n):
    counts = O.synth_ragged_counts(SEED, 0, n, 20, 70)
    packed = lb.synth_ragged_corpus_device(SEED, 0, counts, L)
    recording = lb.synth_ragged_corpus_device(SEED + 7, 0, np.array([N_QUERY], np.uint32), L)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rng = np.random.default_rng(SEED)
    planted = np.sort(rng.choice(n, PLANTS, replace=False))
    first_at = {}                                                 # offset -> the lowest entry planted there
    for e in planted:
        m = int(counts[e])
        o = int(rng.integers(0, N_QUERY - m + 1))
        packed[off[e]:off[e] + m] = recording[o:o + m]
        first_at.setdefault(o, int(e))
    corpus = lb.Corpus.ragged(L, n, int(counts.sum()))
    corpus.append_ragged_packed_device(packed, counts)
    bools = lb.unpack_packed(recording.cpu().numpy(), L).reshape(N_QUERY, L)
    fp = lb.Fingerprint.from_bools(bools)
    torch.cuda.synchronize()

    _, _, total = corpus.query_occurrences_keys_device(fp, T, 1, want_lags=False)
    capacity = int(total[0]) + 1024
    keys = torch.zeros(capacity, dtype=torch.int64, device="cuda")
    klags = torch.zeros(capacity, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    a_keys = torch.zeros(N_QUERY, dtype=torch.int64, device="cuda")
    a_lengths = torch.zeros(N_QUERY, dtype=torch.int32, device="cuda")
    b_scores = torch.zeros(n, dtype=torch.float32, device="cuda")
    b_lags = torch.zeros(n, dtype=torch.int32, device="cuda")

    times = alternate({"a": lambda: corpus.recording_timeline_keys_device(fp=fp, threshold=T, keys_out=a_keys, lengths_out=a_lengths),
                       "b": lambda: corpus.recording_scores_device(fp=fp, scores_out=b_scores, lags_out=b_lags),
                       "c": lambda: corpus.query_occurrences_keys_device(fp, T, capacity, keys_out=keys, lags_out=klags, count_out=count)})
    # after the clock: the plants are where they were planted, and the timeline is the fold of the occurrences list
    idx, sc, ln = lb.decode_timeline_keys(a_keys, a_lengths)
    for o, e in first_at.items():
        assert idx[o] == e and sc[o] == np.float32(1.0) and ln[o] == counts[e], f"offset {o} does not name its planted entry {e}"
    m = int(count.cpu().numpy()[0])
    assert m <= capacity
    k = keys.cpu().numpy().view(np.uint64)[:m]
    lg = klags.cpu().numpy()[:m].astype(np.int64)
    assert (lg <= 0).all()                                        # (no entry is longer than the recording)
    fold = np.zeros(N_QUERY, np.uint64)
    np.maximum.at(fold, -lg, k)
    assert np.array_equal(fold, a_keys.cpu().numpy().view(np.uint64)), "the timeline is not the fold of the occurrences"
    compares = int(((N_QUERY - counts.astype(np.int64) + 1) * counts).sum())
    tiles = -(-(N_QUERY - int(counts.min()) + 1) // 126)
    res = {"leg": name, "reps": REPS, "entries": n, "records": int(counts.sum()), "n_query": N_QUERY, "threshold": T, "plants": PLANTS,
           "compares": compares, "winners": int(np.count_nonzero(fold)), "occurrences": m, "walk": WALK,
           "scratch_bytes": {"a": -(-n // WALK) * tiles * 126 * 8, "b": n * tiles * 8},
           "a": _stats(times["a"]), "b": _stats(times["b"]), "c": _stats(times["c"])}
    res["a_over_b"] = round(res["a"]["median"] / res["b"]["median"], 4)
    res["a_over_c"] = round(res["a"]["median"] / res["c"]["median"], 4)
    res["ps_per_compare"] = {k: round(res[k]["median"] * 1e9 / compares, 3) for k in ("a", "b", "c")}
    res["bar"] = BAR
    res["bar_met"] = res["a"]["median"] <= BAR * res["b"]["median"]
    print(json.dumps(res), flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "recording_timeline_prof.jsonl"), "a") as f:
        f.write(json.dumps(res) + "\n")
    corpus.dispose()
    del packed, corpus
    torch.cuda.empty_cache()
    return res["bar_met"]


torch.cuda.set_device(0)
met = True
for name, n in (("100k", 100_000), ("1m", 1_000_000)):
    if ONLY is None or ONLY == name:
        met = run(f"{n} entries of 20 .. 70, recording of {N_QUERY}", n) and met
sys.exit(0 if met else 1)
