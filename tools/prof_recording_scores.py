#!/usr/bin/env python3
"""The recording-scores call against the scan it stands beside and the occurrences pass it is built from, alternating in one
process after warm-up:
    python3 tools/prof_recording_scores.py [reps] [--out DIR] [--only 100k|1m] [--no-crossover]
Corpus: tools/prof_occurrences.py's -- synth_ragged_corpus_device, lengths synth_ragged_counts(seed, 0, n, 20, 70), 200 Booleans
per sub-fingerprint, at 100 000 and 1 000 000 entries.  Recording: 2 400 synthetic sub-fingerprints (about an hour at the default
settings); 300 entries of the corpus are made verbatim pieces of it (entry e = recording[o_e : o_e + n_e]), so each of them scores
1.0 at lag -o_e.  Legs:
    a        Corpus.recording_scores_device with lags
    b        Corpus.scores_device with the same query on the same corpus: the ragged scan that exists, untouched
    c        Corpus.query_occurrences_keys_device, peaks off, t = 0.7: the same pair loop, run again for the items that match
Device time: hipEvents around the calls on the current stream; medians and quartiles of `reps` (default 7, at least 5) rounds in
ms.  After the clock stops: (a)'s scores equal (b)'s bit for bit, and every planted entry scores 1.0 with the planted
lag.  One JSON line per corpus size, also
appended to DIR/recording_scores_prof.jsonl (default DIR: profiles).  The bar: the median of a is at most one tenth of the median
of b ("bar_met"); the exit status is 1 when a size misses it.  At the 1 M corpus the crossover follows: a and b at queries of 50,
100, 300 and 1 000 sub-fingerprints (prefixes of the recording), reported, not gated ("crossover").
    timeout -k 10 900 python3 tools/prof_recording_scores.py 7"""
import json
import os
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
CROSSOVER = (50, 100, 300, 1000)


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


def run(name, n, crossover):
    counts = O.synth_ragged_counts(SEED, 0, n, 20, 70)
    packed = lb.synth_ragged_corpus_device(SEED, 0, counts, L)
    recording = lb.synth_ragged_corpus_device(SEED + 7, 0, np.array([N_QUERY], np.uint32), L)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rng = np.random.default_rng(SEED)
    planted = np.sort(rng.choice(n, PLANTS, replace=False))
    planted_at = {}
    for e in planted:
        m = int(counts[e])
        o = int(rng.integers(0, N_QUERY - m + 1))
        packed[off[e]:off[e] + m] = recording[o:o + m]
        planted_at[int(e)] = o
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
    a_scores = torch.zeros(n, dtype=torch.float32, device="cuda")
    a_lags = torch.zeros(n, dtype=torch.int32, device="cuda")
    b_scores = [None]

    def scan(q):
        b_scores[0] = corpus.scores_device(q)

    times = alternate({"a": lambda: corpus.recording_scores_device(fp=fp, scores_out=a_scores, lags_out=a_lags),
                       "b": lambda: scan(fp),
                       "c": lambda: corpus.query_occurrences_keys_device(fp, T, capacity, keys_out=keys, lags_out=klags, count_out=count)})
    # after the clock: the two routes to the scores agree, and the plants are where they were planted
    sa, la, sb = a_scores.cpu().numpy(), a_lags.cpu().numpy(), b_scores[0].cpu().numpy()
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), "recording scores and the scan disagree"
    for e, o in planted_at.items():
        assert sa[e] == np.float32(1.0), "a planted entry does not score 1.0"
        assert la[e] == -o, "a planted entry's lag is not its plant's"
    compares = int(((N_QUERY - counts.astype(np.int64) + 1) * counts).sum())
    res = {"leg": name, "reps": REPS, "entries": n, "records": int(counts.sum()), "n_query": N_QUERY, "threshold": T, "plants": PLANTS,
           "compares": compares, "a": _stats(times["a"]), "b": _stats(times["b"]), "c": _stats(times["c"])}
    res["b_over_a"] = round(res["b"]["median"] / res["a"]["median"], 2)
    res["a_over_b"] = round(res["a"]["median"] / res["b"]["median"], 4)
    res["a_over_c"] = round(res["a"]["median"] / res["c"]["median"], 3)
    res["ps_per_compare"] = {k: round(res[k]["median"] * 1e9 / compares, 3) for k in ("a", "b", "c")}
    res["bar_met"] = res["a"]["median"] * 10.0 <= res["b"]["median"]
    if crossover:
        res["crossover"] = []
        for nq in CROSSOVER:
            q = lb.Fingerprint.from_bools(bools[:nq])
            t = alternate({"a": lambda: corpus.recording_scores_device(fp=q, scores_out=a_scores, lags_out=a_lags), "b": lambda: scan(q)})
            assert np.array_equal(a_scores.cpu().numpy().view(np.uint32), b_scores[0].cpu().numpy().view(np.uint32)), nq
            a, b = _stats(t["a"]), _stats(t["b"])
            res["crossover"].append({"n_query": nq, "a": a, "b": b, "a_over_b": round(a["median"] / b["median"], 3)})
    print(json.dumps(res), flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "recording_scores_prof.jsonl"), "a") as f:
        f.write(json.dumps(res) + "\n")
    corpus.dispose()
    del packed, corpus
    torch.cuda.empty_cache()
    return res["bar_met"]


torch.cuda.set_device(0)
met = True
for name, n in (("100k", 100_000), ("1m", 1_000_000)):
    if ONLY is None or ONLY == name:
        met = run(f"{n} entries of 20 .. 70, recording of {N_QUERY}", n, name == "1m" and "--no-crossover" not in sys.argv) and met
sys.exit(0 if met else 1)
