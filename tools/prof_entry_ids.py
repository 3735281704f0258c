#!/usr/bin/env python3
"""The entry ids on one device, legs alternating in one process after a warm-up:
    python3 tools/prof_entry_ids.py [reps] [--out DIR] [--only remove|build|lookup] [--entries N] [--big N]
Legs:
    remove    uniform N (default 1 M) entries x 5 x 200 Booleans, a scattered 1 % removed with remove_keys_device: a corpus WITH
              ids against the same corpus WITHOUT, alternating.  The corpus without ids is the path from before ids existed: it
              has no id block (asserted: has_entry_ids is 0 and the two corpora differ by exactly the id block and the removal's id
              scratch in live bytes).  By bytes moved the ids add 8 to the 128 + 8 bytes of a kept entry each way.
    build     the id index of N and of `big` (default 10 M) entries with random ids, sequential ids and multiples of 2^20: the ids
              are set again before every round (untimed; that makes the index stale), then a one-id KeysFromIds is timed -- the
              init and insert launches and one probe.  Scattered 64-bit compare-and-swaps: no bound was known beforehand, so the
              time, the entries per second and the atomics per second (one CAS and one min per entry, more where probes collide)
              are reported as they are.  The three patterns should lie within each other's spread; if not, the mixer is at fault.
    lookup    KeysFromIds and IdsFromKeys of 1 M-element lists against the `big` corpus, the index warm
Per round the state is restored outside the clock.  Device time: hipEvents around the calls on the current stream (a removal
reads its index back in the middle: the gap is part of it); medians and quartiles of `reps` (default 7) rounds in ms, one JSON
line per leg, also appended to DIR/entry_ids_prof.jsonl (default DIR: profiles).  After the clock has stopped:
KeysFromIds(IdsFromKeys(keys)) names the same entries.  Under its own time limit:
    timeout -k 10 600 python3 tools/prof_entry_ids.py 7"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lbaudiodetective_amd as lb  # noqa: E402

SEED = 0x4C424149
LIST = 1_000_000


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
ONLY = _option("--only")
N = int(_option("--entries", 1_000_000))
BIG = int(_option("--big", 10_000_000))
_skip = {OUT, ONLY, _option("--entries"), _option("--big")}
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in _skip]
REPS = int(args[0]) if args else 7
LOW = np.uint64(0xFFFFFFFF)


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


def report(res):
    print(json.dumps(res), flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "entry_ids_prof.jsonl"), "a") as f:
        f.write(json.dumps(res) + "\n")


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def keys_of(indices):
    """64-bit keys as the query calls write them (score word: 1.0), on the device"""
    return dev64((np.uint64(0x3F800000) << np.uint64(32)) | (LOW - np.asarray(indices, np.uint64)))


def make_ids(pattern, n, rng):
    """n distinct non-zero ids"""
    if pattern == "random":
        return (rng.permutation(n).astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)      # (an odd multiplier permutes 64 bits)
    if pattern == "sequential":
        return np.arange(n, dtype=np.uint64) + np.uint64(1_000_000)
    return (np.arange(n, dtype=np.uint64) + np.uint64(1)) << np.uint64(20)


def want(name):
    return ONLY is None or ONLY == name


torch.cuda.set_device(0)
rng = np.random.default_rng(SEED)

if want("remove"):
    n = N
    packed = lb.synth_corpus_device(SEED, 0, n, 5, 200)
    ids = dev64(make_ids("random", n, rng))
    gone = rng.choice(n, n // 100, replace=False)
    keys = keys_of(gone)
    corpora = {"with ids": lb.Corpus(200, 5, n), "without ids": lb.Corpus(200, 5, n)}
    times = {name: [] for name in corpora}
    live = {}
    for rep in range(REPS + 1):                                   # (round 0 warms up: the scratch grows there)
        for name, c in corpora.items():
            if len(c):
                c.remove_keys_device(keys_of(np.arange(len(c))))  # empty it: a removal of everything moves nothing
            c.append_packed_device(packed)
            if name == "with ids":
                c.set_entry_ids(ids)
            torch.cuda.synchronize()
            before = lb.debug_live_bytes()[0]
            got = []
            t = device_ms(lambda: got.append(c.remove_keys_device(keys)))
            assert got[0] == len(gone) and len(c) == n - len(gone)
            if rep == 0:
                live[name] = lb.debug_live_bytes()[0] - before
            else:
                times[name].append(t)
    assert corpora["with ids"].has_entry_ids and not corpora["without ids"].has_entry_ids
    # what the removal of the corpus with ids reserved beyond the other's: the ids' scratch, 8 bytes per entry from the lowest removed on
    assert live["with ids"] - live["without ids"] == 8 * (n - int(gone.min())), live
    keep = np.ones(n, bool)
    keep[gone] = False
    assert np.array_equal(corpora["with ids"].entry_ids(), ids.cpu().numpy().view(np.uint64)[keep])
    res = {"leg": f"remove, uniform {n} x 5 x 200, scattered 1 %", "reps": REPS, "entries": n, "removed": len(gone)}
    for name, v in times.items():
        res[name] = _stats(v)
    res["with_over_without"] = round(res["with ids"]["median"] / res["without ids"]["median"], 3)
    report(res)
    for c in corpora.values():
        c.dispose()
    del packed, ids
    torch.cuda.empty_cache()

if want("build") or want("lookup"):
    for n in ([N, BIG] if want("build") else [BIG]):
        c = lb.Corpus(200, 1, n)
        c.append_packed_device(lb.synth_corpus_device(SEED, 0, n, 1, 200))
        torch.cuda.empty_cache()
        patterns = {p: dev64(make_ids(p, n, rng)) for p in ("random", "sequential", "multiples of 2^20")}
        one = {p: v[n // 2:n // 2 + 1].clone() for p, v in patterns.items()}
        out = torch.empty(1, dtype=torch.int64, device="cuda")
        if want("build"):
            times = {p: [] for p in patterns}
            for rep in range(REPS + 1):
                for p, ids in patterns.items():
                    c.set_entry_ids(ids)                          # the index is stale
                    torch.cuda.synchronize()
                    t = device_ms(lambda: c.keys_from_ids_device(one[p], out=out))
                    assert int(out.item()) & 0xFFFFFFFF == 0xFFFFFFFF - n // 2
                    if rep:
                        times[p].append(t)
            for p, v in times.items():
                s = _stats(v)
                report({"leg": f"index build, {n} entries, {p} ids", "reps": REPS, "entries": n, "slots": 1 << (2 * n - 1).bit_length(), "ms": s,
                        "entries_per_s": round(n / (s["median"] * 1e-3)), "atomics_per_s": round(2 * n / (s["median"] * 1e-3))})
        if want("lookup") and n == BIG:
            host_ids = patterns["random"].cpu().numpy().view(np.uint64)
            c.set_entry_ids(patterns["random"])
            where = rng.integers(0, n, LIST)
            d_ids, d_keys = dev64(host_ids[where]), keys_of(where)
            got_keys = torch.empty(LIST, dtype=torch.int64, device="cuda")
            got_ids = torch.empty(LIST, dtype=torch.int64, device="cuda")
            c.keys_from_ids_device(d_ids, out=got_keys)           # (builds the index)
            times = {"keys_from_ids": [], "ids_from_keys": []}
            for rep in range(REPS + 1):
                torch.cuda.synchronize()
                t_k = device_ms(lambda: c.keys_from_ids_device(d_ids, out=got_keys))
                t_i = device_ms(lambda: c.ids_from_keys_device(d_keys, out=got_ids))
                if rep:
                    times["keys_from_ids"].append(t_k)
                    times["ids_from_keys"].append(t_i)
            res = {"leg": f"lookups, {LIST} elements against {n} entries, index warm", "reps": REPS, "entries": n, "elements": LIST}
            for k, v in times.items():
                res[k] = _stats(v)
                res[k + "_per_s"] = round(LIST / (res[k]["median"] * 1e-3))
            # after the clock: the keys of the ids of the keys name the same entries
            back = c.keys_from_ids_device(c.ids_from_keys_device(d_keys))
            torch.cuda.synchronize()
            low = lambda t: t.cpu().numpy().view(np.uint64) & LOW           # noqa: E731
            assert np.array_equal(low(back), low(d_keys)) and np.array_equal(low(got_keys), low(d_keys))
            assert np.array_equal(got_ids.cpu().numpy().view(np.uint64), host_ids[where])
            res["round_trip_names_the_same_entries"] = True
            report(res)
        c.dispose()
        del patterns
        torch.cuda.empty_cache()
