#!/usr/bin/env python3
"""The duplicate groups on the device against the host route they replace, on the same build in one process, alternating after
warm-up:
    python3 tools/prof_groups.py [reps] [--out DIR] [--only self100k|self1m|dense]
Legs (5 x 200 Booleans per entry, the synthetic corpus of tools/prof_join.py with 300 planted near-copies):
    self100k, self1m   the keys of the self-join at t = 0.7 (every entry's self-match and the planted pairs)
    dense              the keys of the self-join of 20 k at the scores' median: about 2 x 10^8 edges, one giant component, the
                       worst case for contention on a few roots
Per leg: the join that produced the keys; `group` = LBAudioDetectiveGroupLabelsFromKeysDevice over them (HIP events on the
current stream); `extra` = LBAudioDetectiveGroupExtraKeysFromLabelsDevice (wall clock: the call returns when the keys are
written); `host` = the route without them, wall clock from the keys on the device to the remove list on the device: copy keys
and offsets to the host, decode_join_keys, a union-find there (scipy.sparse.csgraph.connected_components where scipy imports,
else the one below), upload of the remove list.  Both routes' labels are asserted equal.  Medians and quartiles of `reps`
(default 7) rounds in ms (the dense leg's host route: one round), one JSON line per leg, also appended to
DIR/groups_prof.jsonl (default DIR: profiles).  Under a time limit of its own:
    timeout -k 10 1100 python3 tools/prof_groups.py 7"""
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

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
except ImportError:
    connected_components = None

SEED = 0x4C424145
PLANTS = 300


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
ONLY = _option("--only")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in {OUT, ONLY}]
REPS = int(args[0]) if args else 7


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    return {"median": round(q[1], 4), "p25": round(q[0], 4), "p75": round(q[2], 4)}


def synth(seed, n):
    """packed rows [n, 5, 32] on the device with PLANTS near-copies: entry dst = entry src with about 20 Booleans flipped"""
    packed = lb.synth_corpus_device(seed, 0, n, 5, 200)
    g = torch.Generator().manual_seed(seed)
    at = torch.randperm(n, generator=g)[:2 * PLANTS]
    src, dst = at[:PLANTS].cuda(), at[PLANTS:].cuda()
    packed[dst] = packed[src]
    for _ in range(20):
        sub = torch.randint(0, 5, (PLANTS,), generator=g).cuda()
        bit = torch.randint(0, 200, (PLANTS,), generator=g).cuda()
        packed[dst, sub, bit // 8] ^= torch.bitwise_left_shift(torch.ones_like(bit), bit % 8).to(torch.uint8)
    return packed


def corpus_of(packed):
    c = lb.Corpus(200, 5, packed.shape[0])
    c.append_packed_device(packed)
    torch.cuda.synchronize()
    return c


def host_labels(n, rows, idx):
    """labels[i] = the lowest index of i's component of the undirected graph with the edges (rows[k], idx[k])"""
    if connected_components is not None:
        graph = coo_matrix((np.ones(len(rows), np.int8), (rows, idx)), shape=(n, n))
        _, comp = connected_components(graph, directed=False)
        _, first = np.unique(comp, return_index=True)        # (the first occurrence of a component is its lowest index)
        return first[comp].astype(np.int64)
    parent = np.arange(n)
    for a, b in zip(rows.tolist(), idx.tolist()):
        while parent[a] != a:
            a = parent[a]
        while parent[b] != b:
            b = parent[b]
        if a != b:
            parent[max(a, b)] = min(a, b)
    for i in range(n):
        parent[i] = parent[parent[i]]
    return parent.astype(np.int64)


def leg(name, corpus, t, host_reps):
    n = len(corpus)
    _, off = corpus.join_threshold_keys_device(t, 1, skip_same_index=False)      # the total first, then room for all of it
    total = int(off[-1])
    capacity = total + 1024
    keys = torch.zeros(capacity, dtype=torch.int64, device="cuda")
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    host = {}

    def join():
        corpus.join_threshold_keys_device(t, capacity, skip_same_index=False, keys_out=keys, offsets_out=offsets)

    def group():
        lb.group_labels_from_keys_device(keys, n, offsets=offsets, labels=labels, group_count=count, n_slots=total)

    def extra():
        host["extra"] = lb.group_extra_keys_from_labels_device(labels)

    def host_route():
        rows, idx, _, _ = lb.decode_join_keys(keys.cpu(), offsets.cpu())
        got = host_labels(n, rows, idx)
        gone = np.nonzero(got != np.arange(n))[0].astype(np.uint64)
        host["labels"] = got
        host["remove"] = torch.from_numpy((np.uint64(0xFFFFFFFF) - gone).view(np.int64)).cuda()

    for f in (join, group, extra, host_route):               # warm-up, and the two routes against each other
        f()
        torch.cuda.synchronize()
    assert int(offsets[-1]) == total
    got = labels.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(got, host["labels"]), "the device's labels and the host's disagree"
    groups = int(count.item())
    assert groups == int((got == np.arange(n)).sum()) and host["extra"][1] == n - groups == host["remove"].numel()
    assert torch.equal(host["extra"][0][:n - groups] & 0xFFFFFFFF, host["remove"] & 0xFFFFFFFF)
    times = {"join": [], "group": [], "extra": [], "host": []}
    reps = REPS if n < 500_000 else max(2, REPS // 3)          # (a join of 10^12 pairs takes seconds)
    for r in range(reps):
        times["join"].append(device_ms(join))
        times["group"].append(device_ms(group))
        times["extra"].append(wall_ms(extra))
        if r < host_reps:
            times["host"].append(wall_ms(host_route))
    res = {"leg": name, "reps": reps, "host_reps": len(times["host"]), "entries": n, "threshold": t, "edges": total, "groups": groups,
           "largest_group": int(np.bincount(got).max()), "host_union_find": "scipy" if connected_components is not None else "python"}
    for k, v in times.items():
        res[k] = _stats(v)
    res["group_over_join"] = round(res["group"]["median"] / res["join"]["median"], 5)
    res["host_over_device"] = round(res["host"]["median"] / (res["group"]["median"] + res["extra"]["median"]), 2)
    print(json.dumps(res), flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "groups_prof.jsonl"), "a") as f:
        f.write(json.dumps(res) + "\n")


def median_score(n):
    """the median score of a few entries of the synthetic corpus against it: the dense leg's threshold"""
    c = corpus_of(lb.synth_corpus_device(SEED, 0, n, 5, 200))
    s = torch.cat([c.scores_device(lb.Fingerprint.from_bools(O.synth_entry(SEED, e, 5, 200))) for e in (3, 1000, n // 2, n - 7)])
    m = float(s.median())
    c.dispose()
    return m


def run(name, n, t, host_reps, what):
    if ONLY is not None and ONLY != name:
        return
    packed = synth(SEED, n)
    c = corpus_of(packed)
    leg(what, c, t if t is not None else median_score(n), host_reps)
    c.dispose()
    del packed, c
    torch.cuda.empty_cache()


torch.cuda.set_device(0)
run("self100k", 100_000, 0.7, REPS, "keys of the self-join 100000 x 5, t = 0.7")
run("dense", 20_000, None, 1, "keys of the self-join 20000 x 5, dense: t = the scores' median")
run("self1m", 1_000_000, 0.7, REPS, "keys of the self-join 1000000 x 5, t = 0.7")
