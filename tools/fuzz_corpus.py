#!/usr/bin/env python3
"""Randomized GPU-vs-numpy sweep of the corpus queries and maintenance: tools/fuzz_corpus.py [trials] [seed] [--plan-only] [--only T].
The trial is a HISTORY, not a call: a model corpus in numpy (tests/corpus_ref.py) is mutated in step with ONE device handle, and
every read after every step is compared with it word for word -- k_topk, k_threshold, k_query, k_align, k_join, k_join_ragged,
k_groups, k_remove, k_gather, k_ids and their host sides, the plan cache and ring of api_corpus.cpp included: state that
outlives a call (count, offsets, length histogram, plan key, id index, scratch of six families) under an arbitrary history.

A trial draws a uniform corpus (200 Booleans and 1..8 sub-fingerprints, the join's shape, or L of 2, 3, 37, 64, 199) or a ragged
one (L of 1, 2, 37, 64, 199, 200; entries of 1..90 sub-fingerprints, an occasional one of a few hundred), builds it by one or
two appends, sets ids in half of the trials, and then plays 3 to 6 mutations: an append of 1..40 entries (packed or by fingerprint
handle), remove(indices) with its map, remove_keys_device fed the device keys of a threshold, top-K or join call made on the state
before it (zero padding, foreign keys of another index range and repeated keys included, at that call's index base), remove_ids,
deduplicate with drawn rows_per_call and key_capacity (some below a chunk's total: the chunk is redone with half the rows), save
and load into a new handle, a second set_entry_ids over a sub-range, and "remove everything, then append entries of other
lengths".  The generator steers them so that the count returns to an earlier value with other entries, the corpus passes through
empty, the longest entry and the length histogram shrink and grow again, and ids are switched on after a removal.  After the
build and after every step 4 to 7 reads are drawn from: polled query, query_key_device, query_batch, query_packed_keys_device,
scores_device, top-K (host, batch keys-device, packed with lags), threshold (host aligned, batch keys-device, packed with lags),
align_keys_device on top-K keys, match_profile, the self-join of the corpus' kind over a row window and a join of a small second
corpus against it, duplicate_groups, gather_keys_device on a result's keys, gather, gather_ids, ids_from_keys_device,
keys_from_ids_device and entry_ids / len / subfingerprint_total -- every call at least once per trial.  Once per trial save()'s
bytes are compared with those of a fresh handle filled from the model, and at the end every handle is disposed and
debug_live_bytes() is back where the trial started.  Knobs, several at once: the kernel variant, bound pruning and its threshold,
a grid ceiling of 0..3, join and removal scratch limits of one chunk (from the header's formulas), every kind of range, an index
base of 0, small or with base + count = 2^32, K around the number of positives, capacities that cut, fit or leave slack, outputs
given (poisoned, with slack) or allocated by the wrapper, and the null stream or a side stream for all calls of the trial.
About one trial in six is wide and thin: 1..3 sub-fingerprints per entry and a count at an edge (256, 1024, 2048, 4096: the
tiles of the join, the removal, the gather, the top-K candidates and the threshold list) - 1, + 0, + 1 or 2 x edge + 5.
Thresholds are values of the model's own scores, so ties at the threshold are exact.  Keys as 64-bit integers, lags, offsets,
maps and counts exactly, scores as float bit patterns.  A library or HIP error ends the run.  Every trial has a generator of its
own (seed, trial): --only T replays trial T alone (--keep-going reports a refused call as a mismatch and goes on); --plan-only runs the generator and the model without a device (and without
torch) and prints how many trials land in each path bucket (tests/test_fuzz_corpus_cpu.py holds those counts up).

Inputs the generator avoids, because a form refuses them or the header is silent: the uniform join, groups and dedup outside
L = 200 with 1..8 sub-fingerprints; queries of another length than n_sub against a uniform corpus outside query, query_batch,
query_key_device and scores_device (the forms test_gpu_uniform.py shows to take them) and under kernel variant 2; self-joins and
scores_device on an empty corpus; groups and dedup above 64 entries or 1 200 sub-fingerprints (the model's cost, n x n scores, not the device's).

The suite runs 400 trials with seed 20261002 (tests/test_gpu_parity.py).  Wall times on an MI355X machine, process start to exit, in
one session: fuzz_recording.py 200 20261002 took 18.83 s (18.20 s in a second run); this tool took 6.11 s for 100 trials, 15.02 s
for 300, 16.41 s for 350, 17.51 s for 400 and 19.32 s for 450 -- about 0.04 s a trial, two thirds of it the numpy model -- so 400
is the largest measured multiple of 25 that stays below the recording sweep.  Buckets hit by the fewest of the 400 trials: an edge
crossed from below 7 (2048), 8 (4096), 9 (1024) and 13 (256) times, append by fingerprint 17, chunks of the join 20, kernel
variant 2 26; every other bucket 19 times or more.  The counts and the long run are recorded in profiles/fuzz_corpus.txt."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import lbaudiodetective_amd as lb
import align_ref
import corpus_ref as ref
from corpus_ref import Model, bits, pack

EDGES = (256, 1024, 2048, 4096)      # kJoinTileEntries; kRemoveTileEntries, kGatherTileKeys; kCand of k_topk.hip; kThTile
L_UNIFORM = (200, 200, 200, 200, 200, 64, 199, 2, 3, 37)              # (a uniform corpus takes no length below 2)
L_RAGGED = (200, 200, 199, 64, 37, 2, 1)
POISON, POISON32, SLACK = -0x0123456789ABCDEF, 0x5A5A5A5A, 5
GROUPS_MAX, GROUPS_RECORDS = 64, 1200# entries and sub-fingerprints up to which groups and dedup are drawn (n x n scores in the model)
READS = ("query", "query_key_device", "query_batch", "query_packed_keys", "scores_device", "topk_host", "topk_keys", "topk_packed",
         "threshold_host", "threshold_keys", "threshold_packed", "align_keys", "match_profile", "join_self", "join_other",
         "duplicate_groups", "gather_keys", "gather", "gather_ids", "ids_from_keys", "keys_from_ids", "state")
EMPTY_SAFE = ("query", "query_key_device", "query_batch", "topk_keys", "threshold_keys", "gather_keys", "ids_from_keys", "keys_from_ids",
              "state")
MUTATIONS = ("append", "remove", "remove_keys", "remove_ids", "dedup", "save_load", "set_ids", "remove_all")


def rand_fp(rng, n, L, p_zero, p_both):
    pairs = (L + 1) // 2
    pos = rng.random((n, pairs)) < 0.5
    zero = rng.random((n, pairs)) < p_zero
    both = rng.random((n, pairs)) < p_both
    f = np.zeros((n, 2 * pairs), np.uint8)
    f[:, 0::2] = (pos & ~zero) | both
    f[:, 1::2] = (~pos & ~zero) | both
    return np.ascontiguousarray(f[:, :L])


def _noisy(rng, e, p=0.03):
    return e ^ (rng.random(e.shape) < p).astype(np.uint8)


def _pick_threshold(rng, values):
    """a value of the model's own scores (> 0), or the next float above the largest"""
    v = np.sort(np.asarray(values, np.float32).reshape(-1))
    v = v[v > 0]
    if len(v) == 0:
        return np.float32(0.5)
    distinct = np.unique(v)
    kind = rng.choice(5, p=[0.2, 0.06, 0.3, 0.24, 0.2])
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


def _capacity(rng, count):
    return max(1, int(rng.choice([1, count - 1, count, count, count + 1, count + 7])))


class _Gen:
    """the generator's state while one trial is drawn: the true model folded along"""

    def __init__(self, rng):
        self.rng = rng
        self.paths = set()
        self.removals, self.history = [], []                                  # removals of nothing; the states before every step
        self.grow_next, self.back, self.before_bools = 0, 0, []
        self.shrunk = self.removed_any = False

    # -- inputs
    def entries_like(self, n, lens=None):
        rng, t = self.rng, self.t
        if t["kind"] == "uniform":
            lens = np.full(n, t["n_sub"])
        elif lens is None:
            lens = self.lengths(n)
        out = [rand_fp(rng, int(k), t["L"], t["p_zero"], t["p_both"]) for k in lens]
        pool = self.model.bools() + out
        for j in range(n):                                                   # copies of what is there: ties, join pairs, groups
            u = rng.random()
            if u < 0.3 and pool:
                src = pool[int(rng.integers(0, len(pool)))]
                if len(src) == len(out[j]):
                    out[j] = src.copy() if u < 0.12 else _noisy(rng, src, float(rng.choice([0.01, 0.05])))
                elif len(src) > len(out[j]):                                 # a window of a longer entry
                    o = int(rng.integers(0, len(src) - len(out[j]) + 1))
                    out[j] = src[o:o + len(out[j])].copy()
        if rng.integers(0, 6) == 0:
            out[int(rng.integers(0, n))][:] = 0
        return out

    def lengths(self, n):
        rng = self.rng
        if self.t["wide"]:
            return rng.integers(1, 4, n)
        shape = int(rng.integers(0, 5))
        if shape == 0:
            lens = rng.integers(1, 12, n)
        elif shape == 1:
            lens = rng.integers(20, 51, n)
        elif shape == 2:
            lens = rng.integers(1, 91, n)
        elif shape == 3:
            lens = np.full(n, int(rng.integers(1, 40)))
        else:
            lens = rng.integers(1, 25, n)
            lens[rng.integers(0, n)] = int(rng.integers(150, 320))
        return lens.astype(np.int64)

    def base(self):
        kind = self.t["base_kind"]
        return 0 if kind == 0 else self.t["base_small"] if kind == 1 else (1 << 32) - len(self.model)

    # -- one read, its arguments drawn against the model's state
    def read(self, call):
        rng, m, t = self.rng, self.model, self.t
        n, Q = len(m), t["queries"]
        same = [qi for qi in range(len(Q)) if t["kind"] == "ragged" or len(Q[qi]) == t["n_sub"]]
        anyq = list(range(len(Q))) if t["variant"] != 2 else same
        rd = {"call": call, "base": self.base(), "given": bool(rng.integers(0, 2))}
        one = lambda pool: int(pool[int(rng.integers(0, len(pool)))])
        scores = lambda qi: m.scores(("q", qi), Q[qi])[0]
        if t["kind"] == "ragged" and n:                                      # which side slides: read off the lengths
            lens = np.array([len(e) for e in m.bools()])
            for qi in range(len(Q)):
                self.paths.update(name for name, hit in (("case_a", (lens > len(Q[qi])).any()), ("equal_length", (lens == len(Q[qi])).any()),
                                                         ("case_b", (lens < len(Q[qi])).any())) if hit)
        if call in ("query", "query_key_device", "scores_device"):
            rd["q"] = one(anyq)
        elif call == "query_batch":
            rd["qs"] = [one(anyq) for _ in range(int(rng.integers(1, 4)))]
        elif call in ("query_packed_keys", "topk_packed", "threshold_packed"):
            rd["qs"] = [0, 1] if rng.integers(0, 2) else [one(same)]           # (queries 0 and 1 have one length)
        elif call in ("topk_host", "threshold_host", "match_profile"):
            rd["q"] = one(same)
        elif call in ("topk_keys", "threshold_keys", "align_keys"):
            rd["qs"] = [one(same) for _ in range(int(rng.integers(1, 4)))]
        if call in ("topk_host", "topk_keys", "topk_packed", "align_keys"):
            positive = int((scores(rd["qs"][0] if "qs" in rd else rd["q"]) > 0).sum())
            rd["k"] = max(1, min(1024, int(rng.choice([1, 2, positive - 1, positive, positive + 1, positive + 9]))))
            if rd["k"] > positive:
                self.paths.add("k_above_positive")
        if call in ("threshold_host", "threshold_keys", "threshold_packed"):
            qs = rd["qs"] if "qs" in rd else [rd["q"]]
            rd["t"] = float(_pick_threshold(rng, np.concatenate([scores(qi) for qi in qs]) if n else []))
            counts = [int(ref.reaches(scores(qi), rd["t"]).sum()) for qi in qs]
            rd["capacity"] = _capacity(rng, max(counts))
            self.capacity_paths(rd["capacity"], counts)
            rd["empty"] = max(counts) == 0
        if call == "match_profile":
            rd["entry"] = int(rng.integers(0, n))
        if call in ("join_self", "join_other"):
            other = call == "join_other"
            rows_n = len(t["other"]) if other else n
            if not other and 64 < n <= 140 and m.total <= 1500 and (t["join_limit"] or rng.integers(0, 2) == 0):
                first, count = 0, n                                          # every row: more than one chunk of 64 under a limit
            else:
                count = int(rng.integers(1, min(rows_n, 6) + 1))
                first = int(rng.integers(0, rows_n - count + 1))
            rows = self.rows(other, first, count)
            sc = np.concatenate([m.scores(qid, q)[0] for _, qid, q in rows])
            if not other:                                                    # (the self-matches of 1.0 are skipped by default)
                sc = np.concatenate([np.delete(m.scores(qid, q)[0], r) for r, qid, q in rows]) if n > 1 else sc
            rd.update(first=first, count=count, t=float(_pick_threshold(rng, sc)), skip=[None, None, True, False][int(rng.integers(0, 4))])
            total = int(m.join(rows, rd["t"], 1, (not other) if rd["skip"] is None else rd["skip"])[2][-1])
            rd["capacity"] = _capacity(rng, total)
            self.capacity_paths(rd["capacity"], [total])
            rd["empty"] = total == 0
            if t["join_limit"] and count > 64:
                self.paths.add("chunks:join")
        if call == "duplicate_groups":
            rd.update(self.groups_args())
        if call in ("gather_keys", "ids_from_keys"):
            rd["producer"] = self.producer()
            rd["base"] = rd["producer"]["base"]
            if rng.integers(0, 3) == 0:                                      # read at another base: the keys name other entries
                shift = int(rng.choice([max(1, n // 2), n + 3]))              # half of the keys, or none, name entries of this range
                rd["base"] = rd["base"] + shift if rd["base"] + shift + n <= 1 << 32 else 0
                self.paths.add("foreign_keys")
            if call == "gather_keys":
                keys = model_read(m, t, rd["producer"])[0]
                total = int(m.gather(ref.key_indices(keys, rd["base"], n))[1][-1])
                rd["capacity"] = None if rng.integers(0, 3) == 0 else max(0, int(rng.choice([total - 1, total, total + 3, total // 2])))
                if rd["capacity"] is not None:
                    self.capacity_paths(rd["capacity"], [total])
        if call == "gather":
            rd["indices"] = [int(x) for x in rng.integers(0, n, int(rng.integers(0, 9)))] if n else []
            if rd["indices"] and rng.integers(0, 2):
                rd["indices"].append(rd["indices"][0])
        if call in ("gather_ids", "keys_from_ids"):
            rd["ids"] = self.some_ids()
        return rd

    def capacity_paths(self, capacity, counts):
        if any(capacity < c for c in counts):
            self.paths.add("capacity_cuts")
        if any(capacity == c and c > 0 for c in counts):
            self.paths.add("capacity_exact")

    def rows(self, other, first, count):
        if other:
            return [(i, ("o", i), self.t["other"][i]) for i in range(first, first + count)]
        return self.model.self_rows(first, count)

    def groups_args(self):
        rng, m = self.rng, self.model
        n = len(m)
        sc = np.concatenate([np.delete(m.scores(qid, q)[0], r) for r, qid, q in m.self_rows(0, n)]) if n > 1 else np.zeros(0, np.float32)
        t = float(_pick_threshold(rng, sc))
        rows = [None, 1, 3, 7, 64][int(rng.integers(0, 5))]
        per_row = np.diff(m.join(m.self_rows(0, n), t, 1, True)[2])
        total, widest = int(per_row.sum()), int(per_row.max()) if n else 0
        per_call = n if rows is None else max(1, min(rows, n))
        chunk = int(per_row[:per_call].sum())                                # the first chunk's total
        capacity = max(1, total + int(rng.integers(0, 5)))
        if per_call > 1 and chunk > max(1, widest) and rng.integers(0, 2):
            capacity = int(rng.integers(max(1, widest), chunk))              # below the chunk, not below a row: redone with half
            self.paths.add("dedup_redone_with_half_the_rows")
        return {"t": t, "rows_per_call": rows, "key_capacity": capacity}

    def producer(self):
        """a call whose device keys feed a removal, a gather or the ids: a threshold row, a top-K row or a join's key block"""
        kinds = ["threshold_keys", "topk_keys"] + (["join_self"] if self.joinable() and len(self.model) else [])
        rd = self.read(kinds[int(self.rng.integers(0, len(kinds)))])
        rd["given"] = True
        keys = model_read(self.model, self.t, rd)[0]
        if (np.asarray(keys) == 0).any():
            self.paths.add("keys_with_padding")
        return rd

    def joinable(self):
        t = self.t
        if t["kind"] == "uniform":
            return t["L"] == 200 and t["n_sub"] <= 8
        return max([len(e) for e in self.model.bools()] + [len(e) for e in t["other"]]) <= 1024

    def some_ids(self):
        rng, m = self.rng, self.model
        have = [int(x) for x in m.entry_ids().tolist() if x]
        out = [have[int(rng.integers(0, len(have)))] for _ in range(int(rng.integers(0, 6)))] if have else []
        out += [0, int(rng.integers(1, 1 << 62)) | 1 << 62][:int(rng.integers(0, 3))]   # id 0 and an id no entry has
        if out and rng.integers(0, 2):
            out.append(out[0])
        return [out[i] for i in rng.permutation(len(out))]

    # -- one mutation
    def step(self, op):
        rng, m, t = self.rng, self.model, self.t
        n = len(m)
        st = {"op": op}
        if op == "append":
            room = t["entry_capacity"] - n
            k = int(min(room, rng.integers(1, 41)))
            new = self.entries_like(k, lens=self.next_lens(k) if t["kind"] == "ragged" else None)
            if t["kind"] == "ragged":
                while new and m.total + sum(len(e) for e in new) > self.record_capacity:
                    new.pop()
            st["how"] = "fingerprint" if (len(new) <= 4 and rng.integers(0, 2)) else "packed"
            st["entries"] = new
        elif op in ("remove", "remove_all"):
            st["op"] = "remove"
            kind = 5 if op == "remove_all" else int(rng.choice(6, p=[0.06, 0.3, 0.2, 0.14, 0.2, 0.1]))
            if kind == 0 or n == 0:
                idx = []
            elif kind == 1:
                idx = rng.choice(n, max(1, n // int(rng.integers(2, 9))), replace=False).tolist()
            elif kind == 2:
                idx = list(range(int(rng.integers(0, n)), n))                 # a tail: nothing moves
            elif kind == 3:
                idx = [0] + rng.choice(n, max(1, n // 2), replace=False).tolist()
            elif kind == 4 and t["kind"] == "ragged":
                lens = np.array([len(e) for e in m.bools()])
                idx = np.flatnonzero(lens >= np.sort(lens)[len(lens) // 2]).tolist() if lens.max() > lens.min() else [n - 1]
            elif kind == 4:
                idx = list(range(0, n, 2))
            else:
                idx = list(range(n))
            if idx and rng.integers(0, 2):
                idx = idx + idx[:3]
            st["indices"] = [int(i) for i in idx]
        elif op == "remove_keys":
            st["producer"] = self.producer()
            st["base"] = st["producer"]["base"]
            b, extra = st["base"], []
            if rng.integers(0, 2):                                           # keys of another index range, and zero keys
                outside = [x for x in (b - 1, b + n, b + n + 5, 0 if b > 0 else None) if x is not None and 0 <= x < 1 << 32]
                extra = [int(ref.make_keys([0.9], [x])[0]) for x in outside] + [0, 0]
                self.paths.add("foreign_keys")
                self.paths.add("keys_with_padding")
            st["extra"] = extra
            st["repeat"] = int(rng.integers(0, 6))
            if st["repeat"]:
                self.paths.add("repeated_keys")
        elif op == "remove_ids":
            st["ids"] = self.some_ids()
        elif op == "dedup":
            st.update(self.groups_args())
        elif op == "set_ids":
            first = int(rng.integers(0, n)) if n else 0
            k = int(rng.integers(1, n - first + 1)) if n else 0
            if m.ids is None and n:
                first, k = (0, n) if rng.integers(0, 2) else (first, k)
            ids = [int(x) for x in rng.integers(1, 1 << 62, k)]
            if k >= 2 and rng.integers(0, 2):
                ids[-1] = ids[0]                                             # two entries share an id: the lowest index wins
            if k >= 3 and rng.integers(0, 3) == 0:
                ids[1] = 0
            st.update(first=first, ids=ids)
        return st

    def next_lens(self, k):
        """ragged appends: after the longest entries went, longer ones come back"""
        lens = self.lengths(k)
        if self.grow_next and not self.t["wide"]:
            lens[int(self.rng.integers(0, k))] = self.grow_next + int(self.rng.integers(1, 9))
            self.grow_next = 0
        return lens


def apply_step(m, trial, st):
    """one mutation on a model -> what the device call returns"""
    op = st["op"]
    if op == "append":
        m.append(st["entries"])
        return ()
    if op == "remove":
        removed, new = m.remove(st["indices"])
        return (np.int64(removed), new)
    if op == "remove_keys":
        removed, new = m.remove_keys(_fed_keys(model_read(m, trial, st["producer"])[0], st), st["base"])
        return (np.int64(removed), new)
    if op == "remove_ids":
        removed, _ = m.remove_keys(m.keys_from_ids(st["ids"]))
        return (np.int64(removed),)
    if op == "dedup":
        removed, labels = m.dedup(st["t"])
        return (np.int64(removed), labels)
    if op == "set_ids":
        m.set_ids(st["first"], st["ids"])
        return ()
    if op == "save_load":
        m.stale = {}
        return ()
    raise ValueError(op)


def _fed_keys(keys, st):
    keys = np.asarray(keys).astype(np.uint64).reshape(-1)
    return np.concatenate([keys, np.array(st["extra"], np.uint64), keys[:st["repeat"]]])


def model_read(m, trial, rd):
    """one read on a model -> a tuple of arrays, the words the device call must write"""
    call, Q, base, n = rd["call"], trial["queries"], rd["base"], len(m)
    S = lambda qi: m.scores(("q", qi), Q[qi])
    i64 = lambda x: np.asarray(x, np.int64)
    if call == "query":
        _, idx, s = m.top1(S(rd["q"])[0])
        return (i64(idx), np.float32(s))
    if call == "query_key_device":
        return (np.array([m.top1(S(rd["q"])[0], base)[0]], np.uint64),)
    if call == "query_batch":
        got = [m.top1(S(qi)[0]) for qi in rd["qs"]]
        return (i64([g[1] for g in got]), np.array([g[2] for g in got], np.float32))
    if call == "query_packed_keys":
        return (np.array([m.top1(S(qi)[0], base)[0] for qi in rd["qs"]], np.uint64),)
    if call == "scores_device":
        return (S(rd["q"])[0],)
    if call == "topk_host":
        _, _, idx, sc = m.topk(*S(rd["q"]), rd["k"])
        return (idx, sc)
    if call in ("topk_keys", "topk_packed"):
        got = [m.topk(*S(qi), rd["k"], base) for qi in rd["qs"]]
        keys = np.concatenate([g[0] for g in got])
        return (keys,) if call == "topk_keys" else (keys, np.concatenate([g[1] for g in got]))
    if call == "threshold_host":
        _, lags, count, idx, sc = m.threshold(*S(rd["q"]), rd["t"], rd["capacity"])
        return (idx, sc, lags[:len(idx)], i64(count))
    if call in ("threshold_keys", "threshold_packed"):
        got = [m.threshold(*S(qi), rd["t"], rd["capacity"], base) for qi in rd["qs"]]
        keys, counts = np.concatenate([g[0] for g in got]), i64([g[2] for g in got])
        return (keys, counts) if call == "threshold_keys" else (keys, counts, np.concatenate([g[1] for g in got]))
    if call == "align_keys":
        lags, scores = [], []
        for qi in rd["qs"]:
            sc, lg = S(qi)
            at = ref.key_indices(m.topk(sc, lg, rd["k"], base)[0], base, n)
            lags.append(np.array([lg[i] if i >= 0 else 0 for i in at], np.int32))
            scores.append(np.array([sc[i] if i >= 0 else 0 for i in at], np.float32))
        return (np.concatenate(lags), np.concatenate(scores))
    if call == "match_profile":
        q, _ = align_ref.profile(Q[rd["q"]], m.entries[rd["entry"]][1], m.range)
        return (q, i64(0))
    if call in ("join_self", "join_other"):
        other = call == "join_other"
        rows = [(i, ("o", i), trial["other"][i]) for i in range(rd["first"], rd["first"] + rd["count"])] if other else \
            m.self_rows(rd["first"], rd["count"])
        keys, lags, offsets, _ = m.join(rows, rd["t"], rd["capacity"], (not other) if rd["skip"] is None else rd["skip"], base)
        return (keys, lags, offsets) if m.ragged else (keys, offsets)
    if call == "duplicate_groups":
        labels, groups = m.labels(rd["t"])
        return (labels, i64(groups))
    if call == "gather_keys":
        keys = model_read(m, trial, rd["producer"])[0]
        return m.gather(ref.key_indices(keys, base, n), rd["capacity"])
    if call == "gather":
        return m.gather(rd["indices"])
    if call == "gather_ids":
        return m.gather(ref.key_indices(m.keys_from_ids(rd["ids"]), 0, n))
    if call == "ids_from_keys":
        return (m.ids_from_keys(model_read(m, trial, rd["producer"])[0], base),)
    if call == "keys_from_ids":
        return (m.keys_from_ids(rd["ids"], base),)
    if call == "state":
        return (m.entry_ids(), i64(n), i64(m.total), i64(m.ids is not None))
    raise ValueError(call)


def make_trial(rng):
    """one trial as a plain dict: the kind, L, n_sub, the capacities, the queries, the second corpus, the knobs, the stages (each
    a step -- None for the build -- and the reads after it) and the path buckets the trial lands in (`paths`).  Needs no GPU."""
    g = _Gen(rng)
    kind = "uniform" if rng.integers(0, 2) else "ragged"
    wide = bool(rng.integers(0, 6) == 0)
    L = int(rng.choice(L_UNIFORM if kind == "uniform" else L_RAGGED))
    n_sub = 0 if kind == "ragged" else int(rng.integers(1, 4)) if wide else int(rng.integers(1, 9)) if L == 200 else int(rng.integers(1, 6))
    variants = (0, 0, 1, 3, 4) if kind == "ragged" else (0, 0, 1, 2) if L == 200 else (0, 1)
    t = g.t = {"kind": kind, "wide": wide, "L": L, "n_sub": n_sub,
               "range": int(rng.choice([0, 0, 1, L // 2 + 1, L - 1, L, L + 7])),
               "p_zero": float(rng.choice([0.0, 0.02, 0.3])), "p_both": float(rng.choice([0.0, 0.0, 0.05])),
               "variant": int(rng.choice(variants)), "pruning": bool(rng.integers(0, 2)),
               "pruning_threshold": float(rng.choice([0.7, 0.5, 0.95])), "grid_ceiling": int(rng.integers(0, 4)),
               "join_limit": bool(rng.integers(0, 2)), "remove_limit": bool(rng.integers(0, 2)),
               "base_kind": int(rng.integers(0, 3)), "base_small": int(rng.integers(1, 1 << 20)), "side_stream": bool(rng.integers(0, 2))}
    m = g.model = Model(L, n_sub, t["range"])
    if wide:
        edge = int(rng.choice(EDGES))
        n0 = int(rng.choice([edge - 1, edge - 1, edge, edge + 1, 2 * edge + 5]))
    else:
        lo, hi = ((1, 13), (13, 71), (13, 71), (65, 141), (141, 301))[int(rng.integers(0, 5))]
        n0 = int(rng.integers(lo, hi))
    first = g.entries_like(n0)
    if kind == "ragged":
        while len(first) > 1 and sum(len(e) for e in first) > 2500 + 3 * len(first) * wide:
            first = first[:len(first) * 3 // 4]
        n0 = len(first)
    t["entry_capacity"] = n0 + 130
    g.record_capacity = t["record_capacity"] = sum(len(e) for e in first) + 2500 if kind == "ragged" else 0
    cut = int(rng.integers(0, n0 + 1))
    stages = [{"steps": [{"op": "append", "how": "packed", "entries": first[:cut]}, {"op": "append", "how": "packed", "entries": first[cut:]}]}]
    stages[0]["steps"] = [s for s in stages[0]["steps"] if s["entries"]]
    m.append(first)
    # the second corpus (never mutated) and the queries
    t["other"] = g.entries_like(int(rng.integers(3, 7)))
    src = first[int(rng.integers(0, n0))]
    if kind == "uniform":
        q0, q1 = _noisy(rng, src), _noisy(rng, first[int(rng.integers(0, n0))], 0.1)
        q2 = first[int(rng.integers(0, n0))].copy()
        nq = int(rng.choice([1, max(1, n_sub - 1), n_sub + 1, 2 * n_sub + 1]))
        q3 = rand_fp(rng, nq, L, t["p_zero"], t["p_both"])
        q3[:min(nq, n_sub)] = src[:min(nq, n_sub)]
    else:
        nq = int(rng.choice([1, 2, 5, 8, 13, 21, 33, 48, 70]))
        q0, q1 = rand_fp(rng, nq, L, t["p_zero"], t["p_both"]), rand_fp(rng, nq, L, t["p_zero"], t["p_both"])
        for q in (q0, q1):                                                   # a window of an entry, or an entry inside the query
            s = first[int(rng.integers(0, n0))]
            k = min(nq, len(s))
            o, at = int(rng.integers(0, len(s) - k + 1)), int(rng.integers(0, nq - k + 1))
            q[at:at + k] = _noisy(rng, s[o:o + k], 0.02) if rng.integers(0, 2) else s[o:o + k]
        q2 = src.copy()                                                      # equal length: a score of 1.0
        longest = max(first, key=len)
        q3 = np.concatenate([rand_fp(rng, int(rng.integers(1, 5)), L, t["p_zero"], t["p_both"]), longest[:40]])   # case B for most
    t["queries"] = [q0, q1, q2, q3]
    if t["variant"] == 2 and kind == "uniform":
        t["queries"][3] = _noisy(rng, q2, 0.2)
    ids0 = bool(rng.integers(0, 2))
    if ids0:
        stages[0]["steps"].append(g.step("set_ids"))
        stages[0]["steps"][-1].update(first=0, ids=(stages[0]["steps"][-1]["ids"] + [int(x) for x in rng.integers(1, 1 << 62, n0)])[:n0])
        apply_step(m, t, stages[0]["steps"][-1])
    # the history: one steered pair of steps and one to four free ones
    plot = int(rng.integers(0, 4))
    free = lambda: str(rng.choice(MUTATIONS, p=[0.16, 0.14, 0.2, 0.12, 0.14, 0.1, 0.1, 0.04]))
    ops = [free() for _ in range(int(rng.integers(1, 5)))]
    pair = (("remove", "append"), ("remove_all", "append"), ("remove", "append"), ("remove", "set_ids"))[plot]
    at = int(rng.integers(0, len(ops) + 1))
    ops[at:at] = pair
    if wide and n0 < edge:                                                   # the edge is crossed from below by an append
        ops[0:0] = ["append"]
        at += 1
    deck, seen = [], set()
    save_at = int(rng.integers(0, len(ops) + 1))
    for s, op in enumerate([None] + ops):
        n = len(m)
        if op is not None:
            steered = s - 1 == at and plot in (0, 2)
            if op == "dedup" and not (g.joinable() and 0 < n <= GROUPS_MAX and m.total <= GROUPS_RECORDS):
                op = "remove"
            if op == "remove_ids" and m.ids is None:
                op = "set_ids" if n else "append"
            if op in ("remove_keys", "set_ids") and n == 0:
                op = "append"
            if op == "append" and n >= t["entry_capacity"]:
                op = "remove"
            st = g.step(op)
            if steered and plot == 0 and n >= 2:                              # the count comes back with other entries
                st["indices"] = rng.choice(n, min(n - 1, 40, max(1, n // 3)), replace=False).tolist()
                g.back = len(set(st["indices"]))
            if steered and plot == 2 and kind == "ragged" and n >= 2:         # the longest entries go
                lens = np.array([len(e) for e in m.bools()])
                if lens.max() > lens.min():
                    st["indices"] = np.flatnonzero(lens > np.median(lens)).tolist()
                    g.grow_next = int(lens.max())
            if s - 2 == at and plot == 0 and op == "append" and g.back:
                st["entries"] = g.entries_like(g.back, lens=g.lengths(g.back) if kind == "ragged" else None)
                while kind == "ragged" and st["entries"] and m.total + sum(len(e) for e in st["entries"]) > g.record_capacity:
                    st["entries"].pop()                                      # (a loaded corpus has room in proportion to what it held)
                st["how"] = "packed"
            before = {"n": n, "ids": m.ids is not None, "max": max([len(e) for e in m.bools()], default=0),
                      "hist": len({len(e) for e in m.bools()})}
            g.history.append(before)
            g.before_bools = m.bools()
            want = apply_step(m, t, st)
            if st["op"] == "save_load" and kind == "ragged":                 # Load reserves records in proportion to the entry capacity
                cap = t["entry_capacity"]
                g.record_capacity = max(cap, -(-m.total * cap // n)) if n else cap * 64
            _note_step(g, t, st, before, want)
            stages.append({"steps": [st]})
        # the reads of this stage
        n = len(m)
        usable = [c for c in READS if _usable(g, c)]
        k = int(rng.integers(4, 8))
        reads = []
        for _ in range(k):
            if not [c for c in deck if c in usable]:
                deck = deck + [str(c) for c in rng.permutation(READS)]
            call = next(c for c in deck if c in usable)
            deck.remove(call)
            reads.append(call)
        if s == len(ops):                                                    # every call at least once per trial
            reads += [c for c in usable if c not in seen and c not in reads]
        seen.update(reads)
        stages[-1]["reads"] = [g.read(c) for c in reads]
        stages[-1]["save_bytes"] = s == save_at
        for rd in stages[-1]["reads"]:
            g.paths.add("read:" + rd["call"])
    t["stages"] = stages
    _note_trial(g, t)
    t["paths"] = sorted(g.paths)
    t["list_reads"] = [rd["empty"] for rd in list_reads(t)]
    t["removals"] = g.removals
    t["final_count"] = len(m)
    t["cache"] = m.cache
    return t


def list_reads(trial):
    """every threshold and join read of a trial, those that feed a gather, the ids or a removal included"""
    out = []

    def walk(rd):
        if "empty" in rd:
            out.append(rd)
        if "producer" in rd:
            walk(rd["producer"])
    for stage in trial["stages"]:
        for x in stage["steps"] + stage["reads"]:
            walk(x)
    return out


def _usable(g, call):
    m, t = g.model, g.t
    n = len(m)
    if n == 0:
        return call in EMPTY_SAFE
    if call in ("join_self", "join_other"):
        return g.joinable()
    if call == "duplicate_groups":
        return g.joinable() and n <= GROUPS_MAX and m.total <= GROUPS_RECORDS
    return True


def _note_step(g, t, st, before, want):
    m, paths = g.model, g.paths
    n, old = len(m), before["n"]
    paths.add("mutation:" + st["op"] + ("_" + st["how"] if st["op"] == "append" else ""))
    if st["op"] in ("remove", "remove_keys", "remove_ids", "dedup"):
        g.removals.append(int(want[0]) == 0)
        lowest = int(np.flatnonzero(want[1] == ref.GONE)[0]) if len(want) > 1 and (np.asarray(want[1]) == ref.GONE).any() else None
        if st["op"] == "dedup":
            lab = want[1]
            gone = np.flatnonzero(lab != np.arange(len(lab)))
            lowest = int(gone[0]) if len(gone) else None
        if lowest is not None and t["remove_limit"]:
            items = sum(len(e) for e in g.before_bools[lowest:]) if t["kind"] == "ragged" else old - lowest
            if items > 1024:
                paths.add("chunks:remove")
        for edge in EDGES:
            if old >= edge > n:
                paths.add(f"edge_{edge}_from_above")
    if st["op"] == "append":
        for edge in EDGES:
            if old < edge <= n:
                paths.add(f"edge_{edge}_from_below")
    hist = g.history
    if n == 0 and old > 0:
        paths.add("state:through_empty")
    if n > 0 and any(h["n"] == n for h in hist[:-1]) and st["op"] == "append":
        paths.add("state:count_returns")
    now_max = max([len(e) for e in m.bools()], default=0)
    if now_max < before["max"] or len({len(e) for e in m.bools()}) < before["hist"]:
        g.shrunk = True
    if g.shrunk and st["op"] == "append" and now_max > before["max"]:
        paths.add("state:ne_max_shrinks_and_grows")
    if st["op"] == "set_ids" and not before["ids"] and m.ids is not None and g.removed_any:
        paths.add("state:ids_on_after_removal")
    if st["op"] in ("remove", "remove_keys", "remove_ids", "dedup") and int(want[0]):
        g.removed_any = True


def _note_trial(g, t):
    paths = g.paths
    paths.add("kind:" + t["kind"])
    paths.add("wide" if t["wide"] else "small")
    paths.add(f"variant_{t['variant']}")
    paths.add("pruning_on" if t["pruning"] else "pruning_off")
    paths.add(f"grid_ceiling_{t['grid_ceiling']}")
    paths.add("join_limit" if t["join_limit"] else "join_default")
    paths.add("remove_limit" if t["remove_limit"] else "remove_default")
    paths.add("range_0" if t["range"] == 0 else "range_below_L" if t["range"] < t["L"] else "range_at_or_above_L")
    paths.add(("index_base_0", "index_base_small", "index_base_top")[t["base_kind"]])
    paths.add("side_stream" if t["side_stream"] else "null_stream")
    if t["L"] % 2:
        paths.add("odd_L")
    reads = [rd for st in t["stages"] for rd in st["reads"]]
    paths.add("outputs_given" if any(rd["given"] for rd in reads) else "outputs_allocated")
    if any(not rd["given"] for rd in reads):
        paths.add("outputs_allocated")


def expected(trial):
    """the model folded through the trial's steps: per stage (the steps' results, the reads' words).  The scores of (query, entry)
    pairs are the trial's own (`cache`, made once by make_trial); every rule behind them is applied anew."""
    m = Model(trial["L"], trial["n_sub"], trial["range"])
    m.cache = trial["cache"]
    out = []
    for stage in trial["stages"]:
        steps = [apply_step(m, trial, st) for st in stage["steps"]]
        out.append((steps, [model_read(m, trial, rd) for rd in stage["reads"]]))
    return out


def same_values(a, b):
    def norm(x):
        x = np.asarray(x)
        return x.view(np.uint32) if x.dtype == np.float32 else x.astype(np.int64).view(np.uint64) if x.dtype == np.int64 else x
    return len(a) == len(b) and all(norm(x).shape == norm(y).shape and np.array_equal(norm(x), norm(y)) for x, y in zip(a, b))


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
        if x.shape != y.shape:
            return f"output {i}: {x.shape[0]} words for {y.shape[0]}"
        d = np.flatnonzero(bits(x) != bits(y)) if x.dtype == np.float32 else np.flatnonzero(x.astype(np.uint64) != y.astype(np.uint64)) \
            if x.dtype.kind in "iu" and x.dtype.itemsize == 8 else np.flatnonzero(x != y)
        if len(d):
            return f"output {i} word {int(d[0])}: got {x[d[0]]!r} want {y[d[0]]!r}"
    return f"{len(a)} outputs for {len(b)}"


def describe(trial):
    return (f"{trial['kind']} L {trial['L']} n_sub {trial['n_sub']} range {trial['range']} wide {trial['wide']} variant {trial['variant']} "
            f"pruning {trial['pruning']} {trial['pruning_threshold']} grid {trial['grid_ceiling']} limits {trial['join_limit']} "
            f"{trial['remove_limit']} base kind {trial['base_kind']} side stream {trial['side_stream']} steps "
            f"{[s['op'] for st in trial['stages'] for s in st['steps']]}")


# ---- the device half ---------------------------------------------------------------------------------------------------------------
class _Outputs:
    """poison-filled device buffers with slack behind them"""

    def __init__(self, torch):
        self.torch, self.made = torch, []

    def new(self, n, kind):
        dtype, poison = (self.torch.int64, POISON) if kind == "i64" else (self.torch.int32, POISON32)
        t = self.torch.full((n + SLACK,), poison, dtype=dtype, device="cuda")
        self.made.append((t, n, poison))
        return t

    def slack_intact(self):
        return all(bool((t[n:] == poison).all()) for t, n, poison in self.made)


class _Device:
    """one trial's device side: the handle under test, the second corpus, the queries"""

    def __init__(self, torch, trial, tmp):
        self.torch, self.t, self.tmp = torch, trial, tmp
        self.stream = torch.cuda.Stream() if trial["side_stream"] else None
        self.corpus = self.fresh()
        self.configure(self.corpus)
        self.other = self.fresh(len(trial["other"]) + 1, sum(len(e) for e in trial["other"]) + 8)
        self.append(self.other, trial["other"], "packed")
        self.fps = [lb.Fingerprint.from_bools(q) for q in trial["queries"]]
        self.packed = [self.up(pack(q)) for q in trial["queries"]]
        self.handles = [self.other]

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def fresh(self, entries=None, records=None):
        t = self.t
        if t["kind"] == "uniform":
            return lb.Corpus(t["L"], t["n_sub"], entries or t["entry_capacity"])
        return lb.Corpus.ragged(t["L"], entries or t["entry_capacity"], records or t["record_capacity"])

    def configure(self, c):
        t = self.t
        c.set_kernel_variant(t["variant"])
        if t["kind"] == "ragged":
            c.set_bound_pruning(t["pruning"])
            c.set_bound_pruning_threshold(t["pruning_threshold"])

    def limits(self, c, rows_entries):
        """one chunk of 64 rows (the header's formulas), one tile of the removal's bounce buffer"""
        t = self.t
        tiles = (max(1, rows_entries) + 255) // 256
        per_row = (584 if t["kind"] == "uniform" else 8) + 8 * tiles
        c.set_join_scratch_limit(16 + 64 * per_row + 4 * tiles if t["join_limit"] else 0)
        c.set_remove_scratch_limit(1024 * c.entry_stride_bytes if t["remove_limit"] else 0)

    def append(self, c, entries, how):
        if not entries:
            return
        if how == "fingerprint":
            for e in entries:
                fp = lb.Fingerprint.from_bools(e)
                c.append_fingerprint(fp)
                fp.dispose()
        elif self.t["kind"] == "uniform":
            c.append_packed_device(self.up(pack(np.concatenate(entries)).reshape(len(entries), self.t["n_sub"], 32)), stream=self.stream)
        else:
            c.append_ragged_packed_device(self.up(pack(np.concatenate(entries))), np.array([len(e) for e in entries], np.uint32),
                                          stream=self.stream)
        self.torch.cuda.synchronize()

    def host(self, x, n, view=None):
        a = x.reshape(-1)[:n].cpu().numpy()
        return a.view(view) if view is not None else a

    def saved(self, c, name):
        path = os.path.join(self.tmp, name)
        c.save(path)
        with open(path, "rb") as f:
            return f.read()

    # -- a mutation
    def step(self, st, model):
        torch, c, s = self.torch, self.corpus, self.stream
        op = st["op"]
        self.limits(c, len(c))
        if op == "append":
            self.append(c, st["entries"], st["how"])
            return ()
        if op == "remove":
            removed, new = c.remove(st["indices"], return_map=True)
            return (np.int64(removed), new)
        if op == "remove_keys":
            keys = self.read(st["producer"], model, raw=True)
            fed = torch.cat([keys.reshape(-1), self.up(np.array(st["extra"], np.uint64).view(np.int64)), keys.reshape(-1)[:st["repeat"]]])
            o = _Outputs(torch)
            new = o.new(len(c), "i32")
            n_old = len(c)
            removed = c.remove_keys_device(fed.contiguous(), index_base=st["base"], new_indices_out=new, stream=s)
            self.intact = self.intact and o.slack_intact()
            return (np.int64(removed), self.host(new, n_old, np.uint32))
        if op == "remove_ids":
            return (np.int64(c.remove_ids(st["ids"], stream=s)),)
        if op == "dedup":
            removed, labels = c.deduplicate(st["t"], key_capacity=st["key_capacity"], rows_per_call=st["rows_per_call"],
                                            range_=self.t["range"], stream=s)
            return (np.int64(removed), labels.cpu().numpy())
        if op == "set_ids":
            ids = np.array(st["ids"], np.uint64)
            c.set_entry_ids(self.up(ids.view(np.int64)) if len(ids) % 2 else ids, first=st["first"], stream=s)
            return ()
        if op == "save_load":
            path = os.path.join(self.tmp, "history.bin")
            c.save(path)
            new = lb.Corpus.load(path, self.t["L"], self.t["n_sub"], self.t["entry_capacity"])
            c.dispose()
            self.corpus = new
            self.configure(new)
            return ()
        raise ValueError(op)

    # -- a read
    def read(self, rd, model, raw=False):
        """the call on the device -> the tuple model_read gives (raw: the device key block as it is)"""
        torch, c, s, t = self.torch, self.corpus, self.stream, self.t
        call, base, rg, n = rd["call"], rd["base"], t["range"], len(c)
        fps, packed = self.fps, self.packed
        o = _Outputs(torch)
        out = lambda words, kind: o.new(words, kind) if rd["given"] else None
        u64, u32, i32, f32 = np.uint64, np.uint32, np.int32, np.float32
        i64 = lambda x: np.asarray(x, np.int64)
        self.limits(c, n)
        got = None
        if call == "query":
            idx, sc = c.query(fps[rd["q"]], rg)
            got = (i64(idx), f32(sc))
        elif call == "query_key_device":
            key = o.new(1, "i64")
            c.query_key_device(fps[rd["q"]], key, rg, base, stream=s)
            got = (self.host(key, 1, u64),)
        elif call == "query_batch":
            res = c.query_batch([fps[qi] for qi in rd["qs"]], rg)
            got = (i64([r[0] for r in res]), np.array([r[1] for r in res], f32))
        elif call == "query_packed_keys":
            nq = len(rd["qs"])
            block = torch.cat([packed[qi] for qi in rd["qs"]]).contiguous()
            keys = c.query_packed_keys_device(block, nq, len(t["queries"][rd["qs"][0]]), keys_out=out(nq, "i64"), range_=rg, index_base=base,
                                              stream=s)
            got = (self.host(keys, nq, u64),)
        elif call == "scores_device":
            got = (self.host(c.scores_device(fps[rd["q"]], rg, stream=s), n),)
        elif call == "topk_host":
            got = c.query_topk(fps[rd["q"]], rd["k"], rg)
        elif call == "topk_keys":
            nq, k = len(rd["qs"]), rd["k"]
            keys = o.new(nq * k, "i64")
            c.query_batch_topk_keys_device([fps[qi] for qi in rd["qs"]], k, keys, rg, base, stream=s)
            if raw:
                return keys[:nq * k]
            got = (self.host(keys, nq * k, u64),)
        elif call == "topk_packed":
            nq, k = len(rd["qs"]), rd["k"]
            block = torch.cat([packed[qi] for qi in rd["qs"]]).contiguous()
            keys, lags = c.query_packed_topk_keys_device(block, nq, len(t["queries"][rd["qs"][0]]), k, keys_out=out(nq * k, "i64"),
                                                         lags_out=out(nq * k, "i32"), aligned=True, range_=rg, index_base=base, stream=s)
            got = (self.host(keys, nq * k, u64), self.host(lags, nq * k, i32))
        elif call == "threshold_host":
            got = c.query_threshold(fps[rd["q"]], rd["t"], rd["capacity"], rg, aligned=True)
            got = (got[0], got[1], got[2], i64(got[3]))
        elif call in ("threshold_keys", "threshold_packed"):
            nq, cap = len(rd["qs"]), rd["capacity"]
            if call == "threshold_keys":
                keys, counts = c.query_batch_threshold_keys_device([fps[qi] for qi in rd["qs"]], rd["t"], cap, keys_out=out(nq * cap, "i64"),
                                                                   counts_out=out(nq, "i64"), range_=rg, index_base=base, stream=s)
                if raw:
                    return keys.reshape(-1)[:nq * cap]
                got = (self.host(keys, nq * cap, u64), self.host(counts, nq))
            else:
                block = torch.cat([packed[qi] for qi in rd["qs"]]).contiguous()
                keys, counts, lags = c.query_packed_threshold_keys_device(block, nq, len(t["queries"][rd["qs"][0]]), rd["t"], cap,
                                                                          keys_out=out(nq * cap, "i64"), counts_out=out(nq, "i64"),
                                                                          lags_out=out(nq * cap, "i32"), aligned=True, range_=rg,
                                                                          index_base=base, stream=s)
                got = (self.host(keys, nq * cap, u64), self.host(counts, nq), self.host(lags, nq * cap, i32))
        elif call == "align_keys":
            nq, k = len(rd["qs"]), rd["k"]
            keys = o.new(nq * k, "i64")
            qs = [fps[qi] for qi in rd["qs"]]
            c.query_batch_topk_keys_device(qs, k, keys, rg, base, stream=s)
            lags, scores = c.align_keys_device(qs, keys[:nq * k].contiguous(), k, index_base=base, stream=s, want_scores=True, range_=rg)
            got = (self.host(lags, nq * k), self.host(scores, nq * k))
        elif call == "match_profile":
            q, first = c.match_profile(fps[rd["q"]], rd["entry"], rg)
            got = (q, i64(first))
        elif call in ("join_self", "join_other"):
            queries = self.other if call == "join_other" else None
            cap, count = rd["capacity"], rd["count"]
            kw = dict(queries=queries, first=rd["first"], count=count, skip_same_index=rd["skip"], range_=rg, index_base=base,
                      keys_out=out(cap, "i64"), offsets_out=out(count + 1, "i64"), stream=s)
            if t["kind"] == "uniform":
                keys, offsets = c.join_threshold_keys_device(rd["t"], cap, **kw)
                if raw:
                    return keys.reshape(-1)[:cap]
                got = (self.host(keys, cap, u64), self.host(offsets, count + 1))
            else:
                keys, lags, offsets = c.join_ragged_threshold_keys_device(rd["t"], cap, lags_out=out(cap, "i32"), **kw)
                if raw:
                    return keys.reshape(-1)[:cap]
                got = (self.host(keys, cap, u64), self.host(lags, cap, i32), self.host(offsets, count + 1))
        elif call == "duplicate_groups":
            labels, groups = c.duplicate_groups(rd["t"], key_capacity=rd["key_capacity"], rows_per_call=rd["rows_per_call"], range_=rg, stream=s)
            got = (self.host(labels, n), i64(int(groups.cpu()[0])))
        elif call == "gather_keys":
            keys = self.read(rd["producer"], model, raw=True).contiguous()
            cap = rd["capacity"]
            nk = keys.numel()
            if cap is None:
                flat, offsets = c.gather_keys_device(keys, index_base=base, stream=s)
                got = (self.host(flat, flat.numel()).reshape(-1, 32), self.host(offsets, nk + 1))
            else:
                buf = torch.full((cap + SLACK, 32), 0x5A, dtype=torch.uint8, device="cuda")
                flat, offsets = c.gather_keys_device(keys, index_base=base, packed_out=buf, offsets_out=o.new(nk + 1, "i64"), capacity=cap,
                                                     stream=s)
                offsets = self.host(offsets, nk + 1)
                m = min(int(offsets[-1]), cap)
                self.intact = self.intact and bool((buf[m:] == 0x5A).all())
                got = (self.host(buf, m * 32).reshape(m, 32), offsets)
        elif call == "gather":
            flat, offsets = c.gather(rd["indices"])
            got = (flat, offsets.astype(np.int64))
        elif call == "gather_ids":
            flat, offsets = c.gather_ids(rd["ids"], stream=s)
            got = (self.host(flat, flat.numel()).reshape(-1, 32), self.host(offsets, len(rd["ids"]) + 1))
        elif call == "ids_from_keys":
            keys = self.read(rd["producer"], model, raw=True).contiguous()
            ids = c.ids_from_keys_device(keys, index_base=base, out=out(keys.numel(), "i64"), stream=s)
            got = (self.host(ids, keys.numel(), u64),)
        elif call == "keys_from_ids":
            ids = self.up(np.array(rd["ids"], np.uint64).view(np.int64))
            keys = c.keys_from_ids_device(ids, index_base=base, out=out(len(rd["ids"]), "i64"), stream=s)
            got = (self.host(keys, len(rd["ids"]), u64),)
        elif call == "state":
            got = (c.entry_ids(), i64(len(c)), i64(c.subfingerprint_total), i64(c.has_entry_ids))
        else:
            raise ValueError(call)
        self.intact = self.intact and o.slack_intact()
        return got

    def save_bytes_equal(self, model):
        """save()'s bytes against those of a fresh handle of the same capacities filled from the model"""
        fresh = self.fresh()
        self.append(fresh, model.bools(), "packed")
        if model.ids is not None:
            if len(model):
                fresh.set_entry_ids(model.entry_ids())
            else:                                                            # (ids are on, nothing to set: on through one entry that goes again)
                self.append(fresh, [np.zeros((max(1, self.t["n_sub"]), self.t["L"]), np.uint8)], "packed")
                fresh.set_entry_ids([1])
                fresh.remove([0])
        same = self.saved(self.corpus, "a.bin") == self.saved(fresh, "b.bin")
        fresh.dispose()
        return same

    def dispose(self):
        for h in [self.corpus] + self.handles + self.fps:
            h.dispose()


def run_trial(torch, trial, want, tmp):
    """the trial's steps and reads on one device handle -> one line per mismatch.  Errors propagate."""
    import contextlib
    torch.cuda.synchronize()
    live = lb.debug_live_bytes()
    bad = []
    lb.debug_set_grid_ceiling(trial["grid_ceiling"])
    d = _Device(torch, trial, tmp)
    model = Model(trial["L"], trial["n_sub"], trial["range"])
    with torch.cuda.stream(d.stream) if d.stream is not None else contextlib.nullcontext():
        for s, (stage, (want_steps, want_reads)) in enumerate(zip(trial["stages"], want)):
            for st, w in zip(stage["steps"], want_steps):
                d.intact = True
                got = d.step(st, model)
                torch.cuda.synchronize()
                apply_step(model, trial, st)
                if not same_values(got, w) or not d.intact:
                    bad.append(f"step {s} {st['op']}: " + (first_difference(got, w) if not same_values(got, w) else "slack overwritten"))
            for r, (rd, w) in enumerate(zip(stage["reads"], want_reads)):
                d.intact = True
                got = d.read(rd, model)
                if not same_values(got, w) or not d.intact:
                    bad.append(f"step {s} read {r} {rd['call']}: " + (first_difference(got, w) if not same_values(got, w) else "slack overwritten"))
            if stage["save_bytes"] and not d.save_bytes_equal(model):
                bad.append(f"step {s} save: the bytes differ from a fresh corpus'")
        torch.cuda.synchronize()
    d.dispose()
    if lb.debug_live_bytes() != live:
        bad.append(f"end: live bytes {lb.debug_live_bytes()} for {live}")
    return bad


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
    trials = int(args[0]) if len(args) > 0 else 100
    seed = int(args[1]) if len(args) > 1 else 1
    plan_only = "--plan-only" in flags
    torch = None
    if not plan_only:
        import torch
    bad, t0, t_ref = 0, time.time(), 0.0
    buckets = {}
    tmp = tempfile.mkdtemp()
    for t in range(trials) if only is None else [only]:
        t1 = time.time()
        trial = make_trial(trial_rng(seed, t))
        want = expected(trial)
        t_ref += time.time() - t1
        for p in trial["paths"]:
            buckets[p] = buckets.get(p, 0) + 1
        if plan_only:
            continue
        try:
            wrong = run_trial(torch, trial, want, tmp)
        except lb.LBAudioDetectiveError as e:
            if e.status != 1 or "--keep-going" not in flags:                 # (a refused call with --keep-going: a mismatch, the run goes on)
                print("CORPUS ERROR seed", seed, "trial", t, describe(trial), flush=True)
                raise
            import traceback
            wrong = ["refused: " + " | ".join(traceback.format_exc().strip().splitlines()[-4:])]
        except Exception:
            print("CORPUS ERROR seed", seed, "trial", t, describe(trial), flush=True)
            raise
        finally:
            lb.debug_set_grid_ceiling(0)
        if wrong:
            bad += 1
            for line in wrong:
                print("CORPUS MISMATCH seed", seed, "trial", t, line, flush=True)
            print("  trial", t, describe(trial), flush=True)
    done = trials if only is None else 1
    if plan_only:
        for name in sorted(buckets):
            print(f"{name:40s} {buckets[name]}")
        print(f"{done} trials planned, {time.time() - t0:.1f} s")
        return 0
    print(f"{done} trials, {bad} mismatches, {time.time() - t0:.1f} s ({t_ref:.1f} s of it the numpy model); seed {seed}; "
          f"paths {dict(sorted(buckets.items()))}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
