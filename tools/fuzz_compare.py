#!/usr/bin/env python3
"""Randomized GPU-vs-oracle sweep of the compare leg (not part of the test suite): tools/fuzz_compare.py [trials] [seed].
One-off fingerprint compares (sliding, either order, odd lengths and ranges) and corpus queries (single, batch of 1 .. 17
queries, per-entry scores, top-K; planted matches, duplicated entries for the lowest-index tie rule, empty sub-fingerprints,
pairs with both Booleans set in entries and queries, queries shorter and longer than the entries), float bit patterns and
indices compared exactly.  Corpus trials draw L = 200 (the specialised scans' length) one time in three.
Round 2: 60 000 trials (seed 99), 0 mismatches, 1240 s on one MI355X."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lbaudiodetective_amd as lb
from oracle import oracle as O

trials = int(sys.argv[1]) if len(sys.argv) > 1 else 300
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
bad = 0
t0 = time.time()


def bits32(x):
    return np.float32(x).view(np.uint32)


def mutate(e, p):
    q = e.copy()
    full = (q.shape[1] // 2) * 2
    flip = rng.random((q.shape[0], full // 2)) < p
    pos, neg = q[:, 0:full:2].copy(), q[:, 1:full:2].copy()
    q[:, 0:full:2] = np.where(flip, neg, pos)
    q[:, 1:full:2] = np.where(flip, pos, neg)
    return q


def both_set(f, p):
    """Set both Booleans of a fraction p of the pairs (Fingerprint.from_bools accepts them; the fingerprint stage never makes them)."""
    q = f.copy()
    full = (q.shape[-1] // 2) * 2
    sel = rng.random(q.shape[:-1] + (full // 2,)) < p
    q[..., 0:full:2][sel] = 1
    q[..., 1:full:2][sel] = 1
    return q


def top_k(scores, k):
    """The oracle's top-K: entries above 0, score descending, equal scores lowest index first."""
    order = np.lexsort((np.arange(len(scores)), -scores))
    order = order[scores[order] > 0][:k]
    return order, scores[order]


def oracle_scores(q, host, rg):
    """Every entry's score: the Boolean compare (Fp.m:119-149) over the uniform corpus taken as a ragged one."""
    n, n_sub, L = host.shape
    return O.corpus_best_ragged(q, (host.reshape(-1, L), np.full(n, n_sub, np.uint32)), rg, nthreads=8, want_scores=True)[2]


def same_topk(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), want[1].view(np.uint32))


for t in range(trials):
    L = int(rng.choice([1, 2, 3, 7, 31, 32, 33, 63, 64, 65, 127, 128, 199, 200, 201, 255, 256]))
    if rng.integers(0, 2) == 0:
        # ---- one fingerprint against one ----
        n1, n2 = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        a = O.synth_corpus(int(rng.integers(0, 2**31)), 0, 1, n1, L)[0]
        b = O.synth_corpus(int(rng.integers(0, 2**31)), 1, 1, n2, L)[0]
        mode = rng.integers(0, 5)
        if mode == 0:
            m = min(n1, n2); b[:m] = a[n1 - m:]
        elif mode == 1:
            a[rng.integers(0, n1)] = 0
        elif mode == 2:
            b[:] = 0
        elif mode == 3:
            m = min(n1, n2); b[n2 - m:] = mutate(a[:m], 0.1)
        rg = int(rng.choice([0, 1, 2, L // 2 + 1, L, L + 5, 1000]))
        want = bits32(O.compare_fp(a, b, rg if rg else L))
        got = bits32(lb.Fingerprint.from_bools(a).compare_to_fingerprint(lb.Fingerprint.from_bools(b), rg if rg else L))
        if got != want:
            bad += 1
            print("PAIR MISMATCH", t, L, n1, n2, rg, mode, hex(int(got)), hex(int(want)), flush=True)
        continue
    # ---- corpus (sub-fingerprints of at least one pair) ----
    L = 200 if rng.integers(0, 3) == 0 else max(L, 2)
    n_sub = int(rng.integers(1, 9))
    n = int(rng.integers(1, 3000))
    seed = int(rng.integers(0, 2**31))
    host = O.synth_corpus(seed, 0, n, n_sub, L)
    packed = lb.synth_corpus_device(seed, 0, n, n_sub, L)
    # duplicates (ties must go to the lowest index) and empty entries need host-side edits: rebuild the packed form
    edit = rng.integers(0, 4)
    if edit == 3:
        # pairs with both Booleans set in about 2 % of the pairs; packed on the host
        host = both_set(host, 0.02)
        corpus = lb.Corpus(L, n_sub, n)
        corpus.append_packed_device(torch.from_numpy(np.ascontiguousarray(O.pack_bools(host)).view(np.uint8).reshape(n, n_sub, 32)).cuda())
    elif edit:
        for _ in range(int(rng.integers(1, 6))):
            i, j = int(rng.integers(0, n)), int(rng.integers(0, n))
            host[j] = host[i]
        if edit == 2:
            host[int(rng.integers(0, n))] = 0
        corpus = lb.Corpus(L, n_sub, n)
        for e in range(n):
            corpus.append_fingerprint(lb.Fingerprint.from_bools(host[e]))
    else:
        corpus = lb.Corpus(L, n_sub, n)
        corpus.append_packed_device(packed)
    corpus.set_kernel_variant(int(rng.integers(0, 2)))
    nq = int(rng.choice([n_sub, n_sub, max(1, n_sub - 1), n_sub + 1, 1, 2 * n_sub + 1]))
    src = int(rng.integers(0, n))
    base = np.concatenate([host[src], host[(src + 1) % n], host[(src + 2) % n]])[:nq]
    q = mutate(base, float(rng.choice([0.0, 0.05, 0.3])))
    if rng.integers(0, 3) == 0:
        q = both_set(q, 0.03)
    rg = int(rng.choice([0, 1, L // 3 + 1, L, L + 9]))
    fq = lb.Fingerprint.from_bools(q)
    want = O.corpus_best(q, host, rg if rg else L, nthreads=8)
    got = corpus.query(fq, rg)
    if (got[0], bits32(got[1])) != (want[0], bits32(want[1])):
        bad += 1
        print("CORPUS MISMATCH", t, L, n_sub, n, nq, rg, edit, got, want, flush=True)
    if t % 3 == 0:
        # top-K of the same query against the oracle's per-entry scores
        k = int(rng.choice([1, 10, 1024]))
        want_k = top_k(oracle_scores(q, host, rg if rg else L), k)
        if not same_topk(corpus.query_topk(fq, k, rg), want_k):
            bad += 1
            print("TOPK MISMATCH", t, L, n_sub, n, nq, rg, k, flush=True)
    if t % 5 == 0 or (t % 5 == 1 and L == 200):
        bq = [mutate(host[int(rng.integers(0, n))][:n_sub], 0.1) for _ in range(int(rng.integers(1, 18)))]
        bq = [both_set(x, 0.03) if rng.integers(0, 4) == 0 else x for x in bq]
        qs = [lb.Fingerprint.from_bools(x) for x in bq]
        gb = corpus.query_batch(qs, rg)
        sc = [oracle_scores(x, host, rg if rg else L) for x in bq]
        for k, fp in enumerate(qs):
            w = O.corpus_best(bq[k], host, rg if rg else L, nthreads=8)
            if (gb[k][0], bits32(gb[k][1])) != (w[0], bits32(w[1])):
                bad += 1
                print("BATCH MISMATCH", t, L, n_sub, n, rg, len(qs), k, gb[k], w, flush=True)
                break
        if t % 2 == 0:
            k = int(rng.choice([1, 10, 1024]))
            gk = corpus.query_batch_topk(qs, k, rg)
            for j in range(len(qs)):
                if not same_topk(gk[j], top_k(sc[j], k)):
                    bad += 1
                    print("BATCH TOPK MISMATCH", t, L, n_sub, n, rg, len(qs), j, k, flush=True)
                    break
    if t % 7 == 0:
        scores = corpus.scores_device(fq, rg if rg else L).cpu().numpy()
        pick = rng.integers(0, n, size=min(n, 40))
        w = np.array([O.compare_fp(q, host[e], rg if rg else L) for e in pick], np.float32)
        if not np.array_equal(scores[pick].view(np.uint32), w.view(np.uint32)):
            bad += 1
            print("SCORES MISMATCH", t, L, n_sub, n, nq, rg, flush=True)
print(f"{trials} trials, {bad} mismatches, {time.time() - t0:.1f} s")
sys.exit(1 if bad else 0)
