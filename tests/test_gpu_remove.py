"""GPU tests of the removal of corpus entries (LBAudioDetectiveCorpusRemoveIndices, LBAudioDetectiveCorpusRemoveKeysDevice,
LBAudioDetectiveCorpusSetRemoveScratchLimit).  What is expected comes from numpy and the CPU ORACLE: the map is the cumulative
count of the kept entries, the saved bytes are those of a FRESH corpus of the same capacity filled with the kept rows, and the
queries' answers are derived from the oracle's scores on the kept Booleans (oracle.corpus_scores_packed for a uniform corpus,
oracle.corpus_best_ragged's scores for a ragged one).  Everything is compared as integers: indices exactly, scores by their
bits.  The thresholds are values of the oracle's own scores, so ties at the threshold exist by construction.  Output buffers
are poison-filled before every call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON32 = 0xA5A5A5A5
GONE = 0xFFFFFFFF
SEED = 0x52454D4F


def _constant(name):
    src = open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_remove.hip")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))


T = _constant("kRemoveTileEntries")


# ---- the contract, restated ------------------------------------------------------------------------------------------------
def _expected(n, indices):
    """(keep mask, map, removed) of a removal of `indices` (duplicates allowed) from n entries"""
    keep = np.ones(n, bool)
    keep[np.asarray(indices, np.int64)] = False
    new = np.where(keep, np.cumsum(keep) - 1, GONE).astype(np.uint32)
    return keep, new, int(n - keep.sum())


def _removal_sets(n, seed):
    """name -> indices: none; all; the first; the last; every other; one whole tile; all but the last; a random 1 %, 50 %, 99 %;
    a list with duplicates"""
    rng = np.random.default_rng(seed)
    sets = {"none": [], "all": list(range(n)), "first": [0], "last": [n - 1], "every other": list(range(0, n, 2)),
            "all but the last": list(range(n - 1))}
    if n >= 2 * T:
        sets["one whole tile"] = list(range(T, 2 * T))
    elif n >= T:
        sets["one whole tile"] = list(range(T))
    for pct in (1, 50, 99):
        sets[f"random {pct} %"] = rng.choice(n, max(1, n * pct // 100), replace=False).tolist()
    some = rng.choice(n, max(1, n // 7), replace=False)
    sets["duplicates"] = np.concatenate([some, some[::-1], some[:3]]).tolist()
    return sets


def _remove_host(lb, c, indices):
    """LBAudioDetectiveCorpusRemoveIndices through ctypes with poisoned outputs -> (status, removed, map of the old entries)"""
    N = lb._native
    n_old = len(c)
    idx = np.ascontiguousarray(indices, np.uint64)
    new = np.full(max(1, n_old), POISON32, np.uint32)
    removed = N.UInt64(0xDEAD)
    st = lb.lib().LBAudioDetectiveCorpusRemoveIndices(c._ref, idx.ctypes.data_as(C.POINTER(N.UInt64)) if idx.size else None, idx.size,
                                                     new.ctypes.data_as(C.POINTER(N.UInt32)), C.byref(removed))
    return st, int(removed.value), new[:n_old]


def _packed(oracle, bools):
    return np.ascontiguousarray(oracle.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _uniform(lb, gpu, oracle, bools, capacity):
    n, n_sub, length = bools.shape
    c = lb.Corpus(length, n_sub, capacity)
    if n:
        c.append_packed_device(gpu.from_numpy(_packed(oracle, bools)).cuda())
    return c


def _ragged(lb, gpu, oracle, flat, counts, entry_capacity, record_capacity):
    c = lb.Corpus.ragged(flat.shape[1], entry_capacity, record_capacity)
    if len(counts):
        c.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, flat)).cuda(), np.asarray(counts, np.uint32))
    return c


def _saved(c, path):
    c.save(str(path))
    with open(path, "rb") as f:
        return f.read()


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _tie_threshold(scores):
    """a threshold out of the oracle's own scores (the 4th largest positive one, or the largest): ties at it exist"""
    pos = np.sort(scores[scores > 0])
    if len(pos) == 0:
        return np.float32(0.5)
    return np.float32(pos[-4] if len(pos) >= 4 else pos[-1])


def _check_queries(c, fp, scores, what, topk=0):
    """top-1, the threshold list (and a top-K) of one query against the oracle's scores of the kept entries"""
    scores = np.asarray(scores, np.float32)
    n = len(scores)
    best = int(np.argmax(scores)) if n and scores.max() > 0 else -1
    idx, sc = c.query(fp)
    assert idx == best, (what, idx, best)
    assert _bits(sc) == (_bits(scores[best]) if best >= 0 else 0), (what, sc)
    t = _tie_threshold(scores)
    at = np.nonzero(scores >= t)[0]
    gi, gs, cnt = c.query_threshold(fp, float(t), n + 1)
    assert cnt == len(at) and np.array_equal(gi, at) and np.array_equal(_bits(gs), _bits(scores[at])), (what, "threshold", cnt, len(at))
    if topk:
        order = np.lexsort((np.arange(n), -scores.astype(np.float64)))
        order = order[scores[order] > 0][:topk]
        ki, ks = c.query_topk(fp, topk)
        assert np.array_equal(ki, order) and np.array_equal(_bits(ks), _bits(scores[order])), (what, "top-K", ki[:4], order[:4])


# ---- uniform corpora -------------------------------------------------------------------------------------------------------
_UNIFORM = {}


def _uniform_bools(oracle, length, n_sub, n):
    """n entries of one shape, made once and left unchanged (a prefix of one synthetic corpus per shape)"""
    key = (length, n_sub)
    if key not in _UNIFORM:
        _UNIFORM[key] = oracle.synth_corpus(SEED, 0, 3 * T + 5, n_sub, length)
    return _UNIFORM[key][:n]


def _uniform_scores(oracle, q, bools, length):
    if len(bools) == 0:
        return np.zeros(0, np.float32)
    return oracle.corpus_scores_packed(oracle.pack_bools(q), oracle.pack_bools(bools), length, length, nthreads=16)


def _check_uniform(lb, gpu, oracle, tmp_path, bools, indices, what, limit=None):
    """one removal from a fresh corpus of `bools`: results, saved bytes and queries; returns the saved bytes"""
    n, n_sub, length = bools.shape
    keep, new, removed = _expected(n, indices)
    c = _uniform(lb, gpu, oracle, bools, n)
    if limit is not None:
        c.set_remove_scratch_limit(limit)
    st, got_removed, got_map = _remove_host(lb, c, indices)
    assert st == 0, (what, st)
    assert got_removed == removed and len(c) == n - removed, (what, got_removed, removed, len(c))
    assert c.subfingerprint_total == (n - removed) * n_sub
    assert np.array_equal(got_map, new), (what, np.nonzero(got_map != new)[0][:4])
    kept = bools[keep]
    fresh = _uniform(lb, gpu, oracle, kept, n)
    data = _saved(c, tmp_path / "removed.bin")
    assert data == _saved(fresh, tmp_path / "fresh.bin"), what
    fresh.dispose()
    queries = []
    if removed:
        queries.append(("removed", bools[np.nonzero(~keep)[0][0]]))
    if removed < n:
        queries.append(("kept", kept[len(kept) // 2]))
    for name, q in queries:
        scores = _uniform_scores(oracle, q, kept, length)
        _check_queries(c, lb.Fingerprint.from_bools(q), scores, (what, name))
        if name == "removed" and len(kept) and q.any() and not (kept == q).all(axis=(1, 2)).any():
            assert c.query(lb.Fingerprint.from_bools(q))[1] < 1.0, (what, "the removed entry still matches itself")
    c.dispose()
    return data


@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 3 * T + 5])
@pytest.mark.parametrize("shape", [(200, 1), (200, 5), (200, 8), (64, 3)])
def test_uniform_removal_sets(lb, gpu, oracle, tmp_path, shape, n):
    length, n_sub = shape
    bools = _uniform_bools(oracle, length, n_sub, n)
    for name, indices in _removal_sets(n, n * 10 + n_sub).items():
        _check_uniform(lb, gpu, oracle, tmp_path, bools, indices, (shape, n, name))


def test_uniform_chunk_of_one_tile_equals_the_default(lb, gpu, oracle, tmp_path):
    """3T + 5 entries with the scratch limit at one tile (and a little more): several chunks, bit-identical to one chunk"""
    n = 3 * T + 5
    bools = _uniform_bools(oracle, 200, 5, n)
    c = _uniform(lb, gpu, oracle, bools, n)
    one_tile = T * c.entry_stride_bytes
    c.dispose()
    for name, indices in _removal_sets(n, 5).items():
        if name in ("none", "all"):
            continue
        whole = _check_uniform(lb, gpu, oracle, tmp_path, bools, indices, ("default", name))
        for limit in (one_tile, one_tile + 5, 2 * one_tile):
            assert _check_uniform(lb, gpu, oracle, tmp_path, bools, indices, ("limit", limit, name), limit=limit) == whole


def test_limit_below_one_tile_is_refused_and_nothing_changes(lb, gpu, oracle, tmp_path):
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    n = T + 1
    bools = _uniform_bools(oracle, 200, 5, n)
    counts = np.full(40, 30, np.uint32)
    flat = oracle.synth_ragged_entries(SEED, 0, counts, 200)
    for c in (_uniform(lb, gpu, oracle, bools, n), _ragged(lb, gpu, oracle, flat, counts, 40, int(counts.sum()))):
        before = _saved(c, tmp_path / "before.bin")
        c.set_remove_scratch_limit(T * c.entry_stride_bytes - 1)
        st, removed, new = _remove_host(lb, c, [0, 3])
        assert st == bad and removed == 0 and (new == POISON32).all()
        with pytest.raises(lb.LBAudioDetectiveError):
            c.remove([0, 3])
        keys = gpu.zeros(4, dtype=gpu.int64, device="cuda")
        with pytest.raises(lb.LBAudioDetectiveError):
            c.remove_keys_device(keys)
        assert _saved(c, tmp_path / "after.bin") == before
        c.set_remove_scratch_limit(T * c.entry_stride_bytes)
        assert c.remove([0, 3]) == 2
        c.dispose()


def test_host_form_argument_checks(lb, gpu, oracle, tmp_path):
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    n = 10
    bools = _uniform_bools(oracle, 200, 5, n)
    c = _uniform(lb, gpu, oracle, bools, n)
    before = _saved(c, tmp_path / "before.bin")
    for indices in ([n], [0, 1, n], [1 << 40], [0xFFFFFFFF]):
        st, removed, new = _remove_host(lb, c, indices)
        assert st == bad and removed == 0 and (new == POISON32).all(), indices
    assert len(c) == n and _saved(c, tmp_path / "after.bin") == before
    # nothing named: the identity map, with and without a list
    st, removed, new = _remove_host(lb, c, [])
    assert st == 0 and removed == 0 and np.array_equal(new, np.arange(n, dtype=np.uint32))
    assert c.remove([]) == 0 and len(c) == n
    # an empty corpus
    empty = lb.Corpus(200, 5, 4)
    assert empty.remove([]) == 0
    with pytest.raises(lb.LBAudioDetectiveError):
        empty.remove([0])
    keys = gpu.full((8,), -1, dtype=gpu.int64, device="cuda")
    assert empty.remove_keys_device(keys) == 0
    # the Python form with the map
    removed, new = c.remove([3, 3, 7], return_map=True)
    assert removed == 2 and np.array_equal(new, _expected(n, [3, 7])[1])
    empty.dispose()
    c.dispose()


# ---- the keys form ------------------------------------------------------------------------------------------------------------
def _planted(oracle, n, n_sub, seed):
    """a synthetic corpus with near copies of other entries planted: 0, 1, 5, 20 and 60 flipped Booleans, eight of each"""
    b = oracle.synth_corpus(seed, 0, n, n_sub, 200).copy()
    rng = np.random.default_rng(seed)
    free = rng.permutation(n).tolist()
    for flips in (0, 1, 5, 20, 60) * 8:
        src, dst = free.pop(), free.pop()
        b[dst] = b[src]
        flat = b[dst].reshape(-1)
        flat[rng.choice(n_sub * 200, flips, replace=False)] ^= 1
    return b


def _key(score, index):
    return (int(np.float32(score).view(np.uint32)) << 32) | (0xFFFFFFFF - index)


def test_keys_of_a_threshold_query_with_padding_and_foreign_keys(lb, gpu, oracle, tmp_path):
    """the keys of a real query_batch_threshold_keys_device call at a non-zero index base -- zero padding included -- plus keys of
    entries outside [base, base + count) and duplicates: exactly the in-range set goes.  On a stream of its own."""
    n, base = 2 * T + 3, 1000003
    bools = _planted(oracle, n, 5, 91)
    c = _uniform(lb, gpu, oracle, bools, n)
    ids = [5, n // 2, n - 1]
    fps = [lb.Fingerprint.from_bools(bools[i]) for i in ids]
    words = oracle.pack_bools(bools)
    scores = [oracle.corpus_scores_packed(words[i], words, 200, 200, nthreads=16) for i in ids]
    t = np.float32(min(_tie_threshold(s) for s in scores))
    want = sorted(set(np.concatenate([np.nonzero(s >= t)[0] for s in scores]).tolist()))
    capacity = 1024
    assert 3 <= len(want) < n and max(int((s >= t).sum()) for s in scores) < capacity
    gpu.cuda.synchronize()
    s = gpu.cuda.Stream()
    with gpu.cuda.stream(s):
        keys, counts = c.query_batch_threshold_keys_device(fps, float(t), capacity, index_base=base, stream=s)
        foreign = np.array([_key(0.9, base - 1), _key(0.9, 0), _key(1.0, base + n), _key(0.5, 0xFFFFFFFF), 0, 0], np.uint64).view(np.int64)
        every = gpu.cat([keys.reshape(-1), gpu.from_numpy(foreign).cuda(), keys.reshape(-1)[:10]])
        new = gpu.full((n,), POISON32 - (1 << 32), dtype=gpu.int32, device="cuda")
        removed = c.remove_keys_device(every, index_base=base, new_indices_out=new, stream=s)
    assert int((keys.cpu().numpy() == 0).sum()) > 0, "the key block carries no padding"
    keep, exp_map, exp_removed = _expected(n, want)
    assert removed == exp_removed == len(want) and len(c) == n - removed
    assert np.array_equal(new.cpu().numpy().view(np.uint32), exp_map)
    fresh = _uniform(lb, gpu, oracle, bools[keep], n)
    assert _saved(c, tmp_path / "a.bin") == _saved(fresh, tmp_path / "b.bin")
    # at another base the same keys name entries of other shards: nothing goes
    assert c.remove_keys_device(every, index_base=5000000) == 0 and len(c) == n - removed
    fresh.dispose()
    c.dispose()


def test_self_join_then_remove_the_later_duplicates(lb, gpu, oracle, tmp_path):
    """the join's output as an action: of every pair (row, entry > row) at the threshold the entry goes.  The kept set is the
    one the oracle's score matrix gives, and a second self-join finds no pair with entry > row any more."""
    n = 2 * T + 9
    bools = _planted(oracle, n, 5, 92)
    words = oracle.pack_bools(bools)
    S = np.stack([oracle.corpus_scores_packed(words[i], words, 200, 200, nthreads=16) for i in range(n)]).astype(np.float32)
    off = S[~np.eye(n, dtype=bool)]
    d = np.unique(off[off > 0])
    t = np.float32(d[-6])                                   # among the planted near copies: a handful of pairs, ties included
    hit = np.triu(S >= t, 1)                                # (row, entry) with entry > row
    gone = np.nonzero(hit.any(axis=0))[0]
    assert 5 <= len(gone) < n // 2
    c = _uniform(lb, gpu, oracle, bools, n)
    capacity = 4096

    def later_pairs():
        keys = gpu.full((capacity,), -0x0123456789ABCDEF, dtype=gpu.int64, device="cuda")
        keys, offsets = c.join_threshold_keys_device(float(t), capacity, keys_out=keys)
        total = offsets[-1]
        slot = gpu.arange(capacity, device="cuda")
        row = gpu.searchsorted(offsets, slot, right=True) - 1
        entry = 0xFFFFFFFF - (keys & 0xFFFFFFFF)
        return keys[(slot < total) & (entry > row)]

    pairs = later_pairs()
    assert pairs.numel() == int(hit.sum())
    new = gpu.full((n,), POISON32 - (1 << 32), dtype=gpu.int32, device="cuda")
    removed = c.remove_keys_device(pairs, new_indices_out=new)
    keep, exp_map, exp_removed = _expected(n, gone)
    assert removed == exp_removed and len(c) == n - removed
    assert np.array_equal(new.cpu().numpy().view(np.uint32), exp_map)
    fresh = _uniform(lb, gpu, oracle, bools[keep], n)
    assert _saved(c, tmp_path / "a.bin") == _saved(fresh, tmp_path / "b.bin")
    assert later_pairs().numel() == 0
    fresh.dispose()
    c.dispose()


# ---- ragged corpora -----------------------------------------------------------------------------------------------------------
def _ragged_counts(total, seed):
    """entry lengths 1 .. 70 that add up to `total` records"""
    rng = np.random.default_rng(seed)
    counts = []
    left = total
    while left:
        k = int(min(left, rng.integers(1, 71)))
        counts.append(k)
        left -= k
    return np.asarray(counts, np.uint32)


def _ragged_scores(oracle, q, flat, counts, length):
    if len(counts) == 0:
        return np.zeros(0, np.float32)
    return oracle.corpus_best_ragged(q, (flat, counts), length, nthreads=16, want_scores=True)[2]


def _entries_of(flat, off, which):
    if len(which) == 0:
        return flat[:0]
    return np.concatenate([flat[off[e]:off[e + 1]] for e in which])


def _check_ragged(lb, gpu, oracle, tmp_path, flat, counts, indices, what, limit=None, queries=True):
    n, length, total = len(counts), flat.shape[1], int(counts.sum())
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    keep, new, removed = _expected(n, indices)
    c = _ragged(lb, gpu, oracle, flat, counts, n, total)
    if limit is not None:
        c.set_remove_scratch_limit(limit)
    st, got_removed, got_map = _remove_host(lb, c, indices)
    assert st == 0, (what, st)
    kept_ids = np.nonzero(keep)[0]
    kept_counts, kept_flat = counts[keep], _entries_of(flat, off, kept_ids)
    assert got_removed == removed and len(c) == n - removed, (what, got_removed, removed, len(c))
    assert c.subfingerprint_total == int(kept_counts.sum()), what
    assert np.array_equal(got_map, new), (what, np.nonzero(got_map != new)[0][:4])
    fresh = _ragged(lb, gpu, oracle, kept_flat, kept_counts, n, total)
    data = _saved(c, tmp_path / "removed.bin")
    assert data == _saved(fresh, tmp_path / "fresh.bin"), what          # (the restamped index fields and the counts)
    fresh.dispose()
    if queries:
        # shorter than, equal to and longer than typical entries (both sliding sides), and 5 long for the short kernels; cut
        # from a removed entry where there is one, else from a kept one
        src = np.nonzero(~keep)[0] if removed else kept_ids
        long_e = src[np.argmax(counts[src])]
        body = flat[off[long_e]:off[long_e + 1]]
        rng = np.random.default_rng(n)
        qs = [body[:5], body[:min(20, len(body))], body,
              np.concatenate([body, rng.integers(0, 2, (90 - min(len(body), 89), length), dtype=np.uint8)])]
        for q in qs:
            scores = _ragged_scores(oracle, q, kept_flat, kept_counts, length)
            _check_queries(c, lb.Fingerprint.from_bools(q), scores, (what, len(q)), topk=10)
    c.dispose()
    return data


@pytest.mark.parametrize("total", [T - 7, T, T + 9, 3 * T + 5])
@pytest.mark.parametrize("length", [200, 150])
def test_ragged_removal_sets(lb, gpu, oracle, tmp_path, length, total):
    """records fewer than, exactly and a few more than one tile, and several tiles.  'last' and 'all but the last' remove the end
    of the record stream and leave the scan reading behind the new end."""
    counts = _ragged_counts(total, total + length)
    flat = oracle.synth_ragged_entries(SEED + length, 0, counts, length)
    for name, indices in _removal_sets(len(counts), total).items():
        _check_ragged(lb, gpu, oracle, tmp_path, flat, counts, indices, (length, total, name))


def test_ragged_chunk_of_one_tile_equals_the_default(lb, gpu, oracle, tmp_path):
    total = 3 * T + 5
    counts = _ragged_counts(total, 17)
    flat = oracle.synth_ragged_entries(SEED, 0, counts, 200)
    for name, indices in _removal_sets(len(counts), 6).items():
        if name in ("none", "all"):
            continue
        whole = _check_ragged(lb, gpu, oracle, tmp_path, flat, counts, indices, ("default", name), queries=False)
        for limit in (T * 32, T * 32 + 5, 2 * T * 32):
            assert _check_ragged(lb, gpu, oracle, tmp_path, flat, counts, indices, ("limit", limit, name), limit=limit,
                                 queries=False) == whole


def test_ragged_keys_form(lb, gpu, oracle, tmp_path):
    counts = _ragged_counts(T + 300, 23)
    n, total = len(counts), int(counts.sum())
    flat = oracle.synth_ragged_entries(SEED, 0, counts, 200)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    c = _ragged(lb, gpu, oracle, flat, counts, n, total)
    base = 77
    want = [1, 4, n - 1, n // 2]
    keys = np.array([_key(0.8, base + i) for i in want] + [0, 0, _key(0.8, base + n), _key(0.8, base - 1), _key(0.3, base + 4)],
                    np.uint64).view(np.int64)
    new = gpu.full((n,), POISON32 - (1 << 32), dtype=gpu.int32, device="cuda")
    removed = c.remove_keys_device(gpu.from_numpy(keys).cuda(), index_base=base, new_indices_out=new)
    keep, exp_map, exp_removed = _expected(n, want)
    assert removed == exp_removed and len(c) == n - removed
    assert np.array_equal(new.cpu().numpy().view(np.uint32), exp_map)
    kept_ids = np.nonzero(keep)[0]
    fresh = _ragged(lb, gpu, oracle, _entries_of(flat, off, kept_ids), counts[keep], n, total)
    assert _saved(c, tmp_path / "a.bin") == _saved(fresh, tmp_path / "b.bin")
    fresh.dispose()
    c.dispose()


# ---- life cycle ---------------------------------------------------------------------------------------------------------------
def test_uniform_life_cycle(lb, gpu, oracle, tmp_path):
    """remove, append (the new entries land at the new count), remove twice in a row, save -> load; the scratch goes with the
    corpus"""
    gpu.cuda.synchronize()
    live = lb.debug_live_bytes()
    n, extra = T + 50, 40
    every = _uniform_bools(oracle, 200, 5, n + extra)
    bools, more = every[:n], every[n:]
    c = _uniform(lb, gpu, oracle, bools, n)
    first = list(range(10, 300, 3)) + [n - 1]
    keep, _, removed = _expected(n, first)
    assert c.remove(first) == removed
    c.append_packed_device(gpu.from_numpy(_packed(oracle, more)).cuda())
    now = np.concatenate([bools[keep], more])
    assert len(c) == len(now)
    fresh = _uniform(lb, gpu, oracle, now, n)
    assert _saved(c, tmp_path / "a.bin") == _saved(fresh, tmp_path / "b.bin")
    for q in (more[3], bools[10], now[0]):
        _check_queries(c, lb.Fingerprint.from_bools(q), _uniform_scores(oracle, q, now, 200), "after the append", topk=10)
    # twice in a row
    keep2, _, r2 = _expected(len(now), [0, 5, len(now) - 1])
    assert c.remove([0, 5, len(now) - 1]) == r2
    now = now[keep2]
    keep3, _, r3 = _expected(len(now), list(range(1, len(now), 2)))
    assert c.remove(list(range(1, len(now), 2))) == r3
    now = now[keep3]
    fresh2 = _uniform(lb, gpu, oracle, now, n)
    data = _saved(c, tmp_path / "c.bin")
    assert data == _saved(fresh2, tmp_path / "d.bin")
    _check_queries(c, lb.Fingerprint.from_bools(now[7]), _uniform_scores(oracle, now[7], now, 200), "after two removals", topk=10)
    loaded = lb.Corpus.load(str(tmp_path / "c.bin"), 200, 5, n)
    assert len(loaded) == len(now) and _saved(loaded, tmp_path / "e.bin") == data
    _check_queries(loaded, lb.Fingerprint.from_bools(now[7]), _uniform_scores(oracle, now[7], now, 200), "loaded")
    for x in (c, fresh, fresh2, loaded):
        x.dispose()
    assert lb.debug_live_bytes() == live


def test_ragged_life_cycle(lb, gpu, oracle, tmp_path):
    gpu.cuda.synchronize()
    live = lb.debug_live_bytes()
    counts_all = _ragged_counts(T + 700, 31)
    split = len(counts_all) - 8
    counts, more_counts = counts_all[:split], counts_all[split:]
    flat_all = oracle.synth_ragged_entries(SEED, 0, counts_all, 200)
    n, total = len(counts_all), int(counts_all.sum())
    flat, more = flat_all[:int(counts.sum())], flat_all[int(counts.sum()):]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    c = _ragged(lb, gpu, oracle, flat, counts, n, total)
    first = [0, 3, 4, split - 1]
    keep, _, removed = _expected(split, first)
    assert c.remove(first) == removed
    c.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, more)).cuda(), more_counts)
    now_counts = np.concatenate([counts[keep], more_counts])
    now_flat = np.concatenate([_entries_of(flat, off, np.nonzero(keep)[0]), more])
    assert len(c) == len(now_counts) and c.subfingerprint_total == int(now_counts.sum())
    fresh = _ragged(lb, gpu, oracle, now_flat, now_counts, n, total)
    assert _saved(c, tmp_path / "a.bin") == _saved(fresh, tmp_path / "b.bin")
    for q in (more[:12], flat[:5], now_flat[40:75]):
        _check_queries(c, lb.Fingerprint.from_bools(q), _ragged_scores(oracle, q, now_flat, now_counts, 200), "after the append", topk=10)
    # twice in a row
    for indices in ([1, len(now_counts) - 1], list(range(0, len(now_counts) - 2, 2))):
        off_now = np.concatenate([[0], np.cumsum(now_counts)]).astype(np.int64)
        k, _, r = _expected(len(now_counts), indices)
        assert c.remove(indices) == r
        now_flat, now_counts = _entries_of(now_flat, off_now, np.nonzero(k)[0]), now_counts[k]
    fresh2 = _ragged(lb, gpu, oracle, now_flat, now_counts, n, total)
    data = _saved(c, tmp_path / "c.bin")
    assert data == _saved(fresh2, tmp_path / "d.bin")
    q = now_flat[3:30]
    _check_queries(c, lb.Fingerprint.from_bools(q), _ragged_scores(oracle, q, now_flat, now_counts, 200), "after two removals", topk=10)
    loaded = lb.Corpus.load(str(tmp_path / "c.bin"), 200, 0, n)
    assert len(loaded) == len(now_counts) and _saved(loaded, tmp_path / "e.bin") == data
    _check_queries(loaded, lb.Fingerprint.from_bools(q), _ragged_scores(oracle, q, now_flat, now_counts, 200), "loaded")
    for x in (c, fresh, fresh2, loaded):
        x.dispose()
    assert lb.debug_live_bytes() == live
