"""GPU tests of the duplicate groups (LBAudioDetectiveGroupLabelsFromKeysDevice, LBAudioDetectiveGroupExtraKeysFromLabelsDevice,
Corpus.duplicate_groups, Corpus.deduplicate).  The expected labels come from a plain union-find written here: the label of i
is the lowest index of its set.  Labels, group counts and keys are compared exactly; labels, group count and key buffers are
poison-filled before every call that starts a grouping.  End to end the expected adjacency comes from the CPU ORACLE's score
matrix (oracle.corpus_scores_packed row by row) at thresholds that are values of that matrix, so ties at the threshold exist
and nothing needs a tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON32 = 0x5A5A5A5A
POISON64 = -0x0123456789ABCDEF
ONE = 0x3F800000
L = 200


# ---- the reference ----------------------------------------------------------------------------------------------------------
def _union_find(n, edges):
    """labels[i] = the lowest index of i's set after joining every (a, b) of edges"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.int64)


def _key(index, base=0, score_bits=0x3F000000):
    return (score_bits << 32) | (0xFFFFFFFF - (base + index))


def _entry(key, base, n):
    """the entry a key names, None for a zero key and a key of another range"""
    if key == 0:
        return None
    j = 0xFFFFFFFF - (key & 0xFFFFFFFF) - base
    return j if 0 <= j < n else None


def _i64(values):
    return np.array(values, np.uint64).view(np.int64) if len(values) else np.zeros(0, np.int64)


class Rows:
    """rows of raw keys: row r is `rows[r]` (a list of 64-bit keys), entry first + r or the entry row_keys[r] names"""

    def __init__(self, n, rows, base=0, first=0, row_keys=None):
        self.n, self.rows, self.base, self.first, self.row_keys = n, rows, base, first, row_keys

    def row_entry(self, r):
        return self.first + r if self.row_keys is None else _entry(self.row_keys[r], self.base, self.n)

    def edges(self, slots=None):
        """the edges of the first `slots` slots in CSR order (None: all)"""
        out, p = [], 0
        for r, row in enumerate(self.rows):
            a = self.row_entry(r)
            for key in row:
                if slots is not None and p >= slots:
                    return out
                p += 1
                b = _entry(key, self.base, self.n)
                if a is not None and b is not None:
                    out.append((a, b))
        return out

    def csr(self):
        keys = [k for row in self.rows for k in row]
        offsets = np.concatenate([[0], np.cumsum([len(row) for row in self.rows])]).astype(np.int64)
        return _i64(keys), offsets

    def pitched(self, pitch, rng):
        """[R][pitch] with the zero padding spread through the rows"""
        out = np.zeros((len(self.rows), pitch), np.uint64)
        for r, row in enumerate(self.rows):
            assert len(row) <= pitch
            at = np.sort(rng.choice(pitch, len(row), replace=False))
            out[r, at] = np.array(row, np.uint64)
        return out.view(np.int64)


def _labels_call(lb, gpu, g, form="csr", pitch=0, rng=None, slots=None, labels=None, reset=True):
    """one call over the rows of g -> (labels tensor, group count); the outputs are poisoned when the call resets"""
    count = gpu.full((1,), POISON64, dtype=gpu.int64, device="cuda")
    if labels is None:
        assert reset
        labels = gpu.full((g.n,), POISON32, dtype=gpu.int32, device="cuda")
    row_keys = gpu.from_numpy(_i64(g.row_keys)).cuda() if g.row_keys is not None else None
    if form == "csr":
        keys, offsets = g.csr()
        d_keys = gpu.from_numpy(keys if len(keys) else np.zeros(1, np.int64)).cuda()
        lb.group_labels_from_keys_device(d_keys, g.n, offsets=gpu.from_numpy(offsets).cuda(), first_row=g.first, row_keys=row_keys,
                                         index_base=g.base, labels=labels, reset=reset, group_count=count,
                                         n_slots=len(keys) if slots is None else slots)
    else:
        d_keys = gpu.from_numpy(g.pitched(pitch, rng)).cuda()
        lb.group_labels_from_keys_device(d_keys, g.n, first_row=g.first, row_keys=row_keys, index_base=g.base, labels=labels,
                                         reset=reset, group_count=count)
    gpu.cuda.synchronize()
    return labels, int(count.item())


def _check(lb, gpu, g, what, **kw):
    slots = kw.get("slots")
    want = _union_find(g.n, g.edges(slots))
    labels, count = _labels_call(lb, gpu, g, **kw)
    got = labels.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
    assert count == int((want == np.arange(g.n)).sum()), (what, count)
    return want


def _rows_of(n, edges, base=0):
    """edge (a, b) as the key of b in row a; n rows"""
    rows = [[] for _ in range(n)]
    for a, b in edges:
        rows[a].append(_key(b, base))
    return rows


# ---- hand-made graphs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1025])
def test_sizes_without_edges_and_with_one(lb, gpu, n):
    want = _check(lb, gpu, Rows(n, [[] for _ in range(n)]), ("no edges", n))
    assert np.array_equal(want, np.arange(n))
    # no rows at all, and the pitched form with no rows
    _check(lb, gpu, Rows(n, []), ("no rows", n))
    _check(lb, gpu, Rows(n, []), ("no rows, pitched", n), form="pitched", pitch=3, rng=np.random.default_rng(0))
    if n > 1:
        want = _check(lb, gpu, Rows(n, _rows_of(n, [(0, n - 1)])), ("one edge", n))
        assert want[n - 1] == 0 and (want == np.arange(n)).sum() == n - 1
        _check(lb, gpu, Rows(n, _rows_of(n, [(n - 1, 0)])), ("one edge, from the last row", n))


def test_chain(lb, gpu):
    """row i holds only the key of i - 1: the deepest chain of parents the hook pass can build"""
    n = 3000
    want = _check(lb, gpu, Rows(n, _rows_of(n, [(i, i - 1) for i in range(1, n)])), "chain")
    assert (want == 0).all()


def test_path_over_a_permutation(lb, gpu):
    n = 4097
    perm = np.random.default_rng(41).permutation(n)
    want = _check(lb, gpu, Rows(n, _rows_of(n, [(int(perm[k]), int(perm[k + 1])) for k in range(n - 1)])), "path")
    assert (want == 0).all()


def test_stars(lb, gpu):
    n = 2001
    # the centre at the highest index, every edge in its leaf's row; a few vertices beside the star stay alone
    want = _check(lb, gpu, Rows(n + 5, _rows_of(n + 5, [(i, n - 1) for i in range(n - 1)])), "star, centre last")
    assert (want[:n] == 0).all() and np.array_equal(want[n:], np.arange(n, n + 5))
    # the centre at index 0, every edge in the centre's row
    want = _check(lb, gpu, Rows(n, _rows_of(n, [(0, i) for i in range(1, n)])), "star, centre first")
    assert (want == 0).all()
    # K(3, 2000), every edge in both directions: thousands of hooks contending for three roots
    edges = [(a, b) for a in range(3) for b in range(3, 2003)]
    want = _check(lb, gpu, Rows(2003, _rows_of(2003, edges + [(b, a) for a, b in edges])), "K(3, 2000)")
    assert (want == 0).all()


_RANDOM = {}


def _random_rows(base=0):
    """N = 3000 and 1500 random edges (around the percolation point: groups of 1 to hundreds), some of them repeated, in the
    other direction as well, self-edges, zero keys, and keys below and above the index range"""
    if base not in _RANDOM:
        n = 3000
        rng = np.random.default_rng(1234)
        edges = [(int(a), int(b)) for a, b in rng.integers(0, n, (1500, 2))]
        edges += edges[:200] + [(b, a) for a, b in edges[100:400]] + [(int(v), int(v)) for v in rng.integers(0, n, 50)]
        rows = _rows_of(n, edges, base)
        for r in rng.integers(0, n, 120):
            kind = int(rng.integers(0, 3))
            above, below = base + n + int(rng.integers(0, 1000)), base - 1 - int(rng.integers(0, 1000))
            foreign = 0                                      # a zero key, or a key of an index above or below the range
            if kind == 1 and above <= 0xFFFFFFFF:
                foreign = _key(above)
            elif kind == 2 and below >= 0:
                foreign = _key(below)
            rows[int(r)].insert(int(rng.integers(0, len(rows[int(r)]) + 1)), foreign)
        _RANDOM[base] = (n, rows)
    return _RANDOM[base]


def test_random_graph(lb, gpu):
    n, rows = _random_rows(base=5000)
    want = _check(lb, gpu, Rows(n, rows, base=5000), "random")
    sizes = np.bincount(want, minlength=n)
    assert sizes.max() >= 20 and (sizes == 1).sum() >= 100 and (sizes == 2).sum() >= 1


@pytest.mark.parametrize("order", ["rows ascending", "rows descending"])
def test_incremental_calls_equal_one_call(lb, gpu, order):
    n, rows = _random_rows(base=5000)
    want = _union_find(n, Rows(n, rows, base=5000).edges())
    cuts = [0, 700, 2100, n]
    parts = [Rows(n, rows[cuts[i]:cuts[i + 1]], base=5000, first=cuts[i]) for i in range(3)]
    if order == "rows descending":
        parts.reverse()
    labels, count = _labels_call(lb, gpu, parts[0])
    for part in parts[1:]:
        labels, count = _labels_call(lb, gpu, part, labels=labels, reset=False)
    got = labels.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert count == int((want == np.arange(n)).sum())


def test_cut_list_is_used_as_far_as_it_goes(lb, gpu):
    n, rows = _random_rows(base=5000)
    g = Rows(n, rows, base=5000)
    total = len(g.csr()[0])
    full = _union_find(n, g.edges())
    for slots in (total // 3, 1, total - 1):
        want = _check(lb, gpu, g, ("cut", slots), slots=slots)
        assert not np.array_equal(want, full) or slots == total - 1
    # the other cut: offsets whose total lies below the slots given (the keys behind it are not read as edges)
    keys, offsets = g.csr()
    labels = gpu.full((n,), POISON32, dtype=gpu.int32, device="cuda")
    lb.group_labels_from_keys_device(gpu.from_numpy(keys).cuda(), n, offsets=gpu.from_numpy(offsets[:1001].copy()).cuda(), index_base=5000,
                                     labels=labels)
    want = _union_find(n, Rows(n, rows[:1000], base=5000).edges())
    assert np.array_equal(labels.cpu().numpy().astype(np.int64), want)


def test_index_base_at_the_top_of_the_range(lb, gpu):
    """inIndexBase = 2^32 - N: the last entry's low key word is 0 under a score word that is not"""
    n = 3000
    base = (1 << 32) - n
    _, rows = _random_rows(base=base)
    rows = [list(r) for r in rows]
    assert _key(n - 1, base) & 0xFFFFFFFF == 0
    rows[7].append(_key(n - 1, base))
    rows[n - 1].append(_key(11, base))
    want = _check(lb, gpu, Rows(n, rows, base=base), "top of the range")
    assert want[n - 1] == want[7] == want[11] != n - 1


def test_pitched_rows_and_row_keys(lb, gpu):
    n, rows = _random_rows(base=5000)
    pitch = max(len(r) for r in rows) + 3
    rng = np.random.default_rng(5)
    want = _check(lb, gpu, Rows(n, rows, base=5000), "pitched", form="pitched", pitch=pitch, rng=rng)
    # the rows in a shuffled order, named by row keys (and fewer rows than entries)
    order = rng.permutation(n)[:2500]
    row_keys = [_key(int(e), 5000, ONE) for e in order]
    shuffled = Rows(n, [rows[int(e)] for e in order], base=5000, first=17, row_keys=row_keys)
    got = _check(lb, gpu, shuffled, "row keys, pitched", form="pitched", pitch=pitch, rng=rng)
    assert not np.array_equal(got, want)                     # (500 rows are missing)
    _check(lb, gpu, shuffled, "row keys, CSR")
    # some row keys zero or of another range: their rows are empty
    dead = list(row_keys)
    for r in range(0, 2500, 3):
        dead[r] = 0 if r % 2 else _key(n + r, 5000)
    fewer = Rows(n, shuffled.rows, base=5000, row_keys=dead)
    assert len(fewer.edges()) < len(shuffled.edges())
    _check(lb, gpu, fewer, "dead row keys, pitched", form="pitched", pitch=pitch, rng=rng)
    _check(lb, gpu, fewer, "dead row keys, CSR")


# ---- the extra keys ----------------------------------------------------------------------------------------------------------
def _extra_call(lb, gpu, labels, capacity, base=0):
    d_labels = gpu.from_numpy(np.asarray(labels, np.int64).astype(np.uint32).view(np.int32)).cuda()
    keys = gpu.full((capacity + 2,), POISON64, dtype=gpu.int64, device="cuda")
    count = C.c_uint64(12345)
    st = lb.lib().LBAudioDetectiveGroupExtraKeysFromLabelsDevice(d_labels.data_ptr(), len(labels), base, capacity, keys.data_ptr(),
                                                                 C.byref(count), gpu.cuda.current_stream().cuda_stream)
    assert st == 0
    got = keys.cpu().numpy()
    assert (got[capacity:] == POISON64).all()                # nothing behind the capacity
    return got[:capacity].view(np.uint64), int(count.value)


def _check_extra(lb, gpu, labels, capacity, base=0):
    labels = np.asarray(labels, np.int64)
    extra = np.nonzero(labels != np.arange(len(labels)))[0]
    want = np.zeros(capacity, np.uint64)
    m = min(len(extra), capacity)
    want[:m] = (np.uint64(ONE) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - (np.uint64(base) + extra[:m].astype(np.uint64)))
    got, count = _extra_call(lb, gpu, labels, capacity, base)
    assert count == len(extra), (count, len(extra))
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    return count


def test_extra_keys(lb, gpu):
    n, rows = _random_rows(base=5000)
    labels = _union_find(n, Rows(n, rows, base=5000).edges())
    count = _check_extra(lb, gpu, labels, n)
    assert 500 < count < n - 100
    for capacity in (count + 7, count, count - 1, count // 2, 1):
        _check_extra(lb, gpu, labels, capacity)
    assert _check_extra(lb, gpu, np.arange(n), 100) == 0     # every entry alone
    assert _check_extra(lb, gpu, np.zeros(n, np.int64), n) == n - 1      # one giant group
    for m in (1, 1023, 1024, 1025):                          # around one tile
        assert _check_extra(lb, gpu, np.zeros(m, np.int64), m + 1) == m - 1
    # the index base at the top of the range: the last entry's key has a zero low word and is not a zero key
    base = (1 << 32) - n
    top = labels.copy()
    top[n - 1] = 0
    _check_extra(lb, gpu, top, n, base=base)
    # the Python form, and the keys into the removal's and gather's hands: see the end-to-end tests
    keys, c = lb.group_extra_keys_from_labels_device(gpu.from_numpy(labels.astype(np.int32)).cuda())
    assert c == count and keys.numel() == n and int((keys != 0).sum().item()) == count


# ---- end to end: a uniform corpus with planted near-copies -------------------------------------------------------------------
def _corpus_bools(oracle, n, n_sub, seed=77):
    """synth_corpus(seed, 0, n, n_sub, 200) with six copies of other entries with 0, 1, 5, 20, 60 and 150 flipped Booleans, two
    all-zero entries, one all-ones entry, one triple of identical entries"""
    b = oracle.synth_corpus(seed, 0, n, n_sub, L).copy()
    rng = np.random.default_rng(seed * 1000 + n * 10 + n_sub)
    free = list(rng.permutation(n))

    def take(k):
        got = free[:k]
        del free[:k]
        return got

    for flips in (0, 1, 5, 20, 60, 150):
        src, dst = take(2)
        b[dst] = b[src]
        where = rng.choice(n_sub * L, flips, replace=False)
        flat = b[dst].reshape(-1)
        flat[where] ^= 1
    for _ in range(2):
        b[take(1)[0]] = 0
    b[take(1)[0]] = 1
    at = take(3)
    b[at[1]] = b[at[0]]
    b[at[2]] = b[at[0]]
    return b


def _packed(oracle, bools):
    return np.ascontiguousarray(oracle.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _uniform(lb, gpu, oracle, bools, capacity):
    n, n_sub, length = bools.shape
    c = lb.Corpus(length, n_sub, capacity)
    if n:
        c.append_packed_device(gpu.from_numpy(_packed(oracle, bools)).cuda())
    return c


_CASE = {}


def _case(oracle):
    """the corpus' Booleans, the oracle's score matrix and the two thresholds, made once and left unchanged"""
    if not _CASE:
        n = 300
        bools = _corpus_bools(oracle, n, 5)
        w = oracle.pack_bools(bools)
        S = np.stack([oracle.corpus_scores_packed(w[i], w, L, L, nthreads=16) for i in range(n)]).astype(np.float32)
        off = S[~np.eye(n, dtype=bool)]
        d = np.unique(off)
        d = d[d > 0]
        _CASE.update(bools=bools, S=S, thresholds={"selective": np.float32(d[-4]), "median": np.float32(np.sort(S.reshape(-1))[n * n // 2])})
    return _CASE


def _expected_groups(S, t):
    n = len(S)
    D = (S >= np.float32(t)) & ~np.eye(n, dtype=bool)        # the join's ordered pairs
    A = D | D.T
    return _union_find(n, [(int(a), int(b)) for a, b in zip(*np.nonzero(A))]), D


def _saved(c, path):
    c.save(str(path))
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("which", ["selective", "median"])
def test_duplicate_groups_equal_the_oracle(lb, gpu, oracle, which):
    case = _case(oracle)
    t = case["thresholds"][which]
    assert t > 0
    want, D = _expected_groups(case["S"], t)
    n = len(want)
    groups = int((want == np.arange(n)).sum())
    assert 1 <= groups < n and (which != "selective" or groups > n // 2)
    c = _uniform(lb, gpu, oracle, case["bools"], n)
    # a capacity a few rows fit: the halving path, down to chunks of a few rows
    small = 3 * max(1, int(D.sum(axis=1).max()))
    assert small < D.sum()
    for kw in (dict(), dict(key_capacity=small), dict(rows_per_call=64), dict(key_capacity=int(D.sum()), rows_per_call=100)):
        labels, count = c.duplicate_groups(float(t), **kw)
        gpu.cuda.synchronize()
        got = labels.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want), (which, kw, np.nonzero(got != want)[0][:8])
        assert int(count.item()) == groups, (which, kw)
    # a single row that does not fit
    most = int(D.sum(axis=1).max())
    assert most >= 2                                         # (the planted triple)
    with pytest.raises(ValueError):
        c.duplicate_groups(float(t), key_capacity=most - 1)
    c.dispose()


@pytest.mark.parametrize("which", ["selective", "median"])
def test_deduplicate(lb, gpu, oracle, tmp_path, which):
    case = _case(oracle)
    t = case["thresholds"][which]
    want, _ = _expected_groups(case["S"], t)
    n = len(want)
    first = want == np.arange(n)
    c = _uniform(lb, gpu, oracle, case["bools"], n)
    removed, labels = c.deduplicate(float(t))
    assert removed == n - int(first.sum()) and len(c) == int(first.sum())
    assert np.array_equal(labels.cpu().numpy().astype(np.int64), want)
    fresh = _uniform(lb, gpu, oracle, case["bools"][first], n)
    assert _saved(c, tmp_path / "deduplicated.bin") == _saved(fresh, tmp_path / "fresh.bin")
    fresh.dispose()
    # nothing matches anything else any more, in either direction
    _, offsets = c.join_threshold_keys_device(float(t), 16, skip_same_index=True)
    gpu.cuda.synchronize()
    assert int(offsets[len(c)].item()) == 0
    # and a second pass removes nothing
    assert c.deduplicate(float(t))[0] == 0
    c.dispose()


# ---- a ragged corpus' route: gather one length's entries, query them packed, group with the gathered keys as row keys ---------
def test_ragged_route_with_row_keys(lb, gpu, oracle):
    n, length = 60, 22
    counts = np.random.default_rng(9).integers(20, 25, n).astype(np.uint32)
    same = [3, 17, 18, 40, 59]
    counts[same] = length
    flat = oracle.synth_ragged_entries(4242, 0, counts, 200)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    flat[off[18]:off[19]] = flat[off[3]:off[4]]              # planted copies among the entries of this length
    flat[off[59]:off[60]] = flat[off[17]:off[18]]
    c = lb.Corpus.ragged(200, n, int(counts.sum()))
    c.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, flat)).cuda(), counts)
    ids = [e for e in range(n) if counts[e] == length]
    assert set(same) <= set(ids)
    ids = ids[::-1]                                          # (the rows in another order than the entries)
    row_keys = gpu.from_numpy(_i64([_key(e) for e in ids])).cuda()
    packed, _ = c.gather_keys_device(row_keys)
    capacity = n
    # a threshold out of the device's own scores: the 20th largest distinct one
    keys, cnt = c.query_packed_threshold_keys_device(packed, len(ids), length, 1e-6, capacity)
    gpu.cuda.synchronize()
    scores = np.unique(np.concatenate([lb.decode_threshold_keys(keys[q], cnt[q].item())[1] for q in range(len(ids))]))
    t = float(scores[-20])
    keys, cnt = c.query_packed_threshold_keys_device(packed, len(ids), length, t, capacity)
    labels = gpu.full((n,), POISON32, dtype=gpu.int32, device="cuda")
    count = gpu.full((1,), POISON64, dtype=gpu.int64, device="cuda")
    lb.group_labels_from_keys_device(keys, n, row_keys=row_keys, labels=labels, group_count=count)
    gpu.cuda.synchronize()
    edges = []
    for q, e in enumerate(ids):
        idx, _ = lb.decode_threshold_keys(keys[q], cnt[q].item())
        assert e in idx                                      # (the self-match)
        edges += [(e, int(j)) for j in idx]
    want = _union_find(n, edges)
    assert want[18] == 3 and want[59] == 17
    assert np.array_equal(labels.cpu().numpy().astype(np.int64), want)
    assert int(count.item()) == int((want == np.arange(n)).sum())
    c.dispose()
