"""GPU tests of the ragged corpus join (LBAudioDetectiveCorpusJoinRaggedThresholdKeysDevice, LBAudioDetectiveCorpusJoinRaggedThreshold)
and of Corpus.duplicate_groups / Corpus.deduplicate on a ragged corpus.  The expected lists come from the CPU ORACLE: row i is
oracle.corpus_best_ragged(entry i, (flat, counts), range, want_scores=True); the matches are np.nonzero(S[i] >= float32(t)) in
ascending entry index, the rows one after the other, the offsets their cumulative counts; the lags come from align_ref.align
(whose score is asserted equal to the oracle's on every pair it is asked for).  Keys are compared as 64-bit integers, offsets and
lags exactly, the slots behind the total as 0; key, lag and offset buffers are poison-filled before every call.  The thresholds
are values of the oracle's own score matrix (the off-diagonal maximum, the 4th largest, the median, the next float above the
maximum, and the 4th largest distinct off-diagonal value), so ties at the threshold exist by construction and nothing needs a
tolerance.  Where a list has more than LAG_PAIRS matches, the lags of an evenly spaced sample of LAG_PAIRS of them are
compared with align_ref (a Python loop per pair); every other list is compared lag by lag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from align_ref import align

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
L = 200
LAG_PAIRS = 400


def _source(name):
    return open(os.path.join(ROOT, name)).read()


def _constant(name):
    return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name,
                         _source(os.path.join("lbaudiodetective_amd", "csrc", "k_join_ragged.hip"))).group(1))


TE = _constant("kJoinRaggedTileEntries")
TR = _constant("kJoinRaggedTileRows")
CAP = int(re.search(r"^#define\s+LBAD_JOIN_RAGGED_MAX_SUBFINGERPRINTS\s+(\d+)", _source(os.path.join("include", "lbaudiodetective.h")),
                    re.M).group(1))
N_CASE = 2 * TE + 5


# ---- corpora ------------------------------------------------------------------------------------------------------------------
class Entries:
    """a list of [n_e, length] Boolean arrays with what the oracle and the device want of it"""

    def __init__(self, entries):
        self.entries = [np.ascontiguousarray(e, np.uint8) for e in entries]
        self.counts = np.array([len(e) for e in self.entries], np.uint32)
        self.length = self.entries[0].shape[1] if self.entries else L
        self.flat = np.concatenate(self.entries, axis=0) if self.entries else np.zeros((0, self.length), np.uint8)

    def __len__(self):
        return len(self.entries)

    def prefix(self, n):
        return Entries(self.entries[:n])

    def take(self, which):
        return Entries([self.entries[i] for i in which])


def _random_entries(oracle, seed, counts, length=L):
    counts = np.asarray(counts, np.uint32)
    flat = oracle.synth_ragged_entries(seed, 0, counts, length)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [flat[off[i]:off[i + 1]].copy() for i in range(len(counts))]


def _case_entries(oracle):
    """N_CASE entries of 1 .. 40 sub-fingerprints (default_rng(11)) with the fixed entries of the issue among the first 63"""
    rng = np.random.default_rng(11)
    e = _random_entries(oracle, 4242, rng.integers(1, 41, N_CASE))
    pool = _random_entries(oracle, 4343, [1, 1, 40, 40, 17, 22, 150, 300, 63, 64, 65, 20])
    e[4], e[9], e[12], e[20] = pool[0], pool[1], pool[2], pool[3]            # two of 1, two of 40
    e[15] = pool[4]                                                          # three of 17: an exact copy, one with 300 flips
    e[22] = pool[4].copy()
    e[30] = pool[4].copy()
    e[30].reshape(-1)[rng.choice(17 * L, 300, replace=False)] ^= 1
    e[25] = pool[5]                                                          # 22 long, verbatim inside one of 150 and one of 300
    e[33], e[41] = pool[6], pool[7]
    e[33][33:33 + 22] = pool[5]
    e[41][250:250 + 22] = pool[5]
    e[44], e[45], e[46] = pool[8], pool[9], pool[10]                          # 63, 64, 65
    e[50] = np.zeros((10, L), np.uint8)                                      # all zero
    e[53] = np.concatenate([pool[11], pool[11]])                             # the same 20-block twice, and the block
    e[57] = pool[11].copy()
    return Entries(e)


def _packed(oracle, flat):
    return np.ascontiguousarray(oracle.pack_bools(flat)).view(np.uint8).reshape(len(flat), 32)


def _ragged(lb, gpu, oracle, ent, entry_capacity=None, record_capacity=None):
    c = lb.Corpus.ragged(ent.length, entry_capacity or max(1, len(ent)), record_capacity or max(1, len(ent.flat)))
    if len(ent):
        c.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, ent.flat)).cuda(), ent.counts)
    return c


def _score_matrix(oracle, rows, ent, range_=0):
    """S[i, j]: entry i of `rows` as the query against entry j of `ent`, by the CPU oracle"""
    rg = range_ if range_ else ent.length
    return np.stack([oracle.corpus_best_ragged(q, (ent.flat, ent.counts), rg, nthreads=16, want_scores=True)[2]
                     for q in rows.entries]).astype(np.float32)


_CASE = {}


def _case(lb, gpu, oracle, n=N_CASE, range_=0):
    """(the corpus of the first n case entries on the device, those entries, the oracle's score matrix at the range): the
    entries and the full matrix at range 0 are made once, a prefix's matrix is a corner of it"""
    if "entries" not in _CASE:
        _CASE["entries"] = _case_entries(oracle)
        _CASE["S"] = {}
        _CASE["corpus"] = {}
    ent = _CASE["entries"].prefix(n)
    if n not in _CASE["corpus"]:
        _CASE["corpus"][n] = _ragged(lb, gpu, oracle, ent)
    if range_ == 0:
        if 0 not in _CASE["S"]:
            full = _CASE["entries"]
            _CASE["S"][0] = _score_matrix(oracle, full, full)
        S = _CASE["S"][0][:n, :n]
    else:
        if (n, range_) not in _CASE["S"]:
            _CASE["S"][(n, range_)] = _score_matrix(oracle, ent, ent, range_)
        S = _CASE["S"][(n, range_)]
    return _CASE["corpus"][n], ent, S


# ---- thresholds (test_gpu_join.py's) ---------------------------------------------------------------------------------------------
def _off_diagonal(S):
    return S[~np.eye(S.shape[0], dtype=bool)] if S.shape[0] == S.shape[1] and S.shape[0] > 1 else S.reshape(-1)


def _selective(S):
    d = np.unique(_off_diagonal(S))
    d = d[d > 0]
    return np.float32(d[-4] if len(d) >= 4 else d[-1])


def _median(S):
    flat = np.sort(S.reshape(-1))
    return np.float32(flat[len(flat) // 2])


def _thresholds(S):
    flat = np.sort(S.reshape(-1))
    out = []
    if S.shape[0] == S.shape[1] and S.shape[0] > 1:
        out.append(_off_diagonal(S).max())
    if len(flat) >= 4:
        out.append(flat[-4])
    out.append(_median(S))
    out.append(np.nextafter(flat[-1], np.float32(np.inf), dtype=np.float32))
    if (_off_diagonal(S) > 0).any():
        out.append(_selective(S))
    seen = []
    for t in out:
        if t > 0 and np.isfinite(t) and not any(t == s for s in seen):
            seen.append(np.float32(t))
    return seen


# ---- the contract, restated ------------------------------------------------------------------------------------------------
def _expected(S, t, first, count, skip, index_base=0):
    """(every match's key in (row, entry) order as uint64, the count + 1 offsets, the matches' (row, entry)) of rows first ..
    first + count - 1 of S"""
    rows = S[first:first + count]
    m = rows >= np.float32(t)
    if skip:
        for r in range(count):
            if first + r < S.shape[1]:
                m[r, first + r] = False
    rr, jj = np.nonzero(m)
    keys = (rows[rr, jj].view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
           (np.uint64(0xFFFFFFFF) - (np.uint64(index_base) + jj.astype(np.uint64)))
    offsets = np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.uint64)
    return keys, offsets, (rr + first, jj)


_LAGS = {}


def _lag(rows, ent, i, j, range_, score):
    """align_ref's lag of row i against entry j; its score is the oracle's"""
    key = (id(rows.entries[i]), id(ent.entries[j]), range_)
    if key not in _LAGS:
        s, lag = align(rows.entries[i], ent.entries[j], range_)
        _LAGS[key] = (np.float32(s), lag, rows.entries[i], ent.entries[j])     # (the arrays are kept: their ids stay theirs)
    assert _LAGS[key][0].view(np.uint32) == np.float32(score).view(np.uint32), (i, j, _LAGS[key][0], score)
    return _LAGS[key][1]


def _buffers(gpu, capacity, count):
    return (gpu.full((capacity,), POISON, dtype=gpu.int64, device="cuda"), gpu.full((capacity,), POISON32, dtype=gpu.int32, device="cuda"),
            gpu.full((count + 1,), POISON, dtype=gpu.int64, device="cuda"))


def _same(got, want_keys, want_offsets, capacity, what, lag_of=None):
    keys, lags, offsets = got
    keys, offsets = keys.cpu().numpy().view(np.uint64), offsets.cpu().numpy().view(np.uint64)
    assert np.array_equal(offsets, want_offsets), (what, offsets[:8], want_offsets[:8], offsets[-1], want_offsets[-1])
    m = min(len(want_keys), capacity)
    bad = np.nonzero(keys[:m] != want_keys[:m])[0]
    assert len(bad) == 0, (what, len(bad), bad[:4], keys[bad[:4]], want_keys[bad[:4]])
    assert not keys[m:].any(), (what, "keys behind the total")
    if lags is not None:
        lags = lags.cpu().numpy()
        assert not lags[m:].any(), (what, "lags behind the total")
        if lag_of is not None and m:
            at = np.arange(m) if m <= LAG_PAIRS else np.unique(np.linspace(0, m - 1, LAG_PAIRS).astype(np.int64))
            want = np.array([lag_of(int(p)) for p in at], np.int32)
            assert np.array_equal(lags[at], want), (what, "lags", at[lags[at] != want][:4], lags[at][lags[at] != want][:4])


def _join_check(lb, gpu, c, ent, S, t, capacity, what, queries=None, rows=None, first=0, count=None, skip=None, range_=0, index_base=0,
                stream=None, want_lags=True):
    """one device call against the oracle; rows: the Entries of `queries` (None: a self-join of ent)"""
    rows = ent if rows is None else rows
    count = S.shape[0] - first if count is None else count
    keys, lags, offsets = _buffers(gpu, capacity, count)
    if stream is not None:
        gpu.cuda.synchronize()
    got = c.join_ragged_threshold_keys_device(float(t), capacity, queries=queries, first=first, count=count, skip_same_index=skip,
                                              range_=range_, index_base=index_base, keys_out=keys, lags_out=lags if want_lags else None,
                                              offsets_out=offsets, want_lags=want_lags, stream=stream)
    if stream is not None:
        gpu.cuda.synchronize()
    assert (got[1] is None) == (not want_lags)
    want_keys, want_offsets, (rr, jj) = _expected(S, t, first, count, (queries is None) if skip is None else skip, index_base)
    _same(got, want_keys, want_offsets, capacity, what, lambda p: _lag(rows, ent, int(rr[p]), int(jj[p]), range_, S[rr[p], jj[p]]))
    return len(want_keys)


def _capacities(total):
    return sorted({1, max(1, total - 1), max(1, total), total + 7})


# ---- the case corpus itself ----------------------------------------------------------------------------------------------------
def test_the_case_corpus_has_what_the_cases_need(lb, gpu, oracle):
    _, ent, S = _case(lb, gpu, oracle)
    assert list(ent.counts[[4, 9, 12, 20, 15, 22, 30, 25, 33, 41, 44, 45, 46, 53, 57]]) == [1, 1, 40, 40, 17, 17, 17, 22, 150, 300, 63, 64, 65, 40, 20]
    # the planted pairs score 1.0, with lags +-33, +-250 and 0
    for i, j, lag in ((25, 33, 33), (33, 25, -33), (25, 41, 250), (41, 25, -250), (15, 22, 0), (22, 15, 0), (57, 53, 0), (53, 57, 0)):
        assert S[i, j] == 1.0 and _lag(ent, ent, i, j, 0, S[i, j]) == lag, (i, j)
    assert not S[50].any() and not S[:, 50].any()                            # the all-zero entry
    assert 0.5 < S[15, 30] < 1.0                                             # the copy with 300 flipped Booleans
    rng = np.random.default_rng(3)
    for i, j in rng.integers(0, 130, (60, 2)):                               # align_ref equals the oracle
        _lag(ent, ent, int(i), int(j), 0, S[i, j])


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------
SIZES = sorted({1, 2, 63, 64, 65, TE - 1, TE, TE + 1, 2 * TE + 5})


@pytest.mark.parametrize("n", SIZES)
def test_sizes_thresholds_capacities_and_bases(lb, gpu, oracle, n):
    c, ent, S = _case(lb, gpu, oracle, n)
    for t in _thresholds(S):
        total = len(_expected(S, t, 0, n, True)[0])
        for capacity in _capacities(total):
            for base in (0, 12345, (1 << 32) - n):
                _join_check(lb, gpu, c, ent, S, t, capacity, (n, float(t), capacity, base), index_base=base)
    t = _selective(S) if n > 1 else np.float32(0.5)
    _join_check(lb, gpu, c, ent, S, t, len(_expected(S, t, 0, n, False)[0]) + 1, (n, "diagonal kept"), skip=False)
    if n == 1:
        keys, lags, offsets = c.join_ragged_threshold_keys_device(0.5, 4)
        assert offsets.cpu().tolist() == [0, 0] and keys.cpu().tolist() == [0] * 4 and lags.cpu().tolist() == [0] * 4


# ---- 2. ranges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("range_", [0, 200, 199, 64, 33, 2, 1])
def test_ranges(lb, gpu, oracle, range_):
    n = 120
    c, ent, S = _case(lb, gpu, oracle, n, range_)
    if range_ in (0, 200):
        assert np.array_equal(S, _case(lb, gpu, oracle, n, 0)[2])
    for t in _thresholds(S):
        total = len(_expected(S, t, 0, n, True)[0])
        for capacity in sorted({max(1, total // 2), total + 7}):
            _join_check(lb, gpu, c, ent, S, t, capacity, (range_, float(t), capacity), range_=range_)


# ---- 3. other sub-fingerprint lengths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [64, 33])
def test_sub_fingerprint_lengths(lb, gpu, oracle, length):
    n = 80
    counts = np.random.default_rng(length).integers(1, 41, n)
    e = _random_entries(oracle, 99, counts, length)
    e[7] = e[3].copy()
    e[11] = np.concatenate([e[40], e[3], e[41]])                             # entry 3 inside a longer one
    ent = Entries(e)
    c = _ragged(lb, gpu, oracle, ent)
    for range_ in (0, length - 1, 2):
        S = _score_matrix(oracle, ent, ent, range_)
        assert range_ == 2 or (S[3, 7] == 1.0 and S[3, 11] == 1.0)
        for t in _thresholds(S):
            total = len(_expected(S, t, 0, n, True)[0])
            _join_check(lb, gpu, c, ent, S, t, total + 3, (length, range_, float(t)), range_=range_)
    c.dispose()


# ---- 4. lags, and the call without them ---------------------------------------------------------------------------------------
def test_lags_of_every_key_and_null_lags(lb, gpu, oracle):
    n = 120
    c, ent, S = _case(lb, gpu, oracle, n)
    global LAG_PAIRS
    before, LAG_PAIRS = LAG_PAIRS, 1 << 30                                   # every key of every list here
    try:
        for t in (_selective(S), np.float32(np.sort(S.reshape(-1))[-300]), np.float32(1.0)):
            for skip in (True, False):
                total = _join_check(lb, gpu, c, ent, S, t, n * n, ("lags", float(t), skip), skip=skip)
                assert total >= 4
                _join_check(lb, gpu, c, ent, S, t, n * n, ("no lags", float(t), skip), skip=skip, want_lags=False)
    finally:
        LAG_PAIRS = before
    # the raw call with outLags NULL
    keys, _, offsets = _buffers(gpu, 500, n)
    t = _selective(S)
    assert lb.lib().LBAudioDetectiveCorpusJoinRaggedThresholdKeysDevice(c._ref, c._ref, 0, n, 0, float(t), 1, 500, 0, keys.data_ptr(), None,
                                                                     offsets.data_ptr(), None) == 0
    gpu.cuda.synchronize()
    wk, wo, _ = _expected(S, t, 0, n, True)
    _same((keys, None, offsets), wk, wo, 500, "raw, NULL lags")
    # the lags are the alignment call's for the same rows and keys
    keys, lags, offsets = c.join_ragged_threshold_keys_device(float(t), 500)
    keys_h, lags_h, off_h = keys.cpu().numpy(), lags.cpu().numpy(), offsets.cpu().numpy()
    rows = [r for r in range(n) if off_h[r + 1] > off_h[r]][:6]
    for r in rows:
        fp = c.fingerprint(r)
        k = int(off_h[r + 1] - off_h[r])
        got = c.align_keys_device([fp], keys[int(off_h[r]):int(off_h[r + 1])].contiguous(), k)
        got = got[0] if isinstance(got, tuple) else got
        assert np.array_equal(got.cpu().numpy().reshape(-1), lags_h[off_h[r]:off_h[r + 1]]), r
        fp.dispose()


# ---- 5. the documented equality with the threshold query -------------------------------------------------------------------------
def test_rows_equal_the_threshold_query(lb, gpu, oracle):
    n = 120
    c, ent, S = _case(lb, gpu, oracle, n)
    for t in (_selective(S), _median(S)):
        keys, lags, offsets = c.join_ragged_threshold_keys_device(float(t), n * n, skip_same_index=False)
        rows, idx, sc, total = lb.decode_join_keys(keys, offsets)
        lags = lags.cpu().numpy()
        for i in (0, 4, 15, 25, 33, 41, 50, 53, 119):
            fp = c.fingerprint(i)
            q_idx, q_sc, q_lag, q_count = c.query_threshold(fp, float(t), n, aligned=True)
            mine = rows == i
            assert q_count == mine.sum() and np.array_equal(q_idx, idx[mine]), (float(t), i)
            assert np.array_equal(q_sc.view(np.uint32), sc[mine].view(np.uint32)) and np.array_equal(q_lag, lags[:total][mine]), (float(t), i)
            fp.dispose()


# ---- 6. the two directions -------------------------------------------------------------------------------------------------------
def test_directions_of_unequal_lengths_mirror_each_other(lb, gpu, oracle):
    n = 120
    c, ent, S = _case(lb, gpu, oracle, n)
    t = S[S > 0].min()
    rows, idx, sc, lags, total = c.join_ragged_threshold(float(t), n * n, skip_same_index=False)
    assert total == len(rows) == (S > 0).sum()
    cell = {(int(r), int(j)): (np.float32(s).view(np.uint32), int(g)) for r, j, s, g in zip(rows, idx, sc, lags)}
    unequal = differ = 0
    for (i, j), (bits, lag) in cell.items():
        if ent.counts[i] != ent.counts[j]:
            unequal += 1
            assert cell[(j, i)] == (bits, -lag), (i, j)
        elif i != j and cell.get((j, i), (0, 0))[0] != bits:
            differ += 1
    assert unequal > 10000 and differ > 50            # (equal lengths: the directions differ in general)


# ---- 7. row windows ---------------------------------------------------------------------------------------------------------
def test_row_windows_are_slices_of_the_full_list(lb, gpu, oracle):
    n = 2 * TE + 5
    c, ent, S = _case(lb, gpu, oracle, n)
    t = _selective(S)
    full_keys, full_offsets, _ = _expected(S, t, 0, n, True)
    for first, count in ((0, 1), (n - 1, 1), (TR - 1, 2), (5, n - 5), (0, n)):
        got = _buffers(gpu, len(full_keys) + 3, count)
        c.join_ragged_threshold_keys_device(float(t), len(full_keys) + 3, first=first, count=count, keys_out=got[0], lags_out=got[1],
                                            offsets_out=got[2])
        lo, hi = int(full_offsets[first]), int(full_offsets[first + count])
        _same(got, full_keys[lo:hi], full_offsets[first:first + count + 1] - full_offsets[first], len(full_keys) + 3, (first, count))
        _join_check(lb, gpu, c, ent, S, _median(S), 1000, (first, count, "median"), first=first, count=count)


# ---- 8. chunk seams -----------------------------------------------------------------------------------------------------------
def _chunk_bytes(n_entries, rows):
    """the header's formula: the scratch of a chunk of `rows` rows"""
    tiles = (n_entries + TE - 1) // TE
    return 16 + rows * (8 + 8 * tiles) + ((rows + TR - 1) // TR) * 4 * tiles


def test_chunk_seams(lb, gpu, oracle):
    n = 2 * TE + 5
    c, ent, S = _case(lb, gpu, oracle, n)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    try:
        for t in (_selective(S), _median(S)):
            want = _join_check(lb, gpu, c, ent, S, t, 5000, ("one chunk", float(t)))
            for rows in (2 * TR, TR):
                assert n % rows and n // rows >= 3
                c.set_join_scratch_limit(_chunk_bytes(n, rows) + 5)
                for capacity in (5000, max(1, want // 2)):
                    _join_check(lb, gpu, c, ent, S, t, capacity, ("chunks of", rows, float(t), capacity))
                _join_check(lb, gpu, c, ent, S, t, 5000, ("a window over seams", rows), first=rows - 1, count=rows + 2)
            c.set_join_scratch_limit(0)
            _join_check(lb, gpu, c, ent, S, t, 5000, ("the default again", float(t)))
        t = _selective(S)
        c.set_join_scratch_limit(_chunk_bytes(n, TR) - 1)
        with pytest.raises(lb.LBAudioDetectiveError) as e:
            c.join_ragged_threshold_keys_device(float(t), 100)
        assert e.value.status == bad
        c.set_join_scratch_limit(_chunk_bytes(n, TR))
        _join_check(lb, gpu, c, ent, S, t, 2000, "a limit of exactly one row tile")
    finally:
        c.set_join_scratch_limit(0)
    _join_check(lb, gpu, c, ent, S, t, 2000, "the default limit again")


# ---- 9. dense -----------------------------------------------------------------------------------------------------------------
def test_dense_lists_and_cuts_inside_a_row(lb, gpu, oracle):
    n = TE + 1
    c, ent, S = _case(lb, gpu, oracle, n)
    t = S[S > 0].min()
    keys, offsets, _ = _expected(S, t, 0, n, True)
    total = len(keys)
    assert total > n * (n - 8)                                   # close to n^2 keys (the all-zero entry matches nothing)
    row = next(r for r in range(100, n) if offsets[r + 1] - offsets[r] > 10)
    inside = int(offsets[row]) + 3                               # a capacity that ends inside a row
    assert offsets[row] < inside < offsets[row + 1]
    for capacity in (total + 7, total, total - 1, inside, max(1, int(offsets[1]) - 1), 1):
        _join_check(lb, gpu, c, ent, S, t, capacity, ("dense", capacity))
        _join_check(lb, gpu, c, ent, S, t, capacity, ("dense, diagonal kept", capacity), skip=False)


# ---- 10. cross-join -------------------------------------------------------------------------------------------------------------
def test_cross_join(lb, gpu, oracle):
    n, n_rows = 300, 70
    base = _case(lb, gpu, oracle, n)[1]
    q = _random_entries(oracle, 515, np.random.default_rng(5).integers(1, 41, n_rows))
    q[7] = base.entries[41].copy()                        # a row that is an entry elsewhere (the one of 300)
    q[69] = np.zeros((3, L), np.uint8)
    e = list(base.entries)
    e[3] = q[3].copy()                                    # copies of row 3 at entry 3 (the pair the skip drops) and at entry 200
    e[200] = q[3].copy()
    ent, rows = Entries(e), Entries(q)
    corpus, queries = _ragged(lb, gpu, oracle, ent), _ragged(lb, gpu, oracle, rows)
    S = _score_matrix(oracle, rows, ent)
    assert S[3, 3] == 1.0 and S[3, 200] == 1.0 and S[7, 41] == 1.0
    for t in _thresholds(S) + [np.float32(1.0)]:
        for skip in (False, True, None):                  # None: off for two corpora
            total = _join_check(lb, gpu, corpus, ent, S, t, 4000, ("cross", float(t), skip), queries=queries, rows=rows,
                                skip=bool(skip) if skip is not None else None)
            _join_check(lb, gpu, corpus, ent, S, t, max(1, total - 1), ("cross, cut", float(t), skip), queries=queries, rows=rows, skip=skip,
                        index_base=1 << 20)
    r_off, i_off, _, l_off, _ = corpus.join_ragged_threshold(1.0, 100, queries=queries, skip_same_index=False)
    r_on, i_on, _, _, _ = corpus.join_ragged_threshold(1.0, 100, queries=queries, skip_same_index=True)
    pairs_off, pairs_on = list(zip(r_off.tolist(), i_off.tolist())), list(zip(r_on.tolist(), i_on.tolist()))
    assert (3, 3) in pairs_off and (3, 200) in pairs_off and (7, 41) in pairs_off
    assert pairs_on == [p for p in pairs_off if p != (3, 3)]
    assert l_off[pairs_off.index((7, 41))] == 0 and (7, 33) not in pairs_off
    # a window of the rows, and the other way round: 300 rows against 70 entries
    _join_check(lb, gpu, corpus, ent, S, _selective(S), 500, "cross window", queries=queries, rows=rows, first=30, count=35, skip=True)
    St = _score_matrix(oracle, ent, rows)
    for t in (_selective(St), _median(St)):
        _join_check(lb, gpu, queries, rows, St, t, 5000, ("300 rows against 70", float(t)), queries=corpus, rows=ent, skip=True)
    for x in (corpus, queries):
        x.dispose()


# ---- 11. the cap --------------------------------------------------------------------------------------------------------------
def test_the_cap(lb, gpu, oracle):
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    e = _random_entries(oracle, 808, [1, CAP, 1, 1, 2, 1])
    e[2] = e[1][700:701].copy()                               # an entry of 1 that lies inside the longest one
    e[4] = e[1][CAP - 2:].copy()                              # ... and its last two sub-fingerprints
    ent = Entries(e)
    c = _ragged(lb, gpu, oracle, ent, entry_capacity=8, record_capacity=2 * CAP + 64)
    S = _score_matrix(oracle, ent, ent)
    assert S[2, 1] == 1.0 and S[1, 2] == 1.0 and S[4, 1] == 1.0
    for t in _thresholds(S):
        for skip in (True, False):
            _join_check(lb, gpu, c, ent, S, t, 64, ("cap", float(t), skip), skip=skip)
    rows, idx, _, lags, _ = c.join_ragged_threshold(1.0, 64)
    cell = {(int(r), int(j)): int(g) for r, j, g in zip(rows, idx, lags)}
    assert cell[(2, 1)] == 700 and cell[(1, 2)] == -700 and cell[(4, 1)] == CAP - 2 and cell[(1, 4)] == -(CAP - 2)
    # one entry above the cap, on either side
    over = Entries(_random_entries(oracle, 809, [3, CAP + 1]))
    big = _ragged(lb, gpu, oracle, over)
    for corpus, queries in ((big, None), (big, c), (c, big)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            corpus.join_ragged_threshold_keys_device(0.7, 16, queries=queries)
        assert err.value.status == bad
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            corpus.join_ragged_threshold(0.7, 16, queries=queries)
        assert err.value.status == bad
        _join_check(lb, gpu, c, ent, S, _selective(S), 64, "after the refusal")
    for x in (c, big):
        x.dispose()


# ---- 12. streams ---------------------------------------------------------------------------------------------------------------
def test_streams_back_to_back_and_append_then_join(lb, gpu, oracle):
    n = 2 * TE + 5
    c, ent, S = _case(lb, gpu, oracle, n)
    ts = [_selective(S), _median(S), np.float32(1.0)]
    s1, s2, s3 = gpu.cuda.Stream(), gpu.cuda.Stream(), gpu.cuda.Stream()
    outs = [_buffers(gpu, 3000, n) for _ in range(3)]
    gpu.cuda.synchronize()
    for (keys, lags, offsets), t, s in zip(outs, ts, (s1, s1, s2)):      # no host synchronisation in between
        c.join_ragged_threshold_keys_device(float(t), 3000, keys_out=keys, lags_out=lags, offsets_out=offsets, stream=s)
    gpu.cuda.synchronize()
    for got, t in zip(outs, ts):
        wk, wo, (rr, jj) = _expected(S, t, 0, n, True)
        _same(got, wk, wo, 3000, ("streams", float(t)), lambda p: _lag(ent, ent, int(rr[p]), int(jj[p]), 0, S[rr[p], jj[p]]))
    # an append on a third stream, then at once a join on another: the join waits for the append on the device
    packed = gpu.from_numpy(_packed(oracle, ent.flat)).cuda()
    head = int(ent.counts[:100].sum())
    grown = lb.Corpus.ragged(L, n, len(ent.flat))
    grown.append_ragged_packed_device(packed[:head], ent.counts[:100])
    got = _buffers(gpu, 3000, n)
    gpu.cuda.synchronize()
    grown.append_ragged_packed_device(packed[head:], ent.counts[100:], stream=s3)
    grown.join_ragged_threshold_keys_device(float(ts[0]), 3000, keys_out=got[0], lags_out=got[1], offsets_out=got[2], stream=s1)
    gpu.cuda.synchronize()
    wk, wo, _ = _expected(S, ts[0], 0, n, True)
    _same(got, wk, wo, 3000, "append, then join")
    grown.dispose()


# ---- 13. after a removal ---------------------------------------------------------------------------------------------------------
def test_after_remove(lb, gpu, oracle):
    n = TE + 1
    _, ent, S = _case(lb, gpu, oracle, n)
    c = _ragged(lb, gpu, oracle, ent)
    gone = [0, 22, 33, 63, 64, 100, n - 1]
    kept = [i for i in range(n) if i not in gone]
    c.remove(gone)
    assert len(c) == len(kept)
    Sk = np.ascontiguousarray(S[np.ix_(kept, kept)])
    for t in (_selective(Sk), _median(Sk), np.float32(1.0)):
        _join_check(lb, gpu, c, ent.take(kept), Sk, t, 3000, ("after remove", float(t)))
    c.dispose()


# ---- 14. host form ---------------------------------------------------------------------------------------------------------------
def test_host_form_equals_the_decoded_device_form(lb, gpu, oracle):
    n = 120
    c, ent, S = _case(lb, gpu, oracle, n)
    N = lb._native
    for t in (_selective(S), _median(S), np.float32(1.0)):
        for first, count in ((0, n), (17, 90)):
            wk, wo, (rr, jj) = _expected(S, t, first, count, True)
            total = len(wk)
            for capacity in (total + 5, max(1, total - 2)):
                keys, d_lags, offsets = c.join_ragged_threshold_keys_device(float(t), capacity, first=first, count=count)
                d_rows, d_idx, d_sc, d_total = lb.decode_join_keys(keys, offsets, first)
                rows, idx, sc, lags, h_total = c.join_ragged_threshold(float(t), capacity, first=first, count=count)
                assert h_total == d_total == total                       # never cut
                m = min(total, capacity)
                assert np.array_equal(rows, d_rows) and np.array_equal(idx, d_idx) and np.array_equal(sc.view(np.uint32), d_sc.view(np.uint32))
                assert np.array_equal(lags, d_lags.cpu().numpy()[:m])
                assert np.array_equal(rows, rr[:m]) and np.array_equal(idx, jj[:m])
                assert np.array_equal(sc.view(np.uint32), S[rr[:m], jj[:m]].view(np.uint32))
                # the raw call: the padding behind the pairs is -1 / -1 / 0 / 0; without outLags the rest is the same
                for with_lags in (True, False):
                    o_rows, o_idx, o_sc, o_lags, o_total = ((N.SInt64 * capacity)(), (N.SInt64 * capacity)(), (N.Float32 * capacity)(),
                                                            (N.SInt32 * capacity)(*([77] * capacity)), N.UInt64(0))
                    assert lb.lib().LBAudioDetectiveCorpusJoinRaggedThreshold(c._ref, c._ref, first, count, 0, float(t), 1, capacity, o_rows,
                                                                             o_idx, o_sc, o_lags if with_lags else None,
                                                                             C.byref(o_total)) == 0
                    assert o_total.value == total
                    assert list(o_rows)[m:] == [-1] * (capacity - m) and list(o_idx)[m:] == [-1] * (capacity - m)
                    assert list(o_sc)[m:] == [0.0] * (capacity - m) and list(o_rows)[:m] == rows.tolist()
                    assert list(o_lags) == (lags.tolist() + [0] * (capacity - m) if with_lags else [77] * capacity)


# ---- 15. refusals that need a corpus ----------------------------------------------------------------------------------------------
def test_refusals_and_the_call_after_them(lb, gpu, oracle):
    n = 120
    c, ent, S = _case(lb, gpu, oracle, n)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    uniform = lb.Corpus(L, 5, 50)
    uniform.append_packed_device(gpu.from_numpy(_packed(oracle, oracle.synth_corpus(77, 0, 50, 5, L).reshape(-1, L)).reshape(50, 5, 32)).cuda())
    short = _ragged(lb, gpu, oracle, Entries(_random_entries(oracle, 7, [3, 4, 5], 64)))
    t = _selective(S)

    def refused(corpus, **kw):
        with pytest.raises(lb.LBAudioDetectiveError) as e:
            corpus.join_ragged_threshold_keys_device(float(t), 100, **kw)
        assert e.value.status == bad, kw
        with pytest.raises(lb.LBAudioDetectiveError) as e:
            corpus.join_ragged_threshold(float(t), 100, **{k: v for k, v in kw.items() if k != "index_base"})
        assert e.value.status == bad, kw
        _join_check(lb, gpu, c, ent, S, t, 2000, ("after a refusal", kw))      # the next valid call is right

    refused(uniform)
    refused(c, queries=uniform)
    refused(uniform, queries=c)
    refused(c, queries=short)
    refused(short, queries=c)
    refused(c, first=n - 3, count=4)
    refused(c, first=n, count=1)
    refused(c, queries=short, first=0, count=4)
    with pytest.raises(lb.LBAudioDetectiveError) as e:
        c.join_ragged_threshold_keys_device(float(t), 100, index_base=(1 << 32) - n + 1)
    assert e.value.status == bad
    _join_check(lb, gpu, c, ent, S, t, 2000, "base + count == 2^32", index_base=(1 << 32) - n)
    # the uniform join still refuses a ragged corpus
    with pytest.raises(lb.LBAudioDetectiveError) as e:
        c.join_threshold_keys_device(float(t), 100)
    assert e.value.status == bad
    # an empty scanned corpus: zero offsets, keys and lags
    empty = lb.Corpus.ragged(L, 10, 100)
    keys, lags, offsets = _buffers(gpu, 9, n)
    empty.join_ragged_threshold_keys_device(float(t), 9, queries=c, keys_out=keys, lags_out=lags, offsets_out=offsets)
    assert not keys.cpu().numpy().any() and not offsets.cpu().numpy().any() and not lags.cpu().numpy().any()
    short.join_ragged_threshold_keys_device(0.5, 9)           # (a scratch of its own, to be freed below)
    live = lb.debug_live_bytes()[0]
    for x in (uniform, short, empty):
        x.dispose()
    assert lb.debug_live_bytes()[0] < live


# ---- 16. / 17. duplicate groups and deduplication of a ragged corpus ----------------------------------------------------------------
def _union_find(n, edges):
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


def _expected_groups(S, t):
    n = len(S)
    D = (S >= np.float32(t)) & ~np.eye(n, dtype=bool)        # the join's ordered pairs
    A = D | D.T
    return _union_find(n, [(int(a), int(b)) for a, b in zip(*np.nonzero(A))]), D


@pytest.mark.parametrize("which", ["selective", "median"])
def test_duplicate_groups_equal_the_oracle(lb, gpu, oracle, which):
    n = TE + 1
    c, ent, S = _case(lb, gpu, oracle, n)
    t = _selective(S) if which == "selective" else _median(S)
    want, D = _expected_groups(S, t)
    groups = int((want == np.arange(n)).sum())
    assert 1 <= groups < n and (which != "selective" or groups > n // 2)
    small = 3 * max(1, int(D.sum(axis=1).max()))
    for kw in (dict(), dict(key_capacity=small), dict(rows_per_call=64), dict(key_capacity=max(small, int(D.sum()) // 3), rows_per_call=100)):
        labels, count = c.duplicate_groups(float(t), **kw)
        gpu.cuda.synchronize()
        got = labels.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want), (which, kw, np.nonzero(got != want)[0][:8])
        assert int(count.item()) == groups, (which, kw)
    most = int(D.sum(axis=1).max())
    assert most >= 2
    with pytest.raises(ValueError):
        c.duplicate_groups(float(t), key_capacity=most - 1)


def _saved(c, path):
    c.save(str(path))
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("which", ["selective", "median"])
def test_deduplicate(lb, gpu, oracle, tmp_path, which):
    n = TE + 1
    _, ent, S = _case(lb, gpu, oracle, n)
    t = _selective(S) if which == "selective" else _median(S)
    want, _ = _expected_groups(S, t)
    first = want == np.arange(n)
    c = _ragged(lb, gpu, oracle, ent)
    removed, labels = c.deduplicate(float(t))
    assert removed == n - int(first.sum()) and len(c) == int(first.sum())
    assert np.array_equal(labels.cpu().numpy().astype(np.int64), want)
    fresh = _ragged(lb, gpu, oracle, ent.take(np.nonzero(first)[0]), entry_capacity=n, record_capacity=len(ent.flat))
    assert _saved(c, tmp_path / "deduplicated.bin") == _saved(fresh, tmp_path / "fresh.bin")
    fresh.dispose()
    # nothing matches anything else any more, in either direction
    _, _, offsets = c.join_ragged_threshold_keys_device(float(t), 16, skip_same_index=True)
    gpu.cuda.synchronize()
    assert int(offsets[len(c)].item()) == 0
    # and a second pass removes nothing
    assert c.deduplicate(float(t))[0] == 0
    c.dispose()
