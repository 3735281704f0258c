"""GPU tests of the corpus join (LBAudioDetectiveCorpusJoinThresholdKeysDevice, LBAudioDetectiveCorpusJoinThreshold,
LBAudioDetectiveCorpusSetJoinScratchLimit).  The expected lists come from the CPU ORACLE: row i is
oracle.corpus_scores_packed(words[i], words, 200, range); the matches are np.nonzero(scores >= float32(t)) in ascending entry
index, the rows one after the other, the offsets their cumulative counts.  Keys are compared as 64-bit integers, offsets
exactly, the slots behind the total as 0; key and offset buffers are poison-filled before every call.  The thresholds are
values of the oracle's own score matrix (the off-diagonal maximum, the 4th largest, the median, the next float above the
maximum, and the 4th largest distinct off-diagonal value), so ties at the threshold exist by construction and nothing needs a
tolerance."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -0x0123456789ABCDEF
L = 200


def _constant(name):
    src = open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_join.hip")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))


TE = _constant("kJoinTileEntries")
TR = _constant("kJoinTileRows")


# ---- the corpus of the cases -------------------------------------------------------------------------------------------------
def _corpus_bools(oracle, n, n_sub, seed=77):
    """synth_corpus(seed, 0, n, n_sub, 200) with, as far as n distinct entries allow: six copies of other entries with 0, 1, 5,
    20, 60 and 150 flipped Booleans, two all-zero entries, one all-ones entry, one triple of identical entries"""
    b = oracle.synth_corpus(seed, 0, n, n_sub, L).copy()
    rng = np.random.default_rng(seed * 1000 + n * 10 + n_sub)
    free = list(rng.permutation(n))

    def take(k):
        if len(free) < k:
            return None
        got = free[:k]
        del free[:k]
        return got

    for flips in (0, 1, 5, 20, 60, 150):
        at = take(2)
        if at is None:
            break
        src, dst = at
        b[dst] = b[src]
        where = rng.choice(n_sub * L, flips, replace=False)
        flat = b[dst].reshape(-1)
        flat[where] ^= 1
    for _ in range(2):
        at = take(1) if len(free) >= 2 else None           # (a corpus of one entry keeps an entry that is not empty)
        if at is not None:
            b[at[0]] = 0
    at = take(1)
    if at is not None:
        b[at[0]] = 1
    at = take(3)
    if at is not None:
        b[at[1]] = b[at[0]]
        b[at[2]] = b[at[0]]
    return b


def _packed(oracle, bools):
    return np.ascontiguousarray(oracle.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _uniform(lb, gpu, oracle, bools, capacity=None):
    n, n_sub, length = bools.shape
    c = lb.Corpus(length, n_sub, capacity or max(1, n))
    if n:
        c.append_packed_device(gpu.from_numpy(_packed(oracle, bools)).cuda())
    return c


def _score_matrix(oracle, qbools, bools, range_):
    """S[i, j]: row i of qbools as the query against entry j of bools, by the CPU oracle"""
    qw, w = oracle.pack_bools(qbools), oracle.pack_bools(bools)
    rg = range_ if range_ else L
    return np.stack([oracle.corpus_scores_packed(qw[i], w, L, rg, nthreads=16) for i in range(len(qw))]).astype(np.float32)


_CASES = {}


def _case(lb, gpu, oracle, n, n_sub=5, range_=0):
    """(corpus on the device, its Booleans, the oracle's score matrix at the range), made once per shape and left unchanged"""
    key = (n, n_sub)
    if key not in _CASES:
        bools = _corpus_bools(oracle, n, n_sub)
        _CASES[key] = (_uniform(lb, gpu, oracle, bools), bools, {})
    c, bools, mats = _CASES[key]
    if range_ not in mats:
        mats[range_] = _score_matrix(oracle, bools, bools, range_)
    return c, bools, mats[range_]


def _off_diagonal(S):
    return S[~np.eye(S.shape[0], dtype=bool)] if S.shape[0] == S.shape[1] and S.shape[0] > 1 else S.reshape(-1)


def _selective(S):
    """the 4th largest DISTINCT score off the diagonal (the largest where there are fewer): a handful of matches.  With copies
    planted, the off-diagonal maximum and the matrix' 4th largest value are both 1.0; this one lies among the near-copies."""
    d = np.unique(_off_diagonal(S))
    d = d[d > 0]
    return np.float32(d[-4] if len(d) >= 4 else d[-1])


def _median(S):
    flat = np.sort(S.reshape(-1))
    return np.float32(flat[len(flat) // 2])


def _thresholds(S):
    """the off-diagonal maximum, the 4th largest, the median, the next float above the maximum, and _selective -- those that
    are legal (> 0), each once"""
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
    """(every match's key in (row, entry) order as uint64, the count + 1 offsets) of rows first .. first + count - 1 of S"""
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
    return keys, offsets


def _buffers(gpu, capacity, count):
    return (gpu.full((capacity,), POISON, dtype=gpu.int64, device="cuda"), gpu.full((count + 1,), POISON, dtype=gpu.int64, device="cuda"))


def _same(keys, offsets, want_keys, want_offsets, capacity, what):
    keys, offsets = keys.cpu().numpy().view(np.uint64), offsets.cpu().numpy().view(np.uint64)
    assert np.array_equal(offsets, want_offsets), (what, offsets[:8], want_offsets[:8], offsets[-1], want_offsets[-1])
    m = min(len(want_keys), capacity)
    bad = np.nonzero(keys[:m] != want_keys[:m])[0]
    assert len(bad) == 0, (what, len(bad), bad[:4], keys[bad[:4]], want_keys[bad[:4]])
    assert not keys[m:].any(), (what, "keys behind the total")


def _join_check(lb, gpu, c, S, t, capacity, what, queries=None, first=0, count=None, skip=None, range_=0, index_base=0, stream=None):
    count = S.shape[0] - first if count is None else count
    keys, offsets = _buffers(gpu, capacity, count)
    if stream is not None:
        gpu.cuda.synchronize()
    c.join_threshold_keys_device(float(t), capacity, queries=queries, first=first, count=count, skip_same_index=skip, range_=range_,
                                 index_base=index_base, keys_out=keys, offsets_out=offsets, stream=stream)
    if stream is not None:
        gpu.cuda.synchronize()
    want_keys, want_offsets = _expected(S, t, first, count, (queries is None) if skip is None else skip, index_base)
    _same(keys, offsets, want_keys, want_offsets, capacity, what)
    return len(want_keys)


def _capacities(total):
    return sorted({1, max(1, total - 1), max(1, total), total + 7})


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------
SIZES = sorted({1, 2, 63, 64, 65, 255, 256, 257, TE - 1, TE, TE + 1, 2 * TE + 5, TR - 1, TR, TR + 1})


@pytest.mark.parametrize("n", SIZES)
def test_sizes_thresholds_capacities_and_bases(lb, gpu, oracle, n):
    c, _, S = _case(lb, gpu, oracle, n)
    for t in _thresholds(S):
        total = len(_expected(S, t, 0, n, True)[0])
        for capacity in _capacities(total):
            for base in (0, 12345, (1 << 32) - n):
                _join_check(lb, gpu, c, S, t, capacity, (n, float(t), capacity, base), index_base=base)
    t = _selective(S)
    _join_check(lb, gpu, c, S, t, len(_expected(S, t, 0, n, False)[0]) + 1, (n, "diagonal kept"), skip=False)
    if n == 1:
        keys, offsets = c.join_threshold_keys_device(0.5, 4)
        assert offsets.cpu().tolist() == [0, 0] and keys.cpu().tolist() == [0, 0, 0, 0]


# ---- 2. every instance of the kernels, every kind of range ------------------------------------------------------------------------
@pytest.mark.parametrize("n_sub", range(1, 9))
def test_every_sub_fingerprint_count_and_range(lb, gpu, oracle, n_sub):
    n = 300
    for range_ in (0, 200, 199, 64, 33, 2, 1):
        c, _, S = _case(lb, gpu, oracle, n, n_sub, range_)
        ts = _thresholds(S)
        if range_ == 64:
            ts.append(np.float32(0.7))          # at one sub-fingerprint the scores are 32nds: the rows are full of ties
        for t in ts:
            total = len(_expected(S, t, 0, n, True)[0])
            for capacity in sorted({max(1, total // 2), total + 7}):
                _join_check(lb, gpu, c, S, t, capacity, (n_sub, range_, float(t), capacity), range_=range_)


# ---- 3. row windows ---------------------------------------------------------------------------------------------------------
def test_row_windows_are_slices_of_the_full_list(lb, gpu, oracle):
    n = 2 * TE + 5
    c, _, S = _case(lb, gpu, oracle, n)
    t = _selective(S)
    full_keys, full_offsets = _expected(S, t, 0, n, True)
    for first, count in ((0, 1), (n - 1, 1), (TR - 1, 2), (5, n - 5), (0, n)):
        keys, offsets = _buffers(gpu, len(full_keys) + 3, count)
        c.join_threshold_keys_device(float(t), len(full_keys) + 3, first=first, count=count, keys_out=keys, offsets_out=offsets)
        lo, hi = int(full_offsets[first]), int(full_offsets[first + count])
        _same(keys, offsets, full_keys[lo:hi], full_offsets[first:first + count + 1] - full_offsets[first], len(full_keys) + 3,
              (first, count))
        # ... and at the median, where every row has matches
        _join_check(lb, gpu, c, S, _median(S), 1000, (first, count, "median"), first=first, count=count)


# ---- 4. chunk seams -----------------------------------------------------------------------------------------------------------
def _chunk_bytes(n_entries, rows):
    """the header's formula: the scratch of a chunk of `rows` rows"""
    tiles = (n_entries + TE - 1) // TE
    return 16 + rows * (584 + 8 * tiles) + ((rows + TR - 1) // TR) * 4 * tiles


def test_chunk_seams(lb, gpu, oracle):
    n = 600
    c, _, S = _case(lb, gpu, oracle, n)
    try:
        for t in _thresholds(S)[:3]:
            want = _join_check(lb, gpu, c, S, t, 5000, ("one chunk", float(t)))
            for rows in (3 * TR, TR):                    # 600 rows: chunks of 192 (3 whole, 24 left) and of 64 (9 whole, 24 left)
                assert n % rows and n // rows >= 3
                c.set_join_scratch_limit(_chunk_bytes(n, rows) + 5)
                for capacity in (5000, max(1, want // 2)):
                    _join_check(lb, gpu, c, S, t, capacity, ("chunks of", rows, float(t), capacity))
                _join_check(lb, gpu, c, S, t, 5000, ("a window over seams", rows), first=rows - 1, count=rows + 2)
            c.set_join_scratch_limit(0)
            _join_check(lb, gpu, c, S, t, 5000, ("the default again", float(t)))
    finally:
        c.set_join_scratch_limit(0)


# ---- 5. dense -----------------------------------------------------------------------------------------------------------------
def test_dense_lists_and_cuts_inside_a_row(lb, gpu, oracle):
    n = 257
    c, _, S = _case(lb, gpu, oracle, n)
    t = S[S > 0].min()
    keys, offsets = _expected(S, t, 0, n, True)
    total = len(keys)
    assert total > n * (n - 8)                                   # close to n^2 keys
    row = next(r for r in range(100, n) if offsets[r + 1] - offsets[r] > 10)
    inside = int(offsets[row]) + 3                               # a capacity that ends inside a row
    assert offsets[row] < inside < offsets[row + 1]
    for capacity in (total + 7, total, total - 1, inside, max(1, int(offsets[1]) - 1), 1):
        _join_check(lb, gpu, c, S, t, capacity, ("dense", capacity))
        _join_check(lb, gpu, c, S, t, capacity, ("dense, diagonal kept", capacity), skip=False)


# ---- 6. the diagonal, and the documented equality with the threshold query ------------------------------------------------------
def test_diagonal_and_equality_with_the_packed_threshold_query(lb, gpu, oracle):
    n = 200
    c, bools, S = _case(lb, gpu, oracle, n)
    zero = [i for i in range(n) if not bools[i].any()]
    assert len(zero) == 2 and all(S[i, i] == 0 for i in zero) and not S[zero].any() and not S[:, zero].any()
    for t in _thresholds(S):
        for skip in (False, True):
            _join_check(lb, gpu, c, S, t, n * n, ("diagonal", float(t), skip), skip=skip)
    # skip off at a threshold every self-score of a non-zero entry reaches: exactly those diagonals are there
    t = np.float32(1.0)
    rows, idx, _, total = c.join_threshold(float(t), n * n, skip_same_index=False)
    on_diagonal = sorted(int(r) for r, j in zip(rows, idx) if r == j)
    assert on_diagonal == [i for i in range(n) if S[i, i] >= t] == [i for i in range(n) if i not in zero]
    rows, idx, _, _ = c.join_threshold(float(t), n * n, skip_same_index=True)
    assert not any(r == j for r, j in zip(rows, idx)) and len(rows) == total - len(on_diagonal)
    # every row's keys and count equal query_packed_threshold_keys_device on that entry's packed row
    packed = gpu.from_numpy(_packed(oracle, bools)).cuda()
    for t in _thresholds(S)[:3]:
        keys, offsets = c.join_threshold_keys_device(float(t), n * n, skip_same_index=False)
        tk, tc = c.query_packed_threshold_keys_device(packed, n, 5, float(t), n)
        keys, offsets, tk, tc = keys.cpu().numpy(), offsets.cpu().numpy(), tk.cpu().numpy(), tc.cpu().numpy()
        assert np.array_equal(np.diff(offsets), tc)
        for i in range(n):
            assert np.array_equal(keys[offsets[i]:offsets[i + 1]], tk[i, :tc[i]]), (float(t), i)


# ---- 7. cross-join ------------------------------------------------------------------------------------------------------------
def test_cross_join(lb, gpu, oracle):
    n, rows = 700, 130
    c, bools, _ = _case(lb, gpu, oracle, n)
    qb = oracle.synth_corpus(78, 0, rows, 5, L).copy()
    qb[7] = bools[40]                                     # a row that is an entry elsewhere
    qb[129] = 0
    cb = bools.copy()
    cb[3] = qb[3]                                         # copies of row 3 at entry 3 (the pair the skip drops) and at entry 500
    cb[500] = qb[3]
    corpus = _uniform(lb, gpu, oracle, cb)
    queries = _uniform(lb, gpu, oracle, qb)
    S = _score_matrix(oracle, qb, cb, 0)
    assert S[3, 3] == 1.0 and S[3, 500] == 1.0
    for t in _thresholds(S) + [np.float32(1.0)]:
        for skip in (False, True, None):                  # None: off for two corpora
            total = _join_check(lb, gpu, corpus, S, t, 4000, ("cross", float(t), skip), queries=queries, skip=bool(skip) if skip is not None else None)
            _join_check(lb, gpu, corpus, S, t, max(1, total - 1), ("cross, cut", float(t), skip), queries=queries, skip=skip, index_base=1 << 20)
    r_off, i_off, _, _ = corpus.join_threshold(1.0, 100, queries=queries, skip_same_index=False)
    r_on, i_on, _, _ = corpus.join_threshold(1.0, 100, queries=queries, skip_same_index=True)
    pairs_off, pairs_on = list(zip(r_off.tolist(), i_off.tolist())), list(zip(r_on.tolist(), i_on.tolist()))
    assert (3, 3) in pairs_off and (3, 500) in pairs_off and (7, 40) in pairs_off
    assert pairs_on == [p for p in pairs_off if p != (3, 3)]
    # a window of the rows, the other way round too: 700 rows against 130 entries
    _join_check(lb, gpu, corpus, S, _selective(S), 500, "cross window", queries=queries, first=60, count=70, skip=True)
    St = _score_matrix(oracle, cb, qb, 0)
    _join_check(lb, gpu, queries, St, _selective(St), 500, "700 rows against 130", queries=corpus, skip=True)
    for x in (corpus, queries):
        x.dispose()


# ---- 8. streams and reuse -------------------------------------------------------------------------------------------------------
def test_streams_back_to_back_and_append_then_join(lb, gpu, oracle):
    n = 600
    c, bools, S = _case(lb, gpu, oracle, n)
    ts = [_selective(S), _median(S), np.float32(1.0)]
    s1, s2, s3 = gpu.cuda.Stream(), gpu.cuda.Stream(), gpu.cuda.Stream()
    outs = [_buffers(gpu, 3000, n) for _ in range(3)]
    gpu.cuda.synchronize()
    for (keys, offsets), t, s in zip(outs, ts, (s1, s1, s2)):      # no host synchronisation in between
        c.join_threshold_keys_device(float(t), 3000, keys_out=keys, offsets_out=offsets, stream=s)
    gpu.cuda.synchronize()
    for (keys, offsets), t in zip(outs, ts):
        wk, wo = _expected(S, t, 0, n, True)
        _same(keys, offsets, wk, wo, 3000, ("streams", float(t)))
    # an append on a third stream, then at once a join on another: the join waits for the append on the device
    packed = gpu.from_numpy(_packed(oracle, bools)).cuda()
    grown = lb.Corpus(L, 5, n)
    grown.append_packed_device(packed[:100])
    keys, offsets = _buffers(gpu, 3000, n)
    gpu.cuda.synchronize()
    grown.append_packed_device(packed[100:], stream=s3)
    grown.join_threshold_keys_device(float(ts[0]), 3000, keys_out=keys, offsets_out=offsets, stream=s1)
    gpu.cuda.synchronize()
    wk, wo = _expected(S, ts[0], 0, n, True)
    _same(keys, offsets, wk, wo, 3000, "append, then join")
    grown.dispose()


# ---- 9. host form ---------------------------------------------------------------------------------------------------------------
def test_host_form_equals_the_decoded_device_form(lb, gpu, oracle):
    import ctypes as C
    n = 300
    c, _, S = _case(lb, gpu, oracle, n)
    N = lb._native
    for t in (_selective(S), _median(S), np.float32(1.0)):
        for first, count in ((0, n), (17, 200)):
            wk, wo = _expected(S, t, first, count, True)
            total = len(wk)
            for capacity in (total + 5, max(1, total - 2)):
                keys, offsets = c.join_threshold_keys_device(float(t), capacity, first=first, count=count)
                d_rows, d_idx, d_sc, d_total = lb.decode_join_keys(keys, offsets, first)
                rows, idx, sc, h_total = c.join_threshold(float(t), capacity, first=first, count=count)
                assert h_total == d_total == total                       # never cut
                assert np.array_equal(rows, d_rows) and np.array_equal(idx, d_idx) and np.array_equal(sc.view(np.uint32), d_sc.view(np.uint32))
                rr, jj = np.nonzero((S[first:first + count] >= t) & ~np.eye(n, dtype=bool)[first:first + count])
                m = min(total, capacity)
                assert np.array_equal(rows, rr[:m] + first) and np.array_equal(idx, jj[:m])
                assert np.array_equal(sc.view(np.uint32), S[first:first + count][rr[:m], jj[:m]].view(np.uint32))
                # the raw call: the padding behind the pairs is -1 / -1 / 0
                o_rows, o_idx, o_sc, o_total = (N.SInt64 * capacity)(), (N.SInt64 * capacity)(), (N.Float32 * capacity)(), N.UInt64(0)
                assert lb.lib().LBAudioDetectiveCorpusJoinThreshold(c._ref, c._ref, first, count, 0, float(t), 1, capacity, o_rows, o_idx, o_sc,
                                                                   C.byref(o_total)) == 0
                assert o_total.value == total
                assert list(o_rows)[m:] == [-1] * (capacity - m) and list(o_idx)[m:] == [-1] * (capacity - m)
                assert list(o_sc)[m:] == [0.0] * (capacity - m) and list(o_rows)[:m] == rows.tolist()


# ---- 10. refusals that need a corpus ----------------------------------------------------------------------------------------------
def test_refusals_and_the_call_after_them(lb, gpu, oracle):
    n = 300
    c, bools, S = _case(lb, gpu, oracle, n)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    flat = bools.reshape(-1, L)
    ragged = lb.Corpus.ragged(L, n, n * 5)
    ragged.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, flat)).cuda(), np.full(n, 5, np.uint32))
    four = _uniform(lb, gpu, oracle, oracle.synth_corpus(77, 0, 50, 4, L))
    short = _uniform(lb, gpu, oracle, oracle.synth_corpus(77, 0, 50, 5, 64))
    nine = _uniform(lb, gpu, oracle, oracle.synth_corpus(77, 0, 50, 9, L))
    t = _selective(S)

    def refused(corpus, **kw):
        with pytest.raises(lb.LBAudioDetectiveError) as e:
            corpus.join_threshold_keys_device(float(t), 100, **kw)
        assert e.value.status == bad, kw
        with pytest.raises(lb.LBAudioDetectiveError) as e:
            corpus.join_threshold(float(t), 100, **{k: v for k, v in kw.items() if k != "index_base"})
        assert e.value.status == bad, kw
        _join_check(lb, gpu, c, S, t, 2000, ("after a refusal", kw))      # the next valid call is right

    refused(ragged)
    refused(c, queries=ragged)
    refused(ragged, queries=c)
    refused(c, queries=four)
    refused(four, queries=c)
    refused(short)
    refused(c, queries=short)
    refused(nine)
    refused(c, first=n - 3, count=4)
    refused(c, first=n, count=1)
    refused(c, queries=four, first=0, count=51)
    try:
        tiles = (n + TE - 1) // TE
        one_tile = 16 + TR * (584 + 8 * tiles) + 4 * tiles
        c.set_join_scratch_limit(one_tile - 1)
        with pytest.raises(lb.LBAudioDetectiveError) as e:
            c.join_threshold_keys_device(float(t), 100)
        assert e.value.status == bad
        c.set_join_scratch_limit(one_tile)
        _join_check(lb, gpu, c, S, t, 2000, "a limit of exactly one row tile")
    finally:
        c.set_join_scratch_limit(0)
    _join_check(lb, gpu, c, S, t, 2000, "the default limit again")
    with pytest.raises(lb.LBAudioDetectiveError):
        c.join_threshold_keys_device(float(t), 100, index_base=(1 << 32) - n + 1)
    # an empty scanned corpus: zero offsets and keys
    empty = lb.Corpus(L, 5, 10)
    keys, offsets = _buffers(gpu, 9, n)
    empty.join_threshold_keys_device(float(t), 9, queries=c, keys_out=keys, offsets_out=offsets)
    assert not keys.cpu().numpy().any() and not offsets.cpu().numpy().any()
    live = lb.debug_live_bytes()[0]
    for x in (ragged, four, short, nine, empty):
        x.dispose()
    assert lb.debug_live_bytes()[0] < live
