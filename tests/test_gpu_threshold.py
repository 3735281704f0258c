"""GPU tests of the threshold corpus queries (LBAudioDetectiveCorpusQueryThreshold and its batch / aligned / key / packed forms)
and of the selection on its own (LBAudioDetectiveThresholdKeysFromScoresDevice).  The expected lists come from the ORACLE's
per-entry scores: np.nonzero(scores >= float32(t)) in ascending index, cut at the capacity; the count is never cut.  Indices
are compared exactly, scores as float32 bits, counts exactly.  The thresholds are values of the oracle's own score array (its
maximum, its m-th largest, its median), so ties at the threshold exist by construction and nothing needs a tolerance."""
import os
import re

import numpy as np
import pytest

import align_ref

pytestmark = pytest.mark.gpu

CSEED = 0x4C424145
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -0x0123456789ABCDEF


def _tile():
    src = open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_threshold.hip")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+kThTile\s*=\s*(\d+)\s*;", src).group(1))


T = _tile()


# ---- the contract, restated ------------------------------------------------------------------------------------------------
def _matches(scores, t):
    with np.errstate(invalid="ignore"):
        return np.nonzero(np.asarray(scores, np.float32) >= np.float32(t))[0]


def _host_keys(scores, t, capacity, index_base=0):
    scores = np.asarray(scores, np.float32)
    at = _matches(scores, t)
    keys = ((scores[at].view(np.uint32).astype(np.uint64) << np.uint64(32)) |
            (np.uint64(0xFFFFFFFF) - (np.uint64(index_base) + at.astype(np.uint64)))).view(np.int64)[:capacity]
    return np.concatenate([keys, np.zeros(capacity - len(keys), np.int64)]), len(at)


def _same_list(got, scores, t, capacity, what=""):
    """a host form's (indices, scores, [lags,] count) against the oracle's scores"""
    at = _matches(scores, t)
    assert got[-1] == len(at), (what, got[-1], len(at))
    assert np.array_equal(got[0], at[:capacity]), (what, got[0][:8], at[:8])
    assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(scores, np.float32)[at[:capacity]].view(np.uint32)), what


def _packed(oracle, bools):
    return np.ascontiguousarray(oracle.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _uniform(lb, gpu, oracle, host):
    n, nsub, _ = host.shape
    c = lb.Corpus(host.shape[2], nsub, n)
    c.append_packed_device(gpu.from_numpy(_packed(oracle, host)).cuda())
    return c


def _ragged(lb, gpu, oracle, flat, counts):
    c = lb.Corpus.ragged(flat.shape[1], len(counts), int(counts.sum()))
    c.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, flat)).cuda(), counts)
    return c


def _oracle_scores(oracle, q, flat, counts, rg):
    return oracle.corpus_best_ragged(q, (flat, counts), rg if rg else q.shape[1], nthreads=16, want_scores=True)[2]


def _near(rng, base, flips):
    q = base.copy()
    for _ in range(flips):
        s, b = rng.integers(0, q.shape[0]), rng.integers(0, q.shape[1])
        q[s, b] ^= 1
    return q


def _thresholds(scores):
    """max, 4th largest, median of the oracle's scores, and a value above every score"""
    s = np.sort(np.asarray(scores, np.float32))
    return [s[-1], s[-4], s[len(s) // 2], np.nextafter(s[-1], np.float32(np.inf), dtype=np.float32)]


# ---- the selection alone, on crafted arrays ----------------------------------------------------------------------------------
def _select_check(lb, gpu, d_scores, scores, t, capacity, index_base, what):
    rows = scores.shape[0]
    keys = gpu.full((rows, capacity), POISON, dtype=gpu.int64, device="cuda")
    counts = gpu.full((rows,), POISON, dtype=gpu.int64, device="cuda")
    lb.threshold_keys_from_scores_device(d_scores, float(t), capacity, index_base, keys_out=keys, counts_out=counts)
    keys, counts = keys.cpu().numpy(), counts.cpu().numpy()
    for r in range(rows):
        want, n = _host_keys(scores[r], t, capacity, index_base)
        assert counts[r] == n, (what, r, counts[r], n)
        bad = np.nonzero(keys[r] != want)[0]
        assert len(bad) == 0, (what, r, len(bad), bad[:4], keys[r][bad[:4]], want[bad[:4]])


def _random_rows(rng, rows, n):
    """rows whose densities of matches at t = 0.7 differ: 1e-4, 0.5, 0.99, ..."""
    out = np.empty((rows, n), np.float32)
    for r in range(rows):
        dens = (1e-4, 0.5, 0.99)[r % 3]
        hit = rng.random(n) < dens
        out[r] = np.where(hit, 0.75 + 0.25 * rng.random(n), 0.65 * rng.random(n)).astype(np.float32)
    return out


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, T - 1, T, T + 1, 3 * T + 5])
def test_selection_sizes_rows_capacities_and_bases(lb, gpu, n):
    rng = np.random.default_rng(n)
    t = np.float32(0.7)
    for rows in (1, 3, 8, 9):                              # 9 crosses the group of eight; n % 4 != 0 misaligns rows 1, 2, ...
        scores = _random_rows(rng, rows, n)
        d = gpu.from_numpy(scores).cuda()
        most = max(1, max(len(_matches(scores[r], t)) for r in range(rows)))
        for capacity in sorted({1, max(1, most - 1), most, most + 7}):
            for base in (0, 12345, (1 << 32) - n):
                _select_check(lb, gpu, d, scores, t, capacity, base, (n, rows, capacity, base))


def test_selection_patterns_and_special_values(lb, gpu):
    rng = np.random.default_rng(77)
    t = np.float32(0.7)
    below, above = np.nextafter(t, np.float32(0), dtype=np.float32), np.nextafter(t, np.float32(1), dtype=np.float32)
    for n in (3 * T + 5, 2 * T + 2, T + 3):                # all with n % 4 != 0: rows 1.. start off a 16-byte boundary
        pats = {}
        pats["none"] = np.full(n, 0.5, np.float32)
        pats["all"] = np.full(n, 0.9, np.float32)
        x = np.full(n, 0.5, np.float32); x[0] = 0.8; pats["only the first"] = x
        x = np.full(n, 0.5, np.float32); x[n - 1] = 0.8; pats["only the last"] = x
        x = np.full(n, 0.5, np.float32); x[0::T] = 0.8; x[T - 1::T] = 0.75; pats["first and last of every tile"] = x
        x = np.full(n, 0.5, np.float32); x[T + 1024:T + 1024 + 256] = 0.8; pats["one wave, every component"] = x
        x = np.full(n, 0.5, np.float32); x[T + 512:T + 512 + 256:4] = 0.8; pats["one wave, one component"] = x
        x = np.full(n, 0.5, np.float32)
        x[5], x[6], x[7], x[8], x[9], x[10], x[11], x[12] = np.inf, np.nan, -0.0, -3.0, t, below, above, -np.inf
        x[n - 3], x[n - 2], x[n - 1] = np.nan, t, below
        x[T - 1], x[T], x[T + 1] = t, np.nan, above
        pats["special values"] = x
        for name, row in pats.items():
            # the pattern in every row of three (rows 1 and 2 misaligned), rolled so that the rows differ
            scores = np.stack([row, np.roll(row, 1), np.roll(row, -2)])
            d = gpu.from_numpy(scores).cuda()
            most = max(1, len(_matches(row, t)))
            for capacity in sorted({1, max(1, most - 1), most, most + 7}):
                _select_check(lb, gpu, d, scores, t, capacity, 12345, (name, n, capacity))
        # a view that starts 4, 8 and 12 bytes behind an aligned address
        flat = rng.random(n + 3).astype(np.float32)
        d = gpu.from_numpy(flat).cuda()
        for shift in (1, 2, 3):
            _select_check(lb, gpu, d[shift:shift + n - 1].view(1, -1), flat[None, shift:shift + n - 1], t, n, 0, ("shifted", shift))


def test_selection_more_tiles_than_one_chunk_and_one_grid(lb, gpu):
    """1030 tiles a row: the offsets kernel's chunk loop carries, and three rows are more work items than the count and
    scatter launches have workgroups"""
    rng = np.random.default_rng(78)
    n = 1030 * T + 7
    scores = _random_rows(rng, 3, n)
    scores[1, -1] = 0.9
    d = gpu.from_numpy(scores).cuda()
    most = max(len(_matches(scores[r], np.float32(0.7))) for r in range(3))
    for capacity, base in ((most + 7, 0), (most - 1, (1 << 32) - n), (1000, 12345)):
        _select_check(lb, gpu, d, scores, np.float32(0.7), capacity, base, ("many tiles", capacity))


def test_selection_index_base_overflow_and_argument_checks(lb, gpu):
    d = gpu.zeros((2, 100), dtype=gpu.float32, device="cuda")
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(lb.LBAudioDetectiveError):
            lb.threshold_keys_from_scores_device(d, t, 4)
    with pytest.raises(lb.LBAudioDetectiveError):
        lb.threshold_keys_from_scores_device(d, 0.7, 4, index_base=(1 << 32) - 99)
    keys = gpu.zeros(4, dtype=gpu.int64, device="cuda")
    with pytest.raises(lb.LBAudioDetectiveError):
        lb.threshold_keys_from_scores_device(d, 0.7, 0, keys_out=keys, counts_out=keys)          # capacity 0
    # t > 1 is legal and matches nothing
    k, c = lb.threshold_keys_from_scores_device(d + 1.0, 1.5, 4)
    assert not k.cpu().numpy().any() and not c.cpu().numpy().any()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
class _Case:
    """a corpus on the device, its entries on the host, queries and the oracle's scores of each (query, range), computed once"""

    def __init__(self, lb, gpu, oracle, corpus, flat, counts, queries, ranges=(0, 120)):
        self.corpus, self.flat, self.counts, self.queries = corpus, flat, counts, queries
        self.off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.fps = [lb.Fingerprint.from_bools(q) for q in queries]
        self.scores = {(i, rg): _oracle_scores(oracle, q, flat, counts, rg) for i, q in enumerate(queries) for rg in ranges}

    def entry(self, e):
        return self.flat[self.off[e]:self.off[e + 1]]


@pytest.fixture(scope="module")
def planted(lb, gpu, oracle):
    """20 000 entries of 5 x 200 (the specialised shape): the query is a 30-flip near copy of entry 123 and is itself the last
    entry; two more entries are exact copies of entry 123"""
    rng = np.random.default_rng(41)
    n = 20000
    host = oracle.synth_corpus(CSEED, 0, n, 5, 200)
    q = _near(rng, host[123], 30)
    host[7000] = host[123]
    host[15001] = host[123]
    host[n - 1] = q
    return _Case(lb, gpu, oracle, _uniform(lb, gpu, oracle, host), host.reshape(-1, 200), np.full(n, 5, np.uint32), [q])


@pytest.fixture(scope="module")
def generic(lb, gpu, oracle):
    """a uniform corpus of a shape without the specialised scan: 3 x 199"""
    rng = np.random.default_rng(42)
    n = 3001
    host = rng.integers(0, 2, (n, 3, 199), dtype=np.uint8)
    host[rng.integers(0, 100, host.shape, dtype=np.uint8) < 3] = 0
    host[2000] = host[17]
    qs = [_near(rng, host[17], 9), host[2999][:2].copy(), _near(rng, host[5], 3)]
    return _Case(lb, gpu, oracle, _uniform(lb, gpu, oracle, host), host.reshape(-1, 199), np.full(n, 3, np.uint32), qs)


@pytest.fixture(scope="module")
def ragged(lb, gpu, oracle):
    """about 3 000 entries of 1 .. 40 sub-fingerprints; queries of 5, 12, 21 and 60: the systolic scans, the task scan and the
    side of entries not longer than the query all run"""
    rng = np.random.default_rng(43)
    counts = rng.integers(1, 41, 3003).astype(np.uint32)
    flat = oracle.synth_ragged_entries(CSEED, 0, counts, 200)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    qs = []
    for nq in (5, 12, 21):
        e = int(np.nonzero(counts >= nq + 3)[0][nq])
        qs.append(_near(rng, flat[off[e] + 2:off[e] + 2 + nq], 6))
    e = int(np.argmax(counts))
    long_q = (rng.random((60, 200)) < 0.5).astype(np.uint8)
    long_q[11:11 + counts[e]] = flat[off[e]:off[e + 1]]
    qs.append(long_q)
    return _Case(lb, gpu, oracle, _ragged(lb, gpu, oracle, flat, counts), flat, counts, qs)


def _end_to_end(case, what):
    for (i, rg), scores in case.scores.items():
        for t in _thresholds(scores):
            count = len(_matches(scores, t))
            for capacity in sorted({count + 3, max(1, count - 1), 1}):
                got = case.corpus.query_threshold(case.fps[i], float(t), capacity, rg)
                _same_list(got, scores, t, capacity, (what, i, rg, float(t), capacity))


def test_planted_uniform_corpus(lb, planted):
    scores = planted.scores[(0, 0)]
    assert _matches(scores, 0.6).tolist() == [123, 7000, 15001, 19999]            # the four planted entries and nothing else
    assert len({scores[123].tobytes(), scores[7000].tobytes(), scores[15001].tobytes()}) == 1 and scores[19999] == 1.0
    assert len(_matches(scores, np.sort(scores)[len(scores) // 2])) >= len(scores) // 2
    for variant in (0, 1):
        planted.corpus.set_kernel_variant(variant)
        _end_to_end(planted, ("planted", variant))
        idx, sc, n = planted.corpus.query_threshold(planted.fps[0], 0.6, 16)
        assert idx.tolist() == [123, 7000, 15001, 19999] and n == 4
    planted.corpus.set_kernel_variant(0)


def test_generic_uniform_corpus(lb, generic):
    _end_to_end(generic, "generic")


def test_ragged_corpus(lb, ragged):
    _end_to_end(ragged, "ragged")


# ---- equivalences ------------------------------------------------------------------------------------------------------------
def _keys_device(case, ids, t, capacity, rg=0, base=0):
    keys, counts = case.corpus.query_batch_threshold_keys_device([case.fps[i] for i in ids], float(t), capacity, range_=rg, index_base=base)
    return keys.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("which", ["planted", "generic", "ragged"])
def test_batches_equal_single_calls(request, which):
    case = request.getfixturevalue(which)
    nq = len(case.queries)
    t = np.float32(0.53)
    singles = {i: _keys_device(case, [i], t, 300) for i in range(nq)}
    for i in range(nq):                                    # ... and the single calls are the oracle's lists
        want, n = _host_keys(case.scores[(i, 0)], t, 300)
        assert singles[i][1][0] == n and np.array_equal(singles[i][0][0], want), (which, i)
    for nb in (1, 8, 11):                                  # mixed lengths where the case has them; 11 crosses the group of eight
        ids = [(3 * j + nb) % nq for j in range(nb)]
        keys, counts = _keys_device(case, ids, t, 300)
        for row, i in enumerate(ids):
            assert counts[row] == singles[i][1][0] and np.array_equal(keys[row], singles[i][0][0]), (which, nb, row)
        host = case.corpus.query_threshold_batch([case.fps[i] for i in ids], float(t), 300)
        for row, i in enumerate(ids):
            _same_list(host[row], case.scores[(i, 0)], t, 300, (which, nb, row))


@pytest.mark.parametrize("which", ["planted", "generic", "ragged"])
def test_packed_form_and_lags(lb, gpu, oracle, request, which):
    """the packed-device form equals the handle KeysDevice form bit for bit (keys, counts), its lags equal
    LBAudioDetectiveCorpusAlignKeysDevice's on those keys, the host Aligned form's and tests/align_ref.py's"""
    case = request.getfixturevalue(which)
    for i, q in enumerate(case.queries):
        scores = case.scores[(i, 120)]
        for t, capacity in ((np.sort(scores)[-6], 16), (np.sort(scores)[-40], 25), (np.float32(2.0), 4)):
            d_rows = gpu.from_numpy(_packed(oracle, q[None])).cuda()
            pk, pc, pl = case.corpus.query_packed_threshold_keys_device(d_rows, 1, q.shape[0], float(t), capacity, aligned=True, range_=120,
                                                                        index_base=1000)
            hk, hc = case.corpus.query_batch_threshold_keys_device([case.fps[i]], float(t), capacity, range_=120, index_base=1000)
            assert gpu.equal(pk, hk) and gpu.equal(pc, hc), (which, i, capacity)
            want, n = _host_keys(scores, t, capacity, 1000)
            assert int(hc[0]) == n and np.array_equal(hk[0].cpu().numpy(), want)
            lags = case.corpus.align_keys_device([case.fps[i]], hk, capacity, index_base=1000, range_=120)
            assert gpu.equal(pl, lags), (which, i, capacity)
            # without lags the packed form writes the same keys
            pk2, pc2 = case.corpus.query_packed_threshold_keys_device(d_rows, 1, q.shape[0], float(t), capacity, range_=120, index_base=1000)
            assert gpu.equal(pk2, hk) and gpu.equal(pc2, hc)
            idx, sc, lag, cnt = case.corpus.query_threshold(case.fps[i], float(t), capacity, 120, aligned=True)
            _same_list((idx, sc, cnt), scores, t, capacity, (which, i))
            m = min(n, capacity)
            assert np.array_equal(lag, pl[0, :m].cpu().numpy()) and not pl[0, m:].cpu().numpy().any()
            for e, s, lg in zip(idx, sc, lag):
                ws, wl = align_ref.align(q, case.entry(int(e)), 120)
                assert (np.float32(s).view(np.uint32), int(lg)) == (np.float32(ws).view(np.uint32), wl), (which, i, int(e))


@pytest.mark.parametrize("which", ["planted", "ragged"])
def test_sorted_threshold_keys_are_the_head_of_topk(lb, gpu, request, which):
    case = request.getfixturevalue(which)
    k = 1024
    for i in range(len(case.queries)):
        s = np.sort(case.scores[(i, 0)])
        topk = gpu.zeros((1, k), dtype=gpu.int64, device="cuda")
        case.corpus.query_batch_topk_keys_device([case.fps[i]], k, topk)
        topk = topk.cpu().numpy()[0]
        for t in (s[-1], s[-4], s[-30]):
            keys, counts = _keys_device(case, [i], t, k)
            n = int(counts[0])
            assert 1 <= n <= k
            assert np.array_equal(np.sort(keys[0][:n])[::-1], topk[:n]), (which, i, n)


# ---- state shared with the other queries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["planted", "ragged"])
def test_other_queries_are_unchanged_around_a_threshold_call(lb, gpu, request, which):
    case = request.getfixturevalue(which)
    c, fps = case.corpus, case.fps

    def others():
        return ([c.query(f) for f in fps], [tuple(x.tolist() for x in c.query_topk(f, 10)) for f in fps],
                [c.query_aligned(f) for f in fps], [tuple(x.tolist() for x in c.query_topk_aligned(f, 5)) for f in fps])
    before = others()
    for i in range(len(fps)):
        t = np.sort(case.scores[(i, 0)])[-10]
        _same_list(c.query_threshold(fps[i], float(t), 20), case.scores[(i, 0)], t, 20, which)
        g = c.query_threshold(fps[i], float(t), 20, aligned=True)
        _same_list((g[0], g[1], g[3]), case.scores[(i, 0)], t, 20, which)
    assert others() == before
    # capacity grown between calls
    t = np.sort(case.scores[(0, 0)])[len(case.scores[(0, 0)]) // 2]
    for capacity in (5, 300, 40000):
        _same_list(c.query_threshold(fps[0], float(t), capacity), case.scores[(0, 0)], t, capacity, (which, capacity))
    # two calls on two streams, back to back: the second one waits for the scratch
    s1, s2 = gpu.cuda.Stream(), gpu.cuda.Stream()
    ta, tb = np.sort(case.scores[(0, 0)])[-3], np.sort(case.scores[(len(fps) - 1, 0)])[-200]
    ka, ca = (gpu.full((1, 256), POISON, dtype=gpu.int64, device="cuda"), gpu.full((1,), POISON, dtype=gpu.int64, device="cuda"))
    kb, cb = gpu.full((1, 256), POISON, dtype=gpu.int64, device="cuda"), gpu.full((1,), POISON, dtype=gpu.int64, device="cuda")
    gpu.cuda.synchronize()
    c.query_batch_threshold_keys_device([fps[0]], float(ta), 256, ka, ca, stream=s1)
    c.query_batch_threshold_keys_device([fps[-1]], float(tb), 256, kb, cb, stream=s2)
    gpu.cuda.synchronize()
    for (k, n), i, t in (((ka, ca), 0, ta), ((kb, cb), len(fps) - 1, tb)):
        want, cnt = _host_keys(case.scores[(i, 0)], t, 256)
        assert int(n[0]) == cnt and np.array_equal(k[0].cpu().numpy(), want), (which, i)
    assert others() == before


def test_dispose_releases_the_threshold_scratch(lb, gpu, oracle):
    host = oracle.synth_corpus(CSEED, 0, 3000, 5, 200)
    fq = lb.Fingerprint.from_bools(host[5])
    warm = _uniform(lb, gpu, oracle, host[:10])            # (whatever the library sets up once per process)
    warm.query_threshold(fq, 0.6, 4, aligned=True)
    d_rows = gpu.from_numpy(_packed(oracle, host[5][None])).cuda()
    warm.query_packed_threshold_keys_device(d_rows, 1, 5, 0.6, 4, aligned=True)
    gpu.cuda.synchronize()
    warm.dispose()
    first = lb.debug_live_bytes()
    c = _uniform(lb, gpu, oracle, host)
    made = lb.debug_live_bytes()
    idx, sc, lag, n = c.query_threshold(fq, 0.6, 4, aligned=True)
    assert idx.tolist() == [5] and sc.tolist() == [1.0] and lag.tolist() == [0] and n == 1
    c.query_packed_threshold_keys_device(d_rows, 1, 5, 0.6, 4, aligned=True)
    gpu.cuda.synchronize()
    assert lb.debug_live_bytes()[0] > made[0]              # the score row, the tile counts, the key block
    c.dispose()
    assert lb.debug_live_bytes() == first


# ---- shards ----------------------------------------------------------------------------------------------------------------------
def test_two_shards_in_one_process(lb, gpu, oracle, planted):
    n = 20000
    host = planted.flat.reshape(n, 5, 200)
    cut = 9000
    halves = [_uniform(lb, gpu, oracle, host[:cut]), _uniform(lb, gpu, oracle, host[cut:])]
    scores = planted.scores[(0, 0)]
    s = np.sort(scores)
    for t in (np.float32(0.6), s[-1], s[len(s) // 2]):
        total = len(_matches(scores, t))
        in_first = len(_matches(scores[:cut], t))
        for capacity in sorted({total + 5, max(1, in_first + (total - in_first) // 2), max(1, in_first - 1), 1}):   # a cut inside shard 1, inside shard 0
            gk = gpu.zeros((2, 1, capacity), dtype=gpu.int64, device="cuda")
            gc = gpu.zeros((2, 1), dtype=gpu.int64, device="cuda")
            for r, (c, base) in enumerate(zip(halves, (0, cut))):
                c.query_batch_threshold_keys_device([planted.fps[0]], float(t), capacity, gk[r], gc[r], index_base=base)
            merged, totals = lb.merge_threshold_keys(gk, gc, capacity)
            wk, wc = _keys_device(planted, [0], t, capacity)
            assert np.array_equal(merged.cpu().numpy(), wk) and totals.cpu().numpy().tolist() == wc.tolist() == [total], (float(t), capacity)
    assert lb.decode_threshold_keys(merged[0], totals[0])[0].tolist() == _matches(scores, t)[:capacity].tolist()


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def test_argument_checks_and_the_empty_corpus(lb, gpu, oracle, planted):
    c, fq = planted.corpus, planted.fps[0]
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(lb.LBAudioDetectiveError):
            c.query_threshold(fq, t, 4)
        with pytest.raises(lb.LBAudioDetectiveError):
            c.query_threshold(fq, t, 4, aligned=True)
        with pytest.raises(lb.LBAudioDetectiveError):
            c.query_batch_threshold_keys_device([fq], t, 4)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    N, L = lb._native, lb.lib()
    one = (N.Ref * 1)(fq._ref)
    three = (N.Ref * 3)(fq._ref, fq._ref, fq._ref)
    d = gpu.zeros(64, dtype=gpu.int64, device="cuda")
    p, pc = d.data_ptr(), d.data_ptr() + 256
    assert L.LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice(c._ref, one, 1, 0, 0.7, 0, 0, p, p, None) == bad           # capacity 0
    assert L.LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice(c._ref, three, 3, 0, 0.7, 1 << 30, 0, p, p, None) == bad    # 3 x 2^30 slots
    assert L.LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice(c._ref, one, 1, 0, 0.7, 4, (1 << 32) - len(c) + 1, p, p, None) == bad
    assert L.LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice(None, one, 1, 0, 0.7, 4, 0, p, p, None) == bad
    assert L.LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice(c._ref, p, 1, 5, 0, 0.7, 4, (1 << 32) - len(c) + 1, p, p, None, None) == bad
    assert L.LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice(c._ref, one, 1, 0, 0.7, 4, (1 << 32) - len(c), p, pc, None) == 0
    gpu.cuda.synchronize()
    short = lb.Fingerprint.from_bools(planted.queries[0][:, :100])
    with pytest.raises(lb.LBAudioDetectiveError):
        c.query_threshold(short, 0.7, 4)
    # t > 1 is legal and matches nothing
    idx, sc, n = c.query_threshold(fq, 1.5, 4)
    assert len(idx) == 0 and len(sc) == 0 and n == 0
    # an empty corpus: counts 0, keys 0, lags 0
    for empty in (lb.Corpus(200, 5, 10), lb.Corpus.ragged(200, 10, 100)):
        assert empty.query_threshold(fq, 0.7, 4, aligned=True)[-1] == 0
        keys, counts = empty.query_batch_threshold_keys_device([fq, fq], 0.7, 4, gpu.full((2, 4), POISON, dtype=gpu.int64, device="cuda"),
                                                               gpu.full((2,), POISON, dtype=gpu.int64, device="cuda"))
        assert not keys.cpu().numpy().any() and not counts.cpu().numpy().any()
        d_rows = gpu.from_numpy(_packed(oracle, planted.queries[0][None])).cuda()
        keys, counts, lags = empty.query_packed_threshold_keys_device(
            d_rows, 1, 5, 0.7, 4, gpu.full((1, 4), POISON, dtype=gpu.int64, device="cuda"), gpu.full((1,), POISON, dtype=gpu.int64, device="cuda"),
            gpu.full((1, 4), 77, dtype=gpu.int32, device="cuda"))
        assert not keys.cpu().numpy().any() and not counts.cpu().numpy().any() and not lags.cpu().numpy().any()
        empty.dispose()
