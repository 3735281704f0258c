"""GPU tests of the alignment feature (LBAudioDetectiveCorpusQueryAligned, ...QueryBatchTopKAligned, ...AlignKeysDevice,
...MatchProfile).  Expected lags and scores come from the numpy restatement in tests/align_ref.py, whose score is first pinned to
the oracle's compare (oracle.corpus_best_ragged's per-entry scores) bit for bit for every pair checked.  Lags are compared
exactly, scores as float32 bits; indices, scores and counts also against the existing non-aligned calls."""
import ctypes as C

import numpy as np
import pytest

import align_ref

pytestmark = pytest.mark.gpu

SEED = 0x4C424147


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _packed(oracle, bools):
    return np.ascontiguousarray(oracle.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _ragged(lb, gpu, oracle, entries):
    counts = np.array([e.shape[0] for e in entries], np.uint32)
    flat = np.concatenate(entries, axis=0)
    c = lb.Corpus.ragged(flat.shape[1], len(entries), int(counts.sum()))
    c.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, flat)).cuda(), counts)
    return c


def _uniform(lb, gpu, oracle, host):
    c = lb.Corpus(host.shape[2], host.shape[1], host.shape[0])
    c.append_packed_device(gpu.from_numpy(_packed(oracle, host)).cuda())
    return c


class Expected:
    """Restated (score, lag) per (query, entry), each score pinned to the oracle's per-entry score before it is used."""

    def __init__(self, oracle, entries, L):
        self.oracle, self.entries, self.L = oracle, entries, L
        self.cache = {}

    def of(self, qi, q, rg):
        key = (qi, rg)
        if key not in self.cache:
            r = rg if rg else self.L
            _, _, want = self.oracle.corpus_best_ragged(q, self.entries, r, nthreads=16, want_scores=True)
            got = [align_ref.align(q, e, rg) for e in self.entries]
            scores = np.array([s for s, _ in got], np.float32)
            assert np.array_equal(_bits(scores), _bits(want)), "the restatement disagrees with the oracle"
            self.cache[key] = (scores, np.array([lag for _, lag in got], np.int32))
        return self.cache[key]


def _keys_of(scores, base):
    """A key for every entry (score > 0 or not), in entry order."""
    idx = np.arange(len(scores), dtype=np.int64) + base
    return (_bits(scores).astype(np.int64) << 32) | (0xFFFFFFFF - idx)


def _check_lists(got, want_scores, want_lags, what):
    for qi, (idx, sc, lag) in enumerate(got):
        assert np.array_equal(_bits(sc), _bits(want_scores[qi][idx])), (what, qi)
        assert np.array_equal(lag, want_lags[qi][idx]), (what, qi, idx[:8], lag[:8], want_lags[qi][idx][:8])


def _ragged_entries(rng, L, long_ones):
    lens = list(rng.integers(1, 301, 28)) + [1, 2, 5, 21, 48, 100] + [5000] * long_ones
    entries = [(rng.random((int(n), L)) < 0.5).astype(np.uint8) for n in lens]
    entries += [np.zeros((7, L), np.uint8), np.zeros((60, L), np.uint8)]          # all-zero entries: every ratio is 0
    return entries


@pytest.mark.parametrize("L", [200, 199, 57])
def test_ragged_every_pair(lb, gpu, oracle, L):
    """Every entry of a ragged corpus (shorter than, equal to and longer than the query, all-zero ones, two of 5000 at L = 200)
    against queries of 1, 2, 5, 21, 48, 100 and 600 and every range: align_keys_device on a key per entry (index base 1000,
    zero padding, a key outside the corpus) and query_batch_topk_aligned against query_batch_topk."""
    rng = np.random.default_rng(L)
    entries = _ragged_entries(rng, L, 2 if L == 200 else 0)
    c = _ragged(lb, gpu, oracle, entries)
    exp = Expected(oracle, entries, L)
    qs = []
    for nq in (1, 2, 5, 21, 48, 100, 600):
        src = next((e for e in entries if e.shape[0] >= nq + 3), None)
        q = src[3:3 + nq].copy() if src is not None and nq < 100 else (rng.random((nq, L)) < 0.5).astype(np.uint8)
        q[:, ::17] ^= 1
        qs.append(q)
    fps = [lb.Fingerprint.from_bools(q) for q in qs]
    n, base, K = len(entries), 1000, len(entries) + 3
    for rg in (0, 1, 2, 119, 120, L) if L == 200 else (0, 1, 119, L):
        # (the restatement of the two longest queries is the slow part: they take two of the ranges)
        sel = [i for i in range(len(qs)) if qs[i].shape[0] < 100 or rg in (0, 119)]
        qs_r, fps_r = [qs[i] for i in sel], [fps[i] for i in sel]
        want = [exp.of(i, qs[i], rg) for i in sel]
        keys = np.zeros((len(qs_r), K), np.int64)
        for i in range(len(qs_r)):
            keys[i, :n] = _keys_of(want[i][0], base)
            keys[i, n + 1] = (1 << 32) | (0xFFFFFFFF - (base + n))      # one past the corpus: lag 0, score 0
        lags, scores = c.align_keys_device(fps_r, gpu.from_numpy(keys).cuda(), K, index_base=base, want_scores=True, range_=rg)
        lags, scores = lags.cpu().numpy(), scores.cpu().numpy()
        for i in range(len(qs_r)):
            assert np.array_equal(lags[i, :n], want[i][1]), (rg, i, np.flatnonzero(lags[i, :n] != want[i][1])[:8])
            assert np.array_equal(_bits(scores[i, :n]), _bits(want[i][0])), (rg, i)
            assert not lags[i, n:].any() and not scores[i, n:].any()
        got = c.query_batch_topk_aligned(fps_r, 16, rg)
        plain = c.query_batch_topk(fps_r, 16, rg)
        for (gi, gs, _), (pi, ps) in zip(got, plain):
            assert np.array_equal(gi, pi) and np.array_equal(_bits(gs), _bits(ps))
        _check_lists(got, [w[0] for w in want], [w[1] for w in want], ("ragged", L, rg))


def test_planted_matches_and_ties(lb, gpu, oracle):
    rng = np.random.default_rng(7)
    L = 200
    q = (rng.random((21, L)) < 0.5).astype(np.uint8)
    noisy = q.copy()
    noisy[::3, 5] ^= 1
    e_a = (rng.random((300, L)) < 0.5).astype(np.uint8)
    e_a[137:158] = noisy                                   # case A: lag +137
    e_b = q[4:13].copy()                                   # case B: the entry lies inside the query at 4 -> lag -4
    e_b[2, 9] ^= 1
    e_t = (rng.random((90, L)) < 0.5).astype(np.uint8)
    e_t[11:32] = q                                         # two identical plants: the lower offset wins
    e_t[60:81] = q
    filler = [(rng.random((int(m), L)) < 0.5).astype(np.uint8) for m in rng.integers(1, 80, 40)]
    entries = filler[:10] + [e_a] + filler[10:20] + [e_b] + filler[20:] + [e_t]
    ia, ib, it = 10, 21, len(entries) - 1
    c = _ragged(lb, gpu, oracle, entries)
    fq = lb.Fingerprint.from_bools(q)
    assert align_ref.align(q, e_a, 0)[1] == 137 and align_ref.align(q, e_b, 0)[1] == -4 and align_ref.align(q, e_t, 0)[1] == 11
    want_scores, want_lags = Expected(oracle, entries, L).of(0, q, 0)
    got = c.query_topk_aligned(fq, len(entries))
    _check_lists([got], [want_scores], [want_lags], "planted")
    lag_of = dict(zip(got[0].tolist(), got[2].tolist()))
    assert lag_of[ia] == 137 and lag_of[ib] == -4 and lag_of[it] == 11
    assert c.query_aligned(fq) == (it, 1.0, 11)
    for e, want in ((ia, 137), (ib, -4), (it, 11)):
        prof, first = c.match_profile(fq, e)
        assert first == 0 and int(np.argmax(prof)) == abs(want)


def test_uniform_every_nsub(lb, gpu, oracle):
    """NSUB 1..8 at L = 200: query lengths equal to (the specialised scans), shorter and longer than NSUB (the generic scan)."""
    rng = np.random.default_rng(11)
    for nsub in range(1, 9):
        n = 400
        host = (rng.random((n, nsub, 200)) < 0.5).astype(np.uint8)
        host[17] = 0
        c = _uniform(lb, gpu, oracle, host)
        entries = list(host)
        exp = Expected(oracle, entries, 200)
        lens = sorted({nsub, max(1, nsub - 1), nsub + 3, 1})
        qs = []
        for nq in lens:
            q = (rng.random((nq, 200)) < 0.5).astype(np.uint8)
            m = min(nq, nsub)
            q[:m] = host[123 + nq, :m]
            qs.append(q)
        fps = [lb.Fingerprint.from_bools(q) for q in qs]
        for rg in (0, 119):
            want = [exp.of(i, q, rg) for i, q in enumerate(qs)]
            keys = np.stack([_keys_of(w[0], 5) for w in want])
            lags, scores = c.align_keys_device(fps, gpu.from_numpy(keys).cuda(), n, index_base=5, want_scores=True, range_=rg)
            for i in range(len(qs)):
                assert np.array_equal(lags.cpu().numpy()[i], want[i][1]), (nsub, rg, lens[i])
                assert np.array_equal(_bits(scores.cpu().numpy()[i]), _bits(want[i][0])), (nsub, rg, lens[i])
            got = c.query_batch_topk_aligned(fps, 10, rg)
            plain = c.query_batch_topk(fps, 10, rg)
            for (gi, gs, _), (pi, ps) in zip(got, plain):
                assert np.array_equal(gi, pi) and np.array_equal(_bits(gs), _bits(ps))
            _check_lists(got, [w[0] for w in want], [w[1] for w in want], ("uniform", nsub, rg))
            for i, fq in enumerate(fps):
                qi, qsc = c.query(fq, rg)
                ai, asc, alag = c.query_aligned(fq, rg)
                assert (ai, _bits(asc)) == (qi, _bits(qsc)), (nsub, lens[i])
                assert alag == (want[i][1][qi] if qi >= 0 else 0)
        c.set_kernel_variant(1)                            # the generic kernel for the equal-length query too
        i = lens.index(nsub)
        assert c.query_aligned(fps[i])[:2] == c.query(fps[i])
        c.set_kernel_variant(0)


def test_topk_aligned_batches(lb, gpu, oracle):
    """K in {1, 10, 1024}, batches of 1..17 queries (across kQueryBatchMax = 8): indices, scores and counts are
    query_batch_topk's; K = 1 is query_aligned's answer; lags are the restatement's."""
    rng = np.random.default_rng(13)
    L = 200
    entries = [(rng.random((int(m), L)) < 0.5).astype(np.uint8) for m in rng.integers(20, 71, 1500)]
    c = _ragged(lb, gpu, oracle, entries)
    qs = []
    for i in range(17):
        src = entries[(i * 89) % len(entries)]
        q = src[i % 5:i % 5 + 21].copy() if src.shape[0] >= 26 else (rng.random((21, L)) < 0.5).astype(np.uint8)
        q[:, ::(7 + i)] ^= 1
        qs.append(q)
    fps = [lb.Fingerprint.from_bools(q) for q in qs]
    lag_cache = {}

    def lag(qi, e):
        if (qi, e) not in lag_cache:
            lag_cache[(qi, e)] = align_ref.align(qs[qi], entries[e], 0)
        return lag_cache[(qi, e)]

    scores = [oracle.corpus_best_ragged(q, entries, L, nthreads=16, want_scores=True)[2] for q in qs]
    for k in (1, 10, 1024):
        for nb in (1, 8, 9, 17):
            got = c.query_batch_topk_aligned(fps[:nb], k)
            plain = c.query_batch_topk(fps[:nb], k)
            for qi, ((gi, gs, gl), (pi, ps)) in enumerate(zip(got, plain)):
                assert np.array_equal(gi, pi) and np.array_equal(_bits(gs), _bits(ps)) and len(gl) == len(gi)
                check = gi if k < 1024 else gi[::37]
                for j, e in enumerate(gi):
                    if e in check:
                        s, want_lag = lag(qi, int(e))
                        assert _bits(s) == _bits(scores[qi][e]) and gl[j] == want_lag, (k, nb, qi, e)
            if k == 1:
                for qi in range(nb):
                    ai, asc, alag = c.query_aligned(fps[qi])
                    gi, gs, gl = got[qi]
                    assert (ai, _bits(asc), alag) == (int(gi[0]), _bits(gs[0]), int(gl[0]))


def test_query_aligned_with_and_without_pruning(lb, gpu, oracle):
    rng = np.random.default_rng(17)
    entries = [(rng.random((int(m), 200)) < 0.5).astype(np.uint8) for m in rng.integers(1, 120, 3000)]
    c = _ragged(lb, gpu, oracle, entries)
    for nq, src in ((5, 100), (21, 2000), (48, 2500), (130, None)):
        if src is not None and entries[src].shape[0] >= nq + 2:
            q = entries[src][1:1 + nq].copy()
        else:
            q = (rng.random((nq, 200)) < 0.5).astype(np.uint8)
            j = next(j for j in range(77, len(entries)) if entries[j].shape[0] <= nq - 5)
            q[5:5 + entries[j].shape[0]] = entries[j]              # an entry inside the query: case B
        q[:, 3] ^= 1
        fq = lb.Fingerprint.from_bools(q)
        for prune in (True, False):
            c.set_bound_pruning(prune)
            qi, qsc = c.query(fq)
            ai, asc, alag = c.query_aligned(fq)
            assert (ai, _bits(asc)) == (qi, _bits(qsc)), (nq, prune)
            s, want_lag = align_ref.align(q, entries[qi], 0)
            assert _bits(s) == _bits(np.float32(oracle.compare_fp(q, entries[qi], 200, 200)))
            assert _bits(s) == _bits(asc) and alag == want_lag, (nq, prune)


def test_match_profile(lb, gpu, oracle):
    rng = np.random.default_rng(19)
    entries = [(rng.random((int(m), 199)) < 0.5).astype(np.uint8) for m in (1, 7, 30, 300, 30)]
    c = _ragged(lb, gpu, oracle, entries)
    q = (rng.random((30, 199)) < 0.5).astype(np.uint8)
    q[:7] = entries[1]
    fq = lb.Fingerprint.from_bools(q)
    for rg in (0, 57, 120):
        sd = c.scores_device(fq, rg).cpu().numpy()
        for e, ent in enumerate(entries):
            want, _ = align_ref.profile(q, ent, rg)
            assert _bits(max(np.float32(0), want.max())) == _bits(np.float32(oracle.compare_fp(q, ent, rg if rg else 199, 199)))
            got, first = c.match_profile(fq, e, rg)
            assert first == 0 and np.array_equal(_bits(got), _bits(want)), (rg, e)
            assert _bits(max(np.float32(0), got.max())) == _bits(sd[e]), (rg, e)
    # a capacity below the count: the status and the count the caller needs
    L = lb.lib()
    n, first = lb._native.UInt64(0), lb._native.SInt32(7)
    out = (lb._native.Float32 * 10)()
    st = L.LBAudioDetectiveCorpusMatchProfile(c._ref, fq._ref, 0, 3, out, 10, C.byref(n), C.byref(first))
    assert st == lb.constant("kLBAudioDetectiveArgumentInvalid") and n.value == 271 and first.value == 0
    st = L.LBAudioDetectiveCorpusMatchProfile(c._ref, fq._ref, 0, 5, out, 10, C.byref(n), C.byref(first))
    assert st == lb.constant("kLBAudioDetectiveArgumentInvalid")      # no such entry


def test_match_profile_of_a_long_recording(lb, gpu, oracle):
    """A query of 48 against one entry of 200 000 sub-fingerprints: the offsets spread over many workgroups."""
    rng = np.random.default_rng(23)
    long = (rng.random((200_000, 200)) < 0.5).astype(np.uint8)
    q = long[123_456:123_504].copy()
    q[::4, 10] ^= 1
    short = [(rng.random((int(m), 200)) < 0.5).astype(np.uint8) for m in (3, 48, 60)]
    entries = [short[0], long, short[1], short[2]]
    c = _ragged(lb, gpu, oracle, entries)
    fq = lb.Fingerprint.from_bools(q)
    got, first = c.match_profile(fq, 1)
    want, entry_long = align_ref.profile(q, long, 0)
    assert entry_long and first == 0 and len(got) == 200_000 - 48 + 1
    assert np.array_equal(_bits(got), _bits(want))
    assert int(np.argmax(got)) == 123_456
    _, _, sc = oracle.corpus_best_ragged(q, entries, 200, nthreads=16, want_scores=True)
    assert _bits(got.max()) == _bits(sc[1])
    assert c.query_aligned(fq) == (1, float(sc[1]), 123_456)
    # the split launch of the keys path: every entry's key, the long pair spread over many workgroups
    keys = gpu.from_numpy(_keys_of(sc, 0)[None]).cuda()
    lags, scores = c.align_keys_device([fq], keys, 4, want_scores=True)
    want_lags = [align_ref.align(q, e, 0)[1] for e in entries]
    assert lags.cpu().numpy()[0].tolist() == want_lags and np.array_equal(_bits(scores.cpu().numpy()[0]), _bits(sc))


def test_full_size_ragged_topk_aligned(lb, gpu, oracle):
    """1 M synthetic entries of 20..70: eight planted queries, top-10 aligned; every returned entry's lag checked."""
    n = 1_000_000
    counts = oracle.synth_ragged_counts(SEED, 0, n, 20, 70)
    packed = lb.synth_ragged_corpus_device(SEED, 0, counts, 200)
    c = lb.Corpus.ragged(200, n, int(counts.sum()))
    c.append_ragged_packed_device(packed, counts)
    rng = np.random.default_rng(29)
    planted = [5, 123_456, 500_001, 777_777, 999_999, 42, 314_159, 654_321]
    qs = []
    for i, p in enumerate(planted):
        src = oracle.synth_entry(SEED, p, int(counts[p]), 200)
        at = int(rng.integers(0, counts[p] - 21 + 1))
        q = src[at:at + 21].copy()
        q[:, 2 * i + 1] ^= rng.random(21) < 0.5
        qs.append((q, at))
    fps = [lb.Fingerprint.from_bools(q) for q, _ in qs]
    got = c.query_batch_topk_aligned(fps, 10)
    plain = c.query_batch_topk(fps, 10)
    for qi, ((gi, gs, gl), (pi, ps)) in enumerate(zip(got, plain)):
        assert np.array_equal(gi, pi) and np.array_equal(_bits(gs), _bits(ps))
        assert gi[0] == planted[qi] and gl[0] == qs[qi][1], (qi, gi[0], gl[0], qs[qi][1])
        for j, e in enumerate(gi):
            ent = oracle.synth_entry(SEED, int(e), int(counts[e]), 200)
            s, want_lag = align_ref.align(qs[qi][0], ent, 0)
            assert _bits(s) == _bits(gs[j]) and gl[j] == want_lag, (qi, e)
