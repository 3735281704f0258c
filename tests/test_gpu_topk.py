"""GPU tests of the top-K corpus queries (LBAudioDetectiveCorpusQueryTopK and its batch / key forms) and of the selection on its
own (LBAudioDetectiveTopKKeysFromScoresDevice).  The expected lists come from the oracle's per-entry scores: entries scoring
above 0, score descending, equal scores lowest index first, cut at K.  Indices are compared exactly, scores as float32 bits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CSEED = 0x4C424145
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 10, 100, 1024)


def _expected(scores, k):
    scores = np.asarray(scores, np.float32)
    order = np.lexsort((np.arange(len(scores)), -scores))
    order = order[scores[order] > 0][:k]
    return order.astype(np.int64), scores[order]


def _same(got, want, what=""):
    gi, gs = got
    wi, ws = want
    assert np.array_equal(gi, wi), (what, gi[:8], wi[:8], len(gi), len(wi))
    assert np.array_equal(np.asarray(gs, np.float32).view(np.uint32), np.asarray(ws, np.float32).view(np.uint32)), (what, gs[:8], ws[:8])


def _packed(oracle, bools):
    """[..., L] Booleans -> the library's 32-byte packed rows (uint8)."""
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


def test_packing_helper_matches_the_library(lb, oracle):
    rng = np.random.default_rng(1)
    rows = (rng.random((5, 200)) < 0.5).astype(np.uint8)
    assert np.array_equal(_packed(oracle, rows).view(np.uint32), np.stack([lb.pack_subfingerprint(r) for r in rows]))


def test_k1_equals_corpus_query_uniform(lb, gpu, oracle):
    rng = np.random.default_rng(2)
    n = 30000
    host = oracle.synth_corpus(CSEED, 0, n, 5, 200)
    host[17] = host[29000]
    corpus = _uniform(lb, gpu, oracle, host)
    flat, counts = host.reshape(-1, 200), np.full(n, 5, np.uint32)
    for q in (host[29000], _near(rng, host[123], 30), host[5][:3], host[7][:1]):
        for variant in (0, 1, 2):
            corpus.set_kernel_variant(variant)
            if variant == 2 and q.shape[0] != 5:
                with pytest.raises(lb.LBAudioDetectiveError):
                    corpus.query_topk(lb.Fingerprint.from_bools(q), 1)
                continue
            fq = lb.Fingerprint.from_bools(q)
            idx, sc = corpus.query_topk(fq, 1)
            assert (int(idx[0]), float(sc[0])) == corpus.query(fq), (variant, q.shape)
            _same(corpus.query_topk(fq, 10), _expected(_oracle_scores(oracle, q, flat, counts, 200), 10), (variant, q.shape))
    corpus.set_kernel_variant(0)
    assert corpus.query_topk(lb.Fingerprint.from_bools(host[29000]), 3)[0].tolist()[:2] == [17, 29000]


@pytest.mark.parametrize("pruning", [True, False])
def test_k1_equals_corpus_query_ragged(lb, gpu, oracle, pruning):
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 71, 4000).astype(np.uint32)
    flat = oracle.synth_ragged_entries(CSEED, 0, counts, 200)
    corpus = _ragged(lb, gpu, oracle, flat, counts)
    corpus.set_bound_pruning(pruning)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    long_e = int(np.argmax(counts))
    for q in (flat[off[9]:off[9] + 5], flat[off[40]:off[40] + 12], _near(rng, flat[off[long_e]:off[long_e] + 21], 8),
              (rng.random((90, 200)) < 0.5).astype(np.uint8)):
        fq = lb.Fingerprint.from_bools(q)
        idx, sc = corpus.query_topk(fq, 1)
        assert (int(idx[0]) if len(idx) else -1, float(sc[0]) if len(sc) else 0.0) == corpus.query(fq), q.shape
        _same(corpus.query_topk(fq, 100), _expected(_oracle_scores(oracle, q, flat, counts, 200), 100), q.shape)


@pytest.mark.parametrize("nsub,L", [(5, 200), (1, 200), (8, 200), (3, 199), (2, 33), (4, 2)])
def test_random_uniform_corpora(lb, gpu, oracle, nsub, L):
    rng = np.random.default_rng(nsub * 1000 + L)
    n = 200000
    host = rng.integers(0, 2, (n, nsub, L), dtype=np.uint8)
    host[rng.integers(0, 100, (n, nsub, L), dtype=np.uint8) < 3] = 0
    corpus = _uniform(lb, gpu, oracle, host)
    flat, counts = host.reshape(-1, L), np.full(n, nsub, np.uint32)
    for rg in (0, 1, 2, 119, 120, 200):
        q = _near(rng, host[int(rng.integers(0, n))], 3 * nsub)
        fq = lb.Fingerprint.from_bools(q)
        scores = _oracle_scores(oracle, q, flat, counts, rg)
        for k in KS:
            _same(corpus.query_topk(fq, k, rg), _expected(scores, k), (nsub, L, rg, k))
        top = corpus.query(fq, rg)
        idx, sc = corpus.query_topk(fq, 1, rg)
        assert (int(idx[0]) if len(idx) else -1, float(sc[0]) if len(sc) else 0.0) == top


def test_random_ragged_corpora(lb, gpu, oracle):
    rng = np.random.default_rng(5)
    counts = rng.integers(1, 71, 20000).astype(np.uint32)
    flat = oracle.synth_ragged_entries(CSEED + 1, 0, counts, 200)
    corpus = _ragged(lb, gpu, oracle, flat, counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    for nq, rg in ((21, 0), (5, 120), (40, 0), (3, 1)):
        e = int(rng.choice(np.nonzero(counts >= nq)[0]))
        q = _near(rng, flat[off[e]:off[e] + nq], 4)
        fq = lb.Fingerprint.from_bools(q)
        scores = _oracle_scores(oracle, q, flat, counts, rg)
        for k in KS:
            _same(corpus.query_topk(fq, k, rg), _expected(scores, k), (nq, rg, k))


def test_ties_and_degenerate_inputs(lb, gpu, oracle):
    n = 200000
    host = oracle.synth_corpus(CSEED, 0, n, 5, 200)
    q = oracle.synth_entry(CSEED, 123456789, 5, 200)
    for at in (199999, 100003, 7):
        host[at] = q
    corpus = _uniform(lb, gpu, oracle, host)
    idx, sc = corpus.query_topk(lb.Fingerprint.from_bools(q), 5)
    assert idx[:3].tolist() == [7, 100003, 199999] and sc[:3].tolist() == [1.0, 1.0, 1.0]
    # a corpus of identical entries: indices 0 .. K-1
    same = np.broadcast_to(q, (5000, 5, 200)).copy()
    c2 = _uniform(lb, gpu, oracle, same)
    for k in (1, 10, 1024):
        idx, sc = c2.query_topk(lb.Fingerprint.from_bools(q), k)
        assert idx.tolist() == list(range(k)) and (sc == 1.0).all()
    # all-zero query and all-zero corpus: nothing scores above 0
    zero = np.zeros((5, 200), np.uint8)
    idx, sc = corpus.query_topk(lb.Fingerprint.from_bools(zero), 10)
    assert len(idx) == 0 and len(sc) == 0
    c3 = _uniform(lb, gpu, oracle, np.zeros((100, 5, 200), np.uint8))
    assert len(c3.query_topk(lb.Fingerprint.from_bools(q), 10)[0]) == 0
    # K above the number of positive scores, and above the corpus size
    small = host[:40].copy()
    small[::2] = 0
    c4 = _uniform(lb, gpu, oracle, small)
    scores = _oracle_scores(oracle, q, small.reshape(-1, 200), np.full(40, 5, np.uint32), 200)
    for k in (15, 20, 21, 100, 1024):
        _same(c4.query_topk(lb.Fingerprint.from_bools(q), k), _expected(scores, k), k)
    # the padding of the host call: index -1, score 0, through the batch form's raw arrays
    res = c4.query_batch_topk([lb.Fingerprint.from_bools(q)], 1024)[0]
    assert len(res[0]) == int((scores > 0).sum())
    # argument checks
    for bad_k in (0, 1025):
        with pytest.raises(lb.LBAudioDetectiveError):
            corpus.query_topk(lb.Fingerprint.from_bools(q), bad_k)
    with pytest.raises(lb.LBAudioDetectiveError):
        corpus.query_topk(lb.Fingerprint.from_bools(q[:, :100]), 5)
    keys = gpu.zeros(10, dtype=gpu.int64, device="cuda")
    with pytest.raises(lb.LBAudioDetectiveError):
        corpus.query_batch_topk_keys_device([lb.Fingerprint.from_bools(q)], 10, keys, index_base=(1 << 32) - n + 1)


@pytest.mark.parametrize("ragged", [False, True])
def test_batches_equal_single_calls(lb, gpu, oracle, ragged):
    rng = np.random.default_rng(7 + ragged)
    if ragged:
        counts = rng.integers(1, 71, 6000).astype(np.uint32)
        flat = oracle.synth_ragged_entries(CSEED + 2, 0, counts, 200)
        corpus = _ragged(lb, gpu, oracle, flat, counts)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)

        def make_q(i):
            nq = (5, 21, 12, 40)[i % 4]
            e = int(np.nonzero(counts >= nq)[0][i])
            return _near(rng, flat[off[e]:off[e] + nq], 3)
    else:
        n = 50000
        host = oracle.synth_corpus(CSEED, 0, n, 5, 200)
        corpus = _uniform(lb, gpu, oracle, host)
        flat, counts = host.reshape(-1, 200), np.full(n, 5, np.uint32)

        def make_q(i):
            return _near(rng, host[int(rng.integers(0, n))], 10)
    for nb in (1, 3, 8, 9, 17):
        qs = [make_q(i) for i in range(nb)]
        fqs = [lb.Fingerprint.from_bools(q) for q in qs]
        batch = corpus.query_batch_topk(fqs, 10)
        for q, fq, got in zip(qs, fqs, batch):
            _same(got, corpus.query_topk(fq, 10), nb)
            _same(got, _expected(_oracle_scores(oracle, q, flat, counts, 200), 10), nb)
        keys = gpu.zeros((nb, 10), dtype=gpu.int64, device="cuda")
        corpus.query_batch_topk_keys_device(fqs, 10, keys)
        gpu.cuda.synchronize()
        for row, got in zip(keys.cpu(), batch):
            _same(lb.decode_topk_keys(row), got, ("keys", nb))


def _select(lb, gpu, scores, k, index_base=0):
    t = gpu.from_numpy(np.ascontiguousarray(scores, np.float32)).cuda()
    out = lb.topk_keys_from_scores_device(t, k, index_base)
    return out.cpu().numpy()


def _host_keys(scores, k, index_base=0):
    order, s = _expected(np.where(np.isnan(scores), np.float32(-1), scores).astype(np.float32), k)
    keys = (s.view(np.uint32).astype(np.int64) << 32) | (0xFFFFFFFF - (index_base + order))
    return np.concatenate([keys, np.zeros(k - len(keys), np.int64)])


def test_selection_on_crafted_score_arrays(lb, gpu):
    rng = np.random.default_rng(9)
    n = 10_000_000
    cases = {}
    cases["all equal"] = np.full(n, 0.5, np.float32)
    one = np.full(n, 0.5, np.float32)
    one[7654321] = 0.5000001
    cases["all equal but one"] = one
    tie = (0.45 + 0.01 * rng.random(n)).astype(np.float32)
    tie[rng.choice(n, 101, replace=False)] = np.float32(0.9)    # K + 1 ties at the boundary for K = 100
    tie[rng.choice(n, 50, replace=False)] = np.float32(0.95)
    cases["ties at the boundary"] = tie
    ulp = np.full(n, 0.5, np.float32)
    at = rng.choice(n, 3000, replace=False)
    ulp[at] = np.nextafter(np.float32(0.5), np.float32(1), dtype=np.float32) + np.arange(3000) % 7 * np.float32(2 ** -24)
    cases["one ulp apart"] = ulp
    odd = np.zeros(1000, np.float32)
    odd[::3] = np.float32(1e-42)                                 # denormals
    odd[1::7] = np.nan
    odd[2::11] = -0.5
    odd[5] = -0.0
    odd[6] = np.float32(1.4e-45)
    odd[100] = np.inf
    odd[200] = 3.0
    cases["denormals, zeros, NaN"] = odd
    cases["normal"] = np.clip(rng.normal(0.5, 0.03, n), 0, 1).astype(np.float32)
    for name, s in cases.items():
        for k in (1, 100, 1024):
            got = _select(lb, gpu, s, k)
            assert np.array_equal(got, _host_keys(s, k)), (name, k)
    # several rows, and an index base
    rows = np.stack([np.clip(rng.normal(0.5, 0.03, 300000), 0, 1).astype(np.float32) for _ in range(5)])
    rows[2] = 0.25
    got = _select(lb, gpu, rows, 64, index_base=1000)
    for r in range(5):
        assert np.array_equal(got[r], _host_keys(rows[r], 64, 1000)), r
    with pytest.raises(lb.LBAudioDetectiveError):
        _select(lb, gpu, rows[0], 1025)


def test_full_size_uniform_corpus(lb, gpu, oracle):
    n = 10_000_000
    q = oracle.synth_entry(CSEED, 4321, 5, 200)
    rng = np.random.default_rng(11)
    # copies and near-copies (a few Booleans flipped) of the query planted across the corpus
    planted = {9_999_999: 0, 5_000_000: 1, 123: 2, 3_000_001: 4, 7_777_777: 8, 42: 16, 8_000_000: 16}
    packed = lb.synth_corpus_device(CSEED, 0, n, 5, 200)
    host = {}
    for at, flips in planted.items():
        host[at] = _near(rng, q, flips)
        packed[at] = gpu.from_numpy(_packed(oracle, host[at])).cuda()
    corpus = lb.Corpus(200, 5, n)
    corpus.append_packed_device(packed)
    fq = lb.Fingerprint.from_bools(q)
    scores = corpus.scores_device(fq).cpu().numpy()
    # every one of the 10 M scores against the oracle's, from the packed rows as appended
    words = packed.cpu().numpy().view(np.uint64).reshape(n, 5, 4)
    want = oracle.corpus_scores_packed(oracle.pack_bools(q), words, 200, 200, nthreads=16)
    bad = np.nonzero(scores.view(np.uint32) != want.view(np.uint32))[0]
    assert len(bad) == 0, (len(bad), bad[:5])
    for k in (10, 1024):
        idx, sc = corpus.query_topk(fq, k)
        _same((idx, sc), _expected(scores, k), k)
        _same((idx, sc), _expected(want, k), ("oracle", k))
    idx, sc = corpus.query_topk(fq, 10)
    assert sc[0] == 1.0 and 4321 in idx.tolist() and 9_999_999 in idx.tolist()
    for i, s in zip(idx[:6], sc[:6]):
        e = host[int(i)] if int(i) in host else oracle.synth_entry(CSEED, int(i), 5, 200)
        assert np.float32(oracle.compare_fp(q, e, 200)).view(np.uint32) == np.float32(s).view(np.uint32), i
    assert (int(idx[0]), float(sc[0])) == corpus.query(fq)
    # a batch of 8 near-copies against the full corpus
    near = [_near(rng, q, f) for f in range(8)]
    qs = [lb.Fingerprint.from_bools(x) for x in near]
    batch = corpus.query_batch_topk(qs, 10)
    for x, fqi, got in zip(near, qs, batch):
        _same(got, _expected(corpus.scores_device(fqi).cpu().numpy(), 10))
        _same(got, _expected(oracle.corpus_scores_packed(oracle.pack_bools(x), words, 200, 200, nthreads=16), 10), "oracle")


def test_two_shards_in_one_process(lb, gpu, oracle):
    n = 100000
    host = oracle.synth_corpus(CSEED, 0, n, 5, 200)
    q = oracle.synth_entry(CSEED, 99999999, 5, 200)
    for at in (49999, 50000, 3, 99999):
        host[at] = q
    rng = np.random.default_rng(13)
    qs = [q, _near(rng, q, 20), host[777]]
    whole = _uniform(lb, gpu, oracle, host)
    halves = [_uniform(lb, gpu, oracle, host[:50000]), _uniform(lb, gpu, oracle, host[50000:])]
    fqs = [lb.Fingerprint.from_bools(x) for x in qs]
    for k in (1, 10, 1024):
        gathered = gpu.zeros((2, len(qs), k), dtype=gpu.int64, device="cuda")
        for r, (c, base) in enumerate(zip(halves, (0, 50000))):
            c.query_batch_topk_keys_device(fqs, k, gathered[r], index_base=base)
        merged = lb.merge_topk_keys(gathered, k).cpu()
        want = whole.query_batch_topk(fqs, k)
        for row, w in zip(merged, want):
            _same(lb.decode_topk_keys(row), w, k)
    assert lb.decode_topk_keys(merged[0])[0][:4].tolist() == [3, 49999, 50000, 99999]


def test_birds_ranking(lb, gpu, oracle):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import birds_matrix as bm
    suffixes = [bm.ESSAY["tests"][t]["suffix"] for t in bm.TESTS]
    names = bm.BIRDS + [b + s for s in suffixes for b in bm.BIRDS]
    fps = bm.fingerprints_gpu(names, 1, 1, 0)
    archives = [fps[b] for b in bm.BIRDS]
    counts = np.array([a.shape[0] for a in archives], np.uint32)
    corpus = _ragged(lb, gpu, oracle, np.concatenate(archives, axis=0), counts)
    seqs = [fps[b + s] for s in suffixes for b in bm.BIRDS]
    assert len(seqs) == 50
    fqs = [lb.Fingerprint.from_bools(q) for q in seqs]
    batch = corpus.query_batch_topk(fqs, 10)
    for q, fq, got in zip(seqs, fqs, batch):
        _, _, want = oracle.corpus_best_ragged(q, archives, 200, want_scores=True)
        _same(got, _expected(want, 10))
        _same(corpus.query_topk(fq, 10), got)
