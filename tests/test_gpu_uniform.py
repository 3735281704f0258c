"""GPU tests of the uniform corpus' specialised scans (queries of as many sub-fingerprints as the entries, L = 200, NSUB 1..8:
compare_planes_kernel<NSUB>, compare_planes_batch_kernel<NSUB, false / true>) and of the generic scan on the same corpora,
against the oracle's per-entry scores of the packed rows actually appended.  Indices are compared exactly, scores as
float32 bits.

Each corpus holds 600 000 entries (not a multiple of 256, more than twice the threads of the single-query grid: every scan
takes several grid-stride trips with a ragged last one) in a capacity of 601 000 (the plane stride is not the count), written
by three appends: the device generator's block, a host-packed block with pairs of two set Booleans, a few single
fingerprints.  Crafted rows: exact copies of a query at a low and two higher indices, entries 0 and n - 1, all-zero entries,
an entry one sign pair away from a query at Booleans 198 / 199 of its last sub-fingerprint."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CSEED = 0x4C424145
L = 200
N = 600_000
N_SYNTH = 350_017                       # appended first; then the host-packed block; then N_FP single fingerprints
N_FP = 4
N_HOST = N - N_SYNTH - N_FP
CAP = N + 1000
TOP = 1 << 32
RANGES = (0, 1, 2, 3, 119, 120, 199, 200, 201, 1000)
SOME = (0, 3, 199)                      # the ranges of the generic scan's legs
BATCHES = (1, 2, 7, 8, 9, 16, 17)       # across the scan's group of 8 queries twice
NQ = 17
LO_TWIN, HI_TWIN = 3, N_SYNTH + N_HOST - 5
LAST_PAIR = N_SYNTH + 123_457           # query 8 but for the sign pair at Booleans 198 / 199 of the last sub-fingerprint


def _pairs(rng, shape, p00=0.0, p11=0.0):
    """Booleans [..., L] as sign pairs: 00 with p00, 11 with p11, otherwise 01 or 10."""
    u = rng.random(shape[:-1] + (shape[-1] // 2,))
    first = rng.random(u.shape) < 0.5
    out = np.empty(shape, np.uint8)
    out[..., 0::2] = np.where(u < p00, 0, np.where(u < p00 + p11, 1, first))
    out[..., 1::2] = np.where(u < p00, 0, np.where(u < p00 + p11, 1, ~first))
    return out


def _flip(rng, f, frac=0.0, count=0):
    """Swap the two Booleans of a fraction of the pairs (or of `count` pairs with one Boolean set)."""
    q = np.ascontiguousarray(f).copy()
    p = q.reshape(-1, 2)
    sel = rng.choice(np.nonzero(p[:, 0] != p[:, 1])[0], count, replace=False) if count else rng.random(len(p)) < frac
    p[sel] = p[sel][:, ::-1]
    return q


def _with_11(rng, f, frac):
    """Set both Booleans of a fraction of the pairs."""
    q = f.copy()
    sel = rng.random(q.shape[:-1] + (q.shape[-1] // 2,)) < frac
    q[..., 0::2][sel] = 1
    q[..., 1::2][sel] = 1
    return q


def _packed(oracle, bools):
    """[..., L] Booleans -> the library's 32-byte packed rows (uint8)."""
    return np.ascontiguousarray(oracle.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _best_of(scores):
    """The best-match loop of Tests.m:57-91 over per-entry scores: strict '<' from 0.0, lowest index on ties."""
    i = int(np.argmax(scores))
    return (i, float(scores[i])) if scores[i] > 0 else (-1, 0.0)


def _expected(scores, k):
    """Top-K: entries scoring above 0, score descending, equal scores lowest index first."""
    order = np.lexsort((np.arange(len(scores)), -scores))
    order = order[scores[order] > 0][:k]
    return order.astype(np.int64), scores[order]


def _bits(r):
    return int(r[0]), int(np.float32(r[1]).view(np.uint32))


def _shift(r, base):
    return (r[0] + base if r[0] >= 0 else -1), r[1]


def _same_scores(got, want, what):
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


def _same_topk(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, got[0][:8], want[0][:8], len(got[0]), len(want[0]))
    assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), want[1].view(np.uint32)), (what, got[1][:8], want[1][:8])


class Uniform:
    """One corpus of NSUB sub-fingerprints per entry, its 17 queries and the oracle's scores (cached per query and range)."""

    def __init__(self, lb, gpu, oracle, nsub):
        self.nsub, self.oracle = nsub, oracle
        rng = np.random.default_rng(1000 + nsub)
        base = _pairs(rng, (9, nsub, L), p00=0.05)
        base[8, -1, 198:200] = (1, 0)
        q = [base[0],                                       # 0  exact copy of entries LO_TWIN, HI_TWIN, N - 2
             _flip(rng, base[1], count=1),                  # 1  one pair flipped (entry N_SYNTH + 1)
             _flip(rng, base[2], 0.02),                     # 2  2 % (entry N - 1, the last single fingerprint)
             _flip(rng, base[3], 0.10),                     # 3  10 % (entry 0)
             _flip(rng, base[4], 0.30),                     # 4  30 % (entry 299 999)
             _with_11(rng, base[5], 0.03)]                  # 5  pairs 11 (entry N_SYNTH + 77 777 has others)
        one = np.zeros((nsub, L), np.uint8)
        one[nsub // 2, 114] = 1
        q += [one,                                          # 6  possible = 1 in one sub-fingerprint, 0 elsewhere
              _pairs(rng, (nsub, L)),                       # 7  every pair set: possible = 100
              base[8]]                                      # 8  entry LAST_PAIR differs at Booleans 198 / 199
        q += [_pairs(rng, (nsub, L), p00=0.05, p11=0.02 * (i % 2)) for i in range(6)]   # 9..14 random
        q += [np.ones((nsub, L), np.uint8), np.zeros((nsub, L), np.uint8)]            # 15 all set, 16 all zero
        assert len(q) == NQ
        self.q = q
        last = base[8].copy()
        last[-1, 198:200] = (0, 1)
        zero = np.zeros((nsub, L), np.uint8)
        rows = {0: base[3], 1: zero, LO_TWIN: base[0], 299_999: base[4],
                N_SYNTH: zero, N_SYNTH + 1: base[1], N_SYNTH + 77_777: _with_11(rng, base[5], 0.02), LAST_PAIR: last,
                HI_TWIN: base[0], N_SYNTH + N_HOST - 1: zero,
                N - 4: _flip(rng, base[6], 0.05), N - 3: zero, N - 2: base[0], N - 1: base[2]}
        # 1. the device generator's block, crafted rows written over it on the device
        a = lb.synth_corpus_device(CSEED, 0, N_SYNTH, nsub, L)
        for at, r in rows.items():
            if at < N_SYNTH:
                a[at] = gpu.from_numpy(_packed(oracle, r)).cuda()
        # 2. a host-packed block: the generator's rows with about 1.6 % of the pairs 11, crafted rows packed on the host
        hb = lb.synth_corpus_device(CSEED + nsub, 0, N_HOST, nsub, L).cpu().numpy().view(np.uint64).reshape(N_HOST, nsub, 4)
        m = np.frombuffer(rng.bytes(8 * hb.size), np.uint64).reshape(hb.shape)
        for _ in range(5):
            m = m & np.frombuffer(rng.bytes(8 * hb.size), np.uint64).reshape(hb.shape)
        m &= np.uint64(0x5555555555555555)
        m[..., 3] &= np.uint64(0xFF)                        # (Booleans 192..199)
        hb |= m | (m << np.uint64(1))
        for at, r in rows.items():
            if N_SYNTH <= at < N_SYNTH + N_HOST:
                hb[at - N_SYNTH] = oracle.pack_bools(r)
        self.corpus = c = lb.Corpus(L, nsub, CAP)
        c.append_packed_device(a)
        c.append_packed_device(gpu.from_numpy(hb.view(np.uint8).reshape(N_HOST, nsub, 32)).cuda())
        # 3. single fingerprints
        fp_rows = [rows[N - N_FP + i] for i in range(N_FP)]
        for r in fp_rows:
            c.append_fingerprint(lb.Fingerprint.from_bools(r))
        gpu.cuda.synchronize()
        assert len(c) == N
        # the oracle's input: the packed rows as appended
        self.words = np.concatenate([a.cpu().numpy().view(np.uint64).reshape(N_SYNTH, nsub, 4), hb, oracle.pack_bools(np.stack(fp_rows))])
        assert self.words.shape == (N, nsub, 4)
        self.qwords = [oracle.pack_bools(x) for x in q]
        self.fq = [lb.Fingerprint.from_bools(x) for x in q]
        self._scores, self._top = {}, {}

    def score(self, qi, rg):
        if (qi, rg) not in self._scores:
            self._scores[qi, rg] = self.oracle.corpus_scores_packed(self.qwords[qi], self.words, L, rg if rg else L, nthreads=16)
        return self._scores[qi, rg]

    def best(self, qi, rg):
        return _best_of(self.score(qi, rg))

    def top(self, qi, rg, k):
        if (qi, rg) not in self._top:
            self._top[qi, rg] = _expected(self.score(qi, rg), 1024)
        i, s = self._top[qi, rg]
        return i[:k], s[:k]

    def scores_of(self, x, rg):
        return self.oracle.corpus_scores_packed(self.oracle.pack_bools(x), self.words, L, rg if rg else L, nthreads=16)


@pytest.fixture(scope="module", params=range(1, 9), ids=lambda s: f"nsub{s}")
def uni(request, lb, gpu, oracle):
    u = Uniform(lb, gpu, oracle, request.param)
    yield u
    u.corpus.dispose()


def test_batch_queries(uni, lb, gpu):
    """query_batch / query_batch_keys_device (compare_planes_batch_kernel, groups of 8): every key of batches of 1 .. 17,
    the 17-query batch at every range, the largest index base allowed and the first one refused; variant 1 (one generic
    scan per query) on the same queries."""
    c = uni.corpus
    for b in BATCHES:
        order = [(i * 5 + b) % NQ for i in range(b)]
        got = c.query_batch([uni.fq[i] for i in order])
        assert [_bits(g) for g in got] == [_bits(uni.best(i, 0)) for i in order], (uni.nsub, b)
    keys = gpu.zeros(NQ, dtype=gpu.int64, device="cuda")
    base = TOP - N
    for rg in RANGES:
        want = [_bits(uni.best(i, rg)) for i in range(NQ)]
        assert [_bits(g) for g in c.query_batch(uni.fq, rg)] == want, (uni.nsub, rg)
        keys.fill_(-1)
        c.query_batch_keys_device(uni.fq, keys, rg, index_base=base)
        got = [_bits(lb.Corpus.decode_key(int(k))) for k in keys.cpu().tolist()]
        assert got == [_bits(_shift(uni.best(i, rg), base)) for i in range(NQ)], (uni.nsub, rg)
    with pytest.raises(lb.LBAudioDetectiveError) as e:
        c.query_batch_keys_device(uni.fq, keys, 0, index_base=base + 1)
    assert e.value.status == 1
    c.set_kernel_variant(1)
    for rg in (0, 199):
        assert [_bits(g) for g in c.query_batch(uni.fq, rg)] == [_bits(uni.best(i, rg)) for i in range(NQ)], (uni.nsub, rg)
    c.set_kernel_variant(0)


def test_scores_every_entry(uni, gpu):
    """scores_device: all 600 000 scores of every query, specialised (variant 0, every range) and generic (variant 1) scan."""
    c = uni.corpus
    for variant in (0, 1):
        c.set_kernel_variant(variant)
        for qi in range(NQ):
            for rg in RANGES if variant == 0 else SOME:
                _same_scores(c.scores_device(uni.fq[qi], rg).cpu().numpy(), uni.score(qi, rg), (uni.nsub, variant, qi, rg))
    c.set_kernel_variant(0)


def test_top1_entry_points(uni, lb, gpu):
    """query (polled, variants 0 and 2; generic, variant 1) and query_key_device (direct atomic, nonzero index base)."""
    c = uni.corpus
    key = gpu.zeros(1, dtype=gpu.int64, device="cuda")
    base = TOP - N - 12_345
    for qi in range(NQ):
        for rg in RANGES:
            want = _bits(uni.best(qi, rg))
            for variant in (0, 2, 1):
                c.set_kernel_variant(variant)
                assert _bits(c.query(uni.fq[qi], rg)) == want, (uni.nsub, variant, qi, rg)
            c.set_kernel_variant(0)
            c.query_key_device(uni.fq[qi], key, rg, index_base=base)
            assert _bits(lb.Corpus.decode_key(int(key.item()))) == _bits(_shift(uni.best(qi, rg), base)), (uni.nsub, qi, rg)
    # what was planted is what the oracle sees
    assert c.query(uni.fq[0]) == (LO_TWIN, 1.0)
    assert c.query(uni.fq[2])[0] == N - 1 and c.query(uni.fq[3])[0] == 0
    assert c.query(uni.fq[8], 120) == (LAST_PAIR, 1.0)
    idx, sc = c.query(uni.fq[8], 199)
    assert idx == LAST_PAIR and sc < 1.0
    assert c.query(uni.fq[16]) == (-1, 0.0)


def test_topk(uni, gpu):
    """query_topk (K 1, 10, 1024) and query_batch_topk (9 and 17 queries: the scores form of the batch scan in two and three
    groups), and the generic scan's top-K, against the oracle's ranking."""
    c = uni.corpus
    for qi in range(NQ):
        for k in (1, 10, 1024):
            _same_topk(c.query_topk(uni.fq[qi], k), uni.top(qi, 0, k), (uni.nsub, qi, k))
    assert len(c.query_topk(uni.fq[16], 10)[0]) == 0
    for nb in (9, 17):
        order = [(i * 3 + nb) % NQ for i in range(nb)]
        for k, rg in ((10, 199), (1024, 0)):
            for i, got in zip(order, c.query_batch_topk([uni.fq[i] for i in order], k, rg)):
                _same_topk(got, uni.top(i, rg, k), (uni.nsub, nb, i, k, rg))
    c.set_kernel_variant(1)
    for qi in (0, 2, 6, 8, 15):
        _same_topk(c.query_topk(uni.fq[qi], 10), uni.top(qi, 0, 10), (uni.nsub, "generic", qi))
    c.set_kernel_variant(0)


def test_other_query_lengths(uni, lb, gpu):
    """Queries of 1, NSUB - 1, NSUB + 1 and 2 NSUB + 1 sub-fingerprints slide (Fp.m:123-146) in the generic scan: every score
    and the top-1 against the oracle, alone and in a batch with a query of NSUB; variant 2 refuses them."""
    c = uni.corpus
    nsub = uni.nsub
    rng = np.random.default_rng(77 + nsub)
    for nq in sorted({1, nsub - 1, nsub + 1, 2 * nsub + 1} - {0, nsub}):
        if nq < nsub:
            q = _flip(rng, uni.q[1][nsub - nq:], 0.02)      # slides along entry N_SYNTH + 1
        else:
            pre = (nq - nsub) // 2
            q = np.concatenate([_pairs(rng, (pre, L), 0.05), uni.q[3], _pairs(rng, (nq - nsub - pre, L), 0.05)])   # entry 0 inside
        fq = lb.Fingerprint.from_bools(q)
        for rg in (0, 119):
            want = uni.scores_of(q, rg)
            _same_scores(c.scores_device(fq, rg).cpu().numpy(), want, (nsub, nq, rg))
            for variant in (0, 1):
                c.set_kernel_variant(variant)
                assert _bits(c.query(fq, rg)) == _bits(_best_of(want)), (nsub, nq, rg, variant)
            c.set_kernel_variant(0)
            got = c.query_batch([fq, uni.fq[2], fq], rg)
            assert [_bits(g) for g in got] == [_bits(_best_of(want)), _bits(uni.best(2, rg)), _bits(_best_of(want))]
        c.set_kernel_variant(2)
        for call in (lambda: c.query(fq), lambda: c.scores_device(fq)):
            with pytest.raises(lb.LBAudioDetectiveError) as e:
                call()
            assert e.value.status == 1
        c.set_kernel_variant(0)


def test_generic_query_length_limit(lb, gpu, oracle):
    """The generic scan keeps the query in 48 KB of LDS: 1536 sub-fingerprints are accepted and match the oracle (entries
    slide along the query), 1537 are refused with status 1 by every entry point."""
    rng = np.random.default_rng(1536)
    n, nsub = 300, 5
    host = _pairs(rng, (n, nsub, L), p00=0.05, p11=0.02)
    q = _pairs(rng, (1536, L), p00=0.05)
    host[17] = q[700:705]
    host[250] = _flip(rng, q[1531:], 0.1)
    c = lb.Corpus(L, nsub, n + 7)
    c.append_packed_device(gpu.from_numpy(_packed(oracle, host)).cuda())
    words = oracle.pack_bools(host)
    fq = lb.Fingerprint.from_bools(q)
    for rg in (0, 119):
        want = oracle.corpus_scores_packed(oracle.pack_bools(q), words, L, rg if rg else L, nthreads=16)
        _same_scores(c.scores_device(fq, rg).cpu().numpy(), want, rg)
        assert _bits(c.query(fq, rg)) == _bits(_best_of(want)), rg
    assert c.query(fq) == (17, 1.0)
    long = lb.Fingerprint.from_bools(np.concatenate([q, q[:1]]))
    key = gpu.zeros(1, dtype=gpu.int64, device="cuda")
    for call in (lambda: c.query(long), lambda: c.scores_device(long), lambda: c.query_topk(long, 5),
                 lambda: c.query_key_device(long, key)):
        with pytest.raises(lb.LBAudioDetectiveError) as e:
            call()
        assert e.value.status == 1
    c.dispose()
