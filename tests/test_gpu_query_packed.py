"""GPU tests of the packed-query feature: LBAudioDetectiveCorpusQueryPackedKeysDevice / ...QueryPackedTopKKeysDevice (queries that
are already on the device in the packed layout) and identify_clips_device.

Unless stated otherwise "expected" is the handle path on the same commit: the same rows unpacked (unpack_packed), turned into
fingerprint handles (Fingerprint.from_bools) and sent through query_batch_keys_device / query_batch_topk_keys_device /
align_keys_device.  Keys are compared as raw 64-bit words and lags as 32-bit words, every one of them.  Top-1 keys are also
checked against the oracle (index and float bits), so that a mistake shared by both paths cannot hide."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x4C424146
RANGES = (0, 1, 2, 119, 120, 200, 1000)


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _pack(oracle, bools):
    """[..., L] Booleans -> the library's 32-byte packed rows (uint8 [..., 32]), bits from L on zero"""
    return np.ascontiguousarray(oracle.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _garbage(rng, rows, length):
    """the same rows with random bits at the positions >= length"""
    bits = np.unpackbits(rows.reshape(-1, 32), axis=1, bitorder="little")
    bits[:, length:] = rng.integers(0, 2, (bits.shape[0], 256 - length), dtype=np.uint8)
    return np.packbits(bits, axis=1, bitorder="little").reshape(rows.shape)


def _handles(lb, rows, length):
    """packed rows [n, per, 32] (host) -> n fingerprint handles with the same Booleans"""
    n, per = rows.shape[:2]
    bools = lb.unpack_packed(rows.reshape(-1, 32), length).reshape(n, per, length)
    return [lb.Fingerprint.from_bools(b) for b in bools]


def _u64(t):
    return t.cpu().numpy().astype(np.int64).view(np.uint64)


def _key(index, score):
    """what a best match of (index, score) looks like as a decoded key: (index, float bits); (-1, 0) where nothing scores above 0"""
    if index < 0:
        return (-1, 0)
    return (int(index), int(np.float32(score).view(np.uint32)))


def _dec(key):
    """a raw top-1 key as LBAudioDetectiveCorpusDecodeKey reads it: (index, float bits) -- a best score of 0 selects nothing, whatever
    index the scan's maximum carries in its low word"""
    key = int(key)
    bits = key >> 32
    score = np.uint32(bits).view(np.float32)
    return (0xFFFFFFFF - (key & 0xFFFFFFFF), bits) if score > 0 else (-1, 0)


def _expect_top1(gpu, corpus, fps, rg, index_base=0):
    keys = gpu.zeros(len(fps), dtype=gpu.int64, device="cuda")
    corpus.query_batch_keys_device(fps, keys, range_=rg, index_base=index_base)
    return _u64(keys)


def _expect_topk(gpu, corpus, fps, k, rg, index_base=0):
    keys = gpu.zeros((len(fps), k), dtype=gpu.int64, device="cuda")
    corpus.query_batch_topk_keys_device(fps, k, keys, range_=rg, index_base=index_base)
    lags = corpus.align_keys_device(fps, keys, k, index_base=index_base, range_=rg)
    gpu.cuda.synchronize()
    return _u64(keys), lags.cpu().numpy()


def _check_all(gpu, lb, corpus, d_rows, fps, n, per, rg, ks, what):
    """top-1, top-K and lags of the first n queries of d_rows against the handle path; returns the top-1 keys"""
    got = _u64(corpus.query_packed_keys_device(d_rows, n, per, range_=rg))
    want = _expect_top1(gpu, corpus, fps[:n], rg)
    assert np.array_equal(got, want), (what, "top-1", np.flatnonzero(got != want)[:8])
    for k in ks:
        keys, lags = corpus.query_packed_topk_keys_device(d_rows, n, per, k, aligned=True, range_=rg)
        plain = corpus.query_packed_topk_keys_device(d_rows, n, per, k, range_=rg)
        wk, wl = _expect_topk(gpu, corpus, fps[:n], k, rg)
        gk = _u64(keys)
        assert gk.shape == (n, k) and np.array_equal(gk, wk), (what, "top-K keys", k, np.argwhere(gk != wk)[:8])
        assert np.array_equal(_u64(plain), wk), (what, "top-K keys without lags", k)
        gl = lags.cpu().numpy()
        assert gl.dtype == np.int32 and np.array_equal(gl, wl), (what, "lags", k, np.argwhere(gl != wl)[:8])
        # K's first column is the top-1 key wherever something scores above 0 (a top-K list holds no entry of score 0: its key is 0)
        first = np.array([k1 if _dec(k1)[0] >= 0 else 0 for k1 in got], np.uint64)
        assert np.array_equal(gk[:, 0], first), (what, "K's first column is the top-1 key", k)
    return got


# ---- 1. the builders, directly ------------------------------------------------------------------------------------------------
def _bools(rng, n, per, length):
    b = rng.integers(0, 2, (n, per, length)).astype(np.uint8)
    b[0, 0] = 0                      # an all-zero sub-fingerprint: possible = 0, rh = rl = 0
    b[1, per - 1] = 1                # an all-ones one
    b[2] = 0                         # an all-zero query
    return b


@pytest.mark.parametrize("n_sub", range(1, 9))
def test_plane_blocks_equal_the_host_builder(lb, gpu, oracle, n_sub):
    rng = np.random.default_rng(n_sub)
    n = 37
    b = _bools(rng, n, n_sub, 200)
    rows = _pack(oracle, b)
    for rows_in in (rows, _garbage(rng, rows, 200)):
        d = gpu.from_numpy(rows_in).cuda()
        for rg in RANGES:
            want = lb.debug_query_blocks(0, n, n_sub, 200, rg, bools=b)
            got = lb.debug_query_blocks(0, n, n_sub, 200, rg, packed=d)
            assert got.shape == want.shape == (n, 144)
            assert np.array_equal(got, want), (n_sub, rg, np.argwhere(got != want)[:8])
            off = ((n_sub * 200 + 127) // 128) * 4 + 7 * n_sub
            assert not got[0, [off, off + n_sub, off + 2 * n_sub]].any()      # possible, rh, rl of the all-zero sub-fingerprint
    # a source that is only 4-byte aligned
    flat = gpu.zeros(rows.size + 4, dtype=gpu.uint8, device="cuda")
    flat[4:] = gpu.from_numpy(rows.reshape(-1)).cuda()
    got = lb.debug_query_blocks(0, n, n_sub, 200, 0, packed=flat.data_ptr() + 4)
    assert np.array_equal(got, lb.debug_query_blocks(0, n, n_sub, 200, 0, bools=b))


@pytest.mark.parametrize("length", (200, 199, 64, 33))
def test_sliding_and_alignment_blocks_equal_the_host_builders(lb, gpu, oracle, length):
    rng = np.random.default_rng(length)
    n = 19
    for per in (1, 5, 7, 8, 12, 21, 48):
        b = _bools(rng, n, per, length)
        rows = _pack(oracle, b)
        for rows_in in (rows, _garbage(rng, rows, length)):
            d = gpu.from_numpy(rows_in).cuda()
            for rg in RANGES:
                want = lb.debug_query_blocks(1, n, per, length, rg, bools=b)
                got = lb.debug_query_blocks(1, n, per, length, rg, packed=d)
                assert got.shape == want.shape == (n, (per + 1) * 16)
                assert np.array_equal(got, want), (per, length, rg, np.argwhere(got != want)[:8])
                blk = got.reshape(n, per + 1, 16)
                assert not blk[:, per].any() and not blk[0, 0].any()
            for kind in (2, 3):
                want = lb.debug_query_blocks(kind, n, per, length, 0, bools=b)
                got = lb.debug_query_blocks(kind, n, per, length, 0, packed=d)
                assert np.array_equal(got, want), (kind, per, length)


# ---- 2. uniform corpus, the specialised shape ------------------------------------------------------------------------------------
N_UNIFORM = 200_000


def _uniform_case(lb, gpu, rng, n_sub, length, n_entries, per=None, n_queries=300):
    """a synthetic corpus with duplicated and all-zero entries planted, and queries of `per` sub-fingerprints: entries cut from
    the corpus on the device, perturbed copies, random rows and one all-zero query.  Returns (corpus, packed entries on the
    device, packed queries on the device [n, per, 32])"""
    per = n_sub if per is None else per
    entries = lb.synth_corpus_device(SEED, 0, n_entries, n_sub, length)
    entries[n_entries // 2] = entries[11]                       # duplicates: the lower index wins
    entries[n_entries - 1] = entries[n_entries // 3]
    entries[7] = 0
    entries[n_entries // 5] = 0
    corpus = lb.Corpus(length, n_sub, n_entries)
    corpus.append_packed_device(entries)
    picks = gpu.from_numpy(rng.integers(0, n_entries, n_queries)).cuda()
    picks[:6] = gpu.tensor([11, n_entries // 2, n_entries // 3, n_entries - 1, 7, 0], device="cuda")
    if per <= n_sub:
        q = entries[picks][:, :per].clone()
    else:
        q = entries[picks].repeat(1, (per + n_sub - 1) // n_sub, 1)[:, :per].clone()
    # perturbed copies: a few bytes of the used part flipped
    used = (length + 7) // 8
    for i in range(40, 120):
        s, byte = int(rng.integers(0, per)), int(rng.integers(0, used - 1))
        q[i, s, byte] ^= int(rng.integers(1, 256))
    # random rows (cleared from the length on: the garbage test sets those bits on purpose)
    rnd = rng.integers(0, 256, (60, per, 32), dtype=np.uint8)
    bits = np.unpackbits(rnd.reshape(-1, 32), axis=1, bitorder="little")
    bits[:, length:] = 0
    q[120:180] = gpu.from_numpy(np.packbits(bits, axis=1, bitorder="little").reshape(60, per, 32)).cuda()
    q[4] = 0                                                    # the all-zero query
    gpu.cuda.synchronize()
    return corpus, entries, q.contiguous()


def _oracle_top1(oracle, q_rows, entry_words, length, rg):
    """the key the oracle's best-match loop gives for one packed query"""
    idx, score = oracle.corpus_best_packed(q_rows.view(np.uint64).reshape(-1, 4), entry_words, length, rg if rg else length, nthreads=16)
    return _key(idx, score)


@pytest.mark.parametrize("n_sub", range(1, 9))
def test_uniform_specialised_shape(lb, gpu, oracle, n_sub):
    rng = np.random.default_rng(100 + n_sub)
    corpus, entries, q = _uniform_case(lb, gpu, rng, n_sub, 200, N_UNIFORM)
    q_host = q.cpu().numpy()
    fps = _handles(lb, q_host, 200)
    words = entries.cpu().numpy().view(np.uint64).reshape(N_UNIFORM, n_sub, 4)
    for i, rg in enumerate(RANGES):
        # 1, 7, 8, 9, 17 and 300 queries: across kQueryBatchMax and the top-K groups
        counts = (1, 7, 8, 9, 17, 300) if rg in (0, 119) else (1, 7, 8, 9, 17)
        for n in counts:
            ks = ((1, 10, 1024) if n in (1, 9, 17) else ((10,) if n == 300 and rg == 0 else ()))
            got = _check_all(gpu, lb, corpus, q, fps, n, n_sub, rg, ks, (n_sub, rg, n))
        for j in range(len(got)):                               # (the longest run of this range: every one of its keys)
            assert _dec(got[j]) == _oracle_top1(oracle, q_host[j], words, 200, rg), (n_sub, rg, j)
    # index_base travels into the keys
    base = 1_000_000
    got = _u64(corpus.query_packed_keys_device(q, 9, n_sub, index_base=base))
    assert np.array_equal(got, _expect_top1(gpu, corpus, fps[:9], 0, index_base=base))
    keys, lags = corpus.query_packed_topk_keys_device(q, 9, n_sub, 10, aligned=True, index_base=base)
    wk = gpu.zeros((9, 10), dtype=gpu.int64, device="cuda")
    corpus.query_batch_topk_keys_device(fps[:9], 10, wk, index_base=base)
    wl = corpus.align_keys_device(fps[:9], wk, 10, index_base=base)
    assert np.array_equal(_u64(keys), _u64(wk)) and np.array_equal(lags.cpu().numpy(), wl.cpu().numpy())


# ---- 3. uniform corpus, generic shapes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,n_sub,per", [(64, 5, 5), (199, 5, 5), (200, 5, 3), (200, 5, 9), (200, 12, 12), (200, 4, 4)])
def test_uniform_generic_shapes_and_variants(lb, gpu, oracle, length, n_sub, per):
    rng = np.random.default_rng(length * 31 + n_sub * 7 + per)
    n_entries, n = 20_000, 24
    corpus, entries, q = _uniform_case(lb, gpu, rng, n_sub, length, n_entries, per=per, n_queries=180)
    q_host = q.cpu().numpy()
    fps = _handles(lb, q_host, length)
    words = entries.cpu().numpy().view(np.uint64).reshape(n_entries, n_sub, 4)
    specialised = length == 200 and per == n_sub and n_sub <= 8
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    for variant in (0, 1, 2):
        corpus.set_kernel_variant(variant)
        if variant == 2 and not specialised:                    # fails as the handle path does
            for call in (lambda: corpus.query_packed_keys_device(q, n, per),
                         lambda: corpus.query_packed_topk_keys_device(q, n, per, 3),
                         lambda: corpus.query_batch_keys_device(fps[:n], gpu.zeros(n, dtype=gpu.int64, device="cuda"))):
                with pytest.raises(lb.LBAudioDetectiveError) as e:
                    call()
                assert e.value.status == bad
            continue
        for rg in (0, 1, 33, 120, 1000):
            got = _check_all(gpu, lb, corpus, q, fps, n, per, rg, (1, 10, 1024) if rg in (0, 33) else (10,), (length, n_sub, per, variant, rg))
            for j in range(n):
                assert _dec(got[j]) == _oracle_top1(oracle, q_host[j], words, length, rg), (length, n_sub, per, variant, rg, j)
        _check_all(gpu, lb, corpus, q, fps, 1, per, 0, (1,), (length, n_sub, per, variant, "one query"))
    corpus.set_kernel_variant(0)


# ---- 4. ragged corpus -----------------------------------------------------------------------------------------------------------
N_RAGGED = 2500


@pytest.fixture(scope="module")
def ragged_case(lb, gpu, oracle):
    counts = oracle.synth_ragged_counts(SEED, 0, N_RAGGED, 1, 70)
    packed = lb.synth_ragged_corpus_device(SEED, 0, counts, 200)           # [records, 32] on the device
    corpus = lb.Corpus.ragged(200, N_RAGGED, int(counts.sum()))
    corpus.append_ragged_packed_device(packed, counts)
    flat = lb.unpack_packed(packed.cpu().numpy(), 200)
    return corpus, packed, counts, flat


def _ragged_queries(gpu, rng, packed, counts, per, n):
    """device slices of the records at arbitrary sub-fingerprint offsets (inside an entry where one is long enough, else
    across neighbours), a few of them perturbed, plus random rows"""
    off = np.concatenate([[0], np.cumsum(counts)])
    total = int(off[-1])
    q = gpu.empty((n, per, 32), dtype=gpu.uint8, device="cuda")
    long_enough = np.flatnonzero(counts >= per)
    for i in range(n):
        if i % 4 == 3:
            rnd = rng.integers(0, 256, (per, 32), dtype=np.uint8)
            rnd[:, 25:] = 0
            q[i] = gpu.from_numpy(rnd).cuda()
            continue
        if len(long_enough) and i % 4 != 2:
            e = int(rng.choice(long_enough))
            at = int(off[e]) + int(rng.integers(0, counts[e] - per + 1))
        else:
            at = int(rng.integers(0, total - per + 1))
        q[i] = packed[at:at + per]
        if i % 8 == 5:
            q[i, int(rng.integers(0, per)), int(rng.integers(0, 25))] ^= 0x5A
    return q.contiguous()


@pytest.mark.parametrize("per", (1, 5, 7, 8, 10, 12, 21, 48, 100))
def test_ragged(lb, gpu, oracle, ragged_case, per):
    corpus, packed, counts, flat = ragged_case
    rng = np.random.default_rng(1000 + per)
    n = 67                                                       # not a multiple of any launch's share
    q = _ragged_queries(gpu, rng, packed, counts, per, n)
    q_host = q.cpu().numpy()
    fps = _handles(lb, q_host, 200)
    q_bools = lb.unpack_packed(q_host.reshape(-1, 32), 200).reshape(n, per, 200)
    try:
        for variant in (0, 3, 4):
            corpus.set_kernel_variant(variant)
            for pruning in (True, False):
                corpus.set_bound_pruning(pruning)
                for rg in ((0, 119) if variant == 0 else (0,)):
                    what = (per, variant, pruning, rg)
                    got = _check_all(gpu, lb, corpus, q, fps, n, per, rg, (1, 10, 1024) if (variant == 0 and pruning and rg == 0) else (), what)
                    if variant == 0 and pruning:
                        for j in range(64 if rg == 0 else 8):    # 64 queries per shape against the oracle (and a few at the other range)
                            idx, score = oracle.corpus_best_ragged(q_bools[j], (flat, counts), rg if rg else 200, nthreads=16)
                            assert _dec(got[j]) == _key(idx, score), (what, j, idx, score)
                    # several batch sizes: 1, 2, 3, 8, 13 queries (every launch share and a remainder)
                    for m in (1, 2, 3, 8, 13):
                        part = _u64(corpus.query_packed_keys_device(q, m, per, range_=rg))
                        assert np.array_equal(part, got[:m]), (what, m)
        corpus.set_kernel_variant(0)
        corpus.set_bound_pruning(True)
        # top-K with lags on a smaller batch in the other settings, and an index base
        for variant, pruning in ((3, True), (4, False)):
            corpus.set_kernel_variant(variant)
            corpus.set_bound_pruning(pruning)
            _check_all(gpu, lb, corpus, q, fps, 9, per, 0, (10,), (per, variant, pruning, "top-K"))
        corpus.set_kernel_variant(0)
        corpus.set_bound_pruning(True)
        got = _u64(corpus.query_packed_keys_device(q, 13, per, index_base=77))
        assert np.array_equal(got, _expect_top1(gpu, corpus, fps[:13], 0, index_base=77))
    finally:
        corpus.set_kernel_variant(0)
        corpus.set_bound_pruning(True)


def test_ragged_mixed_lengths_back_to_back(lb, gpu, oracle, ragged_case):
    """calls of different query lengths one after the other, nothing awaited in between: every call rebuilds the blocks (and
    where the task kernel runs, the plan) behind the previous call's scans"""
    corpus, packed, counts, flat = ragged_case
    rng = np.random.default_rng(5)
    lengths = (21, 5, 48, 12, 100, 1, 21, 8, 30)
    qs = [_ragged_queries(gpu, rng, packed, counts, per, 11) for per in lengths]
    gpu.cuda.synchronize()
    outs = [corpus.query_packed_keys_device(q, 11, per) for q, per in zip(qs, lengths)]
    tops = [corpus.query_packed_topk_keys_device(q, 5, per, 4, aligned=True) for q, per in zip(qs, lengths)]
    gpu.cuda.synchronize()
    for q, per, keys, (tk, tl) in zip(qs, lengths, outs, tops):
        fps = _handles(lb, q.cpu().numpy(), 200)
        assert np.array_equal(_u64(keys), _expect_top1(gpu, corpus, fps, 0)), per
        wk, wl = _expect_topk(gpu, corpus, fps[:5], 4, 0)
        assert np.array_equal(_u64(tk), wk) and np.array_equal(tl.cpu().numpy(), wl), per


def test_ragged_empty_corpus_gives_zero_keys_and_lags(lb, gpu):
    corpus = lb.Corpus.ragged(200, 10, 100)
    uniform = lb.Corpus(200, 5, 10)
    q = gpu.full((3, 5, 32), 0xFF, dtype=gpu.uint8, device="cuda")
    for c in (corpus, uniform):
        keys = gpu.full((3,), -1, dtype=gpu.int64, device="cuda")
        c.query_packed_keys_device(q, 3, 5, keys_out=keys)
        tk = gpu.full((3, 4), -1, dtype=gpu.int64, device="cuda")
        tl = gpu.full((3, 4), -1, dtype=gpu.int32, device="cuda")
        c.query_packed_topk_keys_device(q, 3, 5, 4, keys_out=tk, lags_out=tl)
        gpu.cuda.synchronize()
        assert not keys.any() and not tk.any() and not tl.any()


# ---- 5. garbage bits ------------------------------------------------------------------------------------------------------------
def test_bits_beyond_the_length_change_nothing(lb, gpu, oracle, ragged_case):
    rng = np.random.default_rng(77)
    for length, n_sub in ((200, 5), (199, 5), (64, 3)):
        corpus, entries, q = _uniform_case(lb, gpu, rng, n_sub, length, 20_000, n_queries=180)
        dirty = gpu.from_numpy(_garbage(rng, q.cpu().numpy(), length)).cuda()
        assert not gpu.equal(dirty, q)
        for variant in (0, 1):
            corpus.set_kernel_variant(variant)
            for rg in (0, 33):
                assert gpu.equal(corpus.query_packed_keys_device(q, 40, n_sub, range_=rg), corpus.query_packed_keys_device(dirty, 40, n_sub, range_=rg))
                a = corpus.query_packed_topk_keys_device(q, 17, n_sub, 10, aligned=True, range_=rg)
                b = corpus.query_packed_topk_keys_device(dirty, 17, n_sub, 10, aligned=True, range_=rg)
                assert gpu.equal(a[0], b[0]) and gpu.equal(a[1], b[1])
    corpus, packed, counts, flat = ragged_case
    for per in (5, 12, 21):
        q = _ragged_queries(gpu, rng, packed, counts, per, 20)
        dirty = gpu.from_numpy(_garbage(rng, q.cpu().numpy(), 200)).cuda()
        assert gpu.equal(corpus.query_packed_keys_device(q, 20, per), corpus.query_packed_keys_device(dirty, 20, per))
        a = corpus.query_packed_topk_keys_device(q, 9, per, 10, aligned=True)
        b = corpus.query_packed_topk_keys_device(dirty, 9, per, 10, aligned=True)
        assert gpu.equal(a[0], b[0]) and gpu.equal(a[1], b[1])


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------
def test_identify_clips_end_to_end(lb, gpu, oracle):
    rate, window, n_clips, n_synth = 44100, 1024, 4096, 1_000_000
    det = lb.Detective().configure(sample_rate=rate, window=window, stride=64)
    clips = lb.synth_clips_device(SEED, 0, n_clips, rate, rate)                 # one second each
    own = det.fingerprint_clips_device(clips)
    per = own.shape[1]
    assert per == 5
    corpus = lb.Corpus(200, per, n_synth + n_clips)
    synth = lb.synth_corpus_device(SEED + 1, 0, n_synth, per, 200)
    corpus.append_packed_device(synth)
    corpus.append_packed_device(own)                                            # straight from the fingerprint output
    keys, lags = lb.identify_clips_device(det, corpus, clips, k=3, aligned=True)
    gpu.cuda.synchronize()
    assert keys.shape == (n_clips, 3) and keys.dtype == gpu.int64 and lags.shape == (n_clips, 3) and lags.dtype == gpu.int32
    own_host = own.cpu().numpy()
    # every clip finds its own entry at score 1.0 -- where two clips share a fingerprint, the lower index of the twins
    _, first, inverse = np.unique(own_host.reshape(n_clips, -1), axis=0, return_index=True, return_inverse=True)
    lowest = first[inverse.reshape(-1)]
    gk = _u64(keys)
    for i in range(n_clips):
        idx, sc = lb.decode_topk_keys(gk[i].view(np.int64))
        assert len(idx) >= 1 and idx[0] == n_synth + lowest[i] and sc[0] == np.float32(1.0), (i, idx, sc)
    assert not lags.cpu().numpy()[:, 0].any()                                   # equal lengths: lag 0
    # the handle path, all 4096
    fps = _handles(lb, own_host, 200)
    wk, wl = _expect_topk(gpu, corpus, fps, 3, 0)
    assert np.array_equal(gk, wk) and np.array_equal(lags.cpu().numpy(), wl)
    plain = lb.identify_clips_device(det, corpus, clips, k=1)
    assert plain.shape == (n_clips, 1) and np.array_equal(_u64(plain)[:, 0], gk[:, 0])
    # the oracle, the first 64: fingerprints and best match
    want_bits = oracle.fingerprint_batch(clips[:64].cpu().numpy(), oracle.Config(rate, window))
    assert np.array_equal(lb.unpack_packed(own_host[:64].reshape(-1, 32), 200).reshape(64, per, 200), want_bits)
    words = np.concatenate([synth.cpu().numpy().view(np.uint64).reshape(n_synth, per, 4), own_host.view(np.uint64).reshape(n_clips, per, 4)])
    for i in range(64):
        idx, score = oracle.corpus_best_packed(oracle.pack_bools(want_bits[i]), words, 200, 200, nthreads=16)
        assert _dec(gk[i, 0]) == _key(idx, score), (i, idx, score)


# ---- 7. ordering ------------------------------------------------------------------------------------------------------------------
# The threshold of the calls below, fixed against the oracle's scores of these corpora and query sets on the CPU: for any value in
# 0.64 .. 0.98 every row that is a copy of a corpus entry has 1 .. 8 entries at or above it (its own at 1.0, or just below where a
# byte was perturbed; a planted duplicate; at most 3 in all), and no row has more than 8.  The largest 9th-best score of any row
# is 0.6263.  The rows that are no copies -- random rows, the all-zero query, ragged slices across two entries -- find little or
# nothing (the best score of a random row lies below other rows' 9th-best): no single threshold gives every row of the full
# sets a match without cutting other rows' lists, so those rows check the empty answer.
THRESHOLD = 0.66


def test_packed_calls_back_to_back_on_two_streams(lb, gpu, oracle, ragged_case):
    rng = np.random.default_rng(9)
    u_corpus, entries, uq = _uniform_case(lb, gpu, rng, 5, 200, N_UNIFORM)
    r_corpus, packed, counts, flat = ragged_case
    rq_small = _ragged_queries(gpu, rng, packed, counts, 21, 5)
    rq_big = _ragged_queries(gpu, rng, packed, counts, 21, 61)
    gpu.cuda.synchronize()
    s1, s2 = gpu.cuda.Stream(), gpu.cuda.Stream()
    # which rows of the full sets are copies of corpus entries (perturbed in a byte at most): all of the uniform set but the
    # all-zero query and the random rows (_uniform_case), and the ragged rows cut from inside one entry (_ragged_queries)
    u_drawn = np.ones(uq.shape[0], bool)
    u_drawn[4] = False
    u_drawn[120:180] = False
    r_drawn = np.arange(rq_big.shape[0]) % 4 < 2
    for corpus, small, big, per, drawn in ((u_corpus, uq[:3].contiguous(), uq, 5, u_drawn), (r_corpus, rq_small, rq_big, 21, r_drawn)):
        n_small, n_big = small.shape[0], big.shape[0]
        fps_small = _handles(lb, small.cpu().numpy(), 200)
        fps_big = _handles(lb, big.cpu().numpy(), 200)
        # a small call, then a larger one (the scratch grows) on another stream, then a small one again, nothing awaited.  Between
        # the small and the larger top-K call the threshold calls, which share the score rows, the key words and the events with
        # them: the handle form on the other stream, then the packed form with lags (and a larger scratch) on the first again
        with gpu.cuda.stream(s1):
            a = corpus.query_packed_topk_keys_device(small, n_small, per, 4, aligned=True, stream=s1)
        with gpu.cuda.stream(s2):
            t1 = corpus.query_batch_threshold_keys_device(fps_small, THRESHOLD, 8, stream=s2)
        with gpu.cuda.stream(s1):
            t2 = corpus.query_packed_threshold_keys_device(big, n_big, per, THRESHOLD, 8, aligned=True, stream=s1)
        with gpu.cuda.stream(s2):
            b = corpus.query_packed_topk_keys_device(big, n_big, per, 4, aligned=True, stream=s2)
            b1 = corpus.query_packed_keys_device(big, n_big, per, stream=s2)
        with gpu.cuda.stream(s1):
            c = corpus.query_packed_keys_device(small, n_small, per, stream=s1)
        # ... and a handle-taking call behind them
        want_small = _expect_top1(gpu, corpus, fps_small, 0)
        gpu.cuda.synchronize()
        wk, wl = _expect_topk(gpu, corpus, fps_small, 4, 0)
        assert np.array_equal(_u64(a[0]), wk) and np.array_equal(a[1].cpu().numpy(), wl)
        wk, wl = _expect_topk(gpu, corpus, fps_big, 4, 0)
        assert np.array_equal(_u64(b[0]), wk) and np.array_equal(b[1].cpu().numpy(), wl)
        assert np.array_equal(_u64(b1), _expect_top1(gpu, corpus, fps_big, 0))
        assert np.array_equal(_u64(c), want_small)
        # the threshold calls: the same calls made alone
        w1 = corpus.query_batch_threshold_keys_device(fps_small, THRESHOLD, 8)
        gpu.cuda.synchronize()
        w2 = corpus.query_packed_threshold_keys_device(big, n_big, per, THRESHOLD, 8, aligned=True)
        gpu.cuda.synchronize()
        for got, want, rows in ((t1, w1, drawn[:n_small]), (t2, w2, drawn)):
            counts = _u64(want[1])
            # every row that was drawn from the corpus finds its own entry, and no list is cut
            assert counts.shape == rows.shape and (counts[rows] >= 1).all() and (counts <= 8).all(), counts
            for g, w in zip(got, want):
                assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.cpu().numpy(), w.cpu().numpy())
