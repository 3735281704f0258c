"""GPU tests of the recording-scores calls (LBAudioDetectiveCorpusRecordingScoresDevice, ...RecordingPackedScoresDevice,
...QueryRecordingTopK, ...QueryPackedRecordingTopKKeysDevice, ...QueryPackedRecordingThresholdKeysDevice).  Every expected value
is numpy (align_ref.align for EVERY entry) or the output of a call that existed before (scores_device, align_keys_device,
query_packed_topk_keys_device, query_packed_threshold_keys_device); scores are compared as bits, lags, keys and counts exactly:
nothing needs a tolerance.  Output buffers are poison-filled before every call.  The corpus is test_gpu_occurrences.py's (its
helpers are copied, not imported) and, like the oracle's answers, made once per module."""
import os
import re

import numpy as np
import pytest

from align_ref import align

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
POISONF = -12345.0
L = 200
N_CASE = 2 * 256 + 5
N_PREFIX = 70


def _source(name):
    return open(os.path.join(ROOT, name)).read()


def _constant(name):
    return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name,
                         _source(os.path.join("lbaudiodetective_amd", "csrc", "k_occurrences.hip"))).group(1))


TILE = _constant("kOcKeep")          # offsets of a tile
BLOCK = _constant("kOcBlock")        # entries a chunk is a multiple of
GROUP = 4 * TILE                     # offsets of an entry a workgroup takes
CAP = int(re.search(r"^#define\s+LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS\s+(\d+)", _source(os.path.join("include", "lbaudiodetective.h")),
                    re.M).group(1))

# where the fixed entries lie (all inside the 70-entry prefix)
E1, E17, E22, E40, E63, E64, E65, EZERO, EDOUBLE, E150, E300, ENOISY, ECONST = 3, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47


def _random(oracle, seed, counts, length=L):
    counts = np.asarray(counts, np.uint32)
    flat = oracle.synth_ragged_entries(seed, 0, counts, length)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [flat[off[i]:off[i + 1]].copy() for i in range(len(counts))]


def _packed(oracle, flat):
    return np.ascontiguousarray(oracle.pack_bools(flat)).view(np.uint8).reshape(len(flat), 32)


def _ragged(lb, gpu, oracle, entries, length=L):
    counts = np.array([len(e) for e in entries], np.uint32)
    c = lb.Corpus.ragged(length, max(1, len(entries)), max(1, int(counts.sum())))
    if len(entries):
        c.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, np.concatenate(entries))).cuda(), counts)
    return c


def _entries(oracle):
    rng = np.random.default_rng(11)
    e = _random(oracle, 4242, rng.integers(1, 41, N_CASE))
    pool = _random(oracle, 4343, [1, 17, 22, 40, 63, 64, 65, 20, 150, 300])
    e[E1], e[E17], e[E22], e[E40], e[E63], e[E64], e[E65] = pool[:7]
    e[EZERO] = np.zeros((10, L), np.uint8)
    e[EDOUBLE] = np.concatenate([pool[7], pool[7]])              # the same 20-block twice
    e[E150], e[E300] = pool[8], pool[9]                          # longer than most queries: case A; the 22 twice inside each
    e[E150][33:55] = pool[2]
    e[E150][100:122] = pool[2]
    e[E300][10:32] = pool[2]
    e[E300][250:272] = pool[2]
    e[ENOISY] = pool[2].copy()                                   # a 700-flip noisy copy of the 22
    e[ENOISY].reshape(-1)[rng.choice(22 * L, 700, replace=False)] ^= 1
    e[ECONST] = np.repeat(pool[0], 5, axis=0)                    # ONE sub-fingerprint five times: plateaus over neighbouring offsets
    return e, pool[7]


def _queries(oracle, e, block20):
    """name -> (Booleans, entries of the corpus it runs against)"""
    r = _random(oracle, 777, [1, 17, 41, 129, 300, 700, 2500, 300, 525, 525])
    q129, q300, q700, q2500, q300b, q525, q525b = r[3], r[4], r[5], r[6], r[7], r[8], r[9]
    q129[0:22] = e[E22]                                          # the same cell of 1.0 at the first offset ...
    q129[107:129] = e[E22]                                       # ... and at the last offset of the 22's profile
    q300[127:149] = e[E22]
    q300[150:172] = e[E22]
    q300[128:145] = e[E17]                                       # (on top of the first 22: two plants whose profiles overlap)
    q700[10:32] = e[E22]                                         # two cells of 1.0 in different tile groups
    q700[600:622] = e[E22]
    q700[200:260] = np.concatenate([block20] * 3)                # the 40 of EDOUBLE at 200 and at 220
    q700[301:309] = np.repeat(e[ECONST][:1], 8, axis=0)          # cells 301 .. 304 of ECONST are 1.0: 301 and 302 are ONE lane's
    q2500[1234:1256] = e[E22]
    q300b[TILE:TILE + 22] = e[E22]                               # the first cell of tile 1 and the last cell of tile 1
    q300b[2 * TILE - 1:2 * TILE + 21] = e[E22]
    q525[GROUP - 1:GROUP + 21] = e[E22]                          # 504 offsets against the 22: the last cell of the first group
    q525b[GROUP:GROUP + 17] = e[E17]                             # 509 offsets against the 17: the first cell of the second group
    return {"q1": (r[0], N_CASE), "q17": (r[1], N_CASE), "q41": (r[2], N_CASE), "q129": (q129, N_CASE), "q300": (q300, N_CASE),
            "q700": (q700, N_CASE), "q2500": (q2500, N_PREFIX), "q22": (e[E22].copy(), N_CASE), "q300b": (q300b, N_CASE),
            "q525": (q525, N_CASE), "q525b": (q525b, N_CASE), "qzero": (np.zeros((30, L), np.uint8), N_CASE)}


_M = {}


def _module(lb, gpu, oracle):
    if not _M:
        e, block20 = _entries(oracle)
        _M["entries"] = e
        _M["queries"] = _queries(oracle, e, block20)
        _M["corpus"] = {N_CASE: _ragged(lb, gpu, oracle, e), N_PREFIX: _ragged(lb, gpu, oracle, e[:N_PREFIX])}
        _M["aligned"] = {}
        _M["fp"] = {}
    return _M


def _aligned(m, name, range_=0):
    """the oracle's (scores float32 [n], lags int32 [n]) of query `name` against every entry of its corpus, made once"""
    if (name, range_) not in m["aligned"]:
        q, n = m["queries"][name]
        got = [align(q, ent, range_) for ent in m["entries"][:n]]
        m["aligned"][(name, range_)] = (np.array([g[0] for g in got], np.float32), np.array([g[1] for g in got], np.int32))
    return m["aligned"][(name, range_)]


def _fp(lb, m, name):
    if name not in m["fp"]:
        m["fp"][name] = lb.Fingerprint.from_bools(m["queries"][name][0])
    return m["fp"][name]


def _dev_packed(gpu, oracle, m, name):
    return gpu.from_numpy(_packed(oracle, m["queries"][name][0])).cuda()


def _scores(gpu, corpus, fp=None, packed=None, per=0, range_=0, want_lags=True, stream=None, n=None):
    """one per-entry call into poison-filled buffers -> (scores float32 [n], lags int32 [n] or None)"""
    n = len(corpus) if n is None else n
    scores = gpu.full((max(1, n),), POISONF, dtype=gpu.float32, device="cuda")
    lags = gpu.full((max(1, n),), POISON32, dtype=gpu.int32, device="cuda") if want_lags else None
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    corpus.recording_scores_device(fp=fp, packed=packed, per_query=per, range_=range_, scores_out=scores, lags_out=lags,
                                   want_lags=want_lags, stream=stream)
    (stream or gpu.cuda.current_stream()).synchronize()
    return scores.cpu().numpy(), lags.cpu().numpy() if want_lags else None


def _same(got, want):
    """scores as bits, lags exactly"""
    assert np.array_equal(got[0].view(np.uint32), np.asarray(want[0], np.float32).view(np.uint32))
    if got[1] is not None:
        assert np.array_equal(got[1], want[1])


def _existing(gpu, corpus, fp, range_=0):
    """the calls that existed before: scores_device, and align_keys_device for the key of EVERY entry"""
    n = len(corpus)
    scores = corpus.scores_device(fp, range_).cpu().numpy()
    keys = (scores.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64))
    lags = corpus.align_keys_device([fp], gpu.from_numpy(keys.view(np.int64)).cuda().reshape(1, n), n, range_=range_)
    return scores, lags.cpu().numpy().reshape(n)


# ---- 1. the per-entry form against the oracle and against the calls that exist ------------------------------------------------
@pytest.mark.parametrize("name", ["q1", "q17", "q22", "q41", "q129", "q300", "q300b", "q525", "q525b", "q700", "q2500"])
def test_scores_and_lags_equal_the_oracle_and_the_existing_calls(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"][m["queries"][name][1]]
    got = _scores(gpu, corpus, _fp(lb, m, name))
    _same(got, _aligned(m, name))
    _same(got, _existing(gpu, corpus, _fp(lb, m, name)))


def test_the_shapes_are_the_seams(lb, gpu, oracle):
    """the oracle's own pairs: one offset, one tile, 126 / 127 offsets, 504 / 505, more than one group, both cases, equal lengths"""
    m = _module(lb, gpu, oracle)
    lengths = np.array([len(x) for x in m["entries"]])

    def offsets(nq):
        return set(np.abs(lengths - nq) + 1)

    assert 1 in offsets(17) and {TILE, TILE + 1} <= offsets(129) and {GROUP, GROUP + 1} <= offsets(525)
    assert max(offsets(700)) > GROUP and max(offsets(300)) > TILE
    assert (lengths > 41).any() and (lengths < 41).any() and (lengths == 17).any() and (lengths == 22).any()


# ---- 2. ties go to the lowest offset ----------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_offset(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"][N_CASE]
    one = np.float32(1.0).view(np.uint32)
    for name, entry, lag in (("q129", E22, 0),            # the 22 at offsets 0 and 107: the ends of ONE tile (108 offsets)
                             ("q700", E22, -10),          # at 10 and 600: different tiles AND different groups
                             ("q300b", E22, -TILE),       # at the first and at the last cell of tile 1
                             ("q700", EDOUBLE, -200),     # the 20-block three times in a row: the 40 at 200 and 220
                             ("q700", ECONST, -301),      # a plateau 301 .. 304: cells 301 and 302 are one lane's
                             ("q525", E22, -(GROUP - 1)), ("q525b", E17, -GROUP),
                             ("q22", E150, 33), ("q22", E300, 10)):      # case A: the 22 twice inside a longer entry
        want = _aligned(m, name)
        assert want[0][entry] == 1.0 and want[1][entry] == lag, (name, entry)      # (the oracle itself)
        scores, lags = _scores(gpu, corpus, _fp(lb, m, name))
        assert scores[entry].view(np.uint32) == one and lags[entry] == lag, (name, entry, scores[entry], lags[entry])


# ---- 3. zeros ---------------------------------------------------------------------------------------------------------------------
def test_zero_query_and_zero_entry(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"][N_CASE]
    scores, lags = _scores(gpu, corpus, _fp(lb, m, "qzero"))
    assert not scores.view(np.uint32).any() and not lags.any()             # +0.0 bits, lag 0
    keys, klags = corpus.query_packed_recording_topk_keys_device(_dev_packed(gpu, oracle, m, "qzero"), 30, 10)
    gpu.cuda.synchronize()
    assert not keys.cpu().numpy().any() and not klags.cpu().numpy().any()
    idx, sc, lg = corpus.query_recording_topk(_fp(lb, m, "qzero"), 10)
    assert len(idx) == 0 and len(sc) == 0 and len(lg) == 0
    for name in ("q41", "q300"):
        scores, lags = _scores(gpu, corpus, _fp(lb, m, name))
        assert scores[EZERO].view(np.uint32) == 0 and lags[EZERO] == 0
        keys, _ = corpus.query_packed_recording_topk_keys_device(_dev_packed(gpu, oracle, m, name), len(m["queries"][name][0]), 1024)
        gpu.cuda.synchronize()
        assert EZERO not in lb.decode_topk_keys(keys)[0]


# ---- 4. ranges and an odd sub-fingerprint length -------------------------------------------------------------------------------------
@pytest.mark.parametrize("range_", [63, 64, 65, 199])
def test_ranges(lb, gpu, oracle, range_):
    m = _module(lb, gpu, oracle)
    for name in ("q300", "q22"):                                  # the masked instances, case B and case A
        got = _scores(gpu, m["corpus"][N_CASE], _fp(lb, m, name), range_=range_)
        _same(got, _aligned(m, name, range_))
        _same(got, _existing(gpu, m["corpus"][N_CASE], _fp(lb, m, name), range_))


def test_odd_subfingerprint_length(lb, gpu, oracle):
    """sub-fingerprints of 199 Booleans: both cases, the full range and a shorter one"""
    rng = np.random.default_rng(5)
    ent = _random(oracle, 99, rng.integers(1, 41, 60), 199)
    ent[5] = _random(oracle, 98, [90], 199)[0]
    q = _random(oracle, 97, [64], 199)[0]
    q[20:20 + len(ent[9])] = ent[9]
    ent[5][20:20 + 64] = q                                        # case A: the query inside a longer entry
    corpus = _ragged(lb, gpu, oracle, ent, 199)
    fp = lb.Fingerprint.from_bools(q)
    for range_ in (0, 20):
        want = [align(q, x, range_) for x in ent]
        want = (np.array([w[0] for w in want], np.float32), np.array([w[1] for w in want], np.int32))
        assert range_ or (want[0][5] == 1.0 and want[1][5] == 20 and want[0][9] == 1.0 and want[1][9] == -20)
        got = _scores(gpu, corpus, fp, range_=range_)
        _same(got, want)
        _same(got, _existing(gpu, corpus, fp, range_))


# ---- 5. packed, handle and host forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q17", "q300", "q22"])
def test_packed_handle_and_host_forms_agree(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    q, n = m["queries"][name]
    corpus, packed = m["corpus"][n], _dev_packed(gpu, oracle, m, name)
    a = _scores(gpu, corpus, _fp(lb, m, name))
    b = _scores(gpu, corpus, packed=packed, per=len(q))
    _same(a, _aligned(m, name))
    _same(b, a)
    for k in (1, 7):
        keys, lags = corpus.query_packed_recording_topk_keys_device(packed, len(q), k)
        gpu.cuda.synchronize()
        want_idx, want_sc = lb.decode_topk_keys(keys)
        idx, sc, lg = corpus.query_recording_topk(_fp(lb, m, name), k)
        assert len(idx) == len(want_idx) == k
        assert np.array_equal(idx, want_idx) and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))
        assert np.array_equal(lg, lags.cpu().numpy()[:k]) and np.array_equal(lg, a[1][idx])
        assert np.array_equal(sc.view(np.uint32), a[0][idx].view(np.uint32))
    # the host form without lags
    C, N = lb._native.C, lb._native
    idx = np.full(3, -1, np.int64)
    sc = np.zeros(3, np.float32)
    cnt = N.UInt32(0)
    st = lb.lib().LBAudioDetectiveCorpusQueryRecordingTopK(corpus._ref, _fp(lb, m, name)._ref, 0, 3, idx.ctypes.data_as(C.POINTER(N.SInt64)),
                                                           sc.ctypes.data_as(C.POINTER(N.Float32)), None, C.byref(cnt))
    assert st == 0 and cnt.value == 3 and np.array_equal(idx, corpus.query_topk(_fp(lb, m, name), 3)[0])


# ---- 6. outLags == NULL -----------------------------------------------------------------------------------------------------------------
def test_no_lags_changes_nothing(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    for name in ("q129", "q22"):
        got = _scores(gpu, m["corpus"][N_CASE], _fp(lb, m, name), want_lags=False)
        assert got[1] is None
        _same(got, _aligned(m, name))


# ---- 7. the top-K form against the top-K query that exists ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q41", "q300", "q22"])
def test_topk_form_equals_the_packed_topk_query(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    q, n = m["queries"][name]
    corpus, packed = m["corpus"][n], _dev_packed(gpu, oracle, m, name)
    positive = int(np.count_nonzero(_aligned(m, name)[0] > 0))
    assert positive < 1024                                        # K = 1024 is above the entries with score > 0
    for base in (0, (1 << 32) - n):
        for k in (1, 10, 1024):
            want_keys, want_lags = corpus.query_packed_topk_keys_device(packed, 1, len(q), k, aligned=True, index_base=base)
            keys = gpu.full((k,), POISON, dtype=gpu.int64, device="cuda")
            lags = gpu.full((k,), POISON32, dtype=gpu.int32, device="cuda")
            corpus.query_packed_recording_topk_keys_device(packed, len(q), k, index_base=base, keys_out=keys, lags_out=lags)
            gpu.cuda.synchronize()
            assert np.array_equal(keys.cpu().numpy(), want_keys.cpu().numpy().reshape(k))
            assert np.array_equal(lags.cpu().numpy(), want_lags.cpu().numpy().reshape(k))
            assert np.count_nonzero(keys.cpu().numpy()) == min(k, positive)
            no_lags = gpu.full((k,), POISON, dtype=gpu.int64, device="cuda")
            corpus.query_packed_recording_topk_keys_device(packed, len(q), k, index_base=base, keys_out=no_lags, want_lags=False)
            gpu.cuda.synchronize()
            assert np.array_equal(no_lags.cpu().numpy(), keys.cpu().numpy())
    with pytest.raises(lb.LBAudioDetectiveError) as err:
        corpus.query_packed_recording_topk_keys_device(packed, len(q), 4, index_base=(1 << 32) - n + 1)
    assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")


def test_k_1_is_the_top1_query(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    q, n = m["queries"]["q129"]
    packed = _dev_packed(gpu, oracle, m, "q129")
    keys, _ = m["corpus"][n].query_packed_recording_topk_keys_device(packed, len(q), 1)
    top1 = m["corpus"][n].query_packed_keys_device(packed, 1, len(q))
    gpu.cuda.synchronize()
    assert keys.cpu().numpy()[0] == top1.cpu().numpy()[0]


# ---- 8. the threshold form against the threshold query that exists -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q41", "q300", "q22"])
def test_threshold_form_equals_the_packed_threshold_query(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    q, n = m["queries"][name]
    corpus, packed = m["corpus"][n], _dev_packed(gpu, oracle, m, name)
    scores = _aligned(m, name)[0]
    distinct = np.unique(scores)
    assert len(distinct) >= 4
    for what, t in (("max", distinct[-1]), ("4th", distinct[-4]), ("above", np.nextafter(distinct[-1], np.float32(np.inf)))):
        total = int(np.count_nonzero(scores >= np.float32(t)))
        assert (total == 0) == (what == "above")
        for capacity in sorted({max(1, total // 2), total + 3}):  # one that cuts the list, one that does not
            for base in (0, (1 << 32) - n):
                want_keys, want_counts, want_lags = corpus.query_packed_threshold_keys_device(packed, 1, len(q), float(t), capacity,
                                                                                              aligned=True, index_base=base)
                keys = gpu.full((capacity,), POISON, dtype=gpu.int64, device="cuda")
                lags = gpu.full((capacity,), POISON32, dtype=gpu.int32, device="cuda")
                count = gpu.full((1,), POISON, dtype=gpu.int64, device="cuda")
                corpus.query_packed_recording_threshold_keys_device(packed, len(q), float(t), capacity, index_base=base, keys_out=keys,
                                                                    lags_out=lags, count_out=count)
                gpu.cuda.synchronize()
                assert int(count.cpu().numpy()[0]) == int(want_counts.cpu().numpy()[0]) == total
                assert np.array_equal(keys.cpu().numpy(), want_keys.cpu().numpy().reshape(capacity))
                assert np.array_equal(lags.cpu().numpy(), want_lags.cpu().numpy().reshape(capacity))
                no_lags, _, count2 = corpus.query_packed_recording_threshold_keys_device(packed, len(q), float(t), capacity,
                                                                                         index_base=base, want_lags=False)
                gpu.cuda.synchronize()
                assert np.array_equal(no_lags.cpu().numpy(), keys.cpu().numpy()) and int(count2.cpu().numpy()[0]) == total


# ---- 9. chunking ------------------------------------------------------------------------------------------------------------------------
def _scratch_bytes(entries, tiles):
    """the header's formula"""
    return entries * tiles * 8


def test_chunks_change_nothing(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus, fp = m["corpus"][N_CASE], _fp(lb, m, "q300")
    packed = _dev_packed(gpu, oracle, m, "q300")
    lengths = np.array([len(x) for x in m["entries"]])
    tiles = -(-int((np.abs(lengths - 300) + 1).max()) // TILE)
    assert tiles == 3
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    try:
        corpus.set_join_scratch_limit(0)
        one = _scores(gpu, corpus, fp)
        _same(one, _aligned(m, "q300"))
        keys1, lags1 = corpus.query_packed_recording_topk_keys_device(packed, 300, 10)
        gpu.cuda.synchronize()
        for chunk, extra in ((3 * BLOCK, 0), (3 * BLOCK, BLOCK * tiles * 8 - 1), (BLOCK, 7)):     # three chunks (192, 192, 133), nine
            assert -(-N_CASE // chunk) >= 3 and N_CASE % chunk % BLOCK != 0
            corpus.set_join_scratch_limit(_scratch_bytes(chunk, tiles) + extra)
            _same(_scores(gpu, corpus, fp), one)
            _same(_scores(gpu, corpus, packed=packed, per=300), one)
            keys, lags = corpus.query_packed_recording_topk_keys_device(packed, 300, 10)
            gpu.cuda.synchronize()
            assert np.array_equal(keys.cpu().numpy(), keys1.cpu().numpy()) and np.array_equal(lags.cpu().numpy(), lags1.cpu().numpy())
        corpus.set_join_scratch_limit(_scratch_bytes(BLOCK, tiles) - 1)
        for call in (lambda: _scores(gpu, corpus, fp), lambda: _scores(gpu, corpus, packed=packed, per=300),
                     lambda: corpus.query_recording_topk(fp, 3),
                     lambda: corpus.query_packed_recording_topk_keys_device(packed, 300, 3),
                     lambda: corpus.query_packed_recording_threshold_keys_device(packed, 300, 0.5, 4)):
            with pytest.raises(lb.LBAudioDetectiveError) as err:
                call()
            assert err.value.status == bad
    finally:
        corpus.set_join_scratch_limit(0)


# ---- 10. an entry at the cap --------------------------------------------------------------------------------------------------------------
def test_an_entry_at_the_cap(lb, gpu, oracle):
    """the longest legal entry against queries one shorter (case A, two offsets), equal, one longer and about twice as long: the
    LDS window at its largest"""
    ent = _random(oracle, 8, [5, CAP, 30])
    corpus = _ragged(lb, gpu, oracle, ent)
    for nq in (CAP - 1, CAP, CAP + 1, 2000):
        q = _random(oracle, 9, [nq])[0]
        if nq == 2000:
            q[700:700 + CAP] = ent[1]
        want = [align(q, x, 0) for x in ent]
        want = (np.array([w[0] for w in want], np.float32), np.array([w[1] for w in want], np.int32))
        assert nq != 2000 or (want[0][1] == 1.0 and want[1][1] == -700)
        fp = lb.Fingerprint.from_bools(q)
        got = _scores(gpu, corpus, fp)
        _same(got, want)
        assert np.array_equal(got[0].view(np.uint32), corpus.scores_device(fp).cpu().numpy().view(np.uint32))
    above = _ragged(lb, gpu, oracle, _random(oracle, 5, [3, CAP + 1, 2]))
    fp = lb.Fingerprint.from_bools(_random(oracle, 9, [41])[0])
    packed = gpu.from_numpy(_packed(oracle, _random(oracle, 9, [41])[0])).cuda()
    for call in (lambda: _scores(gpu, above, fp), lambda: _scores(gpu, above, packed=packed, per=41),
                 lambda: above.query_recording_topk(fp, 3), lambda: above.query_packed_recording_topk_keys_device(packed, 41, 3),
                 lambda: above.query_packed_recording_threshold_keys_device(packed, 41, 0.5, 4)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            call()
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")


# ---- 11. refusals and the empty corpus ------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_corpus(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    fp = _fp(lb, m, "q41")
    packed = _dev_packed(gpu, oracle, m, "q41")

    def refused(call):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            call()
        assert err.value.status == bad

    # a uniform corpus
    uniform = lb.Corpus(L, 4, 8)
    refused(lambda: _scores(gpu, uniform, fp, n=8))
    refused(lambda: _scores(gpu, uniform, packed=packed, per=41, n=8))
    refused(lambda: uniform.query_recording_topk(fp, 3))
    refused(lambda: uniform.query_packed_recording_topk_keys_device(packed, 41, 3))
    refused(lambda: uniform.query_packed_recording_threshold_keys_device(packed, 41, 0.5, 4))
    # a query of another sub-fingerprint length
    other = lb.Fingerprint.from_bools(_random(oracle, 6, [5], 100)[0])
    refused(lambda: _scores(gpu, m["corpus"][N_CASE], other))
    refused(lambda: m["corpus"][N_CASE].query_recording_topk(other, 3))
    # an empty corpus: noErr; the scores forms write nothing, the key forms zeros
    empty = lb.Corpus.ragged(L, 4, 16)
    for kw in (dict(fp=fp), dict(packed=packed, per=41)):
        scores, lags = _scores(gpu, empty, n=1, **kw)
        assert scores[0] == np.float32(POISONF) and lags[0] == POISON32
    keys = gpu.full((6,), POISON, dtype=gpu.int64, device="cuda")
    lags = gpu.full((6,), POISON32, dtype=gpu.int32, device="cuda")
    empty.query_packed_recording_topk_keys_device(packed, 41, 6, keys_out=keys, lags_out=lags)
    gpu.cuda.synchronize()
    assert not keys.cpu().numpy().any() and not lags.cpu().numpy().any()
    keys = gpu.full((6,), POISON, dtype=gpu.int64, device="cuda")
    lags = gpu.full((6,), POISON32, dtype=gpu.int32, device="cuda")
    count = gpu.full((1,), POISON, dtype=gpu.int64, device="cuda")
    empty.query_packed_recording_threshold_keys_device(packed, 41, 0.5, 6, keys_out=keys, lags_out=lags, count_out=count)
    gpu.cuda.synchronize()
    assert not keys.cpu().numpy().any() and not lags.cpu().numpy().any() and int(count.cpu().numpy()[0]) == 0
    idx, sc, lg = empty.query_recording_topk(fp, 6)
    assert len(idx) == 0


# ---- 12. two calls in a row on two streams ------------------------------------------------------------------------------------------------
def test_two_streams_in_a_row(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"][N_CASE]
    names = ("q700", "q129")
    streams = [gpu.cuda.Stream(), gpu.cuda.Stream()]
    outs = []
    for s, name in zip(streams, names):                           # the second call is made while the first may still run
        scores = gpu.full((N_CASE,), POISONF, dtype=gpu.float32, device="cuda")
        lags = gpu.full((N_CASE,), POISON32, dtype=gpu.int32, device="cuda")
        s.wait_stream(gpu.cuda.current_stream())
        corpus.recording_scores_device(fp=_fp(lb, m, name), scores_out=scores, lags_out=lags, stream=s)
        outs.append((scores, lags))
    for s in streams:
        s.synchronize()
    for (scores, lags), name in zip(outs, names):
        _same((scores.cpu().numpy(), lags.cpu().numpy()), _aligned(m, name))
    # ... and the key form on both
    packed = [_dev_packed(gpu, oracle, m, name) for name in names]
    single = [corpus.query_packed_recording_topk_keys_device(p, len(m["queries"][name][0]), 10) for p, name in zip(packed, names)]
    gpu.cuda.synchronize()
    outs = []
    for s, p, name in zip(streams, packed, names):
        s.wait_stream(gpu.cuda.current_stream())
        outs.append(corpus.query_packed_recording_topk_keys_device(p, len(m["queries"][name][0]), 10, stream=s))
    for s in streams:
        s.synchronize()
    for (keys, lags), (keys1, lags1) in zip(outs, single):
        assert np.array_equal(keys.cpu().numpy(), keys1.cpu().numpy()) and np.array_equal(lags.cpu().numpy(), lags1.cpu().numpy())
