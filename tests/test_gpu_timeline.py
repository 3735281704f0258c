"""GPU tests of the recording-timeline calls (LBAudioDetectiveCorpusRecordingTimelineKeysDevice,
...RecordingPackedTimelineKeysDevice, ...QueryRecordingTimeline).  Every expected value is numpy (timeline_ref on
align_ref.profile, for EVERY entry) or the output of a call that existed before (query_occurrences_keys_device folded per offset
in numpy); keys are compared as integers, lengths exactly: nothing needs a tolerance.  Output buffers are poison-filled before
every call.  The corpus is test_gpu_recording.py's (its helpers are copied, not imported) with a second copy of the 22 at a higher
index and, like the reference's profiles, made once per module."""
import os
import re

import numpy as np
import pytest

import timeline_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
L = 200
N_CASE = 2 * 256 + 5
N_PREFIX = 70
T_HIGH, T_LOW = 0.7, 0.3


def _source(name):
    return open(os.path.join(ROOT, name)).read()


def _constant(name, file):
    return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name,
                         _source(os.path.join("lbaudiodetective_amd", "csrc", file))).group(1))


TILE = _constant("kOcKeep", "k_occurrences.hip")        # offsets of a tile
GROUP = 4 * TILE                                        # offsets of an entry a workgroup takes
WALK = _constant("kTlEntries", "k_timeline.hip")        # entries a unit walks: a chunk is a multiple of it
FOLD_ROWS = _constant("kTlFoldRows", "k_timeline.hip")  # more entry blocks than this: the fold takes two levels
CAP = int(re.search(r"^#define\s+LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS\s+(\d+)", _source(os.path.join("include", "lbaudiodetective.h")),
                    re.M).group(1))

# where the fixed entries lie (all inside the 70-entry prefix)
E1, E17, E22, E40, E63, E64, E65, EZERO, EDOUBLE, E150, E300, ENOISY, ECONST, EDUP22 = 3, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53


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
    e[E150], e[E300] = pool[8], pool[9]                          # longer than most queries: they take part in q300 .. q2500 only
    e[E150][33:55] = pool[2]
    e[E150][100:122] = pool[2]
    e[E300][10:32] = pool[2]
    e[E300][250:272] = pool[2]
    e[ENOISY] = pool[2].copy()                                   # a 700-flip noisy copy of the 22
    e[ENOISY].reshape(-1)[rng.choice(22 * L, 700, replace=False)] ^= 1
    e[ECONST] = np.repeat(pool[0], 5, axis=0)                    # ONE sub-fingerprint five times: plateaus over neighbouring offsets
    e[EDUP22] = pool[2].copy()                                   # the 22 once more, at a higher index: it loses every tie
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
    q300b[TILE - 1:TILE + 21] = e[E22]                           # offset 125: the last cell of tile 0 (lane 63's first)
    q300b[2 * TILE:2 * TILE + 22] = e[E22]                       # offset 252: the first cell of tile 2 (lane 0's second)
    q300b[TILE + 30:TILE + 47] = e[E17]                          # ... and, clear of both, the 17 at 156
    q525[GROUP - 1:GROUP + 21] = e[E22]                          # 504 offsets against the 22: the last cell of the first group
    q525[TILE + 1:TILE + 23] = e[E22]                            # ... and offset 127
    q525b[GROUP:GROUP + 17] = e[E17]                             # 509 offsets against the 17: the first cell of the second group
    q525b[TILE:TILE + 22] = e[E22]                               # offset 126: the first cell of tile 1
    q525b[TILE + 40:TILE + 62] = e[E22]                          # ... 166, and 127 + 126 = 253 below
    q525b[2 * TILE + 1:2 * TILE + 23] = e[E22]
    return {"q1": (r[0], N_CASE), "q17": (r[1], N_CASE), "q41": (r[2], N_CASE), "q129": (q129, N_CASE), "q300": (q300, N_CASE),
            "q700": (q700, N_CASE), "q2500": (q2500, N_PREFIX), "q22": (e[E22].copy(), N_CASE), "q300b": (q300b, N_CASE),
            "q525": (q525, N_CASE), "q525b": (q525b, N_CASE), "qzero": (np.zeros((30, L), np.uint8), N_CASE)}


# the offsets at which the 22 (and the 17) lie verbatim and undisturbed: cells of 1.0
PLANTS_22 = {"q22": [0], "q129": [0, 107], "q300": [150], "q700": [10, 600], "q2500": [1234], "q300b": [TILE - 1, 2 * TILE],
             "q525": [TILE + 1, GROUP - 1], "q525b": [TILE, TILE + 40, 2 * TILE + 1]}
PLANTS_17 = {"q300": [128], "q300b": [TILE + 30], "q525b": [GROUP]}

_M = {}


def _module(lb, gpu, oracle):
    if not _M:
        e, block20 = _entries(oracle)
        _M["entries"] = e
        _M["lengths"] = np.array([len(x) for x in e], np.int64)
        _M["queries"] = _queries(oracle, e, block20)
        _M["corpus"] = {N_CASE: _ragged(lb, gpu, oracle, e), N_PREFIX: _ragged(lb, gpu, oracle, e[:N_PREFIX])}
        _M["profiles"] = {}
        _M["fp"] = {}
    return _M


def _want(m, name, t, range_=0, base=0):
    """the reference's (keys uint64 [n_q], lengths uint32 [n_q]); the profiles of a (query, range) are made once"""
    q, n = m["queries"][name]
    if (name, range_) not in m["profiles"]:
        m["profiles"][(name, range_)] = timeline_ref.profiles(q, m["entries"][:n], range_)
    return timeline_ref.fold(len(q), m["profiles"][(name, range_)], t, base)


def _fp(lb, m, name):
    if name not in m["fp"]:
        m["fp"][name] = lb.Fingerprint.from_bools(m["queries"][name][0])
    return m["fp"][name]


def _dev_packed(gpu, oracle, m, name):
    return gpu.from_numpy(_packed(oracle, m["queries"][name][0])).cuda()


def _timeline(gpu, corpus, nq, t, fp=None, packed=None, range_=0, base=0, want_lengths=True, stream=None):
    """one call into poison-filled buffers -> (keys uint64 [n_q], lengths uint32 [n_q] or None)"""
    keys = gpu.full((nq,), POISON, dtype=gpu.int64, device="cuda")
    lengths = gpu.full((nq,), POISON32, dtype=gpu.int32, device="cuda") if want_lengths else None
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    corpus.recording_timeline_keys_device(fp=fp, packed=packed, per_query=nq if packed is not None else 0, threshold=t, range_=range_,
                                          index_base=base, keys_out=keys, lengths_out=lengths, want_lengths=want_lengths, stream=stream)
    (stream or gpu.cuda.current_stream()).synchronize()
    return keys.cpu().numpy().view(np.uint64), lengths.cpu().numpy().view(np.uint32) if want_lengths else None


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    if got[1] is not None:
        assert np.array_equal(got[1], want[1])


def _fold_of_occurrences(gpu, corpus, fp, nq, lengths, t, range_=0, base=0):
    """the call that existed before: every cell at or above t, then per offset the largest key among the entries not longer than
    the query -- (keys uint64 [n_q], lengths uint32 [n_q])"""
    capacity = int((np.abs(lengths - nq) + 1).sum()) + 5                       # above the true count: every cell there is
    keys, lags, count = corpus.query_occurrences_keys_device(fp, t, capacity, peaks=False, range_=range_, index_base=base)
    gpu.cuda.synchronize()
    total = int(count.cpu().numpy()[0])
    assert total <= capacity
    k = keys.cpu().numpy().view(np.uint64)[:total]
    lg = lags.cpu().numpy()[:total].astype(np.int64)
    idx = (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64) - base
    inside = lengths[idx] <= nq                                                # (their lags are -offset)
    out = np.zeros(nq, np.uint64)
    np.maximum.at(out, -lg[inside], k[inside])
    won = (np.uint64(0xFFFFFFFF) - (out & np.uint64(0xFFFFFFFF))).astype(np.int64) - base
    return out, np.where(out != 0, lengths[np.where(out != 0, won, 0)], 0).astype(np.uint32)


NAMES = ["q1", "q17", "q22", "q41", "q129", "q300", "q300b", "q525", "q525b", "q700", "q2500"]


# ---- 1. keys and lengths against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_keys_and_lengths_equal_the_reference(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    q, n = m["queries"][name]
    for t in (T_HIGH, T_LOW):
        want = _want(m, name, t)
        _same(_timeline(gpu, m["corpus"][n], len(q), t, fp=_fp(lb, m, name)), want)
        idx, sc = timeline_ref.decode(want[0])
        for plants, entry in ((PLANTS_22, E22), (PLANTS_17, E17)):              # (the reference itself)
            for o in plants.get(name, []):
                assert idx[o] == entry and sc[o] == 1.0 and want[1][o] == len(m["entries"][entry]), (name, o)
    low = _want(m, name, T_LOW)[0]
    if len(q) >= 129:                                             # at the low threshold most offsets have a noise winner
        assert 2 * np.count_nonzero(low) > len(q), np.count_nonzero(low)
        assert len(np.unique(timeline_ref.decode(low)[0])) > 20


def test_the_shapes_are_the_seams(lb, gpu, oracle):
    """plants at the first and last offset of a profile, at 125 / 126 / 127, at the last cell of group 0 and the first of group
    1, in two groups, and two that overlap"""
    m = _module(lb, gpu, oracle)
    assert (TILE, GROUP) == (126, 504)
    assert PLANTS_22["q129"] == [0, 129 - 22] and PLANTS_22["q22"] == [0]
    assert (PLANTS_22["q300b"][0], PLANTS_22["q525b"][0], PLANTS_22["q525"][0]) == (125, 126, 127)
    assert PLANTS_17["q300"] == [128] and np.array_equal(m["queries"]["q300"][0][127], m["entries"][E22][0])     # the 17 inside a 22 at 127
    assert PLANTS_22["q525"][1] == 503 and PLANTS_17["q525b"] == [504] and PLANTS_22["q300b"][1] == 2 * TILE
    assert PLANTS_22["q700"][0] // GROUP != PLANTS_22["q700"][1] // GROUP
    assert len(m["entries"]) > WALK                              # more than one entry block


# ---- 2. keys against the fold of the occurrences call -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_keys_equal_the_fold_of_the_occurrences(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    q, n = m["queries"][name]
    for t in (T_HIGH, T_LOW):
        got = _timeline(gpu, m["corpus"][n], len(q), t, fp=_fp(lb, m, name))
        _same(got, _fold_of_occurrences(gpu, m["corpus"][n], _fp(lb, m, name), len(q), m["lengths"][:n], t))


# ---- 3. ties go to the lower entry ---------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_entry(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    one = int(np.float32(1.0).view(np.uint32))
    assert np.array_equal(m["entries"][E22], m["entries"][EDUP22]) and E22 < EDUP22
    without = _ragged(lb, gpu, oracle, m["entries"])
    assert without.remove([E22]) == 1
    for name in ("q129", "q700", "q300b", "q525", "q525b"):
        q, n = m["queries"][name]
        keys, lengths = _timeline(gpu, m["corpus"][n], len(q), T_HIGH, fp=_fp(lb, m, name))
        keys2, lengths2 = _timeline(gpu, without, len(q), T_HIGH, fp=_fp(lb, m, name))
        for o in PLANTS_22[name]:
            assert keys[o] == (one << 32) | (0xFFFFFFFF - E22) and lengths[o] == 22, (name, o)
            assert keys2[o] == (one << 32) | (0xFFFFFFFF - (EDUP22 - 1)) and lengths2[o] == 22, (name, o)
    # the plateau: ECONST's cells 301 .. 304 are 1.0 each, neighbouring offsets of one lane and of two
    keys, lengths = _timeline(gpu, m["corpus"][N_CASE], 700, T_HIGH, fp=_fp(lb, m, "q700"))
    idx, sc = timeline_ref.decode(keys)
    # (E1, ONE sub-fingerprint, is ECONST's: at a lower index it wins wherever ECONST scores 1.0)
    assert np.array_equal(m["entries"][E1][0], m["entries"][ECONST][0])
    assert list(idx[301:309]) == [E1] * 8 and np.all(sc[301:309] == 1.0) and list(lengths[301:309]) == [1] * 8
    assert list(idx[[200, 220]]) == [EDOUBLE, EDOUBLE] and np.all(sc[[200, 220]] == 1.0)


# ---- 4. entries longer than the query -------------------------------------------------------------------------------------------------
def test_longer_entries_never_appear(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"][N_CASE]
    for t in (T_HIGH, T_LOW):
        keys, lengths = _timeline(gpu, corpus, 22, t, fp=_fp(lb, m, "q22"))
        _same((keys, lengths), _want(m, "q22", t))
        idx, sc = timeline_ref.decode(keys)
        assert idx[0] == E22 and sc[0] == 1.0 and lengths[0] == 22        # the equal length takes part
        named = idx[idx >= 0]
        assert np.all(m["lengths"][named] <= 22) and E150 not in named and E300 not in named
        assert np.all(np.arange(22)[idx >= 0] + lengths[idx >= 0] <= 22)  # every span lies inside the recording
    # ... although the occurrences call lists the 22 inside both (case A)
    k, lg, total = corpus.query_occurrences_keys_device(_fp(lb, m, "q22"), T_HIGH, 4096)
    gpu.cuda.synchronize()
    assert {E150, E300} <= set(lb.decode_occurrence_keys(k, lg, int(total.cpu().numpy()[0]))[0].tolist())


# ---- 5. zeros --------------------------------------------------------------------------------------------------------------------------
def test_nothing_takes_part(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    fp, packed = _fp(lb, m, "q17"), _dev_packed(gpu, oracle, m, "q17")
    longer = _ragged(lb, gpu, oracle, _random(oracle, 31, [18, 30, 40]))
    empty = lb.Corpus.ragged(L, 4, 16)
    for corpus in (longer, empty):
        for kw in (dict(fp=fp), dict(packed=packed)):
            for want_lengths in (True, False):
                keys, lengths = _timeline(gpu, corpus, 17, T_LOW, want_lengths=want_lengths, **kw)
                assert not keys.any() and (lengths is None or not lengths.any())
        idx, sc, ln = corpus.recording_timeline(fp, T_LOW)
        assert np.all(idx == -1) and not sc.any() and not ln.any() and len(idx) == 17
        assert all(len(x) == 0 for x in corpus.recording_segments(fp, T_LOW))
    # a zero query: every cell is 0, and a zero cell never counts
    keys, lengths = _timeline(gpu, m["corpus"][N_CASE], 30, 1e-30, fp=_fp(lb, m, "qzero"))
    assert not keys.any() and not lengths.any()
    # the zero entry wins nowhere
    for name in ("q41", "q300"):
        keys, _ = _timeline(gpu, m["corpus"][N_CASE], len(m["queries"][name][0]), 1e-30, fp=_fp(lb, m, name))
        assert EZERO not in timeline_ref.decode(keys)[0]


# ---- 6. the threshold is compared as Float32, >= ---------------------------------------------------------------------------------------
def test_threshold_at_and_above_a_cell(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    for name in ("q41", "q300"):
        q, n = m["queries"][name]
        _want(m, name, T_LOW)
        best = max(p[1].max() for p in m["profiles"][(name, 0)] if p is not None)
        assert best > 0 and best.dtype == np.float32
        at = _timeline(gpu, m["corpus"][n], len(q), float(best), fp=_fp(lb, m, name))
        _same(at, _want(m, name, best))
        assert at[0].any() and np.all((at[0][at[0] != 0] >> np.uint64(32)) == best.view(np.uint32))
        above = _timeline(gpu, m["corpus"][n], len(q), float(np.nextafter(best, np.float32(np.inf))), fp=_fp(lb, m, name))
        assert not above[0].any() and not above[1].any()
    above = _timeline(gpu, m["corpus"][N_CASE], 41, 1.5, fp=_fp(lb, m, "q41"))                # above 1 is legal and matches nothing
    assert not above[0].any()


# ---- 7. ranges and an odd sub-fingerprint length ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("range_", [63, 64, 65, 199])
def test_ranges(lb, gpu, oracle, range_):
    m = _module(lb, gpu, oracle)
    for t in (T_HIGH, T_LOW):
        got = _timeline(gpu, m["corpus"][N_CASE], 300, t, fp=_fp(lb, m, "q300"), range_=range_)
        _same(got, _want(m, "q300", t, range_))
        _same(got, _fold_of_occurrences(gpu, m["corpus"][N_CASE], _fp(lb, m, "q300"), 300, m["lengths"], t, range_))


def test_odd_subfingerprint_length(lb, gpu, oracle):
    """sub-fingerprints of 199 Booleans: the full range and a shorter one"""
    rng = np.random.default_rng(5)
    ent = _random(oracle, 99, rng.integers(1, 41, 60), 199)
    ent[5] = _random(oracle, 98, [90], 199)[0]                    # longer than the query
    q = _random(oracle, 97, [64], 199)[0]
    q[20:20 + len(ent[9])] = ent[9]
    corpus = _ragged(lb, gpu, oracle, ent, 199)
    fp = lb.Fingerprint.from_bools(q)
    for range_ in (0, 20):
        profs = timeline_ref.profiles(q, ent, range_)
        for t in (T_HIGH, T_LOW):
            want = timeline_ref.fold(64, profs, t)
            assert range_ or timeline_ref.decode(want[0])[0][20] == 9
            _same(_timeline(gpu, corpus, 64, t, fp=fp, range_=range_), want)


# ---- 8. the index base ---------------------------------------------------------------------------------------------------------------------
def test_index_base(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus, fp, packed = m["corpus"][N_CASE], _fp(lb, m, "q300"), _dev_packed(gpu, oracle, m, "q300")
    zero = _timeline(gpu, corpus, 300, T_LOW, fp=fp)
    base = (1 << 32) - N_CASE
    for kw in (dict(fp=fp), dict(packed=packed)):
        got = _timeline(gpu, corpus, 300, T_LOW, base=base, **kw)
        _same(got, _want(m, "q300", T_LOW, base=base))
        assert np.array_equal(got[0][got[0] != 0] + np.uint64(base), zero[0][zero[0] != 0]) and np.array_equal(got[1], zero[1])
        assert np.array_equal(lb.decode_timeline_keys(got[0], got[1], base)[0], timeline_ref.decode(zero[0])[0])
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            _timeline(gpu, corpus, 300, T_LOW, base=base + 1, **kw)
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")


# ---- 9. packed, handle and host forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q17", "q300", "q700"])
def test_packed_handle_and_host_forms_agree(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    q, n = m["queries"][name]
    corpus, fp, packed = m["corpus"][n], _fp(lb, m, name), _dev_packed(gpu, oracle, m, name)
    for t in (T_HIGH, T_LOW):
        want = _want(m, name, t)
        a = _timeline(gpu, corpus, len(q), t, fp=fp)
        _same(a, want)
        _same(_timeline(gpu, corpus, len(q), t, packed=packed), want)
        _same(_timeline(gpu, corpus, len(q), t, fp=fp, want_lengths=False), (want[0], None))
        _same(_timeline(gpu, corpus, len(q), t, packed=packed, want_lengths=False), (want[0], None))
        idx, sc, ln = corpus.recording_timeline(fp, t)
        want_idx, want_sc = timeline_ref.decode(want[0])
        assert np.array_equal(idx, want_idx) and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32)) and np.array_equal(ln, want[1])
        d_idx, d_sc, d_ln = lb.decode_timeline_keys(a[0].view(np.int64), a[1])
        assert np.array_equal(d_idx, idx) and np.array_equal(d_sc.view(np.uint32), sc.view(np.uint32)) and np.array_equal(d_ln, ln)
        # the host form without lengths, and its count
        C, N = lb._native.C, lb._native
        idx2, sc2, cnt = np.full(len(q), -7, np.int64), np.full(len(q), -7, np.float32), N.UInt64(0)
        st = lb.lib().LBAudioDetectiveCorpusQueryRecordingTimeline(corpus._ref, fp._ref, 0, t, idx2.ctypes.data_as(C.POINTER(N.SInt64)),
                                                                   sc2.ctypes.data_as(C.POINTER(N.Float32)), None, C.byref(cnt))
        assert st == 0 and cnt.value == np.count_nonzero(want[0]) and np.array_equal(idx2, idx) and np.array_equal(sc2, sc)
        # what played when
        seg = corpus.recording_segments(fp, t)
        ref = timeline_ref.segments(want[0], want[1])
        assert [tuple(x) for x in zip(*(s.tolist() for s in seg))] == [(o, j, float(s), k) for o, j, s, k in ref]
        if name == "q700" and t == T_HIGH:
            assert [(o, j) for o, j, _s, _n in ref if _s == 1.0 and _n > 1] == [(10, E22), (200, EDOUBLE), (600, E22)]


# ---- 10. chunking -------------------------------------------------------------------------------------------------------------------------
def _scratch_bytes(entries, tiles):
    """the header's formula"""
    return -(-entries // WALK) * tiles * 126 * 8


def test_chunks_change_nothing(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus, fp = m["corpus"][N_CASE], _fp(lb, m, "q300")
    packed = _dev_packed(gpu, oracle, m, "q300")
    tiles = -(-(300 - min(300, int(m["lengths"].min())) + 1) // TILE)
    assert tiles == 3 and _scratch_bytes(1, tiles) == _scratch_bytes(WALK, tiles) == _scratch_bytes(2 * WALK, tiles) // 2
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    try:
        corpus.set_join_scratch_limit(0)
        one = {t: _timeline(gpu, corpus, 300, t, fp=fp) for t in (T_HIGH, T_LOW)}
        for t in one:
            _same(one[t], _want(m, "q300", t))
        unit = _scratch_bytes(WALK, tiles)
        for units, extra in ((1, 0), (1, unit - 1), (2, 7), (3, 4095)):
            chunk = units * WALK
            assert -(-N_CASE // chunk) >= 2 and N_CASE % chunk != 0          # several chunks, the last one partial
            corpus.set_join_scratch_limit(units * unit + extra)
            for t in one:
                _same(_timeline(gpu, corpus, 300, t, fp=fp), one[t])
                _same(_timeline(gpu, corpus, 300, t, packed=packed), one[t])
                _same(_timeline(gpu, corpus, 300, t, fp=fp, want_lengths=False), (one[t][0], None))
            idx, _sc, ln = corpus.recording_timeline(fp, T_LOW)
            assert np.array_equal(idx, timeline_ref.decode(one[T_LOW][0])[0]) and np.array_equal(ln, one[T_LOW][1])
        corpus.set_join_scratch_limit(unit - 1)
        for call in (lambda: _timeline(gpu, corpus, 300, T_LOW, fp=fp), lambda: _timeline(gpu, corpus, 300, T_LOW, packed=packed),
                     lambda: corpus.recording_timeline(fp, T_LOW), lambda: corpus.recording_segments(fp, T_LOW)):
            with pytest.raises(lb.LBAudioDetectiveError) as err:
                call()
            assert err.value.status == bad
    finally:
        corpus.set_join_scratch_limit(0)


# ---- 11. an entry at the cap ----------------------------------------------------------------------------------------------------------------
def test_an_entry_at_the_cap(lb, gpu, oracle):
    """the longest legal entry against queries equal, one longer and about twice as long (the LDS window at its largest), and
    one shorter: the entry takes no part"""
    ent = _random(oracle, 8, [5, CAP, 30])
    corpus = _ragged(lb, gpu, oracle, ent)
    planted = {CAP: 0, CAP + 1: 1, 2000: 700}
    for nq in (CAP - 1, CAP, CAP + 1, 2000):
        q = _random(oracle, 9, [nq])[0]
        if nq in planted:
            q[planted[nq]:planted[nq] + CAP] = ent[1]
        want = timeline_ref.timeline(q, ent, T_LOW)
        idx = timeline_ref.decode(want[0])[0]
        assert (1 in idx) == (nq in planted)
        assert nq not in planted or (idx[planted[nq]] == 1 and want[0][planted[nq]] >> np.uint64(32) == 0x3F800000)
        got = _timeline(gpu, corpus, nq, T_LOW, fp=lb.Fingerprint.from_bools(q))
        _same(got, want)
        assert nq in planted or 1 not in timeline_ref.decode(got[0])[0]
    above = _ragged(lb, gpu, oracle, _random(oracle, 5, [3, CAP + 1, 2]))
    q = _random(oracle, 9, [41])[0]
    fp, packed = lb.Fingerprint.from_bools(q), gpu.from_numpy(_packed(oracle, q)).cuda()
    for call in (lambda: _timeline(gpu, above, 41, T_LOW, fp=fp), lambda: _timeline(gpu, above, 41, T_LOW, packed=packed),
                 lambda: above.recording_timeline(fp, T_LOW)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            call()
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")


# ---- 12. refusals that need the corpus --------------------------------------------------------------------------------------------------------
def test_refusals(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    fp, packed = _fp(lb, m, "q41"), _dev_packed(gpu, oracle, m, "q41")

    def refused(call):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            call()
        assert err.value.status == bad

    uniform = lb.Corpus(L, 4, 8)
    refused(lambda: _timeline(gpu, uniform, 41, T_LOW, fp=fp))
    refused(lambda: _timeline(gpu, uniform, 41, T_LOW, packed=packed))
    refused(lambda: uniform.recording_timeline(fp, T_LOW))
    other = lb.Fingerprint.from_bools(_random(oracle, 6, [5], 100)[0])
    refused(lambda: _timeline(gpu, m["corpus"][N_CASE], 5, T_LOW, fp=other))
    refused(lambda: m["corpus"][N_CASE].recording_timeline(other, T_LOW))
    for t in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: _timeline(gpu, m["corpus"][N_CASE], 41, t, fp=fp))


# ---- 13. two calls in a row on two streams -----------------------------------------------------------------------------------------------------
def test_two_streams_in_a_row(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"][N_CASE]
    names = ("q700", "q129")
    streams = [gpu.cuda.Stream(), gpu.cuda.Stream()]
    for packed_form in (False, True):
        outs = []
        for s, name in zip(streams, names):                       # the second call is made while the first may still run
            nq = len(m["queries"][name][0])
            keys = gpu.full((nq,), POISON, dtype=gpu.int64, device="cuda")
            lengths = gpu.full((nq,), POISON32, dtype=gpu.int32, device="cuda")
            kw = dict(packed=_dev_packed(gpu, oracle, m, name), per_query=nq) if packed_form else dict(fp=_fp(lb, m, name))
            s.wait_stream(gpu.cuda.current_stream())
            corpus.recording_timeline_keys_device(threshold=T_LOW, keys_out=keys, lengths_out=lengths, stream=s, **kw)
            outs.append((keys, lengths))
        for s in streams:
            s.synchronize()
        for (keys, lengths), name in zip(outs, names):
            _same((keys.cpu().numpy().view(np.uint64), lengths.cpu().numpy().view(np.uint32)), _want(m, name, T_LOW))


# ---- 14. more entry blocks than one level of the fold takes -----------------------------------------------------------------------------------
def test_many_entry_blocks(lb, gpu, oracle):
    """a corpus of more than kTlFoldRows blocks of kTlEntries short entries: the fold's two levels, in one chunk and in chunks
    that take one level each -- against the fold of the occurrences call, and the chunked against the unchunked"""
    n = FOLD_ROWS * WALK + WALK + 5
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 7, n)
    ent = _random(oracle, 515, counts)
    q = _random(oracle, 516, [300])[0]
    q[40:40 + len(ent[n - 2])] = ent[n - 2]                       # a plant in the last, partial block
    q[TILE:TILE + len(ent[0])] = ent[0]
    corpus = _ragged(lb, gpu, oracle, ent)
    fp = lb.Fingerprint.from_bools(q)
    lengths = counts.astype(np.int64)
    try:
        got = _timeline(gpu, corpus, 300, T_LOW, fp=fp)
        _same(got, _fold_of_occurrences(gpu, corpus, fp, 300, lengths, T_LOW))
        idx, sc = timeline_ref.decode(got[0])
        assert sc[40] == 1.0 and sc[TILE] == 1.0 and 2 * np.count_nonzero(got[0]) > 300 and idx.max() > FOLD_ROWS * WALK
        tiles = -(-(300 - int(counts.min()) + 1) // TILE)
        corpus.set_join_scratch_limit(_scratch_bytes(FOLD_ROWS * WALK, tiles) + 3)              # 32 blocks, then the rest
        _same(_timeline(gpu, corpus, 300, T_LOW, fp=fp), got)
    finally:
        corpus.set_join_scratch_limit(0)
