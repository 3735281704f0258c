"""GPU tests of the occurrences calls (LBAudioDetectiveCorpusQueryOccurrencesKeysDevice, ...QueryPackedOccurrencesKeysDevice,
...QueryOccurrences).  The expected list is numpy only: align_ref.profile(query, entry, range) for EVERY entry, the cells >=
float32(t) and, for peaks, (o == 0 or q_o > q_(o-1)) and (o == last or q_o >= q_(o+1)), in (entry, offset) order.  Every cell
of every list is compared: keys as 64-bit integers, lags and the count exactly, the slots behind the count as 0; key, lag and
count buffers are poison-filled before every call.  The thresholds are values of the oracle's own cells (the largest, the 4th
largest distinct, the median) and the next float above the largest, so ties at the threshold exist by construction and nothing
needs a tolerance.  The corpus and the oracle's profiles are made once per module."""
import os
import re

import numpy as np
import pytest

from align_ref import profile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
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
CAP = int(re.search(r"^#define\s+LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS\s+(\d+)", _source(os.path.join("include", "lbaudiodetective.h")),
                    re.M).group(1))

# where the fixed entries lie (all inside the 70-entry prefix)
E1, E17, E22, E40, E63, E64, E65, EZERO, EDOUBLE, E150, E300, ENOISY = 3, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43


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
    return e, pool[7]


def _queries(oracle, e, block20):
    """name -> (Booleans, entries of the corpus it runs against)"""
    r = _random(oracle, 777, [1, 17, 41, 129, 300, 700, 2500, 300])
    q129, q300, q700, q2500, q300b = r[3], r[4], r[5], r[6], r[7]
    q129[0:22] = e[E22]
    q129[107:129] = e[E22]                                       # the last offset of the 22's profile
    q300[127:149] = e[E22]
    q300[150:172] = e[E22]
    q300[128:145] = e[E17]                                       # (on top of the first 22: two plants whose profiles overlap)
    q700[200:260] = np.concatenate([block20] * 3)                # plateaus and adjacent peaks
    q2500[1234:1256] = e[E22]
    q300b[TILE:TILE + 22] = e[E22]                               # the first cell of tile 1 and the last cell of tile 1
    q300b[2 * TILE - 1:2 * TILE + 21] = e[E22]
    return {"q1": (r[0], N_CASE), "q17": (r[1], N_CASE), "q41": (r[2], N_CASE), "q129": (q129, N_CASE), "q300": (q300, N_CASE),
            "q700": (q700, N_CASE), "q2500": (q2500, N_PREFIX), "q22": (e[E22].copy(), N_CASE), "q300b": (q300b, N_CASE)}


_M = {}


def _module(lb, gpu, oracle):
    if not _M:
        e, block20 = _entries(oracle)
        _M["entries"] = e
        _M["queries"] = _queries(oracle, e, block20)
        _M["corpus"] = {N_CASE: _ragged(lb, gpu, oracle, e), N_PREFIX: _ragged(lb, gpu, oracle, e[:N_PREFIX])}
        _M["profiles"] = {}
        _M["fp"] = {}
    return _M


def _profiles(m, name, range_=0):
    """the oracle's profiles of query `name` against its corpus: [(q float32 [n_off], entry_long)] per entry, made once"""
    if (name, range_) not in m["profiles"]:
        q, n = m["queries"][name]
        m["profiles"][(name, range_)] = [profile(q, ent, range_) for ent in m["entries"][:n]]
    return m["profiles"][(name, range_)]


def _fp(lb, m, name):
    if name not in m["fp"]:
        m["fp"][name] = lb.Fingerprint.from_bools(m["queries"][name][0])
    return m["fp"][name]


def _thresholds(profiles):
    cells = np.sort(np.concatenate([p for p, _ in profiles]))
    distinct = np.unique(cells)
    top = cells[-1]
    out = {"max": top, "4th": distinct[-4] if len(distinct) >= 4 else distinct[0], "above": np.nextafter(top, np.float32(np.inf)),
           "median": cells[len(cells) // 2]}
    return {k: np.float32(v) for k, v in out.items() if v > 0}


def _expected(profiles, t, peaks, index_base=0):
    """(keys uint64, lags int32) of every matching cell, entries ascending, offsets ascending"""
    keys, lags = [], []
    for j, (q, entry_long) in enumerate(profiles):
        m = q >= np.float32(t)
        if peaks:
            left = np.ones(len(q), bool)
            right = np.ones(len(q), bool)
            left[1:] = q[1:] > q[:-1]
            right[:-1] = q[:-1] >= q[1:]
            m &= left & right
        o = np.flatnonzero(m)
        keys.append((q[o].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - (index_base + j)))
        lags.append(o if entry_long else -o)
    return np.concatenate(keys).astype(np.uint64), np.concatenate(lags).astype(np.int32)


def _run(gpu, corpus, fp, t, peaks, capacity, range_=0, index_base=0, want_lags=True, stream=None, packed=None, per=0):
    """one device call into poison-filled buffers -> (keys uint64 [capacity], lags int32 [capacity] or None, count)"""
    keys = gpu.full((capacity,), POISON, dtype=gpu.int64, device="cuda")
    lags = gpu.full((capacity,), POISON32, dtype=gpu.int32, device="cuda") if want_lags else None
    count = gpu.full((1,), POISON, dtype=gpu.int64, device="cuda")
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    if packed is None:
        corpus.query_occurrences_keys_device(fp, float(t), capacity, peaks=peaks, range_=range_, index_base=index_base, keys_out=keys,
                                             lags_out=lags, count_out=count, want_lags=want_lags, stream=stream)
    else:
        corpus.query_packed_occurrences_keys_device(packed, per, float(t), capacity, peaks=peaks, range_=range_, index_base=index_base,
                                                    keys_out=keys, lags_out=lags, count_out=count, want_lags=want_lags, stream=stream)
    (stream or gpu.cuda.current_stream()).synchronize()
    return (keys.cpu().numpy().view(np.uint64), lags.cpu().numpy() if want_lags else None, int(count.cpu().numpy().view(np.uint64)[0]))


def _check(got, want_keys, want_lags, capacity):
    keys, lags, count = got
    m = min(len(want_keys), capacity)
    assert count == len(want_keys)
    assert np.array_equal(keys[:m], want_keys[:m])
    assert not keys[m:].any()
    if lags is not None:
        assert np.array_equal(lags[:m], want_lags[:m])
        assert not lags[m:].any()


# ---- 1. the device handle form against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q1", "q17", "q41", "q129", "q300", "q700", "q2500", "q22", "q300b"])
def test_handle_form_equals_the_oracle(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    prof = _profiles(m, name)
    corpus = m["corpus"][m["queries"][name][1]]
    ts = _thresholds(prof)
    assert {"max", "above", "median"} <= set(ts)
    for peaks in (False, True):
        for what, t in ts.items():
            want_keys, want_lags = _expected(prof, t, peaks)
            print(name, what, float(t), "peaks" if peaks else "all", len(want_keys))
            if what == "above":
                assert len(want_keys) == 0
            elif not peaks:
                assert len(want_keys) >= 1
            capacity = len(want_keys) + 5
            _check(_run(gpu, corpus, _fp(lb, m, name), t, peaks, capacity), want_keys, want_lags, capacity)


def test_planted_cells_are_where_they_were_planted(lb, gpu, oracle):
    """the oracle itself: the plants of the table are cells of 1.0 at their offsets (so the lists above hold them)"""
    m = _module(lb, gpu, oracle)
    p129, p300, p300b, p22 = (_profiles(m, n) for n in ("q129", "q300", "q300b", "q22"))
    assert p129[E22][0][0] == 1.0 and p129[E22][0][107] == 1.0 and len(p129[E22][0]) == 108
    assert p300[E22][0][150] == 1.0 and p300[E17][0][128] == 1.0 and p300[E22][0][127] < 1.0
    assert p300b[E22][0][TILE] == 1.0 and p300b[E22][0][2 * TILE - 1] == 1.0
    assert p22[E150][1] and p22[E150][0][33] == 1.0 and p22[E150][0][100] == 1.0
    assert p22[E300][1] and p22[E300][0][10] == 1.0 and p22[E300][0][250] == 1.0
    assert len(_profiles(m, "q17")[E17][0]) == 1 and not _profiles(m, "q17")[E17][1]      # equal lengths: one cell, case B
    d = _profiles(m, "q700")[EDOUBLE][0]
    assert d[200] == 1.0 and d[220] == 1.0


# ---- shape variations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("range_", [63, 64, 65, 199])
def test_ranges(lb, gpu, oracle, range_):
    m = _module(lb, gpu, oracle)
    prof = _profiles(m, "q300", range_)
    for peaks in (False, True):
        for what, t in _thresholds(prof).items():
            want_keys, want_lags = _expected(prof, t, peaks)
            capacity = len(want_keys) + 3
            _check(_run(gpu, m["corpus"][N_CASE], _fp(lb, m, "q300"), t, peaks, capacity, range_=range_), want_keys, want_lags, capacity)


def test_odd_subfingerprint_length(lb, gpu, oracle):
    """sub-fingerprints of 37 Booleans: both cases, the full range and a shorter one"""
    rng = np.random.default_rng(5)
    ent = _random(oracle, 99, rng.integers(1, 41, 60), 37)
    ent[5] = _random(oracle, 98, [90], 37)[0]
    q = _random(oracle, 97, [64], 37)[0]
    q[20:20 + len(ent[9])] = ent[9]
    ent[5][20:20 + 64] = q                                        # case A: the query inside a longer entry
    corpus = _ragged(lb, gpu, oracle, ent, 37)
    fp = lb.Fingerprint.from_bools(q)
    for range_ in (0, 20):
        prof = [profile(q, x, range_) for x in ent]
        assert prof[5][1] and (range_ or prof[5][0][20] == 1.0)
        for peaks in (False, True):
            for what, t in _thresholds(prof).items():
                want_keys, want_lags = _expected(prof, t, peaks)
                capacity = len(want_keys) + 3
                _check(_run(gpu, corpus, fp, t, peaks, capacity, range_=range_), want_keys, want_lags, capacity)


# ---- 2. the packed form and the host form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q17", "q300", "q22"])
def test_packed_and_host_forms_equal_the_handle_form(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    q, n = m["queries"][name]
    corpus = m["corpus"][n]
    packed = gpu.from_numpy(_packed(oracle, q)).cuda()
    ts = _thresholds(_profiles(m, name))
    for peaks in (False, True):
        for t in (ts["median"], ts["4th"]):
            total = _run(gpu, corpus, _fp(lb, m, name), t, peaks, 1)[2]
            capacity = total + 4
            a = _run(gpu, corpus, _fp(lb, m, name), t, peaks, capacity)
            b = _run(gpu, corpus, None, t, peaks, capacity, packed=packed, per=len(q))
            assert a[2] == b[2] == total and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            idx, sc, lags, count = corpus.query_occurrences(_fp(lb, m, name), float(t), capacity, peaks=peaks)
            want_idx, want_sc, want_lags = lb.decode_occurrence_keys(a[0], a[1], a[2])
            assert count == total and np.array_equal(idx, want_idx) and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))
            assert np.array_equal(lags, want_lags)


# ---- 3. the capacity cuts the list, never the count ---------------------------------------------------------------------------
@pytest.mark.parametrize("peaks", [False, True])
def test_capacity_cut(lb, gpu, oracle, peaks):
    m = _module(lb, gpu, oracle)
    prof = _profiles(m, "q300")
    t = _thresholds(prof)["median"]
    want_keys, want_lags = _expected(prof, t, peaks)
    assert len(want_keys) >= 8
    for capacity in (len(want_keys) // 2, 1):
        _check(_run(gpu, m["corpus"][N_CASE], _fp(lb, m, "q300"), t, peaks, capacity), want_keys, want_lags, capacity)
    idx, sc, lags, count = m["corpus"][N_CASE].query_occurrences(_fp(lb, m, "q300"), float(t), 3, peaks=peaks)
    assert count == len(want_keys) and len(idx) == 3 and np.array_equal(lags, want_lags[:3])


# ---- 4. chunking ------------------------------------------------------------------------------------------------------------------
def _scratch_bytes(entries, tiles):
    """the header's formula"""
    return 24 + entries * (16 + 8 * tiles) + -(-entries // BLOCK) * -(-tiles // 4) * 4


def test_chunks_change_nothing(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus, fp = m["corpus"][N_CASE], _fp(lb, m, "q300")
    prof = _profiles(m, "q300")
    tiles = -(-max(len(p) for p, _ in prof) // TILE)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    try:
        for peaks in (False, True):
            t = _thresholds(prof)["median"]
            want_keys, want_lags = _expected(prof, t, peaks)
            capacity = len(want_keys) + 2
            corpus.set_join_scratch_limit(0)
            one = _run(gpu, corpus, fp, t, peaks, capacity)
            _check(one, want_keys, want_lags, capacity)
            for chunk in (2 * BLOCK, BLOCK):                      # 517 entries: five chunks, nine chunks
                assert -(-N_CASE // chunk) >= 3
                corpus.set_join_scratch_limit(_scratch_bytes(chunk, tiles) + (7 if chunk == BLOCK else 0))
                got = _run(gpu, corpus, fp, t, peaks, capacity)
                assert got[2] == one[2] and np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1])
        corpus.set_join_scratch_limit(_scratch_bytes(BLOCK, tiles) - 1)
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            _run(gpu, corpus, fp, 0.5, False, 4)
        assert err.value.status == bad
    finally:
        corpus.set_join_scratch_limit(0)


# ---- 5. outLags == NULL -------------------------------------------------------------------------------------------------------------
def test_no_lags_changes_nothing(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    prof = _profiles(m, "q129")
    t = _thresholds(prof)["median"]
    for peaks in (False, True):
        want_keys, want_lags = _expected(prof, t, peaks)
        capacity = len(want_keys) + 2
        _check(_run(gpu, m["corpus"][N_CASE], _fp(lb, m, "q129"), t, peaks, capacity, want_lags=False), want_keys, want_lags, capacity)


# ---- 6. the index base ------------------------------------------------------------------------------------------------------------
def test_index_base(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    prof = _profiles(m, "q41")
    t = _thresholds(prof)["4th"]
    base = (1 << 32) - N_CASE
    want_keys, want_lags = _expected(prof, t, False, base)
    _check(_run(gpu, m["corpus"][N_CASE], _fp(lb, m, "q41"), t, False, len(want_keys) + 1, index_base=base), want_keys, want_lags,
           len(want_keys) + 1)
    with pytest.raises(lb.LBAudioDetectiveError) as err:
        _run(gpu, m["corpus"][N_CASE], _fp(lb, m, "q41"), t, False, 4, index_base=base + 1)
    assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    fp = _fp(lb, m, "q41")
    packed = gpu.from_numpy(_packed(oracle, m["queries"]["q41"][0])).cuda()
    # an empty corpus: zeros
    empty = lb.Corpus.ragged(L, 4, 16)
    for peaks in (False, True):
        assert _run(gpu, empty, fp, 0.5, peaks, 6)[2] == 0
        k, lg, c = _run(gpu, empty, None, 0.5, peaks, 6, packed=packed, per=41)
        assert c == 0 and not k.any() and not lg.any()
    idx, sc, lags, count = empty.query_occurrences(fp, 0.5, 6)
    assert count == 0 and len(idx) == 0

    def refused(call):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            call()
        assert err.value.status == bad

    # a uniform corpus
    uniform = lb.Corpus(L, 4, 8)
    refused(lambda: _run(gpu, uniform, fp, 0.5, False, 4))
    refused(lambda: _run(gpu, uniform, None, 0.5, False, 4, packed=packed, per=41))
    refused(lambda: uniform.query_occurrences(fp, 0.5, 4))
    # an entry above the cap
    long_ = _ragged(lb, gpu, oracle, _random(oracle, 5, [3, CAP + 1, 2]))
    refused(lambda: _run(gpu, long_, fp, 0.5, False, 4))
    refused(lambda: _run(gpu, long_, None, 0.5, False, 4, packed=packed, per=41))
    refused(lambda: long_.query_occurrences(fp, 0.5, 4))
    at_cap = _ragged(lb, gpu, oracle, _random(oracle, 5, [3, CAP, 2]))
    assert _run(gpu, at_cap, fp, 2.0, False, 4)[2] == 0
    # a query of another sub-fingerprint length
    other = lb.Fingerprint.from_bools(_random(oracle, 6, [5], 100)[0])
    refused(lambda: _run(gpu, m["corpus"][N_CASE], other, 0.5, False, 4))
    refused(lambda: m["corpus"][N_CASE].query_occurrences(other, 0.5, 4))


def test_an_entry_at_the_cap(lb, gpu, oracle):
    """the longest legal entry: the LDS window at its largest (case B, a query of 1 100) and case A with 1 000 offsets"""
    ent = _random(oracle, 8, [5, CAP, 30])
    corpus = _ragged(lb, gpu, oracle, ent)
    for nq in (1100, 25):
        q = _random(oracle, 9, [nq])[0]
        if nq == 25:
            ent_q = ent[1][700:725]
            q = ent_q.copy()
        prof = [profile(q, x, 0) for x in ent]
        fp = lb.Fingerprint.from_bools(q)
        for peaks in (False, True):
            for what, t in _thresholds(prof).items():
                want_keys, want_lags = _expected(prof, t, peaks)
                capacity = len(want_keys) + 3
                _check(_run(gpu, corpus, fp, t, peaks, capacity), want_keys, want_lags, capacity)


# ---- 8. agreement with the calls that exist ---------------------------------------------------------------------------------------
def test_agreement_with_threshold_scores_and_profiles(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus, fp = m["corpus"][N_CASE], _fp(lb, m, "q300")
    prof = _profiles(m, "q300")
    t = _thresholds(prof)["median"]
    total = _run(gpu, corpus, fp, t, False, 1)[2]
    keys, lags, count = _run(gpu, corpus, fp, t, False, total)
    idx, sc, lg = lb.decode_occurrence_keys(keys, lags, count)
    # the entries with at least one cell are query_threshold's, each one's best cell its score, that cell's lag the aligned lag
    t_idx, t_sc, t_lags, t_count = corpus.query_threshold(fp, float(t), N_CASE, aligned=True)
    assert t_count == len(t_idx) and np.array_equal(np.unique(idx), t_idx)
    scores = corpus.scores_device(fp).cpu().numpy()
    for j, want_lag in zip(t_idx, t_lags):
        mine = np.flatnonzero(idx == j)
        best = mine[np.argmax(sc[mine])]                          # (argmax: the first, i.e. the lowest offset)
        assert sc[best].view(np.uint32) == scores[j].view(np.uint32)
        assert lg[best] == want_lag
    # twenty entries' full cell lists are a filter of match_profile
    for j in np.linspace(0, N_CASE - 1, 20).astype(int):
        p, first = corpus.match_profile(fp, int(j))
        o = np.flatnonzero(p >= t)
        mine = idx == j
        assert np.array_equal(sc[mine].view(np.uint32), p[o].view(np.uint32))
        assert np.array_equal(np.abs(lg[mine]), o)


# ---- 9. twice, on two streams in a row ----------------------------------------------------------------------------------------------
def test_two_streams_in_a_row(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    prof = _profiles(m, "q700")
    t = _thresholds(prof)["median"]
    want_keys, want_lags = _expected(prof, t, True)
    capacity = len(want_keys) + 1
    corpus, fp = m["corpus"][N_CASE], _fp(lb, m, "q700")
    streams = [gpu.cuda.Stream(), gpu.cuda.Stream()]
    outs = []
    for s in streams:                                             # the second call is made while the first may still run
        keys = gpu.full((capacity,), POISON, dtype=gpu.int64, device="cuda")
        lags = gpu.full((capacity,), POISON32, dtype=gpu.int32, device="cuda")
        count = gpu.full((1,), POISON, dtype=gpu.int64, device="cuda")
        s.wait_stream(gpu.cuda.current_stream())
        corpus.query_occurrences_keys_device(fp, float(t), capacity, peaks=True, keys_out=keys, lags_out=lags, count_out=count, stream=s)
        outs.append((keys, lags, count))
    for s in streams:
        s.synchronize()
    a, b = [(k.cpu().numpy().view(np.uint64), lg.cpu().numpy(), int(c.cpu().numpy().view(np.uint64)[0])) for k, lg, c in outs]
    _check(a, want_keys, want_lags, capacity)
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
