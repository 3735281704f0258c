"""GPU tests of the batch occurrences and the batch recording threshold
(LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice, LBAudioDetectiveCorpusQueryPackedRecordingThresholdBatchKeysDevice,
k_occurrences_batch.hip, StreamBank.occurrences / matches_above).  Every expected value is numpy (align_ref.profile for EVERY
recording and entry, with the match rule, the peak rule and the selection restated here) or the output of a call that existed
before (query_packed_occurrences_keys_device and query_packed_recording_threshold_keys_device on one row of the block,
query_packed_threshold_keys_device -- the scan -- on the whole block); keys, lags and counts are compared exactly: nothing needs a
tolerance.  Output buffers are poison-filled before every call.  The corpus and the blocks are test_gpu_recording_batch.py's (the
helpers are copied, not imported): 2 x 64 + 5 entries -- 1 .. 40 sub-fingerprints, a planted 17 and a planted 22, a duplicate of
the 22 at a higher index, an all-zero entry and, as the LAST two, one entry of 150 and one of 400 (case A) --, the whole corpus and
its first 131 entries.  The thresholds are values of the reference's own cells, so ties at the threshold exist by construction.
The corpora, the blocks and the reference are made once per module."""
import numpy as np
import pytest

from align_ref import profile

pytestmark = pytest.mark.gpu

POISON = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
L = 200
TILE, GROUP, WALK = 126, 504, 64
N_CASE = 2 * WALK + 5
N_SHORT = N_CASE - 2                     # without the two long entries: still a partial last block
E1, E17, E22, EZERO, EDUP, E150, E400 = 3, 7, 11, 29, 100, N_CASE - 2, N_CASE - 1
FORM_S, FORM_W = 0, 1
ONE = np.float32(1.0)
CAP = 2048                               # slots per row of the oracle cases: the sparse thresholds fit, the median is cut


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
    counts = rng.integers(1, 41, N_CASE)
    counts[E1], counts[5] = 1, 40                                # the plan's shortest and (of the short corpus) longest entry
    counts[E150], counts[E400] = 150, 400
    e = _random(oracle, 4242, counts)
    pool = _random(oracle, 4343, [17, 22])
    e[E17], e[E22] = pool
    e[EDUP] = pool[1].copy()                                     # the 22 once more at a higher index
    e[EZERO] = np.zeros((10, L), np.uint8)                       # every cell 0: never a match
    return e


# name: (form, recordings, sub-fingerprints each).  Form W: five recordings, so that the last group of four global tiles is partial
# and groups of four straddle recordings; form S: 5 tiles, two tile groups
CASES = {"w100": (FORM_W, 5, 100), "w129": (FORM_W, 5, 129), "w300": (FORM_W, 5, 300), "s525": (FORM_S, 3, 525)}
# name: [(recording, offset)] where the 22 / the 17 lie verbatim (cells of 1.0 at those offsets, lag minus the offset)
PLANTS_22 = {"w100": [(0, 0), (1, 100 - 22), (2, 0)], "w129": [(1, 129 - 22), (2, 0)], "w300": [(0, TILE - 1), (1, 300 - 22), (2, 0)],
             "s525": [(0, TILE - 1), (1, GROUP - 1), (2, 0)]}
PLANTS_17 = {"w100": [(3, 50), (4, 20), (4, 60)], "w129": [(0, 10), (0, 70), (4, 100)],
             "w300": [(1, TILE), (3, 2 * TILE), (4, 100), (4, 200)], "s525": [(0, GROUP), (1, TILE)]}
# the recording r whose end and whose successor's start hold the two halves of the 22; neither row holds a whole 22
STRADDLE = {"w100": 3, "w129": 3, "w300": 3}
# (entry, block, recording, offset inside the entry): that recording lies verbatim inside the long entry -- case A, a cell of 1.0
INSIDE = ((E150, "w100", 2, 30), (E400, "w129", 1, 2 * TILE - 2))


def _block(oracle, e, name):
    """Booleans [recordings, per, L]"""
    _form, R, per = CASES[name]
    block = oracle.synth_ragged_entries(777 + per, 0, np.array([R * per], np.uint32), L).reshape(R, per, L).copy()
    for r, o in PLANTS_22[name]:
        block[r, o:o + 22] = e[E22]
    for r, o in PLANTS_17[name]:
        block[r, o:o + 17] = e[E17]
    if name in STRADDLE:
        r = STRADDLE[name]
        block[r, per - 11:] = e[E22][:11]                        # in the packed block the 22 lies verbatim across the seam
        block[r + 1, :11] = e[E22][11:]
        assert np.array_equal(block.reshape(R * per, L)[(r + 1) * per - 11:(r + 1) * per + 11], e[E22])
        assert all(row not in (r, r + 1) for row, _o in PLANTS_22[name])
    return block


_M = {}


def _module(lb, gpu, oracle):
    if not _M:
        e = _entries(oracle)
        _M["blocks"] = {name: _block(oracle, e, name) for name in CASES}
        for entry, name, r, at in INSIDE:
            per = CASES[name][2]
            e[entry][at:at + per] = _M["blocks"][name][r]
        _M["entries"] = e
        _M["lengths"] = np.array([len(x) for x in e], np.int64)
        assert (_M["lengths"][:N_SHORT].min(), _M["lengths"][:N_SHORT].max(), len(e[E22]), len(e[E17]), len(e[E1])) == (1, 40, 22, 17, 1)
        _M["corpus"] = {N_CASE: _ragged(lb, gpu, oracle, e), N_SHORT: _ragged(lb, gpu, oracle, e[:N_SHORT])}
        _M["dev"] = {name: gpu.from_numpy(_packed(oracle, b.reshape(-1, L))).cuda() for name, b in _M["blocks"].items()}
        _M["profiles"] = {}
    return _M


def _profiles(m, name, range_=0):
    """the reference's profiles of every recording of a block against EVERY entry: [[(q float32 [n_off], entry_long)]], made once"""
    if (name, range_) not in m["profiles"]:
        m["profiles"][(name, range_)] = [[profile(rec, ent, range_) for ent in m["entries"]] for rec in m["blocks"][name]]
    return m["profiles"][(name, range_)]


def _thresholds(profiles):
    """values of the reference's own cells -- the largest (1.0 where a plant lies), the 4th largest distinct, the 99.9th percentile
    and the median --, and 1.0 and 1.5 as such"""
    cells = np.sort(np.concatenate([p for row in profiles for p, _ in row]))
    distinct = np.unique(cells)
    out = {"max": cells[-1], "4th": distinct[-4], "p999": cells[int(len(cells) * 0.999)], "median": cells[len(cells) // 2], "one": 1.0,
           "above": 1.5}
    return {k: np.float32(v) for k, v in out.items() if v > 0}


def _expected_row(row, t, peaks, base=0):
    """the match and peak rules restated: (keys uint64, lags int32) of every cell q_o >= t of every entry -- with peaks only the
    cells with (o == 0 or q_o > q_(o-1)) and (o == last or q_o >= q_(o+1)), the first of a plateau -- entries ascending, offsets
    ascending; the lag is +o where the entry is the longer, -o otherwise"""
    keys, lags = [], []
    for j, (q, entry_long) in enumerate(row):
        m = q >= np.float32(t)
        if peaks:
            left = np.ones(len(q), bool)
            right = np.ones(len(q), bool)
            left[1:] = q[1:] > q[:-1]
            right[:-1] = q[:-1] >= q[1:]
            m &= left & right
        o = np.flatnonzero(m)
        keys.append((q[o].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - (base + j)))
        lags.append(o if entry_long else -o)
    return np.concatenate(keys).astype(np.uint64), np.concatenate(lags).astype(np.int32)


def _expected(profiles, n, t, peaks, capacity, base=0):
    """(keys uint64 [R, capacity], lags int32 [R, capacity], counts [R]) against the first n entries: the first capacity matches of
    every row, zeros behind them, the TRUE counts"""
    R = len(profiles)
    keys, lags, counts = np.zeros((R, capacity), np.uint64), np.zeros((R, capacity), np.int32), np.zeros(R, np.int64)
    for r, row in enumerate(profiles):
        k, g = _expected_row(row[:n], t, peaks, base)
        counts[r] = len(k)
        keys[r, :min(len(k), capacity)] = k[:capacity]
        lags[r, :min(len(k), capacity)] = g[:capacity]
    return keys, lags, counts


def _expected_threshold(profiles, n, t, capacity, base=0):
    """the recording threshold restated: per row the entries whose best cell (never below 0) is >= t in ascending index, the key
    of that score, the lag of the LOWEST offset that reaches it; zeros behind, the true counts"""
    R = len(profiles)
    keys, lags, counts = np.zeros((R, capacity), np.uint64), np.zeros((R, capacity), np.int32), np.zeros(R, np.int64)
    for r, row in enumerate(profiles):
        at = 0
        for j, (q, entry_long) in enumerate(row[:n]):
            best = np.float32(max(np.float32(0.0), q.max()))
            if not best >= np.float32(t):
                continue
            if at < capacity:
                o = int(np.flatnonzero(q == best)[0])
                keys[r, at] = (np.uint64(best.view(np.uint32)) << np.uint64(32)) | np.uint64(0xFFFFFFFF - (base + j))
                lags[r, at] = o if entry_long else -o
            at += 1
        counts[r] = at
    return keys, lags, counts


def _outputs(gpu, R, capacity, want_lags):
    keys = gpu.full((R, capacity), POISON, dtype=gpu.int64, device="cuda")
    lags = gpu.full((R, capacity), POISON32, dtype=gpu.int32, device="cuda") if want_lags else None
    counts = gpu.full((R,), POISON, dtype=gpu.int64, device="cuda")
    return keys, lags, counts


def _host(keys, lags, counts):
    return keys.cpu().numpy().view(np.uint64), lags.cpu().numpy() if lags is not None else None, counts.cpu().numpy()


def _batch(gpu, corpus, packed, R, per, t, peaks, capacity, range_=0, base=0, want_lags=True, stream=None):
    """one batch occurrences call into poison-filled buffers -> (keys uint64 [R, capacity], lags int32 or None, counts int64 [R])"""
    keys, lags, counts = _outputs(gpu, R, capacity, want_lags)
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = corpus.query_packed_occurrences_batch_keys_device(packed, R, per, float(t), capacity, peaks=peaks, range_=range_, index_base=base,
                                                            keys_out=keys, lags_out=lags, counts_out=counts, want_lags=want_lags,
                                                            stream=stream)
    assert got[0] is keys and got[1] is lags and got[2] is counts
    (stream or gpu.cuda.current_stream()).synchronize()
    return _host(keys, lags, counts)


def _single(gpu, corpus, packed, R, per, t, peaks, capacity, range_=0, base=0):
    """query_packed_occurrences_keys_device on every row of the block in turn"""
    rows = packed.reshape(R, per, 32)
    keys, lags, counts = _outputs(gpu, R, capacity, True)
    for r in range(R):
        corpus.query_packed_occurrences_keys_device(rows[r], per, float(t), capacity, peaks=peaks, range_=range_, index_base=base,
                                                    keys_out=keys[r], lags_out=lags[r], count_out=counts[r:r + 1])
    gpu.cuda.synchronize()
    return _host(keys, lags, counts)


def _tbatch(gpu, corpus, packed, R, per, t, capacity, range_=0, base=0, want_lags=True, stream=None):
    """one batch recording threshold call into poison-filled buffers"""
    keys, lags, counts = _outputs(gpu, R, capacity, want_lags)
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = corpus.query_packed_recording_threshold_batch_keys_device(packed, R, per, float(t), capacity, range_=range_, index_base=base,
                                                                    keys_out=keys, lags_out=lags, counts_out=counts, want_lags=want_lags,
                                                                    stream=stream)
    assert got[0] is keys and got[1] is lags and got[2] is counts
    (stream or gpu.cuda.current_stream()).synchronize()
    return _host(keys, lags, counts)


def _tsingle(gpu, corpus, packed, R, per, t, capacity, range_=0, base=0):
    """query_packed_recording_threshold_keys_device on every row of the block in turn"""
    rows = packed.reshape(R, per, 32)
    keys, lags, counts = _outputs(gpu, R, capacity, True)
    for r in range(R):
        corpus.query_packed_recording_threshold_keys_device(rows[r], per, float(t), capacity, range_=range_, index_base=base,
                                                            keys_out=keys[r], lags_out=lags[r], count_out=counts[r:r + 1])
    gpu.cuda.synchronize()
    return _host(keys, lags, counts)


def _tscan(gpu, corpus, packed, R, per, t, capacity, range_=0, base=0):
    """the scan's threshold query on the whole block"""
    keys, lags, counts = _outputs(gpu, R, capacity, True)
    corpus.query_packed_threshold_keys_device(packed, R, per, float(t), capacity, keys_out=keys, counts_out=counts, lags_out=lags,
                                              aligned=True, range_=range_, index_base=base)
    gpu.cuda.synchronize()
    return _host(keys, lags, counts)


def _same(got, want):
    """keys, lags and counts exactly; every word of every output"""
    assert got[0].shape == want[0].shape and np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[0], want[0])
    if got[1] is not None:
        assert np.array_equal(got[1], want[1])


def _plan(lb, m, n, R, per, limit=0):
    return lb.debug_occurrences_batch_plan(R, per, int(m["lengths"][:n].min()), int(m["lengths"][:n].max()), n, limit)


def _tiles(per, n):
    most = per                                                   # the shortest entry has one sub-fingerprint
    if n == N_CASE and per < 400:
        most = max(most, 400 - per + 1)
    return -(-most // TILE)


def _scratch(entries, tiles):
    """the single call's scratch formula"""
    return 24 + entries * (16 + 8 * tiles) + -(-entries // WALK) * -(-tiles // 4) * 4


# ---- 1. the oracle: forms and tiles, plants at the seams, case A, no leak from a neighbour --------------------------------------------
@pytest.mark.parametrize("name,n", [("w100", N_SHORT), ("w129", N_SHORT), ("w300", N_SHORT), ("w100", N_CASE), ("w129", N_CASE),
                                    ("w300", N_CASE), ("s525", N_SHORT), ("s525", N_CASE)])
def test_rows_equal_the_reference_and_the_single_call(lb, gpu, oracle, name, n):
    m = _module(lb, gpu, oracle)
    form, R, per = CASES[name]
    plan = _plan(lb, m, n, R, per)
    assert plan["form"] == form and plan["tiles"] == _tiles(per, n) and plan["recordings_per_pass"] == R
    assert form == FORM_S or n == N_SHORT or (R * plan["tiles"]) % 4 != 0      # form W: the last group of four global tiles is partial
    corpus, packed = m["corpus"][n], m["dev"][name]
    prof = [row[:n] for row in _profiles(m, name)]
    ts = _thresholds(prof)
    assert ts["max"] == ONE and set(ts) == {"max", "4th", "p999", "median", "one", "above"}
    for what, t in ts.items():
        for peaks in (False, True):
            want = _expected(prof, n, t, peaks, CAP)
            got = _batch(gpu, corpus, packed, R, per, t, peaks, CAP)
            _same(got, want)
            _same(got, _single(gpu, corpus, packed, R, per, t, peaks, CAP))
            if what == "above":
                assert not want[2].any() and not got[0].any()
            if what == "median":
                assert (want[2] > CAP).any()                      # rows that are cut, with the true count
    # the plants, at threshold 1.0 with peaks: one match per plant, at its offset
    keys, lags, counts = _batch(gpu, corpus, packed, R, per, 1.0, True, CAP)
    found = {(r, 0xFFFFFFFF - int(keys[r, i] & np.uint64(0xFFFFFFFF)), int(lags[r, i])) for r in range(R) for i in range(int(counts[r]))}
    for plants, entries in ((PLANTS_22, (E22, EDUP)), (PLANTS_17, (E17,))):
        for r, o in plants[name]:
            for entry in entries:
                assert (r, entry, -o) in found, (name, r, entry, o)
    # the straddling 22: in the packed block it lies verbatim across the seam of r | r + 1; it matches in neither
    if name in STRADDLE:
        r = STRADDLE[name]
        assert not any(row in (r, r + 1) and entry in (E22, EDUP) for row, entry, _lag in found)
    # case A: the recording lies verbatim inside a longer entry
    for entry, block, r, at in INSIDE:
        if block == name and n == N_CASE:
            assert (r, entry, at) in found
    assert not any(entry == EZERO for _r, entry, _lag in found)


def test_the_shapes_are_the_seams(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    assert len(m["entries"]) == 2 * WALK + 5 and N_SHORT % WALK != 0
    assert (0, TILE - 1) in PLANTS_22["w300"] and (1, TILE) in PLANTS_17["w300"]                       # cells 125 | 126: the tile seam
    assert (1, GROUP - 1) in PLANTS_22["s525"] and (0, GROUP) in PLANTS_17["s525"]                     # 503 | 504: the group seam
    for name, (_form, _R, per) in CASES.items():                  # the last offset of recording r, offset 0 of r + 1
        last = [(r, o, 22) for r, o in PLANTS_22[name] if o == per - 22] + [(r, o, 17) for r, o in PLANTS_17[name] if o == per - 17]
        assert last, name
        assert any((r + 1, 0) in PLANTS_22[name] for r, _o, _size in last), name
    assert 150 - 100 + 1 < TILE < 400 - 129 + 1 and INSIDE[1][3] // TILE == 1                          # case A in tile 0 and beyond it
    assert [_tiles(per, N_SHORT) for per in (100, 129, 300)] == [1, 2, 3]


# ---- 2. the form, the options -----------------------------------------------------------------------------------------------------------
def test_the_form_changes_nothing(lb, gpu, oracle):
    """form S forced where the plan takes form W: identical outputs, and the reference's"""
    m = _module(lb, gpu, oracle)
    try:
        for name, n in (("w129", N_CASE), ("w129", N_SHORT), ("w300", N_SHORT), ("w100", N_CASE)):
            _form, R, per = CASES[name]
            corpus, packed = m["corpus"][n], m["dev"][name]
            prof = [row[:n] for row in _profiles(m, name)]
            for t in (_thresholds(prof)["p999"], _thresholds(prof)["median"]):
                for peaks in (False, True):
                    for range_ in (0, 64):
                        assert _plan(lb, m, n, R, per)["form"] == FORM_W
                        wave = _batch(gpu, corpus, packed, R, per, t, peaks, CAP, range_=range_)
                        lb.debug_set_occurrences_batch_form(True)
                        assert _plan(lb, m, n, R, per)["form"] == FORM_S
                        shared = _batch(gpu, corpus, packed, R, per, t, peaks, CAP, range_=range_)
                        lb.debug_set_occurrences_batch_form(False)
                        _same(shared, wave)
                        if range_ == 0:
                            _same(shared, _expected(prof, n, t, peaks, CAP))
            tw = _tbatch(gpu, corpus, packed, R, per, 0.5, 16)
            lb.debug_set_occurrences_batch_form(True)
            _same(_tbatch(gpu, corpus, packed, R, per, 0.5, 16), tw)
            lb.debug_set_occurrences_batch_form(False)
    finally:
        lb.debug_set_occurrences_batch_form(False)


@pytest.mark.parametrize("name", ["w300", "s525"])
def test_a_masked_range(lb, gpu, oracle, name):
    """a range below the sub-fingerprint length: the non-FULL instances of both forms"""
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"][N_CASE], m["dev"][name]
    prof = _profiles(m, name, 64)
    ts = _thresholds(prof)
    for t in (ts["max"], ts["p999"], ts["median"]):
        for peaks in (False, True):
            got = _batch(gpu, corpus, packed, R, per, t, peaks, CAP, range_=64)
            _same(got, _expected(prof, N_CASE, t, peaks, CAP))
            _same(got, _single(gpu, corpus, packed, R, per, t, peaks, CAP, range_=64))
    got = _batch(gpu, corpus, packed, R, per, 0.75, True, CAP, range_=199)
    _same(got, _single(gpu, corpus, packed, R, per, 0.75, True, CAP, range_=199))


def test_odd_subfingerprint_length(lb, gpu, oracle):
    """sub-fingerprints of 37 Booleans, four recordings of 64: both cases, the full range and a shorter one"""
    rng = np.random.default_rng(5)
    ent = _random(oracle, 99, rng.integers(1, 41, 70), 37)
    ent[5] = _random(oracle, 98, [90], 37)[0]
    block = oracle.synth_ragged_entries(97, 0, np.array([4 * 64], np.uint32), 37).reshape(4, 64, 37).copy()
    block[1, 20:20 + len(ent[9])] = ent[9]
    block[3, 64 - len(ent[12]):] = ent[12]
    ent[5][20:20 + 64] = block[2]                                 # case A: a recording inside a longer entry
    corpus = _ragged(lb, gpu, oracle, ent, 37)
    packed = gpu.from_numpy(_packed(oracle, block.reshape(-1, 37))).cuda()
    for range_ in (0, 20):
        prof = [[profile(rec, x, range_) for x in ent] for rec in block]
        assert prof[2][5][1] and (range_ or prof[2][5][0][20] == 1.0)
        for peaks in (False, True):
            for t in _thresholds(prof).values():
                want = _expected(prof, len(ent), t, peaks, 512)
                got = _batch(gpu, corpus, packed, 4, 64, t, peaks, 512, range_=range_)
                _same(got, want)
                _same(got, _single(gpu, corpus, packed, 4, 64, t, peaks, 512, range_=range_))


@pytest.mark.parametrize("name", ["w129", "s525"])
def test_an_index_base(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"][N_CASE], m["dev"][name]
    prof = _profiles(m, name)
    t = _thresholds(prof)["p999"]
    zero = _batch(gpu, corpus, packed, R, per, t, True, CAP)
    for base in (1000, (1 << 32) - N_CASE):
        got = _batch(gpu, corpus, packed, R, per, t, True, CAP, base=base)
        _same(got, _expected(prof, N_CASE, t, True, CAP, base))
        _same(got, _single(gpu, corpus, packed, R, per, t, True, CAP, base=base))
        assert np.array_equal(got[0][got[0] != 0] + np.uint64(base), zero[0][zero[0] != 0]) and np.array_equal(got[1], zero[1])
        tgot = _tbatch(gpu, corpus, packed, R, per, t, 64, base=base)
        _same(tgot, _expected_threshold(prof, N_CASE, t, 64, base))
    for call in (lambda: _batch(gpu, corpus, packed, R, per, t, True, CAP, base=(1 << 32) - N_CASE + 1),
                 lambda: _tbatch(gpu, corpus, packed, R, per, t, 64, base=(1 << 32) - N_CASE + 1)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            call()
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")


@pytest.mark.parametrize("name", ["w300", "s525"])
def test_no_lags_changes_nothing(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"][N_CASE], m["dev"][name]
    prof = _profiles(m, name)
    for t in (_thresholds(prof)["p999"], _thresholds(prof)["median"]):
        for peaks in (False, True):
            want = _expected(prof, N_CASE, t, peaks, CAP)
            got = _batch(gpu, corpus, packed, R, per, t, peaks, CAP, want_lags=False)
            assert got[1] is None
            _same(got, want)
        want = _expected_threshold(prof, N_CASE, t, 64)
        got = _tbatch(gpu, corpus, packed, R, per, t, 64, want_lags=False)
        assert got[1] is None
        _same(got, want)


# ---- 3. plateaus ---------------------------------------------------------------------------------------------------------------------------
def test_a_plateau_reports_its_first_cell(lb, gpu, oracle):
    """the entry of ONE sub-fingerprint planted at adjacent offsets: neighbouring cells of 1.0 -- three across the tile seam, two at
    offset 0, two at the last offset.  Without peaks every cell matches, with peaks the first of each run only"""
    m = _module(lb, gpu, oracle)
    R, per = 5, 300
    block = m["blocks"]["w300"].copy()
    runs = {1: (TILE - 1, 3), 2: (0, 2), 4: (per - 2, 2)}
    for r, (o, width) in runs.items():
        block[r, o:o + width] = m["entries"][E1][0]
    packed = gpu.from_numpy(_packed(oracle, block.reshape(-1, L))).cuda()
    prof = [[profile(rec, ent, 0) for ent in m["entries"][:N_SHORT]] for rec in block]
    for n in (N_SHORT,):
        corpus = m["corpus"][n]
        flat = _expected(prof, n, 1.0, False, CAP)
        peak = _expected(prof, n, 1.0, True, CAP)
        for r, (o, width) in runs.items():
            q = prof[r][E1][0]
            assert (q[o:o + width] == ONE).all()                  # the reference holds the plateau ...
            mine = (np.uint64(ONE.view(np.uint32)) << np.uint64(32)) | np.uint64(0xFFFFFFFF - E1)
            assert sorted(flat[1][r][flat[0][r] == mine].tolist()) == sorted(-x for x in range(o, o + width))
            assert peak[1][r][peak[0][r] == mine].tolist() == [-o]     # ... and the rule keeps its first cell
        for peaks, want in ((False, flat), (True, peak)):
            got = _batch(gpu, corpus, packed, R, per, 1.0, peaks, CAP)
            _same(got, want)
            _same(got, _single(gpu, corpus, packed, R, per, 1.0, peaks, CAP))
            lb.debug_set_occurrences_batch_form(True)
            try:
                _same(_batch(gpu, corpus, packed, R, per, 1.0, peaks, CAP), want)
            finally:
                lb.debug_set_occurrences_batch_form(False)


# ---- 4. a row that overflows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w300", "s525"])
@pytest.mark.parametrize("peaks", [False, True])
def test_capacity_cut(lb, gpu, oracle, name, peaks):
    """a capacity that one row exceeds and its neighbours stay below, found in the reference: the counts are true, the cut row
    holds its first `capacity` matches, and no slot of another row is touched"""
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"][N_CASE], m["dev"][name]
    prof = _profiles(m, name)
    ts = _thresholds(prof)
    pick = None
    cells = np.sort(np.concatenate([p for row in prof for p, _ in row]))
    for t in [ts["max"], ts["4th"], ts["p999"]] + [cells[int(len(cells) * f)] for f in (0.9999, 0.9995, 0.998, 0.995)]:
        counts = _expected(prof, N_CASE, t, peaks, 1)[2]
        for r in range(R):
            near = [int(counts[x]) for x in (r - 1, r + 1) if 0 <= x < R]
            if int(counts[r]) >= max(near) + 2 and max(near) >= 1:
                pick = pick or (np.float32(t), r, int(counts[r]) - 1, near)
    assert pick is not None
    t, r, capacity, near = pick
    want = _expected(prof, N_CASE, t, peaks, capacity)
    assert want[2][r] > capacity and all(c < capacity for c in near)     # the reference: row r overflows, its neighbours do not
    got = _batch(gpu, corpus, packed, R, per, t, peaks, capacity)
    _same(got, want)                                              # (the neighbours' zero slots behind their matches included)
    _same(got, _single(gpu, corpus, packed, R, per, t, peaks, capacity))
    full = _expected(prof, N_CASE, t, peaks, capacity + 1)
    assert np.array_equal(got[0][r], full[0][r][:capacity]) and full[0][r][capacity] != 0
    # capacity 1: every row with a match is cut
    _same(_batch(gpu, corpus, packed, R, per, t, peaks, 1), _expected(prof, N_CASE, t, peaks, 1))


# ---- 5. passes and chunks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w300", "s525"])
def test_passes_and_chunks_change_nothing(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"][N_CASE], m["dev"][name]
    tiles = _tiles(per, N_CASE)
    prof = _profiles(m, name)
    ts = _thresholds(prof)
    try:
        corpus.set_join_scratch_limit(0)
        default = {(what, peaks): _batch(gpu, corpus, packed, R, per, ts[what], peaks, CAP) for what in ("p999", "median") for peaks in (False, True)}
        tdefault = _tbatch(gpu, corpus, packed, R, per, ts["p999"], 64)
        for key, got in default.items():
            _same(got, _expected(prof, N_CASE, ts[key[0]], key[1], CAP))
        # (a) several passes of two recordings, the last one partial; (b) one recording per pass in 2 and in 3 entry chunks
        for limit, rpp, chunk in ((2 * _scratch(3 * WALK, tiles) + 9, 2, 3 * WALK), (_scratch(3 * WALK, tiles), 1, 3 * WALK),
                                  (_scratch(3 * WALK, tiles) - 1, 1, 2 * WALK), (_scratch(WALK, tiles), 1, WALK)):
            plan = _plan(lb, m, N_CASE, R, per, limit)
            assert (plan["recordings_per_pass"], plan["entries_per_chunk"]) == (rpp, chunk) and plan["scratch_bytes"] <= limit
            corpus.set_join_scratch_limit(limit)
            for (what, peaks), want in default.items():
                _same(_batch(gpu, corpus, packed, R, per, ts[what], peaks, CAP), want)
            _same(_batch(gpu, corpus, packed, R, per, ts["median"], True, CAP, want_lags=False), (default[("median", True)][0], None,
                                                                                                 default[("median", True)][2]))
            _same(_tbatch(gpu, corpus, packed, R, per, ts["p999"], 64), tdefault)
        assert -(-N_CASE // WALK) == 3 and -(-R // 2) >= 2            # three chunks; two passes or more
        # a limit below one block of ONE recording
        corpus.set_join_scratch_limit(_scratch(WALK, tiles) - 1)
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            _batch(gpu, corpus, packed, R, per, ts["p999"], True, CAP)
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    finally:
        corpus.set_join_scratch_limit(0)


@pytest.mark.parametrize("name", ["w300", "s525"])
def test_second_trips(lb, gpu, oracle, name):
    """the grid-stride loops of both forms' kernels and of the compaction take a second trip"""
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"][N_CASE], m["dev"][name]
    prof = _profiles(m, name)
    t = _thresholds(prof)["median"]
    want = _expected(prof, N_CASE, t, True, CAP)
    try:
        for ceiling in (1, 4):
            lb.debug_set_grid_ceiling(ceiling)
            before = lb.debug_grid_ceiling()[1]
            _same(_batch(gpu, corpus, packed, R, per, t, True, CAP), want)
            assert lb.debug_grid_ceiling()[1] > before
            _same(_tbatch(gpu, corpus, packed, R, per, t, 64), _expected_threshold(prof, N_CASE, t, 64))
    finally:
        lb.debug_set_grid_ceiling(0)


# ---- 6. sizes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 17, 700])
def test_one_recording_is_the_single_call(lb, gpu, oracle, per):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"][N_CASE]
    q = _random(oracle, 900 + per, [per])[0]
    if per == 700:
        q[600:622] = m["entries"][E22]
    elif per == 17:
        q[:] = m["entries"][E17]
    packed = gpu.from_numpy(_packed(oracle, q)).cuda()
    prof = [[profile(q, ent, 0) for ent in m["entries"]]]
    for t in _thresholds(prof).values():
        for peaks in (False, True):
            got = _batch(gpu, corpus, packed, 1, per, t, peaks, CAP)
            _same(got, _single(gpu, corpus, packed, 1, per, t, peaks, CAP))
            _same(got, _expected(prof, N_CASE, t, peaks, CAP))
        tgot = _tbatch(gpu, corpus, packed, 1, per, t, 64)
        _same(tgot, _tsingle(gpu, corpus, packed, 1, per, t, 64))
        _same(tgot, _expected_threshold(prof, N_CASE, t, 64))


def test_the_empty_corpus(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    empty = lb.Corpus.ragged(L, 4, 16)
    packed = m["dev"]["w100"]
    for want_lags in (True, False):
        for got in (_batch(gpu, empty, packed, 5, 100, 0.5, True, 7, want_lags=want_lags),
                    _tbatch(gpu, empty, packed, 5, 100, 0.5, 7, want_lags=want_lags)):
            assert got[0].shape == (5, 7) and not got[0].any() and not got[2].any() and (got[1] is None or not got[1].any())


def test_refusals(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    packed = m["dev"]["w100"]
    above = _ragged(lb, gpu, oracle, _random(oracle, 5, [3, 1024 + 1, 2]))
    calls = ("query_packed_occurrences_batch_keys_device", "query_packed_recording_threshold_batch_keys_device")
    for corpus in (lb.Corpus(L, 4, 8), above):                    # a uniform corpus; an entry above the cap
        for call in calls:
            keys, lags, counts = _outputs(gpu, 5, 3, True)
            with pytest.raises(lb.LBAudioDetectiveError) as err:
                getattr(corpus, call)(packed, 5, 100, 0.5, 3, keys_out=keys, lags_out=lags, counts_out=counts)
            assert err.value.status == bad
            gpu.cuda.synchronize()
            assert bool((keys == POISON).all()) and bool((lags == POISON32).all()) and bool((counts == POISON).all())   # nothing written
    # R x capacity > 2^31 and a NULL outCounts: refused before the corpus is looked at, with real handles too
    corpus = m["corpus"][N_CASE]
    occ = lb.lib().LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice
    thr = lb.lib().LBAudioDetectiveCorpusQueryPackedRecordingThresholdBatchKeysDevice
    keys, lags, counts = _outputs(gpu, 5, 3, True)
    p, kp, lp, cp = packed.data_ptr(), keys.data_ptr(), lags.data_ptr(), counts.data_ptr()
    assert occ(corpus._ref, p, 5, 100, 0, 0.5, 1, (1 << 31) // 5 + 1, 0, kp, lp, cp, None) == bad
    assert thr(corpus._ref, p, 5, 100, 0, 0.5, (1 << 31) // 5 + 1, 0, kp, cp, lp, None) == bad
    assert occ(corpus._ref, p, 5, 100, 0, 0.5, 1, 3, 0, kp, lp, None, None) == bad
    assert thr(corpus._ref, p, 5, 100, 0, 0.5, 3, 0, kp, None, lp, None) == bad
    gpu.cuda.synchronize()
    assert bool((keys == POISON).all()) and bool((lags == POISON32).all()) and bool((counts == POISON).all())
    # a limit below one block of one recording
    try:
        corpus.set_join_scratch_limit(_scratch(WALK, _tiles(100, N_CASE)) - 1)
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            corpus.query_packed_occurrences_batch_keys_device(packed, 5, 100, 0.5, 3, keys_out=keys, lags_out=lags, counts_out=counts)
        assert err.value.status == bad
    finally:
        corpus.set_join_scratch_limit(0)


# ---- 7. the recording threshold batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("w100", N_SHORT), ("w129", N_CASE), ("w300", N_CASE), ("s525", N_CASE)])
def test_threshold_rows_equal_the_reference_and_the_existing_calls(lb, gpu, oracle, name, n):
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"][n], m["dev"][name]
    prof = [row[:n] for row in _profiles(m, name)]
    best = np.sort(np.array([max(np.float32(0), q.max()) for row in prof for q, _ in row], np.float32))
    ts = {"max": best[-1], "median": best[len(best) // 2], "low": best[best > 0][0], "one": np.float32(1.0), "above": np.float32(1.5)}
    for what, t in ts.items():
        for capacity in (N_CASE + 3, 5):
            want = _expected_threshold(prof, n, t, capacity)
            got = _tbatch(gpu, corpus, packed, R, per, t, capacity)
            _same(got, want)
            _same(got, _tsingle(gpu, corpus, packed, R, per, t, capacity))
            _same(got, _tscan(gpu, corpus, packed, R, per, t, capacity))
            if what in ("median", "low") and capacity == 5:
                assert (want[2] > capacity).all()                 # a capacity cut, the true counts
    got = _tbatch(gpu, corpus, packed, R, per, ts["median"], 7, range_=64)
    _same(got, _tsingle(gpu, corpus, packed, R, per, ts["median"], 7, range_=64))
    _same(got, _tscan(gpu, corpus, packed, R, per, ts["median"], 7, range_=64))


def test_threshold_of_nine_recordings(lb, gpu, oracle):
    """one recording more than the existing selection takes rows: still one compaction"""
    m = _module(lb, gpu, oracle)
    R, per = 9, 100
    block = oracle.synth_ragged_entries(31337, 0, np.array([R * per], np.uint32), L).reshape(R, per, L).copy()
    block[0, 3:25] = m["entries"][E22]
    block[8, per - 17:] = m["entries"][E17]
    block[7, per - 11:] = m["entries"][E22][:11]                  # the 22 across the seam of 7 | 8
    block[8, :11] = m["entries"][E22][11:]
    packed = gpu.from_numpy(_packed(oracle, block.reshape(-1, L))).cuda()
    prof = [[profile(rec, ent, 0) for ent in m["entries"]] for rec in block]
    corpus = m["corpus"][N_CASE]
    best = np.sort(np.array([q.max() for row in prof for q, _ in row], np.float32))
    for t in (np.float32(1.0), best[len(best) // 2], best[int(len(best) * 0.99)]):
        for capacity in (N_CASE, 4):
            want = _expected_threshold(prof, N_CASE, t, capacity)
            got = _tbatch(gpu, corpus, packed, R, per, t, capacity)
            _same(got, want)
            _same(got, _tsingle(gpu, corpus, packed, R, per, t, capacity))
            _same(got, _tscan(gpu, corpus, packed, R, per, t, capacity))
    one = _tbatch(gpu, corpus, packed, R, per, 1.0, 4)
    assert one[2].tolist() == [2, 0, 0, 0, 0, 0, 0, 0, 1] and one[1][0, :2].tolist() == [-3, -3] and one[1][8, 0] == -(per - 17)
    # the occurrences of the same nine
    t = best[int(len(best) * 0.99)]
    _same(_batch(gpu, corpus, packed, R, per, t, True, CAP), _expected(prof, N_CASE, t, True, CAP))


# ---- 8. two calls in a row on two streams ------------------------------------------------------------------------------------------------------
def test_two_streams_in_a_row(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"][N_CASE]
    names = ("s525", "w300", "w129", "w100")
    streams = [gpu.cuda.Stream() for _ in names]
    ts = {name: _thresholds(_profiles(m, name))["p999"] for name in names}
    outs = []
    for i, (s, name) in enumerate(zip(streams, names)):           # each call is made while the one before may still run
        _form, R, per = CASES[name]
        s.wait_stream(gpu.cuda.current_stream())
        keys, lags, counts = _outputs(gpu, R, 64 if i % 2 else CAP, True)
        if i % 2:
            corpus.query_packed_recording_threshold_batch_keys_device(m["dev"][name], R, per, float(ts[name]), 64, keys_out=keys,
                                                                      lags_out=lags, counts_out=counts, stream=s)
        else:
            corpus.query_packed_occurrences_batch_keys_device(m["dev"][name], R, per, float(ts[name]), CAP, peaks=True, keys_out=keys,
                                                              lags_out=lags, counts_out=counts, stream=s)
        outs.append((keys, lags, counts))
    for s in streams:
        s.synchronize()
    for i, (out, name) in enumerate(zip(outs, names)):
        prof = _profiles(m, name)
        want = _expected_threshold(prof, N_CASE, ts[name], 64) if i % 2 else _expected(prof, N_CASE, ts[name], True, CAP)
        _same(_host(*out), want)


# ---- 9. the stream bank --------------------------------------------------------------------------------------------------------------------------
def test_stream_bank_occurrences_and_matches_above(lb, gpu, oracle):
    """three channels of test_gpu_stream_bank.py's pruned configuration; the corpus holds random entries and, per channel, rows
    [total - 15, total - 5) of its own sub-fingerprints: StreamBank.occurrences and matches_above against the calls on
    window_device's block and against the reference, and two calls on two streams in a row"""
    rate, window, stride, bands, length = 44100, 1024, 64, 32, 200
    hop, frames, n = 128 * stride, 23, 20
    cfg = oracle.Config(rate, window, stride, bands, length)
    sig = [oracle.synth_clip(0x53424B31, c, rate, window + frames * hop + 7) for c in range(3)]
    ref = [oracle.fingerprint_pcm(s, cfg) for s in sig]
    det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
    bank = lb.StreamBank(det, 3, 24)
    bank.push_device(gpu.from_numpy(np.concatenate(sig).astype(np.float32)).cuda(), [s.size for s in sig])
    assert bank.totals().tolist() == [frames] * 3
    ent = _random(oracle, 61, np.random.default_rng(4).integers(1, 16, 30), length)
    ent.append(_random(oracle, 62, [31], length)[0])              # longer than the window: case A
    planted = {}
    for c in range(3):
        planted[c] = len(ent)
        ent.append(ref[c][frames - 15:frames - 5].copy())
    corpus = _ragged(lb, gpu, oracle, ent, length)
    channels = [2, 0, 1]
    win = bank.window_device(channels, n)
    gpu.cuda.synchronize()
    rows = lb.unpack_packed(win.cpu().numpy(), length).reshape(3, n, length)
    prof = [[profile(rows[j], e, 0) for e in ent] for j in range(3)]
    s1, s2 = gpu.cuda.Stream(), gpu.cuda.Stream()
    for s in (s1, s2):
        s.wait_stream(gpu.cuda.current_stream())
    occ = bank.occurrences(corpus, channels, n, 0.9, 16, stream=s1)                 # (peaks by default)
    above = bank.matches_above(corpus, channels, n, 0.9, 16, stream=s2)             # ... while the first may still run
    s1.synchronize()
    s2.synchronize()
    assert occ[0].shape == (3, 16) and occ[0].dtype == gpu.int64 and occ[1].dtype == gpu.int32 and occ[2].shape == (3,)
    _same(_host(*occ), _expected(prof, len(ent), 0.9, True, 16))
    _same(_host(*above), _expected_threshold(prof, len(ent), 0.9, 16))
    _same(_host(*occ), _batch(gpu, corpus, win, 3, n, 0.9, True, 16))
    _same(_host(*above), _tbatch(gpu, corpus, win, 3, n, 0.9, 16))
    flat = bank.occurrences(corpus, channels, n, 0.9, 16, peaks=False, want_lags=False)
    gpu.cuda.synchronize()
    assert flat[1] is None
    _same(_host(*flat), _expected(prof, len(ent), 0.9, False, 16))
    got = _host(*occ)
    for j, c in enumerate(channels):                              # the planted span: 1.0 at offset 5 of a window of 20
        key = (np.uint64(ONE.view(np.uint32)) << np.uint64(32)) | np.uint64(0xFFFFFFFF - planted[c])
        assert got[1][j][got[0][j] == key].tolist() == [-5]
