"""GPU tests of the tail peaks (LBAudioDetectiveCorpusQueryPackedOccurrencesTailPeaksBatchKeysDevice, k_occurrences_tail.hip's PEAKS
instances, StreamBank.new_peaks): the occurrences' peak rule for the cells a push has made judgeable, each judged one sub-fingerprint late.
Every key, lag and count is compared exactly against numpy (occurrences_tail_peaks_ref: align_ref.profile with the judged cells and
the peak rule restated) AND against the batch occurrences call, peaks ON, filtered on the host: nothing needs a tolerance.  Output
buffers are poison-filled before every call.  The corpus and the windows are test_gpu_occurrences_tail.py's: 150 ragged entries of 32
Booleans a sub-fingerprint -- 1 .. 40 sub-fingerprints, with one of 1, a planted 17, 22 and 44, one of 48 (the window), one of 49
and one of 300 --, nine windows of 48 and five of 80.  The thresholds are values of the reference's own cells.  The corpus, the
blocks, the profiles and the batch rows are made once per module."""
import numpy as np
import pytest

import occurrences_tail_peaks_ref as ref

pytestmark = pytest.mark.gpu

POISON = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
L = 32
WALK = 64
N_CASE = 150
E1, E17, E22, E48, E49, E300, E44 = 3, 7, 11, 20, 21, 22, 140
ONE = np.float32(1.0)
PER, R = 48, 9
NEW = [0, 1, 8, 3, 5, 2, 8, 20, 8]        # under max_new = 8 the 20 counts as 8; row 0 is a silent channel
PER80, R80 = 80, 5
NEW80 = [62, 80, 33, 0, 100]              # under max_new = 62
CAP = 64                                  # slots per row: the sparse thresholds fit, the median may be cut
BATCH_CAP = 16384                         # the batch call's rows hold EVERY peak of a window: at most 150 x 80 cells


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
    rng = np.random.default_rng(23)
    counts = rng.integers(1, 41, N_CASE)
    counts[E1], counts[5], counts[E17], counts[E22], counts[E44] = 1, 40, 17, 22, 44
    counts[E48], counts[E49], counts[E300] = PER, PER + 1, 300
    return _random(oracle, 5151, counts)


def _block(oracle, e):
    b = oracle.synth_ragged_entries(808, 0, np.array([R * PER], np.uint32), L).reshape(R, PER, L).copy()
    b[2, PER - 22:] = e[E22]                                      # ends at the newest record: the newest cell, final's
    b[4, PER - 1 - 17:PER - 1] = e[E17]                           # ends one record earlier: the newest JUDGED cell (d = 5)
    b[3, PER - 4 - 17:PER - 4] = e[E17]                           # ends at end - d - 1 (d = 3): judged one push ago
    b[6] = e[E48]                                                 # the window itself: last == 0
    b[8, 2:2 + 44] = e[E44]                                       # 48 - 44 - 8 < 0: the judged cells are clipped at offset 0
    return b


_M = {}


def _module(lb, gpu, oracle):
    if not _M:
        e = _entries(oracle)
        _M["entries"] = e
        _M["lengths"] = np.array([len(x) for x in e], np.int64)
        _M["corpus"] = _ragged(lb, gpu, oracle, e)
        _M["blocks"] = {"w48": _block(oracle, e),
                        "w80": oracle.synth_ragged_entries(909, 0, np.array([R80 * PER80], np.uint32), L).reshape(R80, PER80, L).copy()}
        _M["blocks"]["w80"][0, PER80 - 40:] = e[5]
        _M["blocks"]["w80"][2, PER80 - 33:PER80 - 33 + 22] = e[E22]
        _M["dev"] = {k: gpu.from_numpy(_packed(oracle, b.reshape(-1, L))).cuda() for k, b in _M["blocks"].items()}
        _M["profiles"] = {}
        _M["batch"] = {}
    return _M


def _profiles(m, name, range_=0):
    """align_ref's profiles of every row of a block against every entry, made once per (block, range)"""
    if (name, range_) not in m["profiles"]:
        m["profiles"][(name, range_)] = [ref.profiles(rec, m["entries"], range_) for rec in m["blocks"][name]]
    return m["profiles"][(name, range_)]


def _cells(m, name, new, max_new, final, range_=0):
    """the reference's judged cells of every row of a block, and the clamped counts"""
    per = m["blocks"][name].shape[1]
    ds = tuple(ref.clamp_new(n, max_new, per) for n in new)
    return [ref.judged_cells(p, per, d, final) for p, d in zip(_profiles(m, name, range_), ds)], ds


def _expected(rows, t, capacity, base=0):
    out = [ref.peaks_row(c, t, capacity, base) for c in rows]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64)


def _thresholds(rows):
    """values of the reference's own judged cells -- the largest, the 4th largest distinct and the median --, and 1.0 and 1.5"""
    cells = np.sort(np.array([q for row in rows for (_j, _o, q, _p) in row], np.float32))
    distinct = np.unique(cells)
    out = {"max": cells[-1], "4th": distinct[-min(4, len(distinct))], "median": cells[len(cells) // 2], "one": 1.0, "above": 1.5}
    return {k: np.float32(v) for k, v in out.items() if v > 0}


def _outputs(gpu, rows, capacity, want_lags=True):
    keys = gpu.full((rows, capacity), POISON, dtype=gpu.int64, device="cuda")
    lags = gpu.full((rows, capacity), POISON32, dtype=gpu.int32, device="cuda") if want_lags else None
    counts = gpu.full((rows,), POISON, dtype=gpu.int64, device="cuda")
    return keys, lags, counts


def _host(keys, lags, counts):
    return keys.cpu().numpy().view(np.uint64), lags.cpu().numpy() if lags is not None else None, counts.cpu().numpy()


def _peaks(gpu, corpus, packed, rows, per, new, max_new, final, t, capacity, range_=0, base=0, want_lags=True, stream=None):
    """one call into poison-filled buffers -> (keys uint64 [rows, capacity], lags int32 or None, counts int64 [rows])"""
    keys, lags, counts = _outputs(gpu, rows, capacity, want_lags)
    d_new = gpu.from_numpy(np.asarray(new, np.uint32).view(np.int32)).cuda()
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = corpus.query_packed_occurrences_tail_peaks_batch_keys_device(packed, rows, per, d_new, float(t), capacity, max_new=max_new,
                                                                       final=final, range_=range_, index_base=base, keys_out=keys,
                                                                       lags_out=lags, counts_out=counts, want_lags=want_lags,
                                                                       stream=stream)
    assert got[0] is keys and got[2] is counts and (got[1] is lags)
    if stream is not None:
        stream.synchronize()
    else:
        gpu.cuda.synchronize()
    return _host(keys, lags, counts)


def _filtered(m, gpu, name, ds, final, t, capacity, range_=0, base=0, corpus=None, dev=None, lengths=None):
    """the batch occurrences call with peaks ON on the same windows -- a module block by name (its full rows are kept), or a test's
    own corpus, block and entry lengths --, its rows cut down to the judged cells on the host; no batch row is cut"""
    if name is not None:
        corpus, dev, lengths = m["corpus"], m["dev"][name], m["lengths"]
    rows = len(ds)
    per = dev.shape[0] // rows
    key = (name, float(t), range_, base)
    full = m["batch"].get(key) if name is not None else None
    if full is None:
        keys, lags, counts = _outputs(gpu, rows, BATCH_CAP)
        corpus.query_packed_occurrences_batch_keys_device(dev, rows, per, float(t), BATCH_CAP, peaks=True, range_=range_, index_base=base,
                                                          keys_out=keys, lags_out=lags, counts_out=counts)
        gpu.cuda.synchronize()
        full = _host(keys, lags, counts)
        if name is not None:
            m["batch"][key] = full
    bk, bl, bc = full
    assert bc.max() <= BATCH_CAP                                     # no batch row is cut: the filter is exact
    out = [ref.filter_batch_row(bk[r], bl[r], int(bc[r]), lengths, per, ds[r], final, capacity, base) for r in range(rows)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64)


def _same(got, want):
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[0], want[0])
    if got[1] is not None and want[1] is not None:
        assert np.array_equal(got[1], want[1])


def _key(q, j, base=0):
    return np.uint64(ref.key_of(q, j, base))


def _lags_of(got, r, j, q=ONE):
    return got[1][r][got[0][r] == _key(q, j)].tolist()


SHAPES = [("w48", NEW, 8, 16), ("w48", NEW, 7, 16), ("w48", NEW, 6, 8), ("w48", NEW, 5, 8), ("w48", NEW, 1, 4),
          ("w80", NEW80, 62, 64), ("w80", NEW80, 33, 64), ("w80", NEW80, 30, 32)]


def _check_block(lb, gpu, m, name, new, max_new, final, range_=0, which=None):
    block = m["blocks"][name]
    rows, per = block.shape[0], block.shape[1]
    cells, ds = _cells(m, name, new, max_new, final, range_)
    ts = _thresholds(_cells(m, name, new, max_new, True, range_)[0])
    assert {"one", "above", "max"} <= set(ts)
    counts = {}
    for what, t in ts.items():
        if which and what not in which:
            continue
        want = _expected(cells, t, CAP)
        got = _peaks(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, final, t, CAP, range_=range_)
        _same(got, want)
        _same(got, _filtered(m, gpu, name, ds, final, t, CAP, range_=range_))
        counts[what] = want[2]
        if what == "above":
            assert not want[2].any() and not got[0].any() and not got[1].any()
    return cells, ds, counts


# ---- 1. rows against the reference and against the filtered batch call -----------------------------------------------------------------
@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("name,new,max_new,lanes", SHAPES)
def test_rows_equal_the_reference_and_the_filtered_batch_call(lb, gpu, oracle, name, new, max_new, lanes, final):
    m = _module(lb, gpu, oracle)
    per = m["blocks"][name].shape[1]
    assert lb.debug_occurrences_tail_peaks_plan(len(new), per, 1, 300, N_CASE, max_new)["lanes"] == lanes
    cells, ds, counts = _check_block(lb, gpu, m, name, new, max_new, final)
    assert max(ds) == min(max_new, per) and 0 in ds                 # a device count above the bound is clamped; a silent channel
    assert counts["median"].sum() > 0 and (final or counts["median"][list(ds).index(0)] == 0)
    # the entries longer than the window never appear
    everything = _peaks(gpu, m["corpus"], m["dev"][name], len(new), per, new, max_new, final, 1e-30, 4096)
    idx = 0xFFFFFFFF - (everything[0][everything[0] != 0] & np.uint64(0xFFFFFFFF))
    longer = {j for j in (E48, E49, E300) if m["lengths"][j] > per}
    assert longer and not (set(idx.tolist()) & longer) and everything[2].max() <= 4096


# ---- 2. plateaus ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("range_", [4, 2])
@pytest.mark.parametrize("name,new,max_new", [("w48", NEW, 8), ("w80", NEW80, 62)])
def test_masked_ranges_hold_plateaus(lb, gpu, oracle, name, new, max_new, range_):
    m = _module(lb, gpu, oracle)
    for final in (False, True):
        cells, _ds, _counts = _check_block(lb, gpu, m, name, new, max_new, final, range_=range_)
        t = _thresholds(_cells(m, name, new, max_new, True, range_)[0])["median"]
        flat = 0
        for row in cells:
            at = {(j, o): q for (j, o, q, _p) in row}
            flat += sum(1 for (j, o), q in at.items() if at.get((j, o + 1)) == q and q >= t)
        assert flat > 20, "the masked range leaves no equal neighbouring cells at or above the threshold"


def test_a_run_of_ones_reports_its_first_cell_once(lb, gpu, oracle):
    """a window whose last 30 records repeat one sub-fingerprint against an entry of 10 of the same: cells 18 .. 38 are 1.0, the
    first is reported and no other; cut across two calls (and the final one) the run is reported by exactly one of them"""
    rng = np.random.default_rng(77)
    x = rng.integers(0, 2, L).astype(np.uint8)
    x[0] = 1
    ent = [np.tile(x, (10, 1))] + _random(oracle, 31, [5, 12, 30])
    rec = oracle.synth_ragged_entries(32, 0, np.array([PER], np.uint32), L).copy()
    rec[17, :] = 1 - x                                               # the run begins at record 18
    rec[PER - 30:] = x
    corpus = _ragged(lb, gpu, oracle, ent)
    dev = gpu.from_numpy(_packed(oracle, rec)).cuda()
    q = ref.profiles(rec, ent)[0][1]
    assert (q[18:39] == ONE).all() and q[17] < ONE

    def call(n, d, max_new, final):
        got = _peaks(gpu, corpus, dev[:n].contiguous(), 1, n, [d], max_new, final, 1.0, CAP)
        _same(got, _expected([ref.judged_cells(ref.profiles(rec[:n], ent), n, min(d, n), final)], 1.0, CAP))
        return _lags_of(got, 0, 0)

    assert call(PER, 30, 30, False) == [-18] and call(PER, 30, 62, True) == [-18]       # the whole run in one call: its first cell
    assert call(PER, 8, 8, False) == [] and call(PER, 8, 8, True) == []                  # only inner cells are judged
    # across calls: 40 records with 25 new judge cells 5 .. 29, then 8 more judge 30 .. 37, then the final call judges 38
    assert [call(40, 25, 30, False), call(PER, 8, 8, False), call(PER, 0, 8, True)] == [[-18], [], []]
    # the cut INSIDE the run's head: cells up to 17 first, the run's first cell with the next push
    assert [call(28, 8, 8, False), call(34, 6, 8, False), call(PER, 14, 14, False), call(PER, 0, 1, True)] == [[], [-18], [], []]


# ---- 3. edges --------------------------------------------------------------------------------------------------------------------------
def test_edges(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    got, want = {}, {}
    for final in (False, True):
        cells, ds = _cells(m, "w48", NEW, 8, final)
        assert ds == (0, 1, 8, 3, 5, 2, 8, 8, 8)
        got[final] = _peaks(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, final, 1.0, CAP)
        want[final] = cells
        _same(got[final], _expected(cells, 1.0, CAP))
    # the entry of 44 in a window of 48 with d = 8: judged cells clipped at offset 0; the copy at offset 2
    assert list(ref.judged_range(PER, 44, 8, False)) == [0, 1, 2, 3] and any(j == E44 and o == 0 for (j, o, _q, _p) in want[False][8])
    assert _lags_of(got[False], 8, E44) == [-2] and _lags_of(got[True], 8, E44) == [-2]
    low = _peaks(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, False, 1e-30, 4096)
    _same(low, _expected(want[False], 1e-30, 4096))                  # (the o == 0 branch at every positive cell)
    assert low[2].max() <= 4096
    # the entry of 48: last == 0 -- nothing without final, one cell with it
    assert not any(j == E48 for row in want[False] for (j, _o, _q, _p) in row)
    assert [(o, p) for (j, o, _q, p) in want[True][6] if j == E48] == [(0, True)]
    assert _lags_of(got[False], 6, E48) == [] and _lags_of(got[True], 6, E48) == [0]
    # d == 0: nothing without final, the newest cell alone with it
    assert want[False][0] == [] and not got[False][0][0].any() and got[False][2][0] == 0
    assert all(o == PER - m["lengths"][j] for (j, o, _q, _p) in want[True][0]) and len(want[True][0]) == N_CASE - 2
    # a copy ending at the newest record is silent without final, reported with it
    assert _lags_of(got[False], 2, E22) == [] and _lags_of(got[True], 2, E22) == [-(PER - 22)]
    # a copy ending one record earlier is reported without final; one that ended a push ago by neither
    assert _lags_of(got[False], 4, E17) == [-(PER - 1 - 17)] and _lags_of(got[True], 4, E17) == [-(PER - 1 - 17)]
    assert _lags_of(got[False], 3, E17) == [] and _lags_of(got[True], 3, E17) == []
    assert dict(_profiles(m, "w48")[3])[E17][PER - 4 - 17] == ONE


# ---- 4. segment isolation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_new,lanes", [(2, 4), (6, 8)])
def test_a_neighbouring_recording_never_enters_the_peak_test(lb, gpu, oracle, max_new, lanes):
    """every lane of a recording holds a cell (d = max_new = D - 2); recording 1's newest cell -- its last lane, a peak under final
    by the 'does not exist' branch -- adjoins lane 0 of recording 2, and its lane 0 adjoins the last lane of recording 0.  A 1.0
    planted in those two lanes of the neighbours changes their rows and not recording 1's."""
    m = _module(lb, gpu, oracle)
    assert lb.debug_occurrences_tail_peaks_plan(R, PER, 1, 300, N_CASE, max_new)["lanes"] == lanes == max_new + 2
    new = [max_new] * R
    block = m["blocks"]["w48"].copy()
    profs = ref.profiles(block[1], m["entries"])
    pick = [j for (j, q) in profs if 5 <= m["lengths"][j] <= 30 and 0 < q[-1] < 1 and ref.is_peak(q, len(q) - 1)]
    assert pick, "recording 1 holds an entry whose newest cell is a peak only because nothing lies to its right"
    j = pick[0]
    n_j = int(m["lengths"][j])
    last = PER - n_j
    planted = block.copy()
    planted[2, last - max_new - 1:last - max_new - 1 + n_j] = m["entries"][j]        # lane 0 of recording 2: q = 1.0
    planted[0, last:] = m["entries"][j]                                                # the last lane of recording 0: q = 1.0
    t = np.float32(dict(profs)[j][-1])
    assert dict(ref.profiles(planted[2], m["entries"]))[j][last - max_new - 1] == ONE == dict(ref.profiles(planted[0], m["entries"]))[j][last]
    rows = {}
    for name, b in (("plain", block), ("planted", planted)):
        dev = gpu.from_numpy(_packed(oracle, b.reshape(-1, L))).cuda()
        cells = [ref.judged_cells(ref.profiles(b[r], m["entries"]), PER, max_new, True) for r in (0, 1, 2)]
        got = _peaks(gpu, m["corpus"], dev[:3 * PER], 3, PER, new[:3], max_new, True, t, 2048)
        _same(got, _expected(cells, t, 2048))
        assert got[2].max() <= 2048
        rows[name] = got
        whole = _peaks(gpu, m["corpus"], dev, R, PER, new, max_new, True, t, 2048)   # (all nine: several recordings a wave)
        for k in range(3):
            assert np.array_equal(whole[k][:3], got[k])
    for k in range(3):
        assert np.array_equal(rows["plain"][k][1], rows["planted"][k][1])            # recording 1: unchanged
    assert -last in rows["planted"][1][1][rows["planted"][0][1] == _key(t, j)].tolist()
    assert _key(ONE, j) in rows["planted"][0][0] and _key(ONE, j) not in rows["plain"][0][0]      # recording 0 reports its planted copy


# ---- 5. independence of max_new beyond the clamp ---------------------------------------------------------------------------------------
def test_max_new_beyond_the_clamp_changes_nothing(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    new = [0, 1, 5, 3, 5, 2, 4, 5, 5]
    for final in (False, True):
        cells, ds = _cells(m, "w48", new, 5, final)
        assert ds == tuple(new)
        t = _thresholds(cells)["median"]
        want = _expected(cells, t, CAP)
        for max_new in (5, 8, 20, 62):
            _same(_peaks(gpu, m["corpus"], m["dev"]["w48"], R, PER, new, max_new, final, t, CAP), want)


# ---- 6. overflow -----------------------------------------------------------------------------------------------------------------------
def test_a_row_that_overflows_writes_nothing_next_door(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    cells, _ds = _cells(m, "w48", NEW, 8, False)
    found = None
    for t in list(_thresholds(cells).values()) + [np.float32(1e-30)]:
        counts = _expected(cells, t, 1)[2]
        cap = int(max(counts[1], counts[3]))
        if cap >= 1 and counts[2] > cap:
            found = (t, cap, counts)
    assert found, "the reference holds a capacity that row 2 alone exceeds among its neighbours"
    t, cap, counts = found
    want = _expected(cells, t, cap)
    got = _peaks(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, False, t, cap)
    _same(got, want)
    assert got[2][2] == counts[2] > cap and got[2][1] <= cap and got[2][3] <= cap
    assert np.count_nonzero(got[0][2]) == cap and np.count_nonzero(got[0][1]) == counts[1] and np.count_nonzero(got[0][3]) == counts[3]
    one = _peaks(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, False, t, 1)                     # capacity 1
    _same(one, _expected(cells, t, 1))
    assert one[2].max() > 1


# ---- 7. passes and chunks, 8. second trips ---------------------------------------------------------------------------------------------
def _scratch(entries):
    return 24 + entries * 24 + -(-entries // WALK) * 4


def test_passes_and_chunks_change_nothing(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"]
    try:
        for final in (False, True):
            cells, _ds = _cells(m, "w48", NEW, 8, final)
            ts = _thresholds(cells)
            want = {k: _expected(cells, ts[k], CAP) for k in ("4th", "median")}
            corpus.set_join_scratch_limit(0)
            for k, w in want.items():
                _same(_peaks(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, final, ts[k], CAP), w)
            # passes of two recordings; one recording a pass in chunks of 128 and of 64 entries with the carried total
            for limit, rpp, chunk in ((2 * _scratch(192) + 9, 2, 192), (_scratch(128), 1, 128), (_scratch(WALK), 1, WALK)):
                plan = lb.debug_occurrences_tail_peaks_plan(R, PER, 1, 300, N_CASE, 8, limit)
                assert (plan["recordings_per_pass"], plan["entries_per_chunk"]) == (rpp, chunk) and plan["scratch_bytes"] <= limit
                corpus.set_join_scratch_limit(limit)
                for k, w in want.items():
                    _same(_peaks(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, final, ts[k], CAP), w)
                _same(_peaks(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, final, ts["median"], CAP, want_lags=False),
                      (want["median"][0], None, want["median"][2]))
        corpus.set_join_scratch_limit(_scratch(WALK) - 1)            # a limit below one block of ONE recording
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            _peaks(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, False, 0.5, CAP)
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    finally:
        corpus.set_join_scratch_limit(0)


@pytest.mark.parametrize("name,new,max_new,units", [("w48", NEW, 8, 3), ("w80", NEW80, 62, 6)])
def test_second_trips(lb, gpu, oracle, name, new, max_new, units):
    """the strided unit loop of both kernels takes a second trip: blocks of entries x groups of recordings units under a ceiling"""
    m = _module(lb, gpu, oracle)
    block = m["blocks"][name]
    rows, per = block.shape[0], block.shape[1]
    plan = lb.debug_occurrences_tail_peaks_plan(rows, per, 1, 300, N_CASE, max_new)
    assert -(-N_CASE // WALK) * -(-rows // plan["recordings_per_workgroup"]) == units
    moved = 0
    try:
        for final in (False, True):
            cells, _ds = _cells(m, name, new, max_new, final)
            t = _thresholds(cells)["median"]
            want = _expected(cells, t, CAP)
            assert want[2].sum() > 0
            for ceiling in (1, 3, 4, 6):
                lb.debug_set_grid_ceiling(ceiling)
                before = lb.debug_grid_ceiling()[1]
                _same(_peaks(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, final, t, CAP), want)
                assert units <= ceiling or lb.debug_grid_ceiling()[1] > before
                moved += lb.debug_grid_ceiling()[1] > before
    finally:
        lb.debug_set_grid_ceiling(0)
    assert moved >= 4                                                # the strided-launch counter moved


# ---- 9. long entries -------------------------------------------------------------------------------------------------------------------
def test_long_entries_lower_the_recordings_per_workgroup(lb, gpu, oracle):
    """the entry of 300 in windows of 320: 315 records a window, 12 windows fit the LDS where 16 have lanes; 13 recordings: two groups"""
    m = _module(lb, gpu, oracle)
    per, rows = 320, 13
    ent = m["entries"][:30]                                          # holds the entries of 48, 49 and 300
    lengths = m["lengths"][:30]
    plan = lb.debug_occurrences_tail_peaks_plan(rows, per, 1, 300, len(ent), 8)
    assert (plan["lanes"], plan["recordings_per_workgroup"], plan["window_records"]) == (16, 12, 315)
    assert plan["lds_bytes"] == 12 * 315 * 36 + 5151 * 4 <= 160 * 1024 - 64 < 13 * 315 * 36 + 5151 * 4       # the LDS requested
    new = [8, 3, 0, 5, 1, 8, 8, 2, 7, 8, 4, 6, 8]
    block = oracle.synth_ragged_entries(78, 0, np.array([rows * per], np.uint32), L).reshape(rows, per, L).copy()
    block[0, per - 300 - 1:per - 1] = ent[E300]                      # ends one record before the newest: judged without final
    block[12, per - 300:] = ent[E300]                                # ends at the newest record (the second group): final's
    block[5, per - 300 - 8:per - 8] = ent[E300]                      # the oldest judged cell of d = 8
    corpus = _ragged(lb, gpu, oracle, ent)
    dev = gpu.from_numpy(_packed(oracle, block.reshape(-1, L))).cuda()
    profs = [ref.profiles(rec, ent) for rec in block]
    for final in (False, True):
        cells = [ref.judged_cells(p, per, d, final) for p, d in zip(profs, new)]
        for what, t in _thresholds(cells).items():
            if what in ("4th", "one", "median"):
                got = _peaks(gpu, corpus, dev, rows, per, new, 8, final, t, CAP)
                _same(got, _expected(cells, t, CAP))
                _same(got, _filtered(None, gpu, None, tuple(new), final, t, CAP, corpus=corpus, dev=dev, lengths=lengths))
        got = _peaks(gpu, corpus, dev, rows, per, new, 8, final, 1.0, CAP)
        assert _lags_of(got, 0, E300) == [-19] and _lags_of(got, 5, E300) == [-12] and _lags_of(got, 12, E300) == ([-20] if final else [])


# ---- 10. odds and ends -----------------------------------------------------------------------------------------------------------------
def test_one_recording(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    for final in (False, True):
        cells, _ds = _cells(m, "w48", NEW, 8, final)
        t = _thresholds(cells)["4th"]
        for r in (2, 4, 0, 8):
            got = _peaks(gpu, m["corpus"], m["dev"]["w48"][r * PER:(r + 1) * PER], 1, PER, NEW[r:r + 1], 8, final, t, CAP)
            _same(got, _expected(cells[r:r + 1], t, CAP))


def test_the_empty_corpus_and_no_entry_that_takes_part(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    empty = lb.Corpus.ragged(L, 4, 16)
    longer = _ragged(lb, gpu, oracle, [m["entries"][E49], m["entries"][E300]])
    for final in (False, True):
        for corpus in (empty, longer):
            got = _peaks(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, final, 1e-30, CAP)
            assert not got[0].any() and not got[1].any() and not got[2].any()


def test_no_lags_and_an_index_base(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    cells, ds = _cells(m, "w48", NEW, 8, True)
    ts = _thresholds(cells)
    want = _expected(cells, ts["median"], CAP)
    _same(_peaks(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, True, ts["median"], CAP, want_lags=False), (want[0], None, want[2]))
    base = (1 << 32) - N_CASE                                       # the last index a corpus may have
    for b in (1000, base):
        got = _peaks(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, True, ts["4th"], CAP, base=b)
        _same(got, _expected(cells, ts["4th"], CAP, base=b))
    _same(got, _filtered(m, gpu, "w48", ds, True, ts["4th"], CAP, base=base))


def test_odd_subfingerprint_length(lb, gpu, oracle):
    """sub-fingerprints of 37 Booleans, five windows of 50, the full range and a shorter one"""
    rng = np.random.default_rng(5)
    ent = _random(oracle, 99, rng.integers(1, 41, 70), 37)
    rows, per, new = 5, 50, [3, 8, 0, 5, 1]
    block = oracle.synth_ragged_entries(97, 0, np.array([rows * per], np.uint32), 37).reshape(rows, per, 37).copy()
    block[1, per - 1 - len(ent[9]):per - 1] = ent[9]
    corpus = _ragged(lb, gpu, oracle, ent, 37)
    dev = gpu.from_numpy(_packed(oracle, block.reshape(-1, 37))).cuda()
    lengths = np.array([len(e) for e in ent], np.int64)
    for range_ in (0, 21):
        profs = [ref.profiles(rec, ent, range_) for rec in block]
        for final in (False, True):
            cells = [ref.judged_cells(p, per, d, final) for p, d in zip(profs, new)]
            for t in _thresholds(cells).values():
                got = _peaks(gpu, corpus, dev, rows, per, new, 8, final, t, CAP, range_=range_)
                _same(got, _expected(cells, t, CAP))
                _same(got, _filtered(None, gpu, None, tuple(new), final, t, CAP, range_=range_, corpus=corpus, dev=dev, lengths=lengths))


def test_the_host_sequence_is_the_device_tensor(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    cells, _ds = _cells(m, "w48", NEW, 20, False)
    t = _thresholds(cells)["4th"]
    want = _expected(cells, t, CAP)
    keys, lags, counts = m["corpus"].query_packed_occurrences_tail_peaks_batch_keys_device(m["dev"]["w48"], R, PER, NEW, float(t), CAP)
    gpu.cuda.synchronize()                                          # (max_new: the sequence's maximum, 20)
    assert keys.shape == (R, CAP) and keys.dtype == gpu.int64 and lags.dtype == gpu.int32 and counts.shape == (R,)
    _same(_host(keys, lags, counts), want)
    with pytest.raises(ValueError):
        m["corpus"].query_packed_occurrences_tail_peaks_batch_keys_device(m["dev"]["w48"], R, PER, gpu.zeros(R, dtype=gpu.int32, device="cuda"),
                                                                          float(t), CAP)
    with pytest.raises(lb.LBAudioDetectiveError):                   # above the cap of 62
        m["corpus"].query_packed_occurrences_tail_peaks_batch_keys_device(m["dev"]["w48"], R, PER, NEW, float(t), CAP, max_new=63)


def test_four_calls_on_four_streams(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    shapes = (("w48", NEW, 8, False), ("w80", NEW80, 62, True), ("w48", NEW, 5, True), ("w80", NEW80, 33, False))
    streams = [gpu.cuda.Stream() for _ in shapes]
    outs, wants, held = [], [], []
    for s, (name, new, max_new, final) in zip(streams, shapes):    # each call is made while the one before may still run
        block = m["blocks"][name]
        cells, _ds = _cells(m, name, new, max_new, final)
        t = _thresholds(cells)["median"]
        wants.append(_expected(cells, t, CAP))
        out = _outputs(gpu, block.shape[0], CAP)
        d_new = gpu.from_numpy(np.asarray(new, np.uint32).view(np.int32)).cuda()
        held.append(d_new)
        s.wait_stream(gpu.cuda.current_stream())
        m["corpus"].query_packed_occurrences_tail_peaks_batch_keys_device(m["dev"][name], block.shape[0], block.shape[1], d_new, float(t),
                                                                          CAP, max_new=max_new, final=final, keys_out=out[0],
                                                                          lags_out=out[1], counts_out=out[2], stream=s)
        outs.append(out)
    for s in streams:
        s.synchronize()
    for out, want in zip(outs, wants):
        _same(_host(*out), want)


# ---- 11. a channel's life --------------------------------------------------------------------------------------------------------------
def test_every_peak_of_a_channels_life_exactly_once(lb, gpu, oracle):
    """a recording of 400 sub-fingerprints in random pushes of 0 .. 8, windows of min(total, 64) (the entries of at most 49 + 8 + 1
    fit the condition; the one of 300 is longer than every window), then the final call: the union of the rows at absolute
    positions is the reference's peaks of the whole recording AND the single occurrences call's with peaks on, nothing twice"""
    m = _module(lb, gpu, oracle)
    total, window = 400, 64
    rec = oracle.synth_ragged_entries(4711, 0, np.array([total], np.uint32), L).copy()
    e = m["entries"]
    for at, j in ((0, 5), (30, 9), (41, 33), (100, 60), (160, 5), (230, E48), (399, E1)):
        rec[at:at + len(e[j])][:total - at] = e[j][:total - at]
    rec[300:330] = rec[300]                                          # a run of one sub-fingerprint: plateaus of every short entry's profile
    rec[total - 17:] = e[E17]                                        # ends at the last record: the final call's
    short = [x if len(x) <= window else np.zeros((0, L), np.uint8) for x in e]
    whole = ref.profiles(rec, short)
    values = np.sort(np.concatenate([q for (_j, q) in whole]))
    t = np.float32(values[int(len(values) * 0.97)])
    want = sorted((j, o, int(q[o].view(np.uint32))) for (j, q) in whole for o in range(len(q)) if q[o] >= t and ref.is_peak(q, o))
    flat = sum(1 for (_j, q) in whole for o in range(len(q) - 1) if q[o] == q[o + 1] >= t)
    assert len(want) > 200 and flat > 20 and (E17, total - 17, 0x3F800000) in want and (E48, 230, 0x3F800000) in want
    dev = gpu.from_numpy(_packed(oracle, rec)).cuda()
    rng = np.random.default_rng(8)
    pushes = []
    while sum(pushes) < total:
        pushes.append(int(min(rng.integers(0, 9), total - sum(pushes))))
    assert 0 in pushes and 8 in pushes
    seen = []
    for (fed, n, d, final) in ref.life_calls(pushes, lambda fed, d: window):
        assert n == fed or n >= 49 + d + 1
        keys, lags, counts = m["corpus"].query_packed_occurrences_tail_peaks_batch_keys_device(dev[fed - n:fed].contiguous(), 1, n, [d],
                                                                                               float(t), 2048, max_new=8, final=final)
        gpu.cuda.synchronize()
        assert int(counts[0]) <= 2048
        (idx, sc, start), = lb.decode_tail_occurrences(keys, lags, counts, [fed], n)
        seen.extend(zip(idx.tolist(), start.tolist(), sc.view(np.uint32).tolist()))
    assert len(seen) == len(set(seen)), "a peak is reported twice"
    assert sorted(seen) == want
    keys, lags, count = m["corpus"].query_packed_occurrences_keys_device(dev, total, float(t), 16384, peaks=True)
    gpu.cuda.synchronize()
    assert int(count[0]) <= 16384
    idx, sc, lag = lb.decode_occurrence_keys(keys, lags, int(count[0]))
    single = sorted((int(j), -int(g), int(b)) for j, g, b in zip(idx, lag, sc.view(np.uint32)) if m["lengths"][j] <= window)
    assert single == want


# ---- 12. the stream bank ---------------------------------------------------------------------------------------------------------------
def test_stream_bank_new_peaks(lb, gpu, oracle):
    """three channels of test_gpu_stream_bank.py's pruned configuration, two pushes; the corpus holds random entries and, per
    channel, a span of its own sub-fingerprints that ends at the newest one, and one that ends one earlier: StreamBank.new_peaks
    against the call on window_device's block with the push's new counts, and against the reference; final=True flushes the
    newest cell before a reset"""
    rate, window, stride, bands, length = 44100, 1024, 64, 32, 200
    hop, frames, n = 128 * stride, 23, 20
    cfg = oracle.Config(rate, window, stride, bands, length)
    sig = [oracle.synth_clip(0x53424B31, c, rate, window + frames * hop + 7) for c in range(3)]
    fps = [oracle.fingerprint_pcm(s, cfg) for s in sig]
    det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
    bank = lb.StreamBank(det, 3, 24)
    cuts = [window + 19 * hop + 3, window + 17 * hop + 100, window + 22 * hop + 5]           # 19, 17 and 22 frames first
    first = [s[:c] for s, c in zip(sig, cuts)]
    rest = [s[c:] for s, c in zip(sig, cuts)]
    bank.push_device(gpu.from_numpy(np.concatenate(first).astype(np.float32)).cuda(), [s.size for s in first])
    before = bank.totals().astype(np.int64)
    new, _ = bank.push_device(gpu.from_numpy(np.concatenate(rest).astype(np.float32)).cuda(), [s.size for s in rest])
    assert bank.totals().tolist() == [frames] * 3 and new.tolist() == (frames - before).tolist()
    assert 1 <= new.min() and new.max() <= 8 and len(set(new.tolist())) == 3
    ent = _random(oracle, 61, np.random.default_rng(4).integers(1, 16, 30), length)
    newest, earlier = {}, {}
    for c in range(3):
        newest[c] = len(ent)
        ent.append(fps[c][frames - 10:frames].copy())               # ends at the newest sub-fingerprint
        earlier[c] = len(ent)
        ent.append(fps[c][frames - 8:frames - 1].copy())            # ends one earlier
    corpus = _ragged(lb, gpu, oracle, ent, length)
    channels = [2, 0, 1]
    listed = [int(new[c]) for c in channels]
    got = bank.new_peaks(corpus, channels, n, new, 0.9, 16)
    win = bank.window_device(channels, n)
    gpu.cuda.synchronize()
    _same(_host(*got), _peaks(gpu, corpus, win, 3, n, listed, max(listed), False, 0.9, 16))
    rows = lb.unpack_packed(win.cpu().numpy(), length).reshape(3, n, length)
    profs = [ref.profiles(rows[j], ent) for j in range(3)]
    _same(_host(*got), _expected([ref.judged_cells(profs[j], n, listed[j], False) for j in range(3)], 0.9, 16))
    decoded = lb.decode_tail_occurrences(*got, bank.totals()[channels], n)
    for j, c in enumerate(channels):
        idx, sc, start = decoded[j]
        assert start[(idx == earlier[c]) & (sc == ONE)].tolist() == [frames - 8]
        assert not ((idx == newest[c]) & (start == frames - 10)).any()
    # the end of the stream: no new sub-fingerprints, final -- the newest cell alone, then the channels may be reset
    last = bank.new_peaks(corpus, channels, n, [0, 0, 0], 0.9, 16, final=True)
    gpu.cuda.synchronize()
    _same(_host(*last), _expected([ref.judged_cells(profs[j], n, 0, True) for j in range(3)], 0.9, 16))
    decoded = lb.decode_tail_occurrences(*last, bank.totals()[channels], n)
    for j, c in enumerate(channels):
        idx, sc, start = decoded[j]
        assert start[(idx == newest[c]) & (sc == ONE)].tolist() == [frames - 10]
        assert not ((idx == earlier[c]) & (start == frames - 8)).any()
    bank.reset(channels)
