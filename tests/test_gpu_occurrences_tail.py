"""GPU tests of the tail occurrences (LBAudioDetectiveCorpusQueryPackedOccurrencesTailBatchKeysDevice, k_occurrences_tail.hip,
StreamBank.new_occurrences): of the batch occurrences only the cells whose entry ends inside a recording's newest sub-fingerprints.
Every key, lag and count is compared exactly against numpy (occurrences_tail_ref: align_ref.profile with the cell rule restated)
AND against the batch occurrences call, peaks off, filtered on the host: nothing needs a tolerance.  Output buffers are
poison-filled before every call.  The corpus: 150 ragged entries of 32 Booleans a sub-fingerprint -- 1 .. 40 sub-fingerprints, with
one of 1, a planted 17, 22 and 44, one of 48 (the window), one of 49 and one of 300 (both longer than the window: skipped) --, which
crosses the seams of 64 and 128 entries; nine windows of 48 (not a multiple of any number of recordings a workgroup takes) and five
of 80.  The thresholds are values of the reference's own cells.  The corpus, the blocks and the reference are made once per module."""
import numpy as np
import pytest

import occurrences_tail_ref as ref

pytestmark = pytest.mark.gpu

POISON = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
L = 32
WALK = 64
N_CASE = 150
E1, E17, E22, E48, E49, E300, E44 = 3, 7, 11, 20, 21, 22, 140
ONE = np.float32(1.0)
PER, R = 48, 9
NEW = [0, 1, 8, 3, 5, 2, 8, 20, 8]        # under max_new = 8 the 20 counts as 8; row 2 is longer than both its neighbours
PER64, R64 = 80, 5
NEW64 = [64, 80, 33, 0, 100]              # under max_new = 64
CAP = 64                                  # slots per row: the sparse thresholds fit, the median is cut
BATCH_CAP = 16384                         # the batch call's rows hold EVERY match of a window


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
    b[2, PER - 22:] = e[E22]                                      # ends at the last record: the newest cell
    b[4, PER - 5 + 1 - 17:PER - 5 + 1] = e[E17]                   # ends at end - d + 1 (d = 5): the oldest new cell
    b[3, PER - 3 - 17:PER - 3] = e[E17]                           # ends at end - d (d = 3): one too old
    b[6, PER - 11:] = e[E22][:11]                                 # in the packed block the 22 lies verbatim across the seam 6 | 7
    b[7, :11] = e[E22][11:]
    assert np.array_equal(b.reshape(R * PER, L)[7 * PER - 11:7 * PER + 11], e[E22])
    b[8, 2:2 + 44] = e[E44]                                       # 48 - 44 - 8 + 1 < 0: the cells are clipped at offset 0
    return b


_M = {}


def _module(lb, gpu, oracle):
    if not _M:
        e = _entries(oracle)
        _M["entries"] = e
        _M["lengths"] = np.array([len(x) for x in e], np.int64)
        _M["corpus"] = _ragged(lb, gpu, oracle, e)
        _M["blocks"] = {"w48": _block(oracle, e),
                        "w80": oracle.synth_ragged_entries(909, 0, np.array([R64 * PER64], np.uint32), L).reshape(R64, PER64, L).copy()}
        _M["blocks"]["w80"][0, PER64 - 40:] = e[5]
        _M["blocks"]["w80"][2, PER64 - 33:PER64 - 33 + 22] = e[E22]
        _M["dev"] = {k: gpu.from_numpy(_packed(oracle, b.reshape(-1, L))).cuda() for k, b in _M["blocks"].items()}
        _M["cells"] = {}
        _M["batch"] = {}
    return _M


def _cells(m, name, new, max_new, range_=0):
    """the reference's cells of every row of a block, made once per (block, clamped counts, range)"""
    block = m["blocks"][name]
    ds = tuple(ref.clamp_new(n, max_new, block.shape[1]) for n in new)
    if (name, ds, range_) not in m["cells"]:
        m["cells"][(name, ds, range_)] = [ref.tail_cells(rec, m["entries"], d, range_) for rec, d in zip(block, ds)]
    return m["cells"][(name, ds, range_)], ds


def _expected(rows, t, capacity, base=0):
    out = [ref.tail_row(c, t, capacity, base) for c in rows]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64)


def _thresholds(rows):
    """values of the reference's own cells -- the largest, the 4th largest distinct and the median --, and 1.0 and 1.5 as such"""
    cells = np.sort(np.array([q for row in rows for (_j, _o, q) in row], np.float32))
    distinct = np.unique(cells)
    out = {"max": cells[-1], "4th": distinct[-4], "median": cells[len(cells) // 2], "one": 1.0, "above": 1.5}
    return {k: np.float32(v) for k, v in out.items() if v > 0}


def _outputs(gpu, rows, capacity, want_lags=True):
    keys = gpu.full((rows, capacity), POISON, dtype=gpu.int64, device="cuda")
    lags = gpu.full((rows, capacity), POISON32, dtype=gpu.int32, device="cuda") if want_lags else None
    counts = gpu.full((rows,), POISON, dtype=gpu.int64, device="cuda")
    return keys, lags, counts


def _host(keys, lags, counts):
    return keys.cpu().numpy().view(np.uint64), lags.cpu().numpy() if lags is not None else None, counts.cpu().numpy()


def _tail(gpu, corpus, packed, rows, per, new, max_new, t, capacity, range_=0, base=0, want_lags=True, stream=None, device_counts=True):
    """one tail call into poison-filled buffers -> (keys uint64 [rows, capacity], lags int32 or None, counts int64 [rows])"""
    keys, lags, counts = _outputs(gpu, rows, capacity, want_lags)
    if device_counts:
        new = gpu.from_numpy(np.asarray(new, np.uint32).view(np.int32)).cuda()
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = corpus.query_packed_occurrences_tail_batch_keys_device(packed, rows, per, new, float(t), capacity, max_new=max_new, range_=range_,
                                                                 index_base=base, keys_out=keys, lags_out=lags, counts_out=counts,
                                                                 want_lags=want_lags, stream=stream)
    assert got[0] is keys and got[2] is counts and (got[1] is lags)
    if stream is not None:
        stream.synchronize()
    else:
        gpu.cuda.synchronize()
    return _host(keys, lags, counts)


def _filtered(m, gpu, name, ds, t, capacity, range_=0, base=0, corpus=None, dev=None, lengths=None):
    """the batch occurrences call (peaks off) on the same windows -- a module block by name (its full rows are kept), or a test's own
    corpus, block and entry lengths --, its rows cut down to the tail cells on the host"""
    if name is not None:
        corpus, dev, lengths = m["corpus"], m["dev"][name], m["lengths"]
    rows = len(ds)
    per = dev.shape[0] // rows
    key = (name, float(t), range_, base)
    full = m["batch"].get(key) if name is not None else None
    if full is None:
        keys, lags, counts = _outputs(gpu, rows, BATCH_CAP)
        corpus.query_packed_occurrences_batch_keys_device(dev, rows, per, float(t), BATCH_CAP, peaks=False, range_=range_, index_base=base,
                                                          keys_out=keys, lags_out=lags, counts_out=counts)
        gpu.cuda.synchronize()
        full = _host(keys, lags, counts)
        if name is not None:
            m["batch"][key] = full
    bk, bl, bc = full
    out = [ref.filter_batch_row(bk[r], bl[r], int(bc[r]), lengths, per, ds[r], capacity, base) for r in range(rows)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64)


def _same(got, want):
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[0], want[0])
    if got[1] is not None and want[1] is not None:
        assert np.array_equal(got[1], want[1])


def _key(q, j, base=0):
    return np.uint64(ref.key_of(q, j, base))


# ---- 1. rows against the reference and against the filtered batch call -----------------------------------------------------------------
@pytest.mark.parametrize("name,new,max_new", [("w48", NEW, 8), ("w48", NEW, 5), ("w48", NEW, 1), ("w80", NEW64, 64), ("w80", NEW64, 33)])
def test_rows_equal_the_reference_and_the_filtered_batch_call(lb, gpu, oracle, name, new, max_new):
    m = _module(lb, gpu, oracle)
    block = m["blocks"][name]
    rows, per = block.shape[0], block.shape[1]
    cells, ds = _cells(m, name, new, max_new)
    assert max(ds) == min(max_new, per) and 0 in ds                 # a device count above the bound is clamped; a silent channel
    ts = _thresholds(cells)
    assert set(ts) == {"max", "4th", "median", "one", "above"}
    for what, t in ts.items():
        want = _expected(cells, t, CAP)
        got = _tail(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, t, CAP)
        _same(got, want)
        _same(got, _filtered(m, gpu, name, ds, t, CAP))
        if what == "median" and max_new > 1:
            assert want[2].max() > CAP                              # the median cuts rows: true counts, zeros never, nothing next door
        if what == "above":
            assert not want[2].any() and not got[0].any() and not got[1].any()
    # the skipped entries never appear, the window-long one does
    everything = _tail(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, 1e-30, 4096)
    idx = 0xFFFFFFFF - (everything[0][everything[0] != 0] & np.uint64(0xFFFFFFFF))
    longer = {j for j in (E48, E49, E300) if m["lengths"][j] > per}
    assert longer and not (set(idx.tolist()) & longer) and E1 in idx


def test_the_host_sequence_is_the_device_tensor(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    cells, _ds = _cells(m, "w48", NEW, 20)
    t = _thresholds(cells)["4th"]
    want = _expected(cells, t, CAP)
    keys, lags, counts = m["corpus"].query_packed_occurrences_tail_batch_keys_device(m["dev"]["w48"], R, PER, NEW, float(t), CAP)
    gpu.cuda.synchronize()                                          # (max_new: the sequence's maximum, 20)
    assert keys.shape == (R, CAP) and keys.dtype == gpu.int64 and lags.dtype == gpu.int32 and counts.shape == (R,)
    _same(_host(keys, lags, counts), want)
    with pytest.raises(ValueError):
        m["corpus"].query_packed_occurrences_tail_batch_keys_device(m["dev"]["w48"], R, PER, gpu.zeros(R, dtype=gpu.int32, device="cuda"),
                                                                    float(t), CAP)


# ---- 2. the planted copies at threshold 1.0 --------------------------------------------------------------------------------------------
def test_planted_copies(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    cells, ds = _cells(m, "w48", NEW, 8)
    assert ds == (0, 1, 8, 3, 5, 2, 8, 8, 8)
    got = _tail(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, 1.0, CAP)
    _same(got, _expected(cells, 1.0, CAP))

    def lags_of(r, j):
        return got[1][r][got[0][r] == _key(ONE, j)].tolist()

    assert lags_of(2, E22) == [-(PER - 22)]                         # ends at the last record
    assert lags_of(4, E17) == [-(PER - 17 - 5 + 1)]                 # ends at end - d + 1: the first of the new cells
    assert lags_of(3, E17) == []                                    # ends at end - d: complete one push ago ...
    full = _filtered(m, gpu, "w48", (PER,) * R, 1.0, CAP)           # ... and a cell of 1.0 of the whole window (d = the window)
    assert -(PER - 17 - 3) in full[1][3][full[0][3] == _key(ONE, E17)].tolist()
    assert lags_of(6, E22) == [] and lags_of(7, E22) == []          # across the seam 6 | 7: in neither
    assert ref.tail_range(PER, 44, 8) == range(0, 5)                # clipped at offset 0
    assert lags_of(8, E44) == [-2]
    assert not got[0][0].any() and got[2][0] == 0                   # d = 0: an empty row


# ---- 3. overflow -----------------------------------------------------------------------------------------------------------------------
def test_a_row_that_overflows_writes_nothing_next_door(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    cells, _ds = _cells(m, "w48", NEW, 8)
    found = None
    for t in _thresholds(cells).values():
        counts = _expected(cells, t, 1)[2]
        cap = int(max(counts[1], counts[3]))
        if cap >= 1 and counts[2] > cap:
            found = (t, cap, counts)
    assert found, "the reference holds a capacity that row 2 alone exceeds among its neighbours"
    t, cap, counts = found
    want = _expected(cells, t, cap)
    got = _tail(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, t, cap)
    _same(got, want)
    assert got[2][2] == counts[2] > cap and got[2][1] <= cap and got[2][3] <= cap
    assert np.count_nonzero(got[0][2]) == cap and np.count_nonzero(got[0][1]) == counts[1] and np.count_nonzero(got[0][3]) == counts[3]


# ---- 4. chunks, passes, grids ----------------------------------------------------------------------------------------------------------
def _scratch(entries):
    return 24 + entries * 24 + -(-entries // WALK) * 4


def test_passes_and_chunks_change_nothing(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"]
    cells, _ds = _cells(m, "w48", NEW, 8)
    ts = _thresholds(cells)
    want = {k: _expected(cells, ts[k], CAP) for k in ("4th", "median")}
    try:
        for limit, rpp, chunk in ((2 * _scratch(192) + 9, 2, 192), (_scratch(128), 1, 128), (_scratch(WALK), 1, WALK)):
            plan = lb.debug_occurrences_tail_plan(R, PER, 1, 300, N_CASE, 8, limit)
            assert (plan["recordings_per_pass"], plan["entries_per_chunk"]) == (rpp, chunk) and plan["scratch_bytes"] <= limit
            corpus.set_join_scratch_limit(limit)
            for k, w in want.items():
                _same(_tail(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, ts[k], CAP), w)
            _same(_tail(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, ts["median"], CAP, want_lags=False), (want["median"][0], None, want["median"][2]))
        corpus.set_join_scratch_limit(_scratch(WALK) - 1)            # a limit below one block of ONE recording
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            _tail(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, ts["4th"], CAP)
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    finally:
        corpus.set_join_scratch_limit(0)


@pytest.mark.parametrize("name,new,max_new,units", [("w48", NEW, 8, 3), ("w80", NEW64, 64, 6)])
def test_second_trips(lb, gpu, oracle, name, new, max_new, units):
    """the strided unit loop of both kernels takes a second trip: 3 blocks of entries x groups of recordings units"""
    m = _module(lb, gpu, oracle)
    block = m["blocks"][name]
    rows, per = block.shape[0], block.shape[1]
    plan = lb.debug_occurrences_tail_plan(rows, per, 1, 300, N_CASE, max_new)
    assert -(-N_CASE // WALK) * -(-rows // plan["recordings_per_workgroup"]) == units
    cells, _ds = _cells(m, name, new, max_new)
    t = _thresholds(cells)["median"]
    want = _expected(cells, t, CAP)
    try:
        for ceiling in (1, 4):
            lb.debug_set_grid_ceiling(ceiling)
            before = lb.debug_grid_ceiling()[1]
            _same(_tail(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, t, CAP), want)
            assert units <= ceiling or lb.debug_grid_ceiling()[1] > before
    finally:
        lb.debug_set_grid_ceiling(0)


def test_long_entries_lower_the_recordings_per_workgroup(lb, gpu, oracle):
    """longest entry 1 024 in windows of 1 030: three sub-windows fit the LDS, four recordings make two groups"""
    per, rows, new = 1030, 4, [8, 3, 0, 5]
    plan = lb.debug_occurrences_tail_plan(rows, per, 5, 1024, 6, 8)
    assert (plan["lanes"], plan["recordings_per_workgroup"], plan["window_records"]) == (8, 3, 1030)
    ent = _random(oracle, 77, [1024, 1000, 5, 1020, 17, 1024])      # (1 024: the longest entry a corpus of these calls may hold)
    block = oracle.synth_ragged_entries(78, 0, np.array([rows * per], np.uint32), L).reshape(rows, per, L).copy()
    block[0, 6:] = ent[0]                                           # ends at the last record
    block[3, 2:2 + 1024] = ent[5]                                   # offset 2 of the cells 2 .. 6
    block[1, per - 3 - 5:per - 3] = ent[2]                          # one too old
    corpus = _ragged(lb, gpu, oracle, ent)
    dev = gpu.from_numpy(_packed(oracle, block.reshape(-1, L))).cuda()
    ds = tuple(ref.clamp_new(n, 8, per) for n in new)
    cells = [ref.tail_cells(rec, ent, d) for rec, d in zip(block, ds)]
    lengths = np.array([len(e) for e in ent], np.int64)
    for t in _thresholds(cells).values():
        want = _expected(cells, t, CAP)
        got = _tail(gpu, corpus, dev, rows, per, new, 8, t, CAP)
        _same(got, want)
        _same(got, _filtered(None, gpu, None, ds, t, CAP, corpus=corpus, dev=dev, lengths=lengths))
    got = _tail(gpu, corpus, dev, rows, per, new, 8, 1.0, CAP)
    assert got[1][0][got[0][0] == _key(ONE, 0)].tolist() == [-6] and got[1][3][got[0][3] == _key(ONE, 5)].tolist() == [-2]
    assert _key(ONE, 2) not in got[0][1]


def test_one_recording(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    for r in (2, 4, 0):
        cells, ds = _cells(m, "w48", NEW, 8)
        t = _thresholds(cells)["4th"]
        want = _expected(cells[r:r + 1], t, CAP)
        got = _tail(gpu, m["corpus"], m["dev"]["w48"][r * PER:(r + 1) * PER], 1, PER, NEW[r:r + 1], 8, t, CAP)
        _same(got, want)


def test_the_empty_corpus_and_no_entry_that_takes_part(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    empty = lb.Corpus.ragged(L, 4, 16)
    got = _tail(gpu, empty, m["dev"]["w48"], R, PER, NEW, 8, 0.5, CAP)
    assert not got[0].any() and not got[1].any() and not got[2].any()
    longer = _ragged(lb, gpu, oracle, [m["entries"][E49], m["entries"][E300]])
    got = _tail(gpu, longer, m["dev"]["w48"], R, PER, NEW, 8, 1e-30, CAP)
    assert not got[0].any() and not got[1].any() and not got[2].any()


def test_no_lags_a_masked_range_and_an_index_base(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    cells, ds = _cells(m, "w48", NEW, 8)
    t = _thresholds(cells)["median"]
    want = _expected(cells, t, CAP)
    _same(_tail(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, t, CAP, want_lags=False), (want[0], None, want[2]))
    masked, _ = _cells(m, "w48", NEW, 8, range_=20)
    for t in _thresholds(masked).values():
        got = _tail(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, t, CAP, range_=20)
        _same(got, _expected(masked, t, CAP))
        _same(got, _filtered(m, gpu, "w48", ds, t, CAP, range_=20))
    assert any(a[2] != b[2] for ra, rb in zip(cells, masked) for a, b in zip(ra, rb))     # the range changes cells
    base = (1 << 32) - N_CASE                                       # the last index a corpus may have
    for b in (1000, base):
        got = _tail(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, _thresholds(cells)["4th"], CAP, base=b)
        _same(got, _expected(cells, _thresholds(cells)["4th"], CAP, base=b))
    _same(got, _filtered(m, gpu, "w48", ds, _thresholds(cells)["4th"], CAP, base=base))


def test_odd_subfingerprint_length(lb, gpu, oracle):
    """sub-fingerprints of 37 Booleans, five windows of 50, the full range and a shorter one"""
    rng = np.random.default_rng(5)
    ent = _random(oracle, 99, rng.integers(1, 41, 70), 37)
    rows, per, new = 5, 50, [3, 8, 0, 5, 1]
    block = oracle.synth_ragged_entries(97, 0, np.array([rows * per], np.uint32), 37).reshape(rows, per, 37).copy()
    block[1, per - len(ent[9]):] = ent[9]
    corpus = _ragged(lb, gpu, oracle, ent, 37)
    dev = gpu.from_numpy(_packed(oracle, block.reshape(-1, 37))).cuda()
    lengths = np.array([len(e) for e in ent], np.int64)
    for range_ in (0, 21):
        cells = [ref.tail_cells(rec, ent, d, range_) for rec, d in zip(block, new)]
        for t in _thresholds(cells).values():
            got = _tail(gpu, corpus, dev, rows, per, new, 8, t, CAP, range_=range_)
            _same(got, _expected(cells, t, CAP))
            _same(got, _filtered(None, gpu, None, tuple(new), t, CAP, range_=range_, corpus=corpus, dev=dev, lengths=lengths))


def test_four_calls_on_four_streams(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    shapes = (("w48", NEW, 8), ("w80", NEW64, 64), ("w48", NEW, 5), ("w80", NEW64, 33))
    streams = [gpu.cuda.Stream() for _ in shapes]
    outs, wants = [], []
    held = []
    for s, (name, new, max_new) in zip(streams, shapes):           # each call is made while the one before may still run
        block = m["blocks"][name]
        cells, _ds = _cells(m, name, new, max_new)
        t = _thresholds(cells)["median"]
        wants.append(_expected(cells, t, CAP))
        out = _outputs(gpu, block.shape[0], CAP)
        d_new = gpu.from_numpy(np.asarray(new, np.uint32).view(np.int32)).cuda()
        held.append(d_new)
        s.wait_stream(gpu.cuda.current_stream())
        m["corpus"].query_packed_occurrences_tail_batch_keys_device(m["dev"][name], block.shape[0], block.shape[1], d_new, float(t), CAP,
                                                                    max_new=max_new, keys_out=out[0], lags_out=out[1], counts_out=out[2],
                                                                    stream=s)
        outs.append(out)
    for s in streams:
        s.synchronize()
    for out, want in zip(outs, wants):
        _same(_host(*out), want)


# ---- 5. exactly once -------------------------------------------------------------------------------------------------------------------
def test_every_cell_of_a_channels_life_exactly_once(lb, gpu, oracle):
    """a recording of 200 sub-fingerprints fed as growing, then sliding windows: the first call's d is its window, the later ones'
    1 .. 8 with a window of at least 40 + 8 - 1; the union of the calls' matches at absolute positions is the single occurrences
    call's (peaks off) over the whole recording, as a multiset of (index, position, key bits) -- and the reference's"""
    m = _module(lb, gpu, oracle)
    short = [e for e in m["entries"] if len(e) <= 40]
    corpus = _ragged(lb, gpu, oracle, short)
    total = 200
    rec = oracle.synth_ragged_entries(4711, 0, np.array([total], np.uint32), L).copy()
    for at, j in ((0, 5), (30, 9), (41, 33), (100, 60), (160, 5), (199, 0)):
        rec[at:at + len(short[j])][:total - at] = short[j][:total - at]
    whole = ref.full_cells(rec, short, 40)
    t = np.float32(np.sort(np.array([q for (_j, _o, q) in whole], np.float32))[int(len(whole) * 0.99)])
    want = sorted((j, o, int(np.float32(q).view(np.uint32))) for (j, o, q) in whole if q >= t)
    assert len(want) > 50 and any(q == ONE for (_j, _o, q) in whole)
    dev = gpu.from_numpy(_packed(oracle, rec)).cuda()
    rng = np.random.default_rng(8)
    seen, fed, first, limit = [], 0, True, 60
    while fed < total:
        d = 47 if first else int(min(rng.integers(1, 9), total - fed))
        fed += d
        n = min(fed, limit if not first else fed)
        assert n >= min(fed, 40 + d - 1)
        window = dev[fed - n:fed].contiguous()
        keys, lags, counts = corpus.query_packed_occurrences_tail_batch_keys_device(window, 1, n, [d], float(t), 4096, max_new=64)
        gpu.cuda.synchronize()
        assert int(counts[0]) <= 4096
        (idx, sc, start), = lb.decode_tail_occurrences(keys, lags, counts, [fed], n)
        seen.extend(zip(idx.tolist(), start.tolist(), sc.view(np.uint32).tolist()))
        first = False
    assert sorted(seen) == want
    keys, lags, count = corpus.query_packed_occurrences_keys_device(dev, total, float(t), 8192, peaks=False)
    gpu.cuda.synchronize()
    idx, sc, lag = lb.decode_occurrence_keys(keys, lags, int(count[0]))
    assert int(count[0]) <= 8192
    assert sorted(zip(idx.tolist(), (-lag.astype(np.int64)).tolist(), sc.view(np.uint32).tolist())) == sorted(seen)


# ---- 6. the stream bank ----------------------------------------------------------------------------------------------------------------
def test_stream_bank_new_occurrences(lb, gpu, oracle):
    """three channels of test_gpu_stream_bank.py's pruned configuration, two pushes; the corpus holds random entries and, per
    channel, a span of its own sub-fingerprints that ends inside the second push's: StreamBank.new_occurrences against the call on
    window_device's block with the push's new counts, and against the reference"""
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
    planted = {}
    for c in range(3):
        planted[c] = len(ent)
        ent.append(fps[c][frames - 10:frames].copy())               # ends at the newest sub-fingerprint
    old0 = frames - int(new[0]) - 10
    ent.append(fps[0][old0:old0 + 10].copy())                       # ends one before channel 0's new ones
    corpus = _ragged(lb, gpu, oracle, ent, length)
    channels = [2, 0, 1]
    got = bank.new_occurrences(corpus, channels, n, new, 0.9, 16)
    win = bank.window_device(channels, n)
    gpu.cuda.synchronize()
    listed = [int(new[c]) for c in channels]
    _same(_host(*got), _tail(gpu, corpus, win, 3, n, listed, max(listed), 0.9, 16))
    rows = lb.unpack_packed(win.cpu().numpy(), length).reshape(3, n, length)
    cells = [ref.tail_cells(rows[j], ent, listed[j]) for j in range(3)]
    _same(_host(*got), _expected(cells, 0.9, 16))
    decoded = lb.decode_tail_occurrences(*got, bank.totals()[channels], n)
    for j, c in enumerate(channels):
        idx, sc, start = decoded[j]
        assert start[(idx == planted[c]) & (sc == ONE)].tolist() == [frames - 10]
    idx, _sc, start = decoded[1]                                    # (channel 0) complete one push ago: not a cell of this one
    assert not ((idx == len(ent) - 1) & (start == old0)).any()
