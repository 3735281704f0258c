"""GPU tests of the occurrence segments calls (LBAudioDetectiveOccurrenceSegmentsFromKeysDevice, k_occurrence_segments.hip,
LBAudioDetectiveCorpusEntryLengthsFromKeysDevice, occurrence_segments_device, Corpus.entry_lengths_from_keys_device,
Corpus.recording_occurrence_segments_batch_keys_device, Corpus.recording_occurrence_segments, StreamBank.occurrence_segments).
Every output word -- starts, keys, lags, lengths, counts, the zeros behind the spans -- is compared with the brute-force reference
of occurrence_segments_ref.py as integers; nothing needs a tolerance.  Output buffers are filled with 0xFF bytes before every call.
Score words are drawn from the positive finite floats, as the occurrences calls write them."""
import numpy as np
import pytest

import occurrence_segments_ref as ref
import recording_ref

pytestmark = pytest.mark.gpu

L = 200
INT32_MIN = -(1 << 31)


def _key(score, index):
    return (int(np.float32(score).view(np.uint32)) << 32) | (0xFFFFFFFF - int(index))


def _random_keys(rng, n):
    """distinct-looking keys: score words of floats in [0.125, 1), entries 0 .. 999"""
    hi = rng.integers(0x3E000000, 0x3F800000, n).astype(np.uint64)
    return (hi << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - rng.integers(0, 1000, n).astype(np.uint64))


def _block(keys, lags, lengths):
    keys = np.asarray(keys, np.uint64)
    keys = keys.reshape(-1, keys.shape[-1])
    return keys, np.asarray(lags, np.int32).reshape(keys.shape), np.asarray(lengths, np.uint32).reshape(keys.shape)


def _want(keys, lags, lengths, counts, per, cap):
    """(starts uint32 [R, cap], keys uint64, lags int32, lengths uint32, counts uint32 [R]) from the reference"""
    keys, lags, lengths = _block(keys, lags, lengths)
    st, ks, lg, ln, cn = ref.rows(keys.tolist(), lags.tolist(), lengths.tolist(), per, cap,
                                  None if counts is None else [int(c) for c in np.asarray(counts).reshape(-1)])
    return (np.array(st, np.uint32).reshape(-1, cap), np.array(ks, np.uint64).reshape(-1, cap), np.array(lg, np.int32).reshape(-1, cap),
            np.array(ln, np.uint32).reshape(-1, cap), np.array(cn, np.uint32))


def _run(lb, gpu, keys, lags, lengths, counts, per, cap, want_lags=True, want_lengths=True, stream=None):
    """one call into 0xFF-filled buffers -> (starts, keys, lags or None, lengths or None, counts) as numpy, 2-D"""
    keys, lags, lengths = _block(keys, lags, lengths)
    R = keys.shape[0]
    dk = gpu.from_numpy(keys.view(np.int64).copy()).cuda()
    dg = gpu.from_numpy(lags.copy()).cuda()
    dl = gpu.from_numpy(lengths.view(np.int32).copy()).cuda()
    dc = None if counts is None else gpu.from_numpy(np.asarray(counts, np.uint64).reshape(-1).view(np.int64).copy()).cuda()
    st = gpu.full((R, cap), -1, dtype=gpu.int32, device="cuda")
    ks = gpu.full((R, cap), -1, dtype=gpu.int64, device="cuda")
    lg = gpu.full((R, cap), -1, dtype=gpu.int32, device="cuda") if want_lags else None
    ln = gpu.full((R, cap), -1, dtype=gpu.int32, device="cuda") if want_lengths else None
    cn = gpu.full((R,), -1, dtype=gpu.int32, device="cuda")
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = lb.occurrence_segments_device(dk, dg, dl, dc, per, cap, starts_out=st, keys_out=ks, lags_out=lg, lengths_out=ln, counts_out=cn,
                                        want_lags=want_lags, want_lengths=want_lengths, stream=stream)
    assert got[0] is st and got[1] is ks and got[2] is lg and got[3] is ln and got[4] is cn
    (stream or gpu.cuda.current_stream()).synchronize()
    return _np(got)


def _np(out):
    return (out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy().view(np.uint64),
            out[2].cpu().numpy() if out[2] is not None else None,
            out[3].cpu().numpy().view(np.uint32) if out[3] is not None else None, out[4].cpu().numpy().view(np.uint32))


def _same(got, want):
    assert np.array_equal(got[4], want[4]), (got[4], want[4])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if got[2] is not None:
        assert np.array_equal(got[2], want[2])
    if got[3] is not None:
        assert np.array_equal(got[3], want[3])


def _check(lb, gpu, keys, lags, lengths, counts, per, cap, **kw):
    want = _want(keys, lags, lengths, counts, per, cap)
    _same(_run(lb, gpu, keys, lags, lengths, counts, per, cap, **kw), want)
    return want


def _row(slots, cells):
    """a row of `slots` slots from (score, entry, lag, length) cells in slot order, zeros behind them"""
    keys, lags, lengths = np.zeros(slots, np.uint64), np.zeros(slots, np.int32), np.zeros(slots, np.uint32)
    for p, (score, entry, lag, n) in enumerate(cells):
        keys[p], lags[p], lengths[p] = (_key(score, entry) if score else 0), lag, n
    return keys, lags, lengths


def _rows(slots, rows):
    built = [_row(slots, r) for r in rows]
    return tuple(np.stack([b[i] for b in built]) for i in range(3))


def _starts(want, r=0):
    return want[0][r, :min(int(want[4][r]), want[0].shape[1])].tolist()


def _entries_of(want, r=0):
    return (0xFFFFFFFF - (want[1][r, :min(int(want[4][r]), want[1].shape[1])] & np.uint64(0xFFFFFFFF))).astype(np.int64).tolist()


# ---- 1. hand-made rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 2, 63, 64, 65, 129, 1000])
def test_capacities_that_are_no_power_of_two(lb, gpu, slots):
    rng = np.random.default_rng(slots)
    junk_lags, junk_len = rng.integers(-slots, 1, slots), rng.integers(1, 5, slots)
    # nothing: zero keys, and keys behind a count of 0
    for counts in (None, [0]):
        keys = np.zeros(slots, np.uint64) if counts is None else _random_keys(rng, slots)
        assert _check(lb, gpu, keys, junk_lags, junk_len, counts, slots, 3)[4][0] == 0
    # every slot a candidate of length 1 at a start of its own, in shuffled order: all of them are spans; the cut and the zero fill
    keys = _random_keys(rng, slots)
    lags = -rng.permutation(slots)
    for cap in sorted({1, max(1, slots - 1), slots, slots + 3}):
        want = _check(lb, gpu, keys, lags, np.ones(slots, np.uint32), None, slots, cap)
        assert want[4][0] == slots and _starts(want) == list(range(min(slots, cap)))
    # a mix, in a recording shorter and longer than the row
    for per in (max(1, slots // 3), 2 * slots + 1):
        keys = np.where(rng.random(slots) < 0.7, _random_keys(rng, slots), 0).astype(np.uint64)
        _check(lb, gpu, keys, rng.integers(-per - 2, 3, slots), rng.integers(0, 9, slots), [rng.integers(0, slots + 3)], per, per)


def test_both_caps_at_once(lb, gpu):
    """8192 slots and 8192 offsets: more than 48 KiB of LDS.  Random cells, and every slot a span of its own."""
    n = 8192
    rng = np.random.default_rng(8192)
    keys = np.stack([np.where(rng.random(n) < 0.9, _random_keys(rng, n), 0).astype(np.uint64), _random_keys(rng, n)])
    lags = np.stack([rng.integers(-n - 3, 4, n), -rng.permutation(n)])
    lengths = np.stack([rng.integers(0, 71, n), np.ones(n, np.int64)])
    want = _check(lb, gpu, keys, lags, lengths, None, n, n + 3)
    assert 100 < want[4][0] < n and want[4][1] == n and _starts(want, 1) == list(range(n))
    for slots, per in ((n + 1, n), (n, n + 1)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            _run(lb, gpu, np.zeros((1, slots), np.uint64), np.zeros((1, slots), np.int32), np.zeros((1, slots), np.uint32), None, per, 4)
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")


def test_many_candidates_at_one_start(lb, gpu):
    """what the timeline's segments cannot express: the second best at an offset is reported where the winner there loses"""
    rows = [[(1.0, 3, -12, 10), (0.95, 1, -5, 10), (0.90, 2, -5, 5)],                         # X, W, S: S then X
            [(0.90, 2, -5, 5), (0.95, 1, -5, 10), (1.0, 3, -12, 10)],                         # ... in another slot order
            [(0.5, 1, -5, 3), (0.6, 2, -5, 9), (0.7, 3, -5, 30), (0.8, 4, -7, 1), (0.4, 5, -5, 2)],   # 4 at 7, then 5 at 5
            [(0.5, 9, -5, 4)] * 6 + [(0.5, 8, -5, 4)],                                        # the lower entry index is the higher key
            [(0.9, 1, -8, 4), (0.8, 2, -5, 4), (0.7, 3, -5, 3), (0.6, 4, -5, 2), (0.5, 5, -6, 2), (0.4, 6, -7, 1)]]
    keys, lags, lengths = _rows(8, rows)
    want = _check(lb, gpu, keys, lags, lengths, None, 30, 6)
    assert [_starts(want, r) for r in range(5)] == [[5, 12], [5, 12], [5, 7], [5], [5, 8]]
    assert [_entries_of(want, r) for r in range(5)] == [[2, 3], [2, 3], [5, 4], [8], [3, 1]]
    assert want[2][0, :2].tolist() == [-5, -12] and want[3][0, :2].tolist() == [5, 10]


def test_spans_that_touch_or_cross_a_mask_word(lb, gpu):
    per = 130
    rows = [[(0.5, 1, -60, 4), (0.6, 2, -64, 6)],                       # 63 | 64: touch
            [(0.6, 1, -60, 5), (0.5, 2, -65, 5)],                       # 64 | 65: touch
            [(0.5, 1, -60, 5), (0.6, 2, -64, 6)],                       # one offset shared: the better one stays
            [(0.9, 1, -30, 5), (0.8, 2, -35, 1), (0.8, 3, -29, 1), (0.7, 4, -34, 1), (0.7, 5, -31, 9)],
            [(0.5, 1, 0, 64), (0.5, 2, -64, 64), (0.5, 3, -128, 64), (0.9, 4, -127, 1)],
            [(0.9, 1, -63, 2), (0.8, 2, -62, 1), (0.8, 3, -65, 1), (0.7, 4, -64, 1), (0.7, 5, -63, 1), (0.6, 6, -60, 10)]]
    keys, lags, lengths = _rows(6, rows)
    want = _check(lb, gpu, keys, lags, lengths, None, per, 6)
    assert [_starts(want, r) for r in range(6)] == [[60, 64], [60, 65], [64], [29, 30, 35], [0, 127, 128], [62, 63, 65]]
    # a span of 1 024 offsets from start 1 in a row of 1 100
    keys, lags, lengths = _row(9, [(0.9, 1, -1, 1024), (0.5, 2, 0, 1), (0.6, 3, 0, 2), (0.8, 4, -1024, 1), (0.4, 5, -1025, 1),
                                   (0.8, 6, -600, 2), (0.3, 7, -1025, 75), (0.2, 8, -1026, 1000), (0.95, 9, -1100, 5)])
    want = _check(lb, gpu, keys, lags, lengths, None, 1100, 9)
    assert _starts(want) == [0, 1, 1025, 1026]


def test_the_ends_of_the_recording(lb, gpu):
    per = 77
    rows = [[(0.5, 1, -(per - 5), 5), (0.4, 2, -(per - 10), 5)],            # ends exactly at per, and one that touches it
            [(0.9, 1, -(per - 3), 10), (0.5, 2, -(per - 5), 5), (0.5, 3, -(per - 8), 5)],      # clipped: it still blocks what it covers
            [(0.5, 1, -(per - 1), 70000), (0.4, 2, 0, 70000)],              # lengths that do not fit 16 bits
            [(0.9, 1, 3, 10), (0.8, 2, -6, 2), (0.7, 3, -7, 2)],            # clipped at the front: [0, 7), which 8 touches
            [(0.5, 1, 0, 0xFFFFFFFF), (0.9, 2, -per, 1), (0.9, 3, -(per - 1), 1)]]     # the largest length; a start at per is none
    keys, lags, lengths = _rows(3, rows)
    want = _check(lb, gpu, keys, lags, lengths, None, per, 4)
    assert [_starts(want, r) for r in range(5)] == [[per - 10, per - 5], [per - 8, per - 3], [per - 1], [0, 7], [per - 1]]
    assert want[3][1, 1] == 10 and want[3][2, 0] == 70000 and want[2][3, 0] == 3          # lag and length as they came


def test_ties(lb, gpu):
    k = 0.5, 7
    # an equal key at different starts: the lower start wins, whatever the slot
    cells = [(*k, -o, 5) for o in (41, 15, 99, 14, 12, 40, 10)]
    keys, lags, lengths = _row(8, cells)
    want = _check(lb, gpu, keys, lags, lengths, None, 100, 8)
    assert _starts(want) == [10, 15, 40, 99]
    keys, lags, lengths = np.full(100, _key(*k), np.uint64), -np.arange(99, -1, -1), np.full(100, 3)
    want = _check(lb, gpu, keys, lags, lengths, None, 100, 100)
    assert _starts(want) == list(range(0, 100, 3))
    # an equal key and an equal start -- two lags >= 0 of one long entry -- the lower slot wins
    keys, lags, lengths = _row(4, [(0.4, 1, -3, 2), (*k, 9, 300), (*k, 2, 300), (*k, 0, 300)])
    want = _check(lb, gpu, keys, lags, lengths, None, 50, 4)
    assert _starts(want) == [0] and want[2][0, 0] == 9 and want[4][0] == 1


def test_a_recording_inside_a_longer_entry(lb, gpu):
    """lag > 0 with length > per covers the whole row: it blocks everything of lower key, and loses to anything of higher key"""
    per = 90
    rows = [[(0.5, 1, -10, 5), (0.8, 2, 4, 200), (0.7, 3, -50, 5), (0.79, 4, 0, 90)],
            [(0.5, 1, -10, 5), (0.8, 2, 4, 200), (0.9, 3, -50, 5), (0.79, 4, -60, 9)],
            [(0.8, 2, 4, 94), (0.7, 3, -89, 5), (0.6, 4, -90, 1)],                     # [0, 90) exactly
            [(0.8, 2, 4, 93), (0.7, 3, -89, 5), (0.6, 4, -88, 1)]]                     # [0, 89): 89 is free
    keys, lags, lengths = _rows(4, rows)
    want = _check(lb, gpu, keys, lags, lengths, None, per, 4)
    assert [_starts(want, r) for r in range(4)] == [[0], [10, 50, 60], [0], [0, 89]]
    assert _entries_of(want, 0) == [2] and want[2][0, 0] == 4 and want[3][0, 0] == 200


def test_slots_that_are_no_candidates(lb, gpu):
    per = 40
    none = [(0.9, 1, 5, 5), (0.9, 2, 6, 5), (0.9, 3, -per, 3), (0.9, 4, -per - 1, 3), (0.9, 5, INT32_MIN, 7), (0.9, 6, INT32_MIN, 0xFFFFFFFF),
            (0.9, 7, 0x7FFFFFFF, 0x7FFFFFFF), (0.9, 8, -3, 0), (0, 0, -3, 4)]
    rows = [none,                                                                      # lag >= length, -lag >= per, INT32_MIN, length 0, key 0
            none[:4] + [(0.3, 9, -4, 2)] + none[4:],                                   # ... around one real cell
            [(0.9, 1, -2, 2), (0, 0, -4, 2), (0.8, 2, -6, 2), (0, 0, 0, 40), (0.7, 3, -8, 2)]]        # zero keys in the middle of a row
    keys, lags, lengths = _rows(10, rows)
    want = _check(lb, gpu, keys, lags, lengths, None, per, 5)
    assert [_starts(want, r) for r in range(3)] == [[], [4], [2, 6, 8]]
    assert lags.min() == INT32_MIN and lags.max() == 0x7FFFFFFF


def test_the_counts(lb, gpu):
    """garbage behind inCounts[r] is ignored, a count above the capacity means the whole row, NULL means the whole row"""
    rng = np.random.default_rng(3)
    slots, per = 70, 200
    keys = np.stack([_random_keys(rng, slots)] * 4)
    lags = np.stack([-rng.permutation(per)[:slots]] * 4)
    lengths = np.stack([rng.integers(1, 6, slots)] * 4)
    counts = [10, slots, slots + 1, (1 << 40) + 3]
    want = _check(lb, gpu, keys, lags, lengths, counts, per, slots)
    whole = _check(lb, gpu, keys, lags, lengths, None, per, slots)
    assert want[4][0] <= 10 < want[4][1] and [want[4][r] for r in (1, 2, 3)] == [whole[4][0]] * 3
    assert all(np.array_equal(want[i][r], whole[i][0]) for i in range(4) for r in (1, 2, 3))
    # the best key of the row sits behind the count: it is not there
    keys[0, 10] = _key(0.999, 0)
    again = _check(lb, gpu, keys, lags, lengths, counts, per, slots)
    assert all(np.array_equal(again[i][0], want[i][0]) for i in range(5))


# ---- 2. batches ---------------------------------------------------------------------------------------------------------------
def _sweep(seed, R, slots, per):
    """rows of mixed shapes: few or many distinct keys, starts that collide, spans clipped at both ends, recordings inside longer
    entries, empty spans, zero keys and lengths, counts from 0 to beyond the capacity with cells behind them"""
    rng = np.random.default_rng(seed)
    kinds = int(rng.integers(0, 8))
    if kinds:
        keys = _random_keys(rng, kinds)[rng.integers(0, kinds, (R, slots))]
    else:
        keys = _random_keys(rng, R * slots).reshape(R, slots)
    keys = np.where(rng.random((R, slots)) < 0.9, keys, 0).astype(np.uint64)
    lags = rng.integers(-per - 3, 6, (R, slots)).astype(np.int32)
    lengths = rng.integers(1, 2 * per + 5, (R, slots))
    lengths = np.where(rng.random((R, slots)) < 0.8, rng.integers(1, 12, (R, slots)), lengths)
    lengths = np.where(rng.random((R, slots)) < 0.05, 0, lengths).astype(np.uint32)
    counts = rng.integers(0, slots + 4, R).astype(np.uint64)
    counts[rng.random(R) < 0.5] = slots
    return keys, lags, lengths, counts


def test_rows_do_not_leak_into_each_other(lb, gpu):
    """five recordings with different counts, one of them empty: the batch equals the five single calls"""
    slots, per, cap = 40, 64, 12
    keys, lags, lengths, _ = _sweep(5, 5, slots, per)
    counts = np.array([slots, 7, 0, slots + 9, 23], np.uint64)
    want = _check(lb, gpu, keys, lags, lengths, counts, per, cap)
    assert want[4][2] == 0 and not want[1][2].any() and len(set(want[4].tolist())) > 2
    for r in range(5):
        one = _run(lb, gpu, keys[r], lags[r], lengths[r], counts[r:r + 1], per, cap)
        assert all(np.array_equal(one[i][0], want[i][r]) for i in range(5))


def test_optional_outputs_change_nothing(lb, gpu):
    keys, lags, lengths, counts = _sweep(72, 9, 129, 150)
    want = _want(keys, lags, lengths, counts, 150, 16)
    for want_lags in (True, False):
        for want_lengths in (True, False):
            got = _run(lb, gpu, keys, lags, lengths, counts, 150, 16, want_lags=want_lags, want_lengths=want_lengths)
            assert (got[2] is not None) == want_lags and (got[3] is not None) == want_lengths
            _same(got, want)


def test_a_stream_of_its_own_and_the_python_forms(lb, gpu):
    keys, lags, lengths, counts = _sweep(71, 9, 129, 150)
    want = _want(keys, lags, lengths, counts, 150, 16)
    stream = gpu.cuda.Stream()
    _same(_run(lb, gpu, keys, lags, lengths, counts, 150, 16, stream=stream), want)
    # outputs made by the call, on two streams in a row
    dk, dg, dl, dc = (gpu.from_numpy(x.copy()).cuda() for x in (keys.view(np.int64), lags, lengths.view(np.int32), counts.view(np.int64)))
    streams = [stream, gpu.cuda.Stream()]
    outs = []
    for s in streams:
        s.wait_stream(gpu.cuda.current_stream())
        outs.append(lb.occurrence_segments_device(dk, dg, dl, dc, 150, 16, stream=s))
    for s in streams:
        s.synchronize()
    for out in outs:
        assert out[0].shape == (9, 16) and out[1].dtype == gpu.int64 and out[2].dtype == out[3].dtype == gpu.int32 and out[4].shape == (9,)
        _same(_np(out), want)
    # one recording as 1-D tensors, and the decoder against the host statement
    one = lb.occurrence_segments_device(dk[3], dg[3], dl[3], dc[3:4], 150, 16)
    gpu.cuda.synchronize()
    assert one[0].shape == (16,) and one[4].dim() == 0 and int(one[4]) == want[4][3]
    dec = lb.decode_occurrence_segments(*one)
    m = int(min(counts[3], 129))
    idx, sc, lg = lb.decode_occurrence_keys(keys[3].view(np.int64), lags[3], m)
    idx = np.where(keys[3][:m] != 0, idx, -1)
    host = lb.occurrence_segments(idx, sc, lg, lengths[3][:m], 150)
    n = min(16, len(host[0]))
    assert n > 2 and all(a.dtype == b.dtype and np.array_equal(a, b[:n]) for a, b in zip(dec, host))
    # keys, lags and lengths are integers of 64, 32 and 32 bits, not merely words of that size
    for bad in ((dk.double(), dg, dl), (dk, dg.float(), dl), (dk, dg, dl.float()), (dk.int(), dg, dl), (dk, dg, dl.long())):
        with pytest.raises(ValueError):
            lb.occurrence_segments_device(*bad, dc, 150, 16)


def test_the_grid_changes_nothing(lb, gpu):
    """more recordings than workgroups: the second and later trips of the loop over recordings (the launch's own cap of 65 536
    workgroups is out of a quick test's reach; the ceiling of the tests stands in for it)"""
    keys, lags, lengths, counts = _sweep(70, 70, 90, 120)
    want = _want(keys, lags, lengths, counts, 120, 20)
    _same(_run(lb, gpu, keys, lags, lengths, counts, 120, 20), want)
    try:
        for ceiling in (1, 4):
            lb.debug_set_grid_ceiling(ceiling)
            before = lb.debug_grid_ceiling()[1]
            _same(_run(lb, gpu, keys, lags, lengths, counts, 120, 20), want)
            assert lb.debug_grid_ceiling()[1] > before
    finally:
        lb.debug_set_grid_ceiling(0)
    assert lb.debug_grid_ceiling()[0] == 0


def test_a_timeline_as_rows_gives_the_timeline_segments(lb, gpu):
    """at most one candidate per offset, lag = -o, length <= per, in shuffled slots: starts, keys, lengths and counts equal
    LBAudioDetectiveTimelineSegmentsFromKeysDevice on the same data"""
    R, per, cap = 24, 300, 300
    rng = np.random.default_rng(300)
    pool = _random_keys(rng, 6)
    t_keys = np.where(rng.random((R, per)) < 0.5, pool[rng.integers(0, 6, (R, per))], 0).astype(np.uint64)
    t_keys[R // 2:] = np.where(t_keys[R // 2:] != 0, _random_keys(rng, (R - R // 2) * per).reshape(-1, per), 0)
    t_len = np.where(rng.random((R, per)) < 0.1, 0, rng.integers(1, 71, (R, per))).astype(np.uint32)
    keys, lags, lengths = np.zeros((R, per), np.uint64), np.zeros((R, per), np.int32), np.zeros((R, per), np.uint32)
    counts = np.zeros(R, np.uint64)
    for r in range(R):
        at = rng.permutation(np.flatnonzero(t_keys[r]))
        keys[r, :len(at)], lags[r, :len(at)], lengths[r, :len(at)], counts[r] = t_keys[r, at], -at, t_len[r, at], len(at)
    old = lb.timeline_segments_device(gpu.from_numpy(t_keys.view(np.int64).copy()).cuda(),
                                      gpu.from_numpy(t_len.view(np.int32).copy()).cuda(), cap)
    gpu.cuda.synchronize()
    for c in (counts, None):
        got = _run(lb, gpu, keys, lags, lengths, c, per, cap)
        assert np.array_equal(got[0], old[0].cpu().numpy().view(np.uint32)) and np.array_equal(got[1], old[1].cpu().numpy().view(np.uint64))
        assert np.array_equal(got[3], old[2].cpu().numpy().view(np.uint32)) and np.array_equal(got[4], old[3].cpu().numpy().view(np.uint32))
        assert np.array_equal(got[2], -got[0].astype(np.int64)) and got[4].min() > 3


# ---- 3. random sweep ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,slots,per", [(60, 7, 20), (60, 64, 64), (60, 100, 300), (60, 200, 90), (40, 513, 1000), (20, 65, 130)])
def test_random_sweep(lb, gpu, R, slots, per):
    keys, lags, lengths, counts = _sweep(1000 + slots, R, slots, per)
    cap = min(slots, per)
    want = _check(lb, gpu, keys, lags, lengths, counts, per, cap)
    assert want[4].max() > 1 and want[4].max() <= cap


# ---- 4. the lengths call -------------------------------------------------------------------------------------------------------
def _random(oracle, seed, counts, length=L):
    counts = np.asarray(counts, np.uint32)
    flat = oracle.synth_ragged_entries(seed, 0, counts, length)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [flat[off[i]:off[i + 1]].copy() for i in range(len(counts))]


def _packed(oracle, flat):
    return np.ascontiguousarray(oracle.pack_bools(flat)).view(np.uint8).reshape(len(flat), 32)


def _ragged(lb, gpu, oracle, entries, length=L):
    counts = np.array([len(e) for e in entries], np.uint32)
    c = lb.Corpus.ragged(length, len(entries), int(counts.sum()))
    c.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, np.concatenate(entries))).cuda(), counts)
    return c


def _length_keys(rng, n_entries, base):
    """keys from inside, below and above [base, base + n_entries), zero keys between them, any score word"""
    idx = np.concatenate([np.arange(n_entries) + base, [base - 1, base - 2, 0, base + n_entries, base + n_entries + 1, 0xFFFFFFFE],
                          rng.integers(0, base + 2 * n_entries, 300)]).astype(np.int64)
    idx = rng.permutation(idx)
    keys = (rng.integers(0, 1 << 31, len(idx)).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx.astype(np.uint64))
    zero = rng.random(len(idx)) < 0.1
    return np.where(zero, 0, keys).astype(np.uint64), idx, zero


def _lengths_of(lb, gpu, corpus, keys, base, shape=None, stream=None):
    dk = gpu.from_numpy(keys.view(np.int64).copy()).cuda()
    dk = dk.reshape(shape) if shape else dk
    out = gpu.full(dk.shape, -1, dtype=gpu.int32, device="cuda")
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = corpus.entry_lengths_from_keys_device(dk, index_base=base, out=out, stream=stream)
    assert got is out
    (stream or gpu.cuda.current_stream()).synchronize()
    return out.cpu().numpy().view(np.uint32)


def test_entry_lengths_of_a_ragged_and_a_uniform_corpus(lb, gpu, oracle):
    rng = np.random.default_rng(44)
    base = 1000
    counts = np.concatenate([[1], rng.integers(20, 71, 30), [1024], [1]])
    ragged = _ragged(lb, gpu, oracle, _random(oracle, 808, counts))
    n_sub = 4
    uniform = lb.Corpus(L, n_sub, 16)
    flat = oracle.synth_ragged_entries(809, 0, np.array([11 * n_sub], np.uint32), L)
    uniform.append_packed_device(gpu.from_numpy(_packed(oracle, flat)).cuda().reshape(11, n_sub, 32))
    for corpus, each in ((ragged, counts), (uniform, np.full(11, n_sub))):
        assert len(corpus) == len(each)
        keys, idx, zero = _length_keys(rng, len(each), base)
        inside = ~zero & (idx >= base) & (idx < base + len(each))
        want = np.where(inside, np.asarray(each)[np.clip(idx - base, 0, len(each) - 1)], 0).astype(np.uint32)
        assert inside.sum() >= len(each) // 2 and (~inside & ~zero).sum() > 5 and zero.sum() > 5
        assert np.array_equal(_lengths_of(lb, gpu, corpus, keys, base), want)
        got = _lengths_of(lb, gpu, corpus, keys[:300], base, shape=(3, 100), stream=gpu.cuda.Stream())     # a block, a stream
        assert got.shape == (3, 100) and np.array_equal(got.reshape(-1), want[:300])
        assert np.array_equal(_lengths_of(lb, gpu, corpus, keys[:1], base), want[:1])
        # without a base the same keys name other entries or none
        low = idx < len(each)
        want0 = np.where(~zero & low, np.asarray(each)[np.clip(idx, 0, len(each) - 1)], 0).astype(np.uint32)
        assert np.array_equal(_lengths_of(lb, gpu, corpus, keys, 0), want0)
        with pytest.raises(lb.LBAudioDetectiveError) as err:        # index base + entries above 2^32: what needs the corpus
            _lengths_of(lb, gpu, corpus, keys, (1 << 32) - len(each) + 1)
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
T = 0.7
X_AT, W_AT, S_AT = (12, 22), (5, 15), (5, 10)


def _flipped(rows, every, phase):
    e = rows.copy()
    e[:, phase::every] ^= 1
    return e


def _planted(oracle, R=3, per=96):
    """37 random entries of 5 .. 40 sub-fingerprints and one of 120, three recordings of 96, and three entries cut from recording
    0: X = [12, 22) verbatim, W = [5, 15) with every 40th Boolean flipped, S = [5, 10) with every 20th flipped"""
    counts = np.random.default_rng(77).integers(5, 41, 37)
    ent = _random(oracle, 7001, counts) + _random(oracle, 7003, [120])
    block = oracle.synth_ragged_entries(7002, 0, np.array([R * per], np.uint32), L).reshape(R, per, L).copy()
    block[1, 30:30 + len(ent[4])] = ent[4]
    x, w, s = len(ent), len(ent) + 1, len(ent) + 2
    ent += [block[0, slice(*X_AT)].copy(), _flipped(block[0, slice(*W_AT)], 40, 3), _flipped(block[0, slice(*S_AT)], 20, 1)]
    return ent, block, (x, w, s)


def _reference_rows(lb, keys, lags, lengths, counts, per, cap):
    k, g, n, c = (x.cpu().numpy() for x in (keys, lags, lengths, counts))
    return _want(k.view(np.uint64), g, n.view(np.uint32), c.view(np.uint64), per, cap)


def test_the_composite_on_real_fingerprints(lb, gpu, oracle):
    R, per, cap, out_cap, base = 3, 96, 64, 10, 500
    ent, block, (x, w, s) = _planted(oracle, R, per)
    corpus = _ragged(lb, gpu, oracle, ent)
    packed = gpu.from_numpy(_packed(oracle, block.reshape(-1, L))).cuda()
    # the occurrences, decoded: the three cells are there, and X > W > S >= T
    keys, lags, counts = corpus.query_packed_occurrences_batch_keys_device(packed, R, per, T, cap, peaks=True, index_base=base)
    gpu.cuda.synchronize()
    assert int(counts.max()) <= cap
    idx, sc, lg = lb.decode_occurrence_keys(keys[0], lags[0], int(counts[0]))
    cell = {(int(i) - base, int(g)): float(v) for i, v, g in zip(idx, sc, lg)}
    sx, sw, ss = cell[(x, -X_AT[0])], cell[(w, -W_AT[0])], cell[(s, -S_AT[0])]
    print("scores at the planted cells:", sx, sw, ss)
    assert sx > sw > ss >= np.float32(T)
    # ... as the numpy restatement of the family has them
    cs = recording_ref.cells(block[0], ent)
    rk, rl, rc = recording_ref.occurrences(cs, T, True, cap, base)
    assert rc == int(counts[0]) and np.array_equal(rk, keys[0].cpu().numpy().view(np.uint64)) and np.array_equal(rl, lags[0].cpu().numpy())
    # the composite: the reference greedy over those rows
    lengths = corpus.entry_lengths_from_keys_device(keys, index_base=base)
    gpu.cuda.synchronize()
    want = _reference_rows(lb, keys, lags, lengths, counts, per, out_cap)
    stream = gpu.cuda.Stream()
    stream.wait_stream(gpu.cuda.current_stream())
    out = corpus.recording_occurrence_segments_batch_keys_device(packed, R, per, T, cap, out_cap, peaks=True, index_base=base, stream=stream)
    stream.synchronize()
    assert len(out) == 6 and out[0].shape == (R, out_cap) and out[4].shape == (R,) and gpu.equal(out[5], counts)
    _same(_np(out), want)
    dec = lb.decode_occurrence_segments(*out[:5], index_base=base)
    st, ix, score, lag, ln = dec[0]
    assert st.tolist()[:2] == [S_AT[0], X_AT[0]] and ix.tolist()[:2] == [s, x] and ln.tolist()[:2] == [5, 10] and lag.tolist()[:2] == [-5, -12]
    assert score[0] == np.float32(ss) and score[1] == 1.0
    st1, ix1 = dec[1][0].tolist(), dec[1][1].tolist()
    assert (30, 4) in zip(st1, ix1)
    # the timeline's segments on the same window do not hold S: W wins offset 5 and loses to X
    old = lb.decode_segments(*corpus.recording_segments_batch_keys_device(packed, R, per, T, out_cap, index_base=base), index_base=base)
    assert X_AT[0] in old[0][0].tolist() and S_AT[0] not in old[0][0].tolist() and s not in old[0][1].tolist()
    # the key block goes into the calls that read keys as it is
    again = corpus.entry_lengths_from_keys_device(out[1], index_base=base)
    gpu.cuda.synchronize()
    assert gpu.equal(again, out[3])
    # the one-recording convenience: the same spans, decoded
    one = corpus.recording_occurrence_segments(lb.Fingerprint.from_bools(block[0]), T)
    assert len(one[0]) == int(out[4][0]) <= out_cap and all(np.array_equal(a, b) for a, b in zip(one, dec[0]))
    # a capacity the row overflows: the counts say so, and the spans are those of the cells that were kept
    cut = corpus.recording_occurrence_segments_batch_keys_device(packed, R, per, T, 2, out_cap, peaks=True, index_base=base)
    gpu.cuda.synchronize()
    assert gpu.equal(cut[5], counts) and int(counts[0]) > 2
    k2, g2, c2 = corpus.query_packed_occurrences_batch_keys_device(packed, R, per, T, 2, peaks=True, index_base=base)
    n2 = corpus.entry_lengths_from_keys_device(k2, index_base=base)
    gpu.cuda.synchronize()
    _same(_np(cut), _reference_rows(lb, k2, g2, n2, c2, per, out_cap))


def test_stream_bank_occurrence_segments(lb, gpu, oracle):
    """three channels of test_gpu_stream_bank.py's pruned configuration; the corpus holds random entries and, per channel, rows
    [total - 15, total - 5) of its own sub-fingerprints and the first half of them once more: StreamBank.occurrence_segments after
    the pushes equals the composite on window_device's output, and the planted span starts at offset 5 of a window of 20"""
    rate, window, stride, bands, length = 44100, 1024, 64, 32, 200
    hop, frames, n, cap, out_cap, t = 128 * stride, 23, 20, 64, 6, 0.7
    cfg = oracle.Config(rate, window, stride, bands, length)
    sig = [oracle.synth_clip(0x53424B31, c, rate, window + frames * hop + 7) for c in range(3)]
    fps = [oracle.fingerprint_pcm(x, cfg) for x in sig]
    det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
    bank = lb.StreamBank(det, 3, 24)
    half = [x.size // 2 for x in sig]
    for part in ([x[:h] for x, h in zip(sig, half)], [x[h:] for x, h in zip(sig, half)]):
        bank.push_device(gpu.from_numpy(np.concatenate(part).astype(np.float32)).cuda(), [p.size for p in part])
    assert bank.totals().tolist() == [frames] * 3
    ent = _random(oracle, 61, np.random.default_rng(4).integers(1, 16, 30), length)
    planted = {}
    for c in range(3):
        planted[c] = len(ent)
        ent.append(fps[c][frames - 15:frames - 5].copy())
        ent.append(fps[c][frames - 15:frames - 10].copy())
    corpus = _ragged(lb, gpu, oracle, ent, length)
    channels = [2, 0, 1]
    stream = gpu.cuda.Stream()
    stream.wait_stream(gpu.cuda.current_stream())
    out = bank.occurrence_segments(corpus, channels, n, t, cap, out_cap, stream=stream)
    stream.synchronize()
    win = bank.window_device(channels, n)
    direct = corpus.recording_occurrence_segments_batch_keys_device(win.reshape(3 * n, 32), 3, n, t, cap, out_cap)
    gpu.cuda.synchronize()
    assert len(out) == 6 and all(gpu.equal(a, b) for a, b in zip(out, direct))
    keys, lags, counts = corpus.query_packed_occurrences_batch_keys_device(win.reshape(3 * n, 32), 3, n, t, cap, peaks=True)
    lengths = corpus.entry_lengths_from_keys_device(keys)
    gpu.cuda.synchronize()
    _same(_np(out), _reference_rows(lb, keys, lags, lengths, counts, n, out_cap))
    for j, (st, idx, sc, lag, ln) in enumerate(lb.decode_occurrence_segments(*out[:5])):
        at = st.tolist().index(5)
        assert (idx[at], sc[at], lag[at], ln[at]) == (planted[channels[j]], 1.0, -5, 10)
