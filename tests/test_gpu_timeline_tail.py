"""GPU tests of the timeline tail (LBAudioDetectiveCorpusRecordingPackedTimelineTailBatchKeysDevice, k_timeline_tail.hip,
LiveTimeline): every channel's timeline kept current from each push -- the previous timeline shifted left by the push's count,
merged by unsigned maximum with the cells the push completed.  Every key and length is compared exactly: against numpy
(timeline_tail_ref on occurrences_tail_ref's cells), against the batch occurrences call (peaks off) filtered and folded on the host,
and -- the invariant -- device against device with the batch timeline call on the same windows.  Nothing needs a tolerance.  The
corpus and the blocks are test_gpu_occurrences_tail's, made once: 150 ragged entries across the seams of 64 and 128 entries, lengths
1, 48 (the window), 49 and 300 (both skipped), the 44 that clips at offset 0, the entry planted across the row seam 6 | 7.  Outputs
are poison-filled between guard words.  The thresholds are values of the reference's own cells."""
import numpy as np
import pytest

import occurrences_tail_ref as tail
import test_gpu_occurrences_tail as ot
import timeline_ref
import timeline_tail_ref as ref

pytestmark = pytest.mark.gpu

POISON = ot.POISON
POISON32 = ot.POISON32
GUARD = 16                                 # words on each side of an output that must stay poison
L, PER, R, NEW, PER64, R64, NEW64, N_CASE = ot.L, ot.PER, ot.R, ot.NEW, ot.PER64, ot.R64, ot.NEW64, ot.N_CASE
WALK = 64
BATCH_CAP = ot.BATCH_CAP
PREV_NEW = [0, 1, 8, 3, 48, 2, 100, 20, 8]  # under max_new = 8: silent, within the bound, the window itself, beyond it, above the bound


class _Out:
    """keys (and lengths) of rows x per words, poison-filled, between poison guard words"""

    def __init__(self, gpu, rows, per, want_lengths=True):
        n = rows * per
        self.n, self.shape = n, (rows, per)
        self.kbuf = gpu.full((n + 2 * GUARD,), POISON, dtype=gpu.int64, device="cuda")
        self.lbuf = gpu.full((n + 2 * GUARD,), POISON32, dtype=gpu.int32, device="cuda") if want_lengths else None
        self.keys = self.kbuf[GUARD:GUARD + n].view(rows, per)
        self.lengths = self.lbuf[GUARD:GUARD + n].view(rows, per) if want_lengths else None

    def host(self):
        """(keys uint64 [rows, per], lengths uint32 or None); the guards still hold the poison"""
        k = self.kbuf.cpu().numpy()
        assert np.all(k[:GUARD] == POISON) and np.all(k[GUARD + self.n:] == POISON)
        keys = k[GUARD:GUARD + self.n].view(np.uint64).reshape(self.shape)
        if self.lbuf is None:
            return keys, None
        w = self.lbuf.cpu().numpy()
        assert np.all(w[:GUARD] == POISON32) and np.all(w[GUARD + self.n:] == POISON32)
        return keys, w[GUARD:GUARD + self.n].view(np.uint32).reshape(self.shape)


def _tail(gpu, corpus, packed, rows, per, new, max_new, t, prev=None, range_=0, base=0, want_lengths=True, stream=None):
    """one call into poison-filled buffers -> (keys uint64 [rows, per], lengths uint32 [rows, per] or None)"""
    out = _Out(gpu, rows, per, want_lengths)
    d_new = gpu.from_numpy(np.asarray(new, np.uint32).view(np.int32)).cuda()
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = corpus.recording_timeline_tail_batch_keys_device(packed, rows, per, d_new, float(t), max_new=max_new, prev_keys=prev,
                                                           keys_out=out.keys, lengths_out=out.lengths, want_lengths=want_lengths,
                                                           range_=range_, index_base=base, stream=stream)
    assert got[0] is out.keys and got[1] is out.lengths
    if stream is not None:
        stream.synchronize()
    else:
        gpu.cuda.synchronize()
    return out.host()


def _expected(m, cells, t, per, news, prev=None, base=0):
    """the reference's rows from the cells of every row: (keys uint64 [rows, per], lengths uint32 [rows, per])"""
    keys = np.stack([ref.roll(None if prev is None else prev[r], min(int(news[r]), per), ref.strip_of_cells(per, c, t, base))
                     for r, c in enumerate(cells)])
    return keys, ref.lengths_of(keys, m["lengths"], base)


def _folded(filtered, per):
    """the filtered batch occurrences rows (keys, lags, counts: every tail match of a row, not cut) folded per offset"""
    keys, lags, counts = filtered
    out = np.zeros((len(counts), per), np.uint64)
    for r, c in enumerate(counts):
        assert c <= keys.shape[1]
        for k, lag in zip(keys[r][:c], lags[r][:c]):
            if k > out[r][-lag]:
                out[r][-lag] = k
    return out


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    if got[1] is not None and want[1] is not None:
        assert np.array_equal(got[1], want[1])


def _prev(m, rows, per, seed=77):
    """a previous state of random non-zero keys: scores in (0, 1], indices inside AND behind the corpus"""
    rng = np.random.default_rng(seed)
    score = rng.uniform(0.05, 1.0, (rows, per)).astype(np.float32)
    idx = rng.integers(0, 2 * N_CASE, (rows, per)).astype(np.uint64)
    keys = (score.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)
    assert keys.all() and (idx >= N_CASE).any() and (idx < N_CASE).any()
    return keys


# ---- 1. one call, no previous state ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,new,max_new", [("w48", NEW, 8), ("w48", NEW, 5), ("w48", NEW, 1), ("w80", NEW64, 64), ("w80", NEW64, 33)])
def test_strips_equal_the_reference_and_the_folded_batch_call(lb, gpu, oracle, name, new, max_new):
    m = ot._module(lb, gpu, oracle)
    block = m["blocks"][name]
    rows, per = block.shape[0], block.shape[1]
    cells, ds = ot._cells(m, name, new, max_new)
    assert max(ds) == min(max_new, per) and 0 in ds                 # a device count above the bound is clamped; a silent channel
    ts = ot._thresholds(cells)
    assert set(ts) == {"max", "4th", "median", "one", "above"} and ts["above"] == 1.5
    for what, t in ts.items():
        want = _expected(m, cells, t, per, new)
        got = _tail(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, t)
        _same(got, want)
        assert np.array_equal(got[0], _folded(ot._filtered(m, gpu, name, ds, t, BATCH_CAP), per))
        if what == "median":
            assert np.count_nonzero(want[0]) > rows                 # many offsets hold a winner ...
            beaten = sum(len({o for (_j, o, q) in c if q >= t}) < sum(q >= t for (_j, _o, q) in c) for c in cells)
            assert max_new == 1 or beaten                           # ... and several entries met in one slot
        if what == "above":
            assert not got[0].any() and not got[1].any()
    # the skipped entries never win, the window-long one can (offset 0 alone)
    everything = _tail(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, 1e-30)
    idx = 0xFFFFFFFF - (everything[0][everything[0] != 0] & np.uint64(0xFFFFFFFF))
    longer = {j for j in (ot.E48, ot.E49, ot.E300) if m["lengths"][j] > per}
    assert longer and not (set(idx.tolist()) & longer)
    d0 = [r for r, d in enumerate(ds) if d == 0]
    assert d0 and not everything[0][d0].any() and not everything[1][d0].any()     # d = 0: an empty row


def test_no_lengths_an_index_base_a_range_and_a_side_stream(lb, gpu, oracle):
    m = ot._module(lb, gpu, oracle)
    cells, ds = ot._cells(m, "w48", NEW, 8)
    ts = ot._thresholds(cells)
    dev = m["dev"]["w48"]
    want = _expected(m, cells, ts["median"], PER, NEW)
    got = _tail(gpu, m["corpus"], dev, R, PER, NEW, 8, ts["median"], want_lengths=False)
    assert got[1] is None and np.array_equal(got[0], want[0])
    side = gpu.cuda.Stream()
    for t in (ts["median"], ts["4th"]):
        _same(_tail(gpu, m["corpus"], dev, R, PER, NEW, 8, t, stream=side), _expected(m, cells, t, PER, NEW))
        _same(_tail(gpu, m["corpus"], dev, R, PER, NEW, 8, t, stream=side, want_lengths=False), (_expected(m, cells, t, PER, NEW)[0], None))
    for base in (1000, (1 << 32) - N_CASE):                         # ... the last index a corpus may have
        want = _expected(m, cells, ts["median"], PER, NEW, base=base)
        got = _tail(gpu, m["corpus"], dev, R, PER, NEW, 8, ts["median"], base=base)
        _same(got, want)
        assert got[1].any()
        assert np.array_equal(got[0], _folded(ot._filtered(m, gpu, "w48", ds, ts["median"], BATCH_CAP, base=base), PER))
    masked, _ = ot._cells(m, "w48", NEW, 8, range_=20)
    t = ot._thresholds(masked)["median"]
    _same(_tail(gpu, m["corpus"], dev, R, PER, NEW, 8, t, range_=20), _expected(m, masked, t, PER, NEW))
    # the host sequence is the device tensor (max_new: the sequence's maximum, 20)
    c20, _ = ot._cells(m, "w48", NEW, 20)
    keys, lengths = m["corpus"].recording_timeline_tail_batch_keys_device(dev, R, PER, NEW, float(ts["4th"]))
    gpu.cuda.synchronize()
    assert keys.shape == (R, PER) and keys.dtype == gpu.int64 and lengths.shape == (R, PER) and lengths.dtype == gpu.int32
    _same((keys.cpu().numpy().view(np.uint64), lengths.cpu().numpy().view(np.uint32)), _expected(m, c20, ts["4th"], PER, NEW))


# ---- 2. one call with a previous state -----------------------------------------------------------------------------------------------------
def test_a_previous_state_is_shifted_per_row_and_the_lengths_are_looked_up(lb, gpu, oracle):
    m = ot._module(lb, gpu, oracle)
    cells, ds = ot._cells(m, "w48", PREV_NEW, 8)
    assert ds == (0, 1, 8, 3, 8, 2, 8, 8, 8)
    prev = _prev(m, R, PER)
    d_prev = gpu.from_numpy(prev.view(np.int64)).cuda()
    ts = ot._thresholds(cells)
    for t, base in ((ts["median"], 0), (ts["4th"], 0), (np.float32(1.5), 0), (ts["median"], 40)):
        want = _expected(m, cells, t, PER, PREV_NEW, prev=prev, base=base)
        got = _tail(gpu, m["corpus"], m["dev"]["w48"], R, PER, PREV_NEW, 8, t, prev=d_prev, base=base)
        _same(got, want)
        # the shift is the TRUE count's, row by row; behind it the strip alone
        strip = _expected(m, cells, t, PER, PREV_NEW, base=base)[0]
        for r, new in enumerate(PREV_NEW):
            s = min(new, PER)
            assert np.array_equal(got[0][r][:PER - s], np.maximum(prev[r][s:], strip[r][:PER - s]))
            assert np.array_equal(got[0][r][PER - s:], strip[r][PER - s:])
        assert np.array_equal(got[0][0], prev[0])                   # a silent channel keeps its row
        assert np.array_equal(got[0][6], strip[6]) and np.array_equal(got[0][4], strip[4])   # counts >= n: nothing survives
        # an index behind the corpus (or in front of the index base) has length 0, every other key its entry's
        idx = (0xFFFFFFFF - (got[0] & np.uint64(0xFFFFFFFF))).astype(np.int64) - base
        inside = (idx >= 0) & (idx < N_CASE)
        assert (~inside).any() and inside.any() and not got[1][~inside].any()
        assert np.array_equal(got[1][inside], m["lengths"][idx[inside]].astype(np.uint32))
    # the previous state alone: an empty corpus, and one whose entries are all longer than the window
    empty = lb.Corpus.ragged(L, 4, 16)
    longer = ot._ragged(lb, gpu, oracle, [m["entries"][ot.E49], m["entries"][ot.E300]])
    moved = np.stack([ref.roll(prev[r], min(n, PER), np.zeros(PER, np.uint64)) for r, n in enumerate(PREV_NEW)])
    for corpus, lengths in ((empty, []), (longer, [PER + 1, 300])):
        got = _tail(gpu, corpus, m["dev"]["w48"], R, PER, PREV_NEW, 8, 1e-30, prev=d_prev)
        _same(got, (moved, ref.lengths_of(moved, lengths)))
        got = _tail(gpu, corpus, m["dev"]["w48"], R, PER, PREV_NEW, 8, 1e-30)
        assert not got[0].any() and not got[1].any()
    # overlapping blocks are refused, a block that only touches is not
    both = gpu.zeros(2 * R * PER + 1, dtype=gpu.int64, device="cuda")
    d_new = gpu.from_numpy(np.asarray(PREV_NEW, np.int32)).cuda()
    with pytest.raises(lb.LBAudioDetectiveError) as err:
        m["corpus"].recording_timeline_tail_batch_keys_device(m["dev"]["w48"], R, PER, d_new, 0.5, max_new=8, prev_keys=both[1:],
                                                              keys_out=both[:R * PER])
    assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    both[R * PER:2 * R * PER] = d_prev.reshape(-1)
    m["corpus"].recording_timeline_tail_batch_keys_device(m["dev"]["w48"], R, PER, d_new, float(ts["median"]), max_new=8,
                                                          prev_keys=both[R * PER:], keys_out=both[:R * PER], want_lengths=False)
    gpu.cuda.synchronize()
    assert np.array_equal(both[:R * PER].cpu().numpy().view(np.uint64).reshape(R, PER),
                          _expected(m, cells, ts["median"], PER, PREV_NEW, prev=prev)[0])


# ---- 3. the invariant --------------------------------------------------------------------------------------------------------------------
CHANNELS, UPDATES, TOTAL = 9, 6, 330


def _long_recording(oracle, m):
    """one long recording with planted entries, and per channel where its window ends at first and its push schedule"""
    e = m["entries"]
    rec = oracle.synth_ragged_entries(2718, 0, np.array([TOTAL], np.uint32), L).copy()
    rng = np.random.default_rng(31)
    short = [j for j in range(N_CASE) if 2 <= len(e[j]) <= 40]
    at = 3
    while at < TOTAL - 45:
        j = short[int(rng.integers(len(short)))]
        rec[at:at + len(e[j])] = e[j]
        at += len(e[j]) + int(rng.integers(0, 9))
    ends = [PER + 29 * c for c in range(CHANNELS)]
    schedule = rng.integers(0, 9, (UPDATES, CHANNELS))
    schedule[0, :3], schedule[1, 3:5], schedule[2, 0] = (0, 8, 1), (8, 0), 8
    assert max(ends) + int(schedule.sum(axis=0).max()) <= TOTAL
    return rec, ends, schedule


def _windows(rec, ends):
    return np.stack([rec[end - PER:end] for end in ends])


def test_updates_from_a_seed_equal_the_batch_timeline_of_every_window(lb, gpu, oracle):
    """nine channels cut from one long recording, each with its own push schedule (0 .. 8 new sub-fingerprints a push, max_new 8):
    seeded with the batch timeline, after each of six updates keys and lengths are the batch timeline's of the same windows, bit
    for bit, and the segments of both are equal blocks.  On the reference alone, before any device call: the final state holds a
    key of the seed, a key an EARLIER update brought and later ones shifted, a slot where a new cell beat a previous key and a
    slot where a previous key beat a new cell."""
    m = ot._module(lb, gpu, oracle)
    ent, lengths = m["entries"], m["lengths"]
    rec, ends, schedule = _long_recording(oracle, m)
    first = [tail.tail_cells(w, ent, 8) for w in _windows(rec, ends)]
    t = ot._thresholds(first)["median"]
    # ---- the reference: the states, and where every key of a state came from (0: the seed, u: update u; -1: no key)
    state = [timeline_ref.timeline(w, ent, t)[0] for w in _windows(rec, ends)]
    born = [np.where(s != 0, 0, -1) for s in state]
    new_beat_prev = prev_beat_new = 0
    at = list(ends)
    expected = []
    for u in range(UPDATES):
        at = [a + int(n) for a, n in zip(at, schedule[u])]
        for c, w in enumerate(_windows(rec, at)):
            n = int(schedule[u][c])
            strip = ref.strip(w, ent, n, t)
            moved, moved_born = ref.roll(state[c], n, np.zeros(PER, np.uint64)), np.full(PER, -1)
            moved_born[:PER - n] = born[c][n:]
            new_beat_prev += int(np.count_nonzero((strip > moved) & (moved != 0)))
            prev_beat_new += int(np.count_nonzero((moved > strip) & (strip != 0)))
            state[c] = np.maximum(strip, moved)
            born[c] = np.where(strip > moved, u + 1, np.where(moved != 0, moved_born, -1))
        expected.append((np.stack(state), ref.lengths_of(np.stack(state), lengths)))
    final_born = np.stack(born)
    assert (final_born == 0).any(), "the final state holds a key that came from the seed"
    later = np.array([[int(schedule[b:, c].sum()) if b >= 1 else 0 for b in row] for c, row in enumerate(final_born)])
    assert ((final_born >= 1) & (later > 0)).any(), "... and a key an earlier update brought, shifted since"
    assert new_beat_prev > 0 and prev_beat_new > 0, (new_beat_prev, prev_beat_new)
    assert np.array_equal(expected[-1][0], np.stack([timeline_ref.timeline(w, ent, t)[0] for w in _windows(rec, at)]))
    # ---- the device
    corpus = m["corpus"]

    def packed(ends_):
        return gpu.from_numpy(ot._packed(oracle, _windows(rec, ends_).reshape(-1, L))).cuda()

    at = list(ends)
    keys, lens = corpus.recording_timeline_batch_keys_device(packed(at), CHANNELS, PER, float(t))
    spare = None
    for u in range(UPDATES):
        at = [a + int(n) for a, n in zip(at, schedule[u])]
        dev = packed(at)
        out = spare if spare is not None else (gpu.empty_like(keys), gpu.empty_like(lens))
        out[0].fill_(POISON)
        out[1].fill_(POISON32)
        d_new = gpu.from_numpy(schedule[u].astype(np.int32)).cuda()
        got = corpus.recording_timeline_tail_batch_keys_device(dev, CHANNELS, PER, d_new, float(t), max_new=8, prev_keys=keys,
                                                               keys_out=out[0], lengths_out=out[1])
        full = corpus.recording_timeline_batch_keys_device(dev, CHANNELS, PER, float(t))
        gpu.cuda.synchronize()
        assert gpu.equal(got[0], full[0]) and gpu.equal(got[1], full[1]), u
        assert np.array_equal(got[0].cpu().numpy().view(np.uint64), expected[u][0]), u
        assert np.array_equal(got[1].cpu().numpy().view(np.uint32), expected[u][1]), u
        seg_a = lb.timeline_segments_device(got[0], got[1], 24)
        seg_b = lb.timeline_segments_device(full[0], full[1], 24)
        gpu.cuda.synchronize()
        assert all(gpu.equal(a, b) for a, b in zip(seg_a, seg_b)) and int(seg_a[3].min()) > 0, u
        spare, (keys, lens) = (keys, lens), got


# ---- 4. grids and passes -----------------------------------------------------------------------------------------------------------------
def test_grids_and_passes_change_nothing(lb, gpu, oracle):
    """a grid ceiling of one workgroup sends both kernels' strided loops on a second trip (3 blocks of entries, 432 cells); join
    scratch limits give passes of four, two and one recording -- the strips do not grow with the entries, so no limit cuts the
    entries into chunks: the smallest limit that is accepted is ONE recording's strip, one below it is refused"""
    m = ot._module(lb, gpu, oracle)
    corpus = m["corpus"]
    cells, _ds = ot._cells(m, "w48", PREV_NEW, 8)
    prev = _prev(m, R, PER, seed=5)
    d_prev = gpu.from_numpy(prev.view(np.int64)).cuda()
    t = ot._thresholds(cells)["median"]
    plan = lb.debug_timeline_tail_plan(R, PER, 1, 300, N_CASE, 8)
    width = plan["strip_width"]
    assert width == PER - 1 + 8 and -(-N_CASE // WALK) * -(-R // plan["recordings_per_workgroup"]) == 3 and R * PER > 256
    unforced = _tail(gpu, corpus, m["dev"]["w48"], R, PER, PREV_NEW, 8, t, prev=d_prev)
    _same(unforced, _expected(m, cells, t, PER, PREV_NEW, prev=prev))
    bare = _tail(gpu, corpus, m["dev"]["w48"], R, PER, PREV_NEW, 8, t)
    try:
        for ceiling in (1, 2):
            lb.debug_set_grid_ceiling(ceiling)
            before = lb.debug_grid_ceiling()[1]
            _same(_tail(gpu, corpus, m["dev"]["w48"], R, PER, PREV_NEW, 8, t, prev=d_prev), unforced)
            assert lb.debug_grid_ceiling()[1] >= before + (2 if ceiling == 1 else 1)        # both kernels / the compute kernel
            _same(_tail(gpu, corpus, m["dev"]["w48"], R, PER, PREV_NEW, 8, t), bare)
    finally:
        lb.debug_set_grid_ceiling(0)
    try:
        for limit, rpp in ((4 * width * 8 + 9, 4), (2 * width * 8, 2), (width * 8, 1)):
            assert lb.debug_timeline_tail_plan(R, PER, 1, 300, N_CASE, 8, limit)["recordings_per_pass"] == rpp
            corpus.set_join_scratch_limit(limit)
            _same(_tail(gpu, corpus, m["dev"]["w48"], R, PER, PREV_NEW, 8, t, prev=d_prev), unforced)
            _same(_tail(gpu, corpus, m["dev"]["w48"], R, PER, PREV_NEW, 8, t, want_lengths=False), (bare[0], None))
        lb.debug_set_grid_ceiling(1)                                # passes of two AND second trips
        corpus.set_join_scratch_limit(2 * width * 8)
        _same(_tail(gpu, corpus, m["dev"]["w48"], R, PER, PREV_NEW, 8, t, prev=d_prev), unforced)
        lb.debug_set_grid_ceiling(0)
        corpus.set_join_scratch_limit(width * 8 - 1)                # a limit below ONE recording's strip
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            _tail(gpu, corpus, m["dev"]["w48"], R, PER, PREV_NEW, 8, t, prev=d_prev)
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    finally:
        lb.debug_set_grid_ceiling(0)
        corpus.set_join_scratch_limit(0)
    # max_new beyond the clamp changes nothing: counts of at most 8 under a bound of 8, 13 and 64 (other lanes, another strip width)
    small = [min(n, 8) for n in NEW]
    c8, _ = ot._cells(m, "w48", small, 8)
    want = _expected(m, c8, t, PER, small, prev=prev)
    for max_new in (8, 13, 64):
        _same(_tail(gpu, corpus, m["dev"]["w48"], R, PER, small, max_new, t, prev=d_prev), want)


def test_long_entries_lower_the_recordings_per_workgroup(lb, gpu, oracle):
    """longest entry 1 024 against the shortest 5 in windows of 1 090 with 64 lanes: two sub-windows of 1 087 records with their
    strips of 1 083 slots fit the LDS where the tail lists take three sub-windows, so four recordings make two groups"""
    per, rows, new = 1090, 4, [8, 64, 0, 33]
    plan = lb.debug_timeline_tail_plan(rows, per, 5, 1024, 6, 64)
    assert (plan["lanes"], plan["recordings_per_workgroup"], plan["window_records"], plan["strip_width"]) == (64, 2, 1087, 1083)
    assert lb.debug_occurrences_tail_plan(rows, per, 5, 1024, 6, 64)["recordings_per_workgroup"] == 3
    ent = ot._random(oracle, 77, [1024, 1000, 5, 1020, 17, 1024])
    block = oracle.synth_ragged_entries(78, 0, np.array([rows * per], np.uint32), L).reshape(rows, per, L).copy()
    block[0, per - 1024:] = ent[0]                                  # ends at the last record: slot 1 024 - 5 of the strip
    block[3, 40:40 + 1024] = ent[5]                                 # offset 40 of the cells 34 .. 66
    block[1, per - 3 - 5:per - 3] = ent[2]
    corpus = ot._ragged(lb, gpu, oracle, ent)
    dev = gpu.from_numpy(ot._packed(oracle, block.reshape(-1, L))).cuda()
    ds = tuple(tail.clamp_new(n, 64, per) for n in new)
    cells = [tail.tail_cells(rec, ent, d) for rec, d in zip(block, ds)]
    fake = {"lengths": np.array([len(e) for e in ent], np.int64)}
    for t in ot._thresholds(cells).values():
        _same(_tail(gpu, corpus, dev, rows, per, new, 64, t), _expected(fake, cells, t, per, new))
    got = _tail(gpu, corpus, dev, rows, per, new, 64, 1.0)
    one = np.uint64(ref.key_of(np.float32(1.0), 0))
    assert got[0][0][per - 1024] == one and got[1][0][per - 1024] == 1024 and got[0][3][40] == np.uint64(ref.key_of(np.float32(1.0), 5))
    assert got[0][1][per - 8] == np.uint64(ref.key_of(np.float32(1.0), 2)) and got[1][1][per - 8] == 5


# ---- 5. the stream bank ------------------------------------------------------------------------------------------------------------------
def test_live_timeline_on_a_stream_bank(lb, gpu, oracle):
    """three channels of test_gpu_stream_bank.py's pruned configuration; the corpus holds random entries and spans of the
    channels' own sub-fingerprints.  After each of four pushes within max_new the state equals StreamBank.timeline, bit for bit; a
    push above max_new seeds again; segments equals StreamBank.segments"""
    rate, window, stride, bands, length = 44100, 1024, 64, 32, 200
    hop, n, max_new = 128 * stride, 20, 5
    first = [21, 20, 23]
    pushes = [[3, 0, 5], [1, 4, 2], [5, 5, 0], [2, 1, 3], [9, 2, 1], [1, 1, 4]]       # the fifth is above max_new on channel 0
    frames = [f + sum(p[c] for p in pushes) for c, f in enumerate(first)]
    cfg = oracle.Config(rate, window, stride, bands, length)
    sig = [oracle.synth_clip(0x4C54494D, c, rate, window + frames[c] * hop + 11) for c in range(3)]
    fps = [oracle.fingerprint_pcm(s, cfg) for s in sig]
    assert [len(f) for f in fps] == frames
    ent = ot._random(oracle, 61, np.random.default_rng(4).integers(1, 16, 30), length)
    planted = []
    for c in range(3):
        for a, b in ((first[c] - 6, first[c] + 2), (first[c] + 4, first[c] + 9), (frames[c] - 12, frames[c])):
            planted.append(len(ent))
            ent.append(fps[c][a:b].copy())
    corpus = ot._ragged(lb, gpu, oracle, ent, length)
    det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
    bank = lb.StreamBank(det, 3, 24)
    channels = [2, 0, 1]
    live = {t: lb.LiveTimeline(bank, corpus, channels, n, t, max_new=max_new) for t in (0.9, 0.55)}
    fed = [0, 0, 0]

    def push(counts):
        """the samples that complete `counts` more frames on each channel"""
        chunks = []
        for c in range(3):
            target = window + (totals[c] + counts[c]) * hop + 3 if totals[c] + counts[c] else 0
            target = max(target, fed[c])
            chunks.append(sig[c][fed[c]:target])
            fed[c] = target
        new, _ = bank.push_device(gpu.from_numpy(np.concatenate(chunks).astype(np.float32)).cuda(), [s.size for s in chunks])
        for c in range(3):
            totals[c] += counts[c]
        assert new.tolist() == list(counts) and bank.totals().tolist() == totals
        return new

    totals = [0, 0, 0]
    new = push(first)
    winners = set()
    for step in range(len(pushes) + 1):
        if step:
            new = push(pushes[step - 1])
        for t, lt in live.items():
            before = lt._state
            keys, lens = lt.update(new)
            want = bank.timeline(corpus, channels, n, t)
            gpu.cuda.synchronize()
            assert keys.shape == (3, n) and gpu.equal(keys, want[0]) and gpu.equal(lens, want[1]), (step, t)
            if before is not None:
                assert keys.data_ptr() != before[0].data_ptr()      # the two pairs take turns
            idx, _sc, _ln = lb.decode_timeline_batch_keys(keys, lens)
            winners |= set(np.asarray(idx).reshape(-1).tolist())
            seg = lt.segments(8)
            seg_want = bank.segments(corpus, channels, n, t, 8)
            gpu.cuda.synchronize()
            assert all(gpu.equal(a, b) for a, b in zip(seg, seg_want)), (step, t)
    assert len(winners & set(planted)) >= 6
    # the tail call itself with the count above the bound lacks cells the seeded state has: update() did seed again
    lt = lb.LiveTimeline(bank, corpus, channels, n, 0.55, max_new=max_new)
    lt.update(new)
    lt.reseed()
    assert lt._state is None
    keys, lens = lt.update([0, 0, 0])
    want = bank.timeline(corpus, channels, n, 0.55)
    gpu.cuda.synchronize()
    assert gpu.equal(keys, want[0]) and gpu.equal(lens, want[1])
    keys2, _ = lt.update([0, 0, 0])                                 # a silent push through the tail call: the same rows
    gpu.cuda.synchronize()
    assert gpu.equal(keys2, want[0]) and keys2.data_ptr() != keys.data_ptr()
