"""GPU tests of the recording tail (LBAudioDetectiveCorpusRecordingPackedScoresTailBatchDevice, the top-K and threshold key forms
behind it, k_recording_tail.hip, StreamBank.new_best / new_matches_above): the cells a push has completed folded to one value per
(recording, entry).  Every score, lag, key and count is compared exactly against numpy (recording_tail_ref: the fold of
occurrences_tail_ref's cells by recording_ref's rules) AND, device against device, against the tail occurrences call folded on the
host: nothing needs a tolerance.  Output buffers are poison-filled before every call and stand between guard words.  The corpus,
the windows and the reference's cells are test_gpu_occurrences_tail.py's, made once and shared with it: 150 ragged entries of 32
Booleans (blocks of 64, 64 and 22 entries; lengths 1 .. 40, one of 1, one of 48 -- the window --, one of 49 and one of 300, both
skipped), nine windows of 48 with new counts 0, 1, 8, 3, 5, 2, 8, 20 (clamped) and 8, five windows of 80.  The thresholds are
values of the reference's own folded scores."""
import numpy as np
import pytest

import occurrences_tail_ref as tail
import recording_tail_ref as ref
import test_gpu_occurrences_tail as T

pytestmark = pytest.mark.gpu

POISON, POISON32 = T.POISON, T.POISON32
L, WALK, N_CASE, CAP = T.L, T.WALK, T.N_CASE, T.CAP
PER, R, NEW, NEW64 = T.PER, T.R, T.NEW, T.NEW64
E1, E17, E22, E44, E48, E49, E300 = T.E1, T.E17, T.E22, T.E44, T.E48, T.E49, T.E300
ONE = np.float32(1.0)
GUARD = 16                                # words on each side of every output buffer
SHAPES = [("w48", NEW, 8), ("w48", NEW, 5), ("w48", NEW, 1), ("w80", NEW64, 64), ("w80", NEW64, 33)]


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _fold(m, name, new, max_new, range_=0):
    """(scores float32 [rows, entries], lags int32 [rows, entries], clamped counts) of a module block, made once"""
    cells, ds = T._cells(m, name, new, max_new, range_)
    key = ("fold", name, ds, range_)
    if key not in m["cells"]:
        out = [ref.fold_cells(c, len(m["entries"])) for c in cells]
        m["cells"][key] = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))
    return (*m["cells"][key], ds)


def _thresholds(sc):
    """values of the reference's own folded scores -- the largest, the 4th largest distinct and the median of those above 0 --,
    and 1.0 and 1.5 as such"""
    pos = np.sort(sc[sc > 0])
    distinct = np.unique(pos)
    return {"max": np.float32(pos[-1]), "4th": np.float32(distinct[-4]), "median": np.float32(pos[len(pos) // 2]),
            "one": np.float32(1.0), "above": np.float32(1.5)}


def _want_topk(sc, lags, k, base=0):
    out = [ref.topk_row(s, l, k, base) for s, l in zip(sc, lags)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _want_threshold(sc, lags, t, capacity, base=0):
    out = [ref.threshold_row(s, l, t, capacity, base) for s, l in zip(sc, lags)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64)


# ---- the calls, into poison between guard words ------------------------------------------------------------------------------------
class _Buf:
    """n words of `dtype` filled with poison, GUARD more on each side"""

    def __init__(self, gpu, shape, dtype, poison):
        self.n = int(np.prod(shape))
        self.poison = poison
        self.whole = gpu.full((self.n + 2 * GUARD,), poison, dtype=dtype, device="cuda")
        self.inner = self.whole[GUARD:GUARD + self.n].view(*shape) if self.n else self.whole[GUARD:GUARD]

    def host(self):
        """the words as numpy, once the guards on both sides are seen untouched"""
        w = self.whole.cpu().numpy()
        assert (w[:GUARD] == self.poison).all() and (w[GUARD + self.n:] == self.poison).all(), "a guard word was written"
        return w[GUARD:GUARD + self.n]


def _dev_counts(gpu, new):
    return gpu.from_numpy(np.asarray(new, np.uint32).view(np.int32)).cuda()


def _sync(gpu, stream):
    if stream is not None:
        stream.synchronize()
    else:
        gpu.cuda.synchronize()


def _scores(gpu, corpus, packed, rows, per, new, max_new, range_=0, want_lags=True, stream=None):
    """the scores form -> (score bits uint32 [rows, entries], lags int32 or None)"""
    n = len(corpus)
    sc = _Buf(gpu, (rows, n), gpu.int32, POISON32)
    lg = _Buf(gpu, (rows, n), gpu.int32, POISON32) if want_lags else None
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = corpus.recording_scores_tail_batch_device(packed, rows, per, _dev_counts(gpu, new), max_new=max_new, range_=range_,
                                                    scores_out=sc.inner.view(gpu.float32), lags_out=lg.inner if lg else None,
                                                    want_lags=want_lags, stream=stream)
    assert (got[1] is None) == (not want_lags)
    _sync(gpu, stream)
    return sc.host().view(np.uint32).reshape(rows, n), lg.host().reshape(rows, n) if lg else None


def _topk(gpu, corpus, packed, rows, per, new, max_new, k, range_=0, base=0, want_lags=True, stream=None):
    """the top-K form -> (keys uint64 [rows, k], lags int32 or None)"""
    keys = _Buf(gpu, (rows, k), gpu.int64, POISON)
    lg = _Buf(gpu, (rows, k), gpu.int32, POISON32) if want_lags else None
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    corpus.query_packed_recording_topk_tail_batch_keys_device(packed, rows, per, _dev_counts(gpu, new), k, max_new=max_new, range_=range_,
                                                              index_base=base, keys_out=keys.inner, lags_out=lg.inner if lg else None,
                                                              stream=stream)
    _sync(gpu, stream)
    return keys.host().view(np.uint64).reshape(rows, k), lg.host().reshape(rows, k) if lg else None


def _threshold(gpu, corpus, packed, rows, per, new, max_new, t, capacity, range_=0, base=0, want_lags=True, stream=None):
    """the threshold form -> (keys uint64 [rows, capacity], lags int32 or None, counts int64 [rows])"""
    keys = _Buf(gpu, (rows, capacity), gpu.int64, POISON)
    lg = _Buf(gpu, (rows, capacity), gpu.int32, POISON32) if want_lags else None
    counts = _Buf(gpu, (rows,), gpu.int64, POISON)
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    corpus.query_packed_recording_threshold_tail_batch_keys_device(packed, rows, per, _dev_counts(gpu, new), float(t), capacity,
                                                                   max_new=max_new, range_=range_, index_base=base, keys_out=keys.inner,
                                                                   lags_out=lg.inner if lg else None, counts_out=counts.inner,
                                                                   want_lags=want_lags, stream=stream)
    _sync(gpu, stream)
    return keys.host().view(np.uint64).reshape(rows, capacity), lg.host().reshape(rows, capacity) if lg else None, counts.host()


def _same(got, want):
    for g, w in zip(got, want):
        if g is not None and w is not None:
            assert np.array_equal(g, w)


def _all_forms(gpu, corpus, packed, rows, per, new, max_new, sc, lags, range_=0, base=0, want_lags=True, ks=(3,), ts=None):
    """the three calls against the reference's rows: every score and lag word, the K best for each K, the rows at each threshold"""
    got = _scores(gpu, corpus, packed, rows, per, new, max_new, range_, want_lags)
    _same(got, (sc.view(np.uint32), lags))
    for k in ks:
        _same(_topk(gpu, corpus, packed, rows, per, new, max_new, k, range_, base, want_lags), _want_topk(sc, lags, k, base))
    for t in (ts if ts is not None else [_thresholds(sc)["4th"]]):
        got = _threshold(gpu, corpus, packed, rows, per, new, max_new, t, CAP, range_, base, want_lags)
        want = _want_threshold(sc, lags, t, CAP, base)
        _same(got, want)
        assert np.array_equal(got[2], want[2])


# ---- 1. the scores form: every word ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,new,max_new", SHAPES)
def test_every_score_and_lag_equals_the_reference(lb, gpu, oracle, name, new, max_new):
    m = T._module(lb, gpu, oracle)
    block = m["blocks"][name]
    rows, per = block.shape[:2]
    sc, lags, ds = _fold(m, name, new, max_new)
    assert max(ds) == min(max_new, per) and 0 in ds                 # a device count above the bound is clamped; a silent channel
    got = _scores(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new)
    assert np.array_equal(got[0], sc.view(np.uint32)) and np.array_equal(got[1], lags)
    silent = ds.index(0)
    assert not got[0][silent].any() and not got[1][silent].any()    # d = 0: +0 and 0 in every word
    longer = [j for j in (E48, E49, E300) if m["lengths"][j] > per]
    assert longer and not got[0][:, longer].any() and not got[1][:, longer].any()      # the skipped entries: +0 and 0
    assert (got[0][[r for r, d in enumerate(ds) if d], E1] != 0).all()                  # the entry of one record takes part
    # NULL lags: the scores are the same
    assert np.array_equal(_scores(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, want_lags=False)[0], got[0])


# ---- 2. the key forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,new,max_new", SHAPES)
def test_key_forms_equal_the_reference_and_the_selected_scores(lb, gpu, oracle, name, new, max_new):
    m = T._module(lb, gpu, oracle)
    block = m["blocks"][name]
    rows, per = block.shape[:2]
    sc, lags, _ds = _fold(m, name, new, max_new)
    dev_sc, dev_lags = _scores(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new)
    dev_sc = dev_sc.view(np.float32)
    for k in (1, 3, 200):                                           # 200 > the entries: the zero tail
        want = _want_topk(sc, lags, k)
        got = _topk(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, k)
        _same(got, want)
        _same(got, _want_topk(dev_sc, dev_lags, k))                 # the scores form's rows, selected on the host
        if k == 200:
            assert (np.count_nonzero(got[0], axis=1) < N_CASE).all() and not got[0][:, N_CASE:].any() and not got[1][:, N_CASE:].any()
            assert not got[1][got[0] == 0].any()                    # lag 0 for a zero key
    ts = _thresholds(sc)
    for what, t in ts.items():
        want = _want_threshold(sc, lags, t, CAP)
        got = _threshold(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, t, CAP)
        _same(got, want)
        _same(got, _want_threshold(dev_sc, dev_lags, t, CAP))
        if what == "median":
            assert want[2].max() > CAP                              # at least one row is cut: the true count, the first CAP by index
            assert (np.count_nonzero(got[0], axis=1) == np.minimum(want[2], CAP)).all()
        if what == "4th":
            assert want[2].max() >= 1 and want[2].max() <= CAP      # a row is non-empty and none is cut
        if what == "above":
            assert not want[2].any() and not got[0].any() and not got[1].any() and not got[2].any()


# ---- 3. device against device: the tail occurrences call, folded on the host ---------------------------------------------------------
@pytest.mark.parametrize("name,new,max_new", [("w48", NEW, 8), ("w80", NEW64, 64), ("w80", NEW64, 33)])
def test_threshold_rows_are_the_folded_tail_occurrences(lb, gpu, oracle, name, new, max_new):
    m = T._module(lb, gpu, oracle)
    block = m["blocks"][name]
    rows, per = block.shape[:2]
    sc, _lags, ds = _fold(m, name, new, max_new)
    big = max(ds) * N_CASE                                          # d x entries: no row of the occurrences call is cut
    for what, t in _thresholds(sc).items():
        if what == "above":
            continue
        occ = T._tail(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, t, big)
        assert occ[2].max() <= big
        folded = [ref.fold_occurrence_row(occ[0][r], occ[1][r], int(occ[2][r]), CAP) for r in range(rows)]
        got = _threshold(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, t, CAP)
        assert np.array_equal(got[0], np.stack([f[0] for f in folded]))
        assert np.array_equal(got[1], np.stack([f[1] for f in folded]))
        assert got[2].tolist() == [f[2] for f in folded]


# ---- 4. ties and planted copies ------------------------------------------------------------------------------------------------------
def test_ties_and_planted_copies(lb, gpu, oracle):
    """the windows of 48 with two rows changed, the corpus with three entries behind it: E22 once more (equal scores: the lower index
    first), an entry of period 3 whose copies end at two tail offsets of row 7 (equal q_o: the lower offset), and a copy of the
    entry of ONE record one record older than the two new, empty records of row 5 (every tail cell 0: score +0)"""
    m = T._module(lb, gpu, oracle)
    e = m["entries"]
    a = T._random(oracle, 333, [3])[0]
    periodic = np.concatenate([a, a])                               # 6 records of period 3
    extra = [e[E22].copy(), periodic]
    DUP, PERIODIC = N_CASE, N_CASE + 1
    block = m["blocks"]["w48"].copy()
    block[7, PER - 9:] = np.concatenate([a, a, a])                  # the entry fits at offsets PER - 9 and PER - 6, both new (d = 8)
    block[5, PER - 2:] = 0                                          # (d = 2) two empty records ...
    block[5, PER - 3] = e[E1][0]                                    # ... behind a copy of the entry of one record: one record too old
    corpus = T._ragged(lb, gpu, oracle, e + extra)
    dev = gpu.from_numpy(T._packed(oracle, block.reshape(-1, L))).cuda()
    cells, ds = T._cells(m, "w48", NEW, 8)
    assert ds == (0, 1, 8, 3, 5, 2, 8, 8, 8)
    rows = []
    for r in range(R):
        base = tail.tail_cells(block[r], e, ds[r]) if r in (5, 7) else cells[r]
        more = [(N_CASE + j, o, q) for (j, o, q) in tail.tail_cells(block[r], extra, ds[r])]
        rows.append(ref.fold_cells(base + more, N_CASE + 2))
    sc, lags = np.stack([x[0] for x in rows]), np.stack([x[1] for x in rows])
    # each kind of tie and place is present in the reference ...
    assert sc[2, E22] == ONE == sc[2, DUP] and lags[2, E22] == lags[2, DUP] == -(PER - 22)       # ends at the newest record
    q7 = {o: q for (j, o, q) in tail.tail_cells(block[7], [periodic], 8)}
    assert q7[PER - 9] == ONE == q7[PER - 6] and sc[7, PERIODIC] == ONE and lags[7, PERIODIC] == -(PER - 9)
    assert sc[4, E17] == ONE and lags[4, E17] == -(PER - 17 - 5 + 1)                              # ends at the oldest new record
    assert sc[3, E17] < ONE and (-lags[3, E17]) in tail.tail_range(PER, 17, 3)                    # one record too old: not reported,
    assert (PER - 17 - 3) not in tail.tail_range(PER, 17, 3)                                      # ... its offset no tail cell
    assert sc[5, E1] == 0 and lags[5, E1] == -(PER - 2)             # every tail cell is 0: +0, and the lowest offset equals it
    assert sc[8, E44] == ONE and lags[8, E44] == -2 and tail.tail_range(PER, 44, 8) == range(0, 5)   # clipped at offset 0
    # ... and on the device
    _all_forms(gpu, corpus, dev, R, PER, NEW, 8, sc, lags, ks=(1, 2, 5), ts=[ONE])
    keys, klags = _topk(gpu, corpus, dev, R, PER, NEW, 8, 2)
    assert keys[2].tolist() == [T._key(ONE, E22), T._key(ONE, DUP)] and klags[2].tolist() == [-(PER - 22)] * 2
    assert keys[7][0] == T._key(ONE, PERIODIC) and klags[7][0] == -(PER - 9)
    tk, tl, tc = _threshold(gpu, corpus, dev, R, PER, NEW, 8, 1.0, CAP)
    assert T._key(ONE, E17) in tk[4] and T._key(ONE, E17) not in tk[3] and not tk[0].any() and tc[0] == 0
    assert tl[8][tk[8] == T._key(ONE, E44)].tolist() == [-2]


# ---- 5. independence -------------------------------------------------------------------------------------------------------------------
def test_passes_change_nothing(lb, gpu, oracle):
    """two recordings a pass, then one, in the key forms (the scores form takes every recording in one pass whatever the limit)"""
    m = T._module(lb, gpu, oracle)
    corpus = m["corpus"]
    sc, lags, _ds = _fold(m, "w48", NEW, 8)
    ts = _thresholds(sc)
    try:
        for limit, rpp in ((2 * N_CASE * 8 + 5, 2), (1600, 1)):
            assert lb.debug_recording_tail_plan(R, PER, 300, N_CASE, 8, limit, True)["recordings_per_pass"] == rpp
            assert lb.debug_recording_tail_plan(R, PER, 300, N_CASE, 8, limit, False)["recordings_per_pass"] == R
            corpus.set_join_scratch_limit(limit)
            _all_forms(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, sc, lags, ks=(1, 3), ts=[ts["4th"], ts["median"]])
            _all_forms(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, sc, lags, want_lags=False, ts=[ts["median"]])
        corpus.set_join_scratch_limit(T._scratch(WALK) - 1)          # the tail occurrences' refusal: below one block of ONE recording
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            _topk(gpu, corpus, m["dev"]["w48"], R, PER, NEW, 8, 3)
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    finally:
        corpus.set_join_scratch_limit(0)


@pytest.mark.parametrize("name,new,max_new,units", [("w48", NEW, 8, 3), ("w80", NEW64, 64, 6)])
def test_second_trips(lb, gpu, oracle, name, new, max_new, units):
    """the strided unit loop takes a second trip: 3 blocks of entries x groups of recordings units under a ceiling of 1 and of 4"""
    m = T._module(lb, gpu, oracle)
    block = m["blocks"][name]
    rows, per = block.shape[:2]
    plan = lb.debug_recording_tail_plan(rows, per, 300, N_CASE, max_new)
    assert -(-N_CASE // WALK) * -(-rows // plan["recordings_per_workgroup"]) == units
    sc, lags, _ds = _fold(m, name, new, max_new)
    try:
        for ceiling in (1, 4):
            lb.debug_set_grid_ceiling(ceiling)
            before = lb.debug_grid_ceiling()[1]
            _all_forms(gpu, m["corpus"], m["dev"][name], rows, per, new, max_new, sc, lags)
            assert units <= ceiling or lb.debug_grid_ceiling()[1] > before
    finally:
        lb.debug_set_grid_ceiling(0)


def test_max_new_matters_only_through_the_clamp(lb, gpu, oracle):
    """counts of at most 8 under the bounds 8, 20 and 64 (8, 32 and 64 lanes a recording): the same words"""
    m = T._module(lb, gpu, oracle)
    new = [min(n, 8) for n in NEW]
    sc, lags, _ds = _fold(m, "w48", new, 8)
    for max_new in (8, 20, 64):
        _all_forms(gpu, m["corpus"], m["dev"]["w48"], R, PER, new, max_new, sc, lags)


def test_one_recording(lb, gpu, oracle):
    m = T._module(lb, gpu, oracle)
    sc, lags, _ds = _fold(m, "w48", NEW, 8)
    t = _thresholds(sc)["4th"]
    for r in (2, 4, 0):
        _all_forms(gpu, m["corpus"], m["dev"]["w48"][r * PER:(r + 1) * PER], 1, PER, NEW[r:r + 1], 8, sc[r:r + 1], lags[r:r + 1], ts=[t])


def test_long_entries_lower_the_recordings_per_workgroup(lb, gpu, oracle):
    """longest entry 1 024 in windows of 1 030: three sub-windows fit the LDS, four recordings make two groups"""
    per, rows, new = 1030, 4, [8, 3, 0, 5]
    plan = lb.debug_recording_tail_plan(rows, per, 1024, 6, 8)
    assert (plan["lanes"], plan["recordings_per_workgroup"], plan["window_records"]) == (8, 3, 1030)
    ent = T._random(oracle, 77, [1024, 1000, 5, 1020, 17, 1024])
    block = oracle.synth_ragged_entries(78, 0, np.array([rows * per], np.uint32), L).reshape(rows, per, L).copy()
    block[0, 6:] = ent[0]                                           # ends at the last record
    block[3, 2:2 + 1024] = ent[5]                                   # offset 2 of the cells 2 .. 6
    block[1, per - 3 - 5:per - 3] = ent[2]                          # one too old
    corpus = T._ragged(lb, gpu, oracle, ent)
    dev = gpu.from_numpy(T._packed(oracle, block.reshape(-1, L))).cuda()
    sc, lags = ref.rows(block, ent, new, 8)
    assert sc[0, 0] == ONE and lags[0, 0] == -6 and sc[3, 5] == ONE and lags[3, 5] == -2 and sc[1, 2] < ONE and not sc[2].any()
    _all_forms(gpu, corpus, dev, rows, per, new, 8, sc, lags, ks=(1, 6), ts=[ONE, np.float32(sc[sc > 0].min())])


def test_a_masked_range_and_index_bases(lb, gpu, oracle):
    m = T._module(lb, gpu, oracle)
    sc, lags, _ds = _fold(m, "w48", NEW, 8)
    masked, mlags, _ = _fold(m, "w48", NEW, 8, range_=20)
    assert not np.array_equal(sc, masked)                           # the range changes cells
    ts = _thresholds(masked)
    _all_forms(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, masked, mlags, range_=20, ts=[ts["max"], ts["4th"], ts["median"]])
    for base in (1000, (1 << 32) - N_CASE):                         # ... the last index a corpus may have
        _all_forms(gpu, m["corpus"], m["dev"]["w48"], R, PER, NEW, 8, sc, lags, base=base)


def test_odd_subfingerprint_length(lb, gpu, oracle):
    """sub-fingerprints of 37 Booleans, five windows of 50, the full range and a shorter one"""
    rng = np.random.default_rng(5)
    ent = T._random(oracle, 99, rng.integers(1, 41, 70), 37)
    rows, per, new = 5, 50, [3, 8, 0, 5, 1]
    block = oracle.synth_ragged_entries(97, 0, np.array([rows * per], np.uint32), 37).reshape(rows, per, 37).copy()
    block[1, per - len(ent[9]):] = ent[9]
    corpus = T._ragged(lb, gpu, oracle, ent, 37)
    dev = gpu.from_numpy(T._packed(oracle, block.reshape(-1, 37))).cuda()
    for range_ in (0, 21):
        sc, lags = ref.rows(block, ent, new, 8, range_)
        assert range_ or sc[1, 9] == ONE
        _all_forms(gpu, corpus, dev, rows, per, new, 8, sc, lags, range_=range_)


def test_four_calls_on_four_streams(lb, gpu, oracle):
    """each call is made while the one before may still run; the key forms share the corpus' selection scratch"""
    m = T._module(lb, gpu, oracle)
    shapes = (("w48", NEW, 8, "topk"), ("w80", NEW64, 64, "threshold"), ("w48", NEW, 5, "scores"), ("w80", NEW64, 33, "topk"))
    streams = [gpu.cuda.Stream() for _ in shapes]
    held, checks = [], []
    for s, (name, new, max_new, form) in zip(streams, shapes):
        block = m["blocks"][name]
        rows, per = block.shape[:2]
        sc, lags, _ds = _fold(m, name, new, max_new)
        d_new = _dev_counts(gpu, new)
        held.append(d_new)
        s.wait_stream(gpu.cuda.current_stream())
        if form == "scores":
            bufs = (_Buf(gpu, (rows, N_CASE), gpu.int32, POISON32), _Buf(gpu, (rows, N_CASE), gpu.int32, POISON32))
            m["corpus"].recording_scores_tail_batch_device(m["dev"][name], rows, per, d_new, max_new=max_new,
                                                           scores_out=bufs[0].inner.view(gpu.float32), lags_out=bufs[1].inner, stream=s)
            want = (sc.view(np.uint32).view(np.int32).reshape(-1), lags.reshape(-1))
        elif form == "topk":
            bufs = (_Buf(gpu, (rows, 3), gpu.int64, POISON), _Buf(gpu, (rows, 3), gpu.int32, POISON32))
            m["corpus"].query_packed_recording_topk_tail_batch_keys_device(m["dev"][name], rows, per, d_new, 3, max_new=max_new,
                                                                           keys_out=bufs[0].inner, lags_out=bufs[1].inner, stream=s)
            w = _want_topk(sc, lags, 3)
            want = (w[0].view(np.int64).reshape(-1), w[1].reshape(-1))
        else:
            t = _thresholds(sc)["median"]
            bufs = (_Buf(gpu, (rows, CAP), gpu.int64, POISON), _Buf(gpu, (rows, CAP), gpu.int32, POISON32), _Buf(gpu, (rows,), gpu.int64, POISON))
            m["corpus"].query_packed_recording_threshold_tail_batch_keys_device(m["dev"][name], rows, per, d_new, float(t), CAP,
                                                                                max_new=max_new, keys_out=bufs[0].inner,
                                                                                lags_out=bufs[1].inner, counts_out=bufs[2].inner, stream=s)
            w = _want_threshold(sc, lags, t, CAP)
            want = (w[0].view(np.int64).reshape(-1), w[1].reshape(-1), w[2])
        checks.append((bufs, want))
    for s in streams:
        s.synchronize()
    for bufs, want in checks:
        for b, w in zip(bufs, want):
            assert np.array_equal(b.host(), w)


# ---- 6. corner cases -------------------------------------------------------------------------------------------------------------------
def test_the_empty_corpus_and_no_entry_that_takes_part(lb, gpu, oracle):
    m = T._module(lb, gpu, oracle)
    dev = m["dev"]["w48"]
    empty = lb.Corpus.ragged(L, 4, 16)
    sc, lags = _Buf(gpu, (1,), gpu.int32, POISON32), _Buf(gpu, (1,), gpu.int32, POISON32)
    empty.recording_scores_tail_batch_device(dev, R, PER, NEW, max_new=8, scores_out=sc.inner.view(gpu.float32), lags_out=lags.inner)
    gpu.cuda.synchronize()                                          # noErr, and nothing is written
    assert sc.host().tolist() == [POISON32] and lags.host().tolist() == [POISON32]
    keys, klags = _topk(gpu, empty, dev, R, PER, NEW, 8, 3)
    assert not keys.any() and not klags.any()
    got = _threshold(gpu, empty, dev, R, PER, NEW, 8, 0.5, CAP)
    assert not got[0].any() and not got[1].any() and not got[2].any()
    longer = T._ragged(lb, gpu, oracle, [m["entries"][E49], m["entries"][E300]])
    got = _scores(gpu, longer, dev, R, PER, NEW, 8)                 # entries exist, none takes part: +0 scores and 0 lags
    assert got[0].shape == (R, 2) and not got[0].any() and not got[1].any()
    assert not _scores(gpu, longer, dev, R, PER, NEW, 8, want_lags=False)[0].any()
    keys, klags = _topk(gpu, longer, dev, R, PER, NEW, 8, 3)
    assert not keys.any() and not klags.any()
    got = _threshold(gpu, longer, dev, R, PER, NEW, 8, 1e-30, CAP)
    assert not got[0].any() and not got[1].any() and not got[2].any()


def test_the_host_sequence_is_the_device_tensor(lb, gpu, oracle):
    m = T._module(lb, gpu, oracle)
    sc, lags, _ds = _fold(m, "w48", NEW, 20)                        # (max_new: the sequence's maximum, 20)
    got = m["corpus"].recording_scores_tail_batch_device(m["dev"]["w48"], R, PER, NEW)
    keys, klags = m["corpus"].query_packed_recording_topk_tail_batch_keys_device(m["dev"]["w48"], R, PER, NEW, 3, aligned=True)
    tk, tl, tc = m["corpus"].query_packed_recording_threshold_tail_batch_keys_device(m["dev"]["w48"], R, PER, NEW, 1.0, CAP)
    gpu.cuda.synchronize()
    assert got[0].dtype == gpu.float32 and got[1].dtype == gpu.int32 and tuple(got[0].shape) == (R, N_CASE)
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), sc.view(np.uint32)) and np.array_equal(got[1].cpu().numpy(), lags)
    _same((keys.cpu().numpy().view(np.uint64), klags.cpu().numpy()), _want_topk(sc, lags, 3))
    _same((tk.cpu().numpy().view(np.uint64), tl.cpu().numpy(), tc.cpu().numpy()), _want_threshold(sc, lags, 1.0, CAP))
    with pytest.raises(ValueError):
        m["corpus"].recording_scores_tail_batch_device(m["dev"]["w48"], R, PER, gpu.zeros(R, dtype=gpu.int32, device="cuda"))


# ---- 7. the stream bank ----------------------------------------------------------------------------------------------------------------
def test_stream_bank_new_best_and_new_matches_above(lb, gpu, oracle):
    """three channels of test_gpu_stream_bank.py's pruned configuration, two pushes; the corpus holds random entries and, per
    channel, a span of its own sub-fingerprints that ends inside the second push's: StreamBank.new_best and new_matches_above
    against the numpy fold of the second push, and decode_tail_matches against totals()"""
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
    ent = T._random(oracle, 61, np.random.default_rng(4).integers(1, 16, 30), length)
    planted = {}
    for c in range(3):
        planted[c] = len(ent)
        ent.append(fps[c][frames - 10:frames].copy())               # ends at the newest sub-fingerprint
    old0 = frames - int(new[0]) - 10
    ent.append(fps[0][old0:old0 + 10].copy())                       # ends one before channel 0's new ones
    corpus = T._ragged(lb, gpu, oracle, ent, length)
    channels = [2, 0, 1]
    best = bank.new_best(corpus, channels, n, new, k=2)
    above = bank.new_matches_above(corpus, channels, n, new, 0.9, 16)
    win = bank.window_device(channels, n)
    gpu.cuda.synchronize()
    listed = [int(new[c]) for c in channels]
    rows = lb.unpack_packed(win.cpu().numpy(), length).reshape(3, n, length)
    sc, lags = ref.rows(rows, ent, listed, max(listed))
    _same((best[0].cpu().numpy().view(np.uint64), best[1].cpu().numpy()), _want_topk(sc, lags, 2))
    want = _want_threshold(sc, lags, 0.9, 16)
    _same((above[0].cpu().numpy().view(np.uint64), above[1].cpu().numpy(), above[2].cpu().numpy()), want)
    totals = bank.totals()[channels]
    decoded = lb.decode_tail_matches(above[0], above[1], totals, n, counts=above[2])
    top = lb.decode_tail_matches(best[0], best[1], totals, n)
    for j, c in enumerate(channels):
        idx, score, start = decoded[j]
        assert start[(idx == planted[c]) & (score == ONE)].tolist() == [frames - 10]
        assert top[j][0][0] == planted[c] and top[j][1][0] == ONE and top[j][2][0] == frames - 10
        assert len(idx) == len(set(idx.tolist())) == want[2][j]     # an entry once per push
    idx, score, _start = decoded[1]                                 # (channel 0) complete one push ago: not this push's best cell
    assert not ((idx == len(ent) - 1) & (score == ONE)).any()
