"""GPU tests of the SECOND TRIP of every strided loop in the list-building kernels.  The occurrences, recording-scores, timeline,
join and align kernels share one shape: a workgroup takes a work item and, where the launch holds more items than its grid, walks
on with w += gridDim.x -- with state carried in LDS from one trip to the next (the staged query window, s_any, s_cnt, s_w,
JrTile, the quotient table loaded once in front of the loop) behind barriers written for "the unit before has left".  The grid
ceilings (65 536 units, 2^20 join items) cannot be crossed by a test of seconds, so

  a. the ceiling tests lower them through LBAudioDetectiveDebugSetGridCeiling: ceiling 1 makes ONE workgroup walk every unit
     (every unit boundary is a second trip), ceiling 4 leaves 9, 10 and 27 items with uneven trip counts per workgroup.  Every
     case asserts that the strided-launch counter grew: that is how a case proves it was on the path;
  b. the step loops inside a launch (the row scan's 1024 counts per step, the offsets kernel's 1024 rows per step with its
     64-bit carry, the recording fold's 64 tiles per trip, the row scan's 4096-row grid) are crossed by shapes, with the
     ceiling as it comes, 0.

Every comparison is exact -- keys as 64-bit integers, lags, counts, CSR offsets, scores as bits, output buffers poison-filled --
against the numpy references the families' own tests use (align_ref.profile, timeline_ref, the join files' oracle matrices),
through those files' corpora, queries, _expected, _check and _run helpers (imported, not copied; their module caches are
shared).  The thresholds are values of the reference's own cells: nothing needs a tolerance.  The fixture below is the only
place the ceiling is set, and it puts 0 back on every path."""
import contextlib

import numpy as np
import pytest

import align_ref
import timeline_ref
import test_gpu_align as AL
import test_gpu_join as JN
import test_gpu_join_ragged as JR
import test_gpu_occurrences as OC
import test_gpu_recording as RC
import test_gpu_timeline as TL

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[1, 4], ids=["ceiling1", "ceiling4"])
def ceiling(request, lb):
    """the grid ceiling of the test, 0 again whatever the test did"""
    lb.debug_set_grid_ceiling(request.param)
    try:
        yield request.param
    finally:
        lb.debug_set_grid_ceiling(0)


@pytest.fixture
def ceiling1(lb):
    lb.debug_set_grid_ceiling(1)
    try:
        yield 1
    finally:
        lb.debug_set_grid_ceiling(0)


@contextlib.contextmanager
def _strides(lb):
    """the calls inside launched at least one grid below its work"""
    before = lb.debug_grid_ceiling()[1]
    yield
    after = lb.debug_grid_ceiling()[1]
    assert after > before, "no launch in here had a grid below its work: the case was not on the strided path"


# ---- a. occurrences ---------------------------------------------------------------------------------------------------------------
# q300: case B, one tile group, 9 units.  q700: 6 tiles in 2 groups, the second with two waves of tile >= tiles (the `continue`
# in front of further trips).  q2500 on the 70-entry prefix: 5 groups x 2 blocks.  q17: case A against the long entries.
@pytest.mark.parametrize("name", ["q300", "q700", "q2500", "q17"])
def test_occurrences_under_a_ceiling(lb, gpu, oracle, ceiling, name):
    m = OC._module(lb, gpu, oracle)
    prof = OC._profiles(m, name)
    corpus = m["corpus"][m["queries"][name][1]]
    ts = OC._thresholds(prof)
    for peaks in (False, True):
        for what in ("median", "max"):
            want_keys, want_lags = OC._expected(prof, ts[what], peaks)
            assert peaks or len(want_keys) >= 1
            capacity = len(want_keys) + 5
            with _strides(lb):
                got = OC._run(gpu, corpus, OC._fp(lb, m, name), ts[what], peaks, capacity)
            OC._check(got, want_keys, want_lags, capacity)


def test_occurrences_masked_instances_under_a_ceiling(lb, gpu, oracle, ceiling):
    """range 64: the FULL = false instances of both kernels"""
    m = OC._module(lb, gpu, oracle)
    prof = OC._profiles(m, "q300", 64)
    ts = OC._thresholds(prof)
    for peaks in (False, True):
        for what in ("median", "max"):
            want_keys, want_lags = OC._expected(prof, ts[what], peaks)
            capacity = len(want_keys) + 3
            with _strides(lb):
                got = OC._run(gpu, m["corpus"][OC.N_CASE], OC._fp(lb, m, "q300"), ts[what], peaks, capacity, range_=64)
            OC._check(got, want_keys, want_lags, capacity)


def test_occurrences_capacity_cut_in_an_early_block_under_a_ceiling(lb, gpu, oracle, ceiling):
    """the list is full inside entry block 0: the scatter takes row_base[n.e0] >= capacity -> continue in front of every later
    unit, which it must still skip correctly; the count is never cut"""
    m = OC._module(lb, gpu, oracle)
    prof = OC._profiles(m, "q300")
    t = OC._thresholds(prof)["median"]
    for peaks in (False, True):
        want_keys, want_lags = OC._expected(prof, t, peaks)
        entry = 0xFFFFFFFF - (want_keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        in_block0 = int(np.count_nonzero(entry < OC.BLOCK))
        assert 8 <= in_block0 < len(want_keys) and entry.max() >= 2 * OC.BLOCK
        for capacity in (in_block0 - 3, in_block0, 1):
            with _strides(lb):
                got = OC._run(gpu, m["corpus"][OC.N_CASE], OC._fp(lb, m, "q300"), t, peaks, capacity)
            OC._check(got, want_keys, want_lags, capacity)


def test_occurrences_in_chunks_under_ceiling_1(lb, gpu, oracle, ceiling1):
    """the scratch limit at two entry blocks: five chunks, every one walked by one workgroup"""
    m = OC._module(lb, gpu, oracle)
    corpus, fp = m["corpus"][OC.N_CASE], OC._fp(lb, m, "q300")
    prof = OC._profiles(m, "q300")
    tiles = -(-max(len(p) for p, _ in prof) // OC.TILE)
    t = OC._thresholds(prof)["median"]
    assert -(-OC.N_CASE // (2 * OC.BLOCK)) >= 2
    try:
        corpus.set_join_scratch_limit(OC._scratch_bytes(2 * OC.BLOCK, tiles))
        for peaks in (False, True):
            want_keys, want_lags = OC._expected(prof, t, peaks)
            for capacity in (len(want_keys) + 2, len(want_keys) // 2):
                with _strides(lb):
                    got = OC._run(gpu, corpus, fp, t, peaks, capacity)
                OC._check(got, want_keys, want_lags, capacity)
    finally:
        corpus.set_join_scratch_limit(0)


# ---- a. recording scores and lags ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q17", "q300", "q700", "q2500"])
def test_recording_scores_under_a_ceiling(lb, gpu, oracle, ceiling, name):
    m = RC._module(lb, gpu, oracle)
    corpus = m["corpus"][m["queries"][name][1]]
    want = RC._aligned(m, name)
    with _strides(lb):
        got = RC._scores(gpu, corpus, RC._fp(lb, m, name))
    RC._same(got, want)


def test_recording_scores_masked_instance_under_a_ceiling(lb, gpu, oracle, ceiling):
    m = RC._module(lb, gpu, oracle)
    for name in ("q300", "q22"):                                  # case B and case A
        want = RC._aligned(m, name, 64)
        with _strides(lb):
            got = RC._scores(gpu, m["corpus"][RC.N_CASE], RC._fp(lb, m, name), range_=64)
        RC._same(got, want)


def test_recording_scores_in_chunks_under_ceiling_1(lb, gpu, oracle, ceiling1):
    """three chunks of three entry blocks (192, 192, 133 entries), each walked by one workgroup"""
    m = RC._module(lb, gpu, oracle)
    corpus, fp = m["corpus"][RC.N_CASE], RC._fp(lb, m, "q300")
    want = RC._aligned(m, "q300")
    try:
        corpus.set_join_scratch_limit(RC._scratch_bytes(3 * RC.BLOCK, 3))
        with _strides(lb):
            got = RC._scores(gpu, corpus, fp)
        RC._same(got, want)
    finally:
        corpus.set_join_scratch_limit(0)


# ---- a. timeline (a unit is 128 entries: 517 entries make 5 blocks) ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["q17", "q300", "q700"])
def test_timeline_under_a_ceiling(lb, gpu, oracle, ceiling, name):
    m = TL._module(lb, gpu, oracle)
    q, n = m["queries"][name]
    assert -(-n // TL.WALK) == 5
    for t in (TL.T_HIGH, TL.T_LOW):
        want = TL._want(m, name, t)
        with _strides(lb):
            got = TL._timeline(gpu, m["corpus"][n], len(q), t, fp=TL._fp(lb, m, name))
        TL._same(got, want)


def test_timeline_masked_instance_under_a_ceiling(lb, gpu, oracle, ceiling):
    m = TL._module(lb, gpu, oracle)
    for t in (TL.T_HIGH, TL.T_LOW):
        want = TL._want(m, "q300", t, 64)
        with _strides(lb):
            got = TL._timeline(gpu, m["corpus"][TL.N_CASE], 300, t, fp=TL._fp(lb, m, "q300"), range_=64)
        TL._same(got, want)


def test_timeline_in_chunks_under_ceiling_1(lb, gpu, oracle, ceiling1):
    """chunks of two entry blocks (256, 256 and 5 entries), each walked by one workgroup"""
    m = TL._module(lb, gpu, oracle)
    corpus, fp = m["corpus"][TL.N_CASE], TL._fp(lb, m, "q300")
    try:
        corpus.set_join_scratch_limit(2 * TL._scratch_bytes(TL.WALK, 3) + 7)
        for t in (TL.T_HIGH, TL.T_LOW):
            want = TL._want(m, "q300", t)
            with _strides(lb):
                got = TL._timeline(gpu, corpus, 300, t, fp=fp)
            TL._same(got, want)
    finally:
        corpus.set_join_scratch_limit(0)


# ---- a. the uniform join ------------------------------------------------------------------------------------------------------------
N_JOIN = 2 * JN.TE + 5                                        # 9 row tiles x 3 entry tiles = 27 items; 517 rows for the row scan


@pytest.mark.parametrize("n_sub", range(1, 9))
def test_uniform_join_every_instance_under_a_ceiling(lb, gpu, oracle, ceiling, n_sub):
    """test_gpu_join.py's test_every_sub_fingerprint_count_and_range at 517 entries: a self-join, the diagonal skipped"""
    for range_ in (0, 64, 1):
        c, _, S = JN._case(lb, gpu, oracle, N_JOIN, n_sub, range_)
        ts = JN._thresholds(S)
        if range_ == 64:
            ts.append(np.float32(0.7))
        for t in ts:
            total = len(JN._expected(S, t, 0, N_JOIN, True)[0])
            for capacity in sorted({max(1, total // 2), total + 7}):
                with _strides(lb):
                    JN._join_check(lb, gpu, c, S, t, capacity, (n_sub, range_, float(t), capacity), range_=range_)


def test_uniform_join_cut_inside_a_row_and_cross_join_under_a_ceiling(lb, gpu, oracle, ceiling):
    c, bools, S = JN._case(lb, gpu, oracle, N_JOIN)
    t = JN._median(S)
    _, offsets = JN._expected(S, t, 0, N_JOIN, True)
    row = next(r for r in range(2 * JN.TR, N_JOIN) if offsets[r + 1] - offsets[r] > 10)
    inside = int(offsets[row]) + 3                                # a capacity that ends inside a row of the third row tile
    assert offsets[row] < inside < offsets[row + 1]
    with _strides(lb):
        JN._join_check(lb, gpu, c, S, t, inside, ("cut inside row", row))
    # a cross join: 130 rows (3 row tiles) against the 517 entries, copies of row 3 at entries 3 and 500
    rows = 130
    qb = oracle.synth_corpus(78, 0, rows, 5, JN.L).copy()
    qb[7] = bools[40]
    qb[129] = 0
    cb = bools.copy()
    cb[3] = qb[3]
    cb[500] = qb[3]
    corpus, queries = JN._uniform(lb, gpu, oracle, cb), JN._uniform(lb, gpu, oracle, qb)
    try:
        Sx = JN._score_matrix(oracle, qb, cb, 0)
        assert Sx[3, 3] == 1.0 and Sx[3, 500] == 1.0 and Sx[7, 40] == 1.0
        for t in JN._thresholds(Sx) + [np.float32(1.0)]:
            for skip in (False, True):
                with _strides(lb):
                    total = JN._join_check(lb, gpu, corpus, Sx, t, 4000, ("cross", float(t), skip), queries=queries, skip=skip)
                with _strides(lb):
                    JN._join_check(lb, gpu, corpus, Sx, t, max(1, total - 1), ("cross, cut", float(t), skip), queries=queries, skip=skip,
                                   index_base=1 << 20)
    finally:
        for x in (corpus, queries):
            x.dispose()


# ---- a. the ragged join ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("range_", [0, 64])
def test_ragged_join_under_a_ceiling(lb, gpu, oracle, ceiling, range_):
    """the N_CASE corpus, both FULL instances, lags on and NULL, one capacity cut"""
    c, ent, S = JR._case(lb, gpu, oracle, JR.N_CASE, range_)
    for t in (JR._selective(S), JR._median(S)):
        total = len(JR._expected(S, t, 0, JR.N_CASE, True)[0])
        assert total >= 4
        for capacity, want_lags in ((total + 7, True), (total + 7, False), (max(1, total // 2), True)):
            with _strides(lb):
                JR._join_check(lb, gpu, c, ent, S, t, capacity, (range_, float(t), capacity, want_lags), range_=range_, want_lags=want_lags)


# ---- a. align --------------------------------------------------------------------------------------------------------------------------
def _align_case(lb, gpu, c, exp, qs, K, n, base, what):
    fps = [lb.Fingerprint.from_bools(q) for q in qs]
    want = [exp.of((what, i), q, 0) for i, q in enumerate(qs)]
    keys = np.zeros((len(qs), K), np.int64)
    for i in range(len(qs)):
        keys[i, :n] = AL._keys_of(want[i][0], base)
    with _strides(lb):
        lags, scores = c.align_keys_device(fps, gpu.from_numpy(keys).cuda(), K, index_base=base, want_scores=True)
    lags, scores = lags.cpu().numpy(), scores.cpu().numpy()
    for i in range(len(qs)):
        assert np.array_equal(lags[i, :n], want[i][1]), (what, i, np.flatnonzero(lags[i, :n] != want[i][1])[:8])
        assert np.array_equal(AL._bits(scores[i, :n]), AL._bits(want[i][0])), (what, i)
        assert not lags[i, n:].any() and not scores[i, n:].any()


def test_align_keys_under_a_ceiling(lb, gpu, oracle, ceiling):
    """align_keys_device, ragged and uniform: a long query and few keys (parts > 1: the keys kernel's items are pairs x parts and
    the finish kernel runs -- with more than 256 pairs it strides under ceiling 1) and short queries (parts == 1)"""
    rng = np.random.default_rng(200)
    L = 200
    # ragged, entries of 1 .. 300
    entries = AL._ragged_entries(rng, L, 0)
    c = AL._ragged(lb, gpu, oracle, entries)
    exp = AL.Expected(oracle, entries, L)
    n = len(entries)
    qs = [(rng.random((nq, L)) < 0.5).astype(np.uint8) for nq in (600, 5, 21, 48, 100, 2, 1)]
    qs[2][:] = entries[28 + 4][10:31]                             # (the entry of 48: a planted match, lag +10)
    assert (n + 3) * len(qs) > 256 and 16384 // ((n + 3) * len(qs)) > 1
    _align_case(lb, gpu, c, exp, qs, n + 3, n, 1000, "ragged, parts > 1")
    assert exp.of(("ragged, parts > 1", 2), qs[2], 0)[1][28 + 4] == 10
    # ragged, entries of 1 .. 40 and queries of at most 48: no pair has more than one tile of offsets
    short = [e for e in entries if len(e) <= 48 and e.any()]
    short += [(rng.random((int(k), L)) < 0.5).astype(np.uint8) for k in rng.integers(1, 41, 30)]
    c2 = AL._ragged(lb, gpu, oracle, short)
    assert max(len(e) for e in short) <= 48
    _align_case(lb, gpu, c2, AL.Expected(oracle, short, L), qs[1:4], len(short), len(short), 0, "ragged, parts == 1")
    # uniform, 5 sub-fingerprints per entry
    host = (rng.random((100, 5, L)) < 0.5).astype(np.uint8)
    host[17] = 0
    cu = AL._uniform(lb, gpu, oracle, host)
    expu = AL.Expected(oracle, list(host), L)
    qu = [(rng.random((nq, L)) < 0.5).astype(np.uint8) for nq in (5, 4, 8, 1)]
    qu[0][:] = host[60]
    _align_case(lb, gpu, cu, expu, qu, 100, 100, 5, "uniform, parts == 1")
    qlong = [(rng.random((300, L)) < 0.5).astype(np.uint8), qu[0]]
    qlong[0][100:105] = host[61]
    _align_case(lb, gpu, cu, expu, qlong, 100, 100, 5, "uniform, parts > 1")
    assert expu.of(("uniform, parts > 1", 0), qlong[0], 0)[1][61] == -100


def test_match_profile_under_a_ceiling(lb, gpu, oracle, ceiling):
    """one pair with more tiles of 64 offsets than the ceiling: a ragged and a uniform corpus, both cases"""
    rng = np.random.default_rng(201)
    L = 200
    entries = [(rng.random((int(k), L)) < 0.5).astype(np.uint8) for k in (3, 700, 30)]
    c = AL._ragged(lb, gpu, oracle, entries)
    host = (rng.random((10, 4, L)) < 0.5).astype(np.uint8)
    cu = AL._uniform(lb, gpu, oracle, host)
    for nq in (30, 1000):                                         # 671 offsets of case A, 301 and 971 of case B
        q = (rng.random((nq, L)) < 0.5).astype(np.uint8)
        fq = lb.Fingerprint.from_bools(q)
        for corpus, e, ent in ((c, 1, entries[1]), (c, 2, entries[2]), (cu, 7, host[7])):
            want, _ = align_ref.profile(q, ent, 0)
            if len(want) <= 64 * 4:
                continue
            with _strides(lb):
                got, first = corpus.match_profile(fq, e)
            assert first == 0 and np.array_equal(AL._bits(got), AL._bits(want)), (nq, e)


# ---- b. step loops, the ceiling as it comes ---------------------------------------------------------------------------------------
N_REC = 129_700                                               # ceil(129 700 / 126) = 1030 tiles
EARLY, LATE = 500, 1026 * 126 + 3                             # below and above offset 1024 x 126


def test_a_long_recording_crosses_the_step_loops(lb, gpu, oracle):
    """A recording of 129 700 sub-fingerprints against 12 entries of 1 .. 40: 1030 tiles per entry, so the row scan takes a
    second step of 6 counts per row, the recording fold 17 trips of tile += 64, the timeline folds 1030 x 126 offsets.  Two
    entries lie verbatim in the recording, once below offset 1024 x 126 and once above: the late match's slot depends on the
    carry out of the first scan step."""
    assert lb.debug_grid_ceiling()[0] == 0
    lengths = [1, 40, 7, 22, 13, 2, 31, 5, 17, 40, 9, 26]
    ent = OC._random(oracle, 6161, lengths)
    q = OC._random(oracle, 6262, [N_REC])[0]
    a, b = 3, 8                                                   # the 22 and the 17
    q[EARLY:EARLY + 22] = ent[a]
    q[LATE:LATE + 22] = ent[a]
    q[EARLY + 100:EARLY + 117] = ent[b]
    q[LATE + 100:LATE + 117] = ent[b]
    tiles = -(-N_REC // OC.TILE)
    assert tiles == 1030 and tiles > 1024 and tiles > 16 * 64 and EARLY // OC.TILE < 1024 < LATE // OC.TILE
    prof = [align_ref.profile(q, e, 0) for e in ent]              # the reference, once: every cell of every pair
    assert all(not entry_long and len(p) == N_REC - len(e) + 1 for (p, entry_long), e in zip(prof, ent))
    for j, plant in ((a, 0), (b, 100)):
        assert prof[j][0][EARLY + plant] == 1.0 and prof[j][0][LATE + plant] == 1.0
    corpus = OC._ragged(lb, gpu, oracle, ent)
    fp = lb.Fingerprint.from_bools(q)
    # the occurrences list
    cells = np.sort(np.concatenate([p for p, _ in prof]))
    for what, t in (("max", cells[-1]), ("the 3000th", cells[-3000]), ("median", cells[len(cells) // 2])):
        for peaks in (False, True):
            want_keys, want_lags = OC._expected(prof, t, peaks)
            print(what, float(t), "peaks" if peaks else "all", len(want_keys))
            assert len(want_keys) >= 4
            capacity = len(want_keys) + 5
            OC._check(OC._run(gpu, corpus, fp, t, peaks, capacity), want_keys, want_lags, capacity)
    # scores and lags: align_ref.align's rule on the cells above
    best = np.array([max(np.float32(0.0), p.max()) for p, _ in prof], np.float32)
    lags = np.array([-int(np.flatnonzero(p == s)[0]) if p.max() == s else 0 for (p, _), s in zip(prof, best)], np.int32)
    assert best[a] == 1.0 and lags[a] == -EARLY and best[b] == 1.0 and lags[b] == -(EARLY + 100)
    RC._same(RC._scores(gpu, corpus, fp), (best, lags))
    # the timeline
    profs = [(len(e), p) for e, (p, _) in zip(ent, prof)]
    for t in (TL.T_HIGH, TL.T_LOW):
        want = timeline_ref.fold(N_REC, profs, t)
        idx, sc = timeline_ref.decode(want[0])
        assert idx[EARLY] == a and idx[LATE] == a and idx[LATE + 100] == b and sc[LATE] == 1.0
        TL._same(TL._timeline(gpu, corpus, N_REC, t, fp=fp), want)


def test_many_short_entries_cross_the_row_grid_and_the_offsets_steps(lb, gpu, oracle):
    """test_gpu_timeline.py's test_many_entry_blocks corpus, 4229 entries of 1 .. 6, against a query of 300: the row scan strides
    past its 4096 workgroups (the strided-launch counter says so without a ceiling), join_offsets_kernel takes five steps of
    1024 rows with its carry.  The occurrences list itself is compared with numpy, a match planted in each of the row ranges
    0 .. 1023, 1024 .. 2047 and 4096 .. 4228."""
    assert lb.debug_grid_ceiling()[0] == 0
    n = TL.FOLD_ROWS * TL.WALK + TL.WALK + 5
    assert n == 4229
    counts = np.random.default_rng(3).integers(1, 7, n)
    ent = OC._random(oracle, 515, counts)
    q = OC._random(oracle, 516, [300])[0]
    planted = {0: OC.TILE, 1500: 200, n - 2: 40}                  # entry -> offset
    for j, o in planted.items():
        q[o:o + len(ent[j])] = ent[j]
    prof = [align_ref.profile(q, e, 0) for e in ent]
    for j, o in planted.items():
        assert prof[j][0][o] == 1.0
    cells = np.sort(np.concatenate([p for p, _ in prof]))
    corpus = OC._ragged(lb, gpu, oracle, ent)
    fp = lb.Fingerprint.from_bools(q)
    for what, t in (("a few hundred", cells[-300]), ("max", cells[-1])):
        for peaks in (False, True):
            want_keys, want_lags = OC._expected(prof, t, peaks)
            print(what, float(t), "peaks" if peaks else "all", len(want_keys))
            entry = 0xFFFFFFFF - (want_keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
            assert set(planted) <= set(entry.tolist()) and len(want_keys) < 100_000
            capacity = len(want_keys) + 5
            with _strides(lb):
                got = OC._run(gpu, corpus, fp, t, peaks, capacity)
            OC._check(got, want_keys, want_lags, capacity)


# ---- the ceiling is left at 0 ------------------------------------------------------------------------------------------------------
def test_the_ceiling_is_back_at_zero(lb, gpu):
    assert lb.debug_grid_ceiling()[0] == 0
