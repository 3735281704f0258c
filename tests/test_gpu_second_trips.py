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
place the ceiling is set, and it puts 0 back on every path.

The plain grid-stride kernels -- nothing carried, x += gridDim.x * threads -- of the duplicate groups (init, hook, flatten), the
gather's two copy launches and the top-K selection's histogram and gather passes take their grids from the same ceiling and
run under a. as well: the groups' own test bodies, the gather's _check and the top-K file's numpy sort, under a ceiling.  Their
single-workgroup scans (groups_extra_tiles_kernel, gather_tiles_kernel, remove_offsets_kernel: 256 tiles per step, a carry from
step to step) are b.: crossed by 256 * 1024 + 1024 + 7 entries, keys or vertices -- 258 tiles, the second step holding two,
the last one partial."""
import contextlib
import os
import re

import numpy as np
import pytest

import align_ref
import timeline_ref
import test_gpu_align as AL
import test_gpu_gather as GA
import test_gpu_groups as GR
import test_gpu_join as JN
import test_gpu_join_ragged as JR
import test_gpu_occurrences as OC
import test_gpu_recording as RC
import test_gpu_remove as RM
import test_gpu_timeline as TL
import test_gpu_topk as TK

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


# ---- a. duplicate groups: init, hook and flatten stride by 256 vertices or key slots per workgroup -------------------------------
# The bodies are test_gpu_groups.py's own: every graph in them has more than 4 x 256 vertices, so init and flatten stride under
# both ceilings (4 097 vertices under ceiling 1: 17 trips, the last with one live lane -- flatten's ballot needs every lane of a
# wave to make all of them), and every list of edges has more slots than that where the hook pass is the point: the chain's
# 2 999, the path's 4 096, K(3, 2000)'s 12 000 in both directions, the random graph's 2 000 and more.
_GROUP_BODIES = {
    "chain of 3000": lambda lb, gpu: GR.test_chain(lb, gpu),
    "path over a permutation of 4097": lambda lb, gpu: GR.test_path_over_a_permutation(lb, gpu),
    "stars and K(3, 2000)": lambda lb, gpu: GR.test_stars(lb, gpu),
    "random graph at base 5000": lambda lb, gpu: GR.test_random_graph(lb, gpu),
    "pitched rows and row keys": lambda lb, gpu: GR.test_pitched_rows_and_row_keys(lb, gpu),
    "incremental, rows ascending": lambda lb, gpu: GR.test_incremental_calls_equal_one_call(lb, gpu, "rows ascending"),
    "incremental, rows descending": lambda lb, gpu: GR.test_incremental_calls_equal_one_call(lb, gpu, "rows descending"),
    "list cut by n_slots": lambda lb, gpu: GR.test_cut_list_is_used_as_far_as_it_goes(lb, gpu),
}


@pytest.mark.parametrize("body", list(_GROUP_BODIES))
def test_groups_under_a_ceiling(lb, gpu, ceiling, body):
    """labels against _union_find, the group count against the number of roots, both poison-filled: see the bodies"""
    with _strides(lb):
        _GROUP_BODIES[body](lb, gpu)


def test_groups_second_trip_with_one_live_lane(lb, gpu, ceiling1):
    """257 vertices under ceiling 1: two trips, the second with one live lane in wave 0 and none in the other three"""
    n = 257
    with _strides(lb):
        want = GR._check(lb, gpu, GR.Rows(n, [[] for _ in range(n)]), "257, no edges")
    assert np.array_equal(want, np.arange(n))
    with _strides(lb):
        want = GR._check(lb, gpu, GR.Rows(n, GR._rows_of(n, [(256, 0), (255, 256)])), "257, the last vertex hooked")
    assert want[256] == 0 and want[255] == 0 and (want == np.arange(n)).sum() == n - 2


# ---- a. gather: the two copy launches stride by 256 output sub-fingerprints per workgroup ------------------------------------------
def _gather_lists(n, rng):
    """name -> GLOBAL indices at base 0 (-1: a zero key; n and above: a key of another index range); 900 keys each"""
    mixed = rng.integers(0, n, 900)
    mixed[::7] = mixed[3]                                         # duplicates (copies of one entry all through the list)
    mixed[5::11] = -1
    mixed[2::13] = n + np.arange(len(mixed[2::13])) % 2
    mixed[[100, 600]] = 0xFFFFFFFF                                # (a zero low word under a score word)
    return {"900 of a shuffle": rng.permutation(n)[:900].astype(np.int64), "duplicates, zero and foreign keys": mixed.astype(np.int64)}


def _gather_cases(lb, gpu, c, rows, what, seed, min_len):
    rng = np.random.default_rng(seed)
    n = len(rows)
    for base in (0, GA.BASE):
        for name, rel in _gather_lists(n, rng).items():
            g = np.where(rel >= 0, np.minimum(rel + base, 0xFFFFFFFF), -1)
            exp_off, _ = GA._expected(rows, g, base)
            assert int(exp_off[-1]) > 4 * 256                     # more output than one trip of four workgroups
            with _strides(lb):
                GA._check(gpu, c, rows, g, base, rng, (what, base, name))
            # a capacity that cuts the output inside a row, behind the first trip of every workgroup
            k = next(i for i in range(2 * len(g) // 3, len(g)) if exp_off[i + 1] - exp_off[i] >= min_len)
            cap = int(exp_off[k]) + 1
            assert cap > 4 * 256 and exp_off[k] < cap < exp_off[k + 1]
            with _strides(lb):
                GA._check(gpu, c, rows, g, base, rng, (what, base, name, "cut inside row", k), capacity=cap)


@pytest.mark.parametrize("shape", [(200, 5), (33, 3)])
def test_gather_uniform_under_a_ceiling(lb, gpu, oracle, ceiling, shape):
    """gather_copy_planes_kernel: offsets, bytes and the poison behind min(total, capacity) against the rows appended"""
    length, n_sub = shape
    n = 2 * GA.T + 3
    bools = GA._uniform_bools(length, n_sub, n)
    c = GA._uniform(lb, gpu, oracle, bools, n + 5)
    try:
        _gather_cases(lb, gpu, c, list(GA._packed(oracle, bools)), shape, length + n_sub, n_sub)
    finally:
        c.dispose()


@pytest.mark.parametrize("length", [200, 199])
def test_gather_ragged_under_a_ceiling(lb, gpu, oracle, ceiling, length):
    """gather_copy_records_kernel: the binary search of every trip's position in the offsets"""
    flat, counts = GA._ragged_made(length)
    c = GA._ragged(lb, gpu, oracle, flat, counts, len(counts) + 3, int(counts.sum()) + 11)
    try:
        _gather_cases(lb, gpu, c, GA._ragged_rows(oracle, flat, counts), ("ragged", length), length, 3)
    finally:
        c.dispose()


# ---- a. top-K selection: the histogram and gather passes stride by 1024 scores per workgroup ---------------------------------------
N_SCORES = 5000                                               # 5 trips of 1024 under ceiling 1, the last one partial
TOPK_POISON = -0x0123456789ABCDEF


def _select_poisoned(lb, gpu, scores, k, index_base=0):
    """test_gpu_topk.py's _select with the key block (and three words behind it) poison-filled before the call"""
    s = gpu.from_numpy(np.ascontiguousarray(scores, np.float32)).cuda()
    rows, n = (1, s.numel()) if s.dim() == 1 else (s.shape[0], s.shape[1])
    out = gpu.full((rows * k + 3,), TOPK_POISON, dtype=gpu.int64, device="cuda")
    st = lb.lib().LBAudioDetectiveTopKKeysFromScoresDevice(s.data_ptr(), n, rows, k, index_base, out.data_ptr(),
                                                           gpu.cuda.current_stream().cuda_stream)
    assert st == 0, st
    gpu.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[rows * k:] == TOPK_POISON).all(), "words behind the keys were written"
    return got[:rows * k].reshape(rows, k)


def _score_patterns():
    """name -> a row of N_SCORES scores; the patterns of test_selection_on_crafted_score_arrays, what decides them placed at
    indices of the later trips"""
    rng = np.random.default_rng(99)
    n = N_SCORES
    cases = {"all equal": np.full(n, 0.5, np.float32)}
    one = np.full(n, 0.5, np.float32)
    one[4321] = 0.5000001
    cases["all equal but one"] = one
    tie = (0.45 + 0.01 * rng.random(n)).astype(np.float32)
    at = rng.permutation(n)
    tie[at[:1100]] = np.float32(0.7)                              # the 1024th lies among 1100 equal scores
    tie[at[1100:1111]] = np.float32(0.9)                          # the 10th among 11
    tie[at[1111:1114]] = np.float32(0.95)                         # the 1st among 3
    cases["ties at the k-th score"] = tie
    ulp = np.full(n, 0.5, np.float32)
    some = rng.choice(n, 1500, replace=False)
    ulp[some] = np.nextafter(np.float32(0.5), np.float32(1), dtype=np.float32) + np.arange(1500) % 7 * np.float32(2 ** -24)
    cases["one ulp apart"] = ulp
    odd = np.zeros(n, np.float32)
    odd[::3] = np.float32(1e-42)                                  # denormals
    odd[1::7] = np.nan
    odd[2::11] = -0.5
    odd[1025] = -0.0
    odd[2050] = np.float32(1.4e-45)
    odd[4999] = np.inf
    odd[3100] = 3.0
    odd[4100] = -np.inf
    cases["NaN, inf, -0.0, denormals"] = odd
    cases["normal"] = np.clip(rng.normal(0.5, 0.03, n), 0, 1).astype(np.float32)
    return cases


def test_topk_selection_under_a_ceiling(lb, gpu, ceiling):
    """rows of 5000 scores against the numpy sort by (score descending, index ascending) of test_gpu_topk.py, keys compared as
    64-bit integers: every pattern alone, then two rows in one call (grid.y) with an index base"""
    cases = _score_patterns()
    assert -(-N_SCORES // 1024) > 4
    for name, s in cases.items():
        for k in (1, 10, 1024):
            with _strides(lb):
                got = _select_poisoned(lb, gpu, s, k)
            assert np.array_equal(got[0], TK._host_keys(s, k)), (name, k)
    names = list(cases)
    for a, b in zip(names, names[1:] + names[:1]):
        rows = np.stack([cases[a], cases[b]])
        for k in (1, 10, 1024):
            with _strides(lb):
                got = _select_poisoned(lb, gpu, rows, k, index_base=1000)
            for r in range(2):
                assert np.array_equal(got[r], TK._host_keys(rows[r], k, 1000)), (a, b, r, k)


# ---- b. step loops, the ceiling as it comes ---------------------------------------------------------------------------------------
N_REC = 129_700                                              # ceil(129 700 / 126) = 1030 tiles
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


# ---- b. the single-workgroup scans of remove, gather and the groups' extra keys: 256 tiles per step -----------------------------
def _constant(file, name):
    src = open(os.path.join(RM.ROOT, "lbaudiodetective_amd", "csrc", file)).read()
    return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))


T = RM.T
STEP = _constant("k_remove.hip", "kRmThreads")                # tiles per step of each of the three scans
N_BIG = STEP * T + T + 7                                      # 258 tiles: step 2 holds two, the last one partial
SEED_BIG = 0x32545250
_BIG = {}


def test_the_three_scans_share_their_tile_and_step():
    assert T == GA.T == _constant("k_groups.hip", "kGrTile") == 1024
    assert STEP == _constant("k_gather.hip", "kGaThreads") == _constant("k_groups.hip", "kGrThreads") == 256
    assert N_BIG == 263_175 and -(-N_BIG // T) == STEP + 2 and N_BIG % T == 7


def _big(oracle):
    """N_BIG + 15 entries of one sub-fingerprint of 200 Booleans and their packed bytes, made once and read-only: the uniform
    corpus is the first N_BIG of them, the ragged ones cut their records out of the same rows"""
    if not _BIG:
        bools = oracle.synth_corpus(SEED_BIG, 0, N_BIG + 15, 1, 200)
        packed = RM._packed(oracle, bools)
        for a in (bools, packed):
            a.setflags(write=False)
        _BIG.update(bools=bools, packed=packed)
    return _BIG


def _big_uniform(lb, gpu, oracle):
    c = lb.Corpus(200, 1, N_BIG)
    c.append_packed_device(gpu.from_numpy(_big(oracle)["packed"][:N_BIG].copy()).cuda())
    return c


def _in_order_keys(n):
    return np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64)


def _contents(gpu, c, want_bytes, want_counts, what):
    """every entry of c, gathered in order into poisoned buffers, against the expected bytes [records, 32] and entry lengths"""
    records = len(want_bytes)
    off, packed = GA._gather_dev(gpu, c, _in_order_keys(len(c)), 0, records)
    want_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(want_counts, dtype=np.uint64)])
    assert np.array_equal(off, want_off), (what, "entry offsets", np.flatnonzero(off != want_off)[:4])
    bad = np.flatnonzero((packed[:records] != want_bytes).any(axis=1))
    assert len(bad) == 0, (what, "bytes of records", len(bad), bad[:4])
    assert (packed[records:] == GA.POISON8).all(), what


def _big_removal_sets(n):
    """name -> sorted indices out of n entries (n in tile 257)"""
    rng = np.random.default_rng(77)
    late = np.arange(STEP * T, n)
    return {"i": np.sort(rng.choice(late, len(late) // 2, replace=False)),                  # only in tiles >= 256
            "ii": np.union1d([3 * T + 17], rng.choice(n, n // 100, replace=False)),          # one in tile 3 and a random 1 %
            "iii": np.arange(0, n, 2)}                                                       # every other


@pytest.mark.parametrize("which", ["i", "ii", "iii"])
def test_uniform_removal_crosses_the_offsets_step(lb, gpu, oracle, which):
    """remove_offsets_kernel's second step over 258 tiles: the kept count carried into tiles 256 and 257, and the lowest removed
    index -- (i) found only by step 2 while step 1 carries "none", (ii) found by step 1 and not to be overwritten, (iii) the
    largest carry.  The count, the whole old -> new map (poison-filled), every byte of the corpus afterwards (a gather of all
    kept entries: more than 256 tiles of keys in (i) and (ii), so gather_tiles_kernel's second step as well), and two queries
    against oracle.corpus_best on the kept Booleans."""
    assert lb.debug_grid_ceiling()[0] == 0
    big = _big(oracle)
    bools, packed = big["bools"][:N_BIG], big["packed"][:N_BIG]
    indices = _big_removal_sets(N_BIG)[which]
    keep, new, removed = RM._expected(N_BIG, indices)
    assert removed == len(indices) and 3 * T + 17 in _big_removal_sets(N_BIG)["ii"]
    assert (indices.min() >= STEP * T) == (which == "i") and indices.max() >= STEP * T
    c = _big_uniform(lb, gpu, oracle)
    try:
        st, got_removed, got_map = RM._remove_host(lb, c, indices)
        assert st == 0
        assert got_removed == removed and len(c) == N_BIG - removed, (got_removed, removed, len(c))
        assert np.array_equal(got_map, new), np.flatnonzero(got_map != new)[:8]
        _contents(gpu, c, packed[keep].reshape(-1, 32), np.ones(N_BIG - removed, np.uint64), which)
        kept = np.ascontiguousarray(bools[keep])
        last_tile = np.arange((STEP + 1) * T, N_BIG)
        for name, e in (("kept, last tile", last_tile[keep[last_tile]][-1]), ("removed", indices[-1])):
            want = oracle.corpus_best(bools[e], kept, 200, nthreads=16)
            got = c.query(lb.Fingerprint.from_bools(bools[e]))
            assert got[0] == want[0] and RM._bits(got[1]) == RM._bits(want[1]), (which, name, got, want)
            assert (name == "removed") or (want == (int(new[e]), 1.0))
    finally:
        c.dispose()


def test_ragged_removal_crosses_the_offsets_step(lb, gpu, oracle):
    """N_BIG + 3 entries of one record each but three of five, in tiles 0, 255 and 257; every other entry from tile 256 on goes,
    the long one of tile 257 stays: its records' new place is the sum of step 1's carry, what tile 256 keeps and what goes in
    front of it inside its own tile"""
    assert lb.debug_grid_ceiling()[0] == 0
    n = N_BIG + 3
    long_ones = [5, (STEP - 1) * T + 9, (STEP + 1) * T + 3]
    counts = np.ones(n, np.uint32)
    counts[long_ones] = 5
    total = int(counts.sum())
    assert total == n + 12
    big = _big(oracle)
    flat, packed = big["bools"][:total, 0, :], big["packed"][:total, 0, :]
    indices = np.arange(STEP * T, n, 2)
    assert long_ones[2] not in indices and -(-n // T) == STEP + 2 and indices[-1] > long_ones[2]
    keep, new, removed = RM._expected(n, indices)
    c = RM._ragged(lb, gpu, oracle, flat, counts, n, total)
    try:
        st, got_removed, got_map = RM._remove_host(lb, c, indices)
        assert st == 0
        assert got_removed == removed and len(c) == n - removed, (got_removed, removed, len(c))
        assert c.subfingerprint_total == int(counts[keep].sum())
        assert np.array_equal(got_map, new), np.flatnonzero(got_map != new)[:8]
        _contents(gpu, c, packed[np.repeat(keep, counts)], counts[keep], "ragged")
    finally:
        c.dispose()


def test_gather_of_more_keys_than_one_step_of_tiles(lb, gpu, oracle):
    """gather_tiles_kernel's second step.  N_BIG keys of the uniform corpus of N_BIG entries -- a permutation, every 50th key zero,
    every 97th of another index range: the offsets are sums of 0 or 1; then N_BIG keys drawn with repetition from a ragged corpus
    of 3000 entries of 1 .. 40 records: the carry out of step 1 is a sum of real lengths.  Offsets (N_BIG + 1 words), total and
    every gathered byte against numpy."""
    assert lb.debug_grid_ceiling()[0] == 0
    big = _big(oracle)
    rng = np.random.default_rng(31)
    # uniform
    g = rng.permutation(N_BIG).astype(np.int64)
    g[::50] = -1
    g[::97] = N_BIG + np.arange(len(g[::97]))
    valid = (g >= 0) & (g < N_BIG)
    assert valid[STEP * T:].any() and not valid[STEP * T:].all()
    want_off = np.concatenate([[0], np.cumsum(valid)]).astype(np.uint64)
    want = big["packed"][:N_BIG, 0, :][g[valid]]
    c = _big_uniform(lb, gpu, oracle)
    try:
        off, packed = GA._gather_dev(gpu, c, GA._keys(g, rng), 0, len(want))
        assert np.array_equal(off, want_off), ("uniform", np.flatnonzero(off != want_off)[:4], off[-1], len(want))
        assert np.array_equal(packed[:len(want)], want) and (packed[len(want):] == GA.POISON8).all()
    finally:
        c.dispose()
    # ragged: most entries of 1 .. 3 records, every 20th of 1 .. 40
    n_e = 3000
    counts = rng.integers(1, 4, n_e).astype(np.uint32)
    counts[::20] = rng.integers(1, 41, len(counts[::20]))
    counts[7], counts[8] = 40, 1
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    flat, rows = big["bools"][:first[-1], 0, :], big["packed"][:first[-1], 0, :]
    g = rng.integers(0, n_e, N_BIG).astype(np.int64)
    g[3::50] = -1
    g[5::97] = n_e + 4
    valid = (g >= 0) & (g < n_e)
    lens = np.where(valid, counts[np.where(valid, g, 0)], 0).astype(np.int64)
    want_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(want_off[-1])
    assert lens[STEP * T:].sum() > T and total < 1_500_000        # (at most 48 MB of output)
    record = np.repeat(first[np.where(valid, g, 0)], lens) + (np.arange(total) - np.repeat(want_off[:-1], lens))
    c = GA._ragged(lb, gpu, oracle, flat, counts, n_e, int(first[-1]))
    try:
        off, packed = GA._gather_dev(gpu, c, GA._keys(g, rng), 0, total)
        assert np.array_equal(off.astype(np.int64), want_off), ("ragged", np.flatnonzero(off.astype(np.int64) != want_off)[:4], off[-1], total)
        bad = np.flatnonzero((packed[:total] != rows[record]).any(axis=1))
        assert len(bad) == 0, ("ragged, bytes of records", len(bad), bad[:4])
        assert (packed[total:] == GA.POISON8).all()
    finally:
        c.dispose()


def test_extra_keys_of_more_tiles_than_one_step(lb, gpu):
    """groups_extra_tiles_kernel's second step, and the largest shape of init, hook and flatten.  About 4 000 edges over N_BIG
    vertices, every one inside tile 0, tile 255, tile 256 or the partial tile 257, or between two of them: the extra vertices lie
    there and nowhere in tiles 1 .. 254.  Labels against _union_find, then the extra keys of the DEVICE's labels against numpy
    -- every i with labels[i] != i, ascending, and the count -- with room for all of them and with a capacity that ends inside
    tile 256."""
    assert lb.debug_grid_ceiling()[0] == 0
    rng = np.random.default_rng(53)
    n = N_BIG
    spans = [(0, T), ((STEP - 1) * T, STEP * T), (STEP * T, (STEP + 1) * T), ((STEP + 1) * T, n)]
    edges = []
    for lo, hi in spans:
        edges += [(int(a), int(b)) for a, b in rng.integers(lo, hi, (1200 if hi - lo == T else 6, 2))]
    for (lo_a, hi_a), (lo_b, hi_b) in ((spans[0], spans[3]), (spans[1], spans[2]), (spans[3], spans[1])):
        edges += [(int(rng.integers(lo_a, hi_a)), int(rng.integers(lo_b, hi_b))) for _ in range(100)]
    g = GR.Rows(n, GR._rows_of(n, edges))
    want = GR._union_find(n, g.edges())
    labels, count = GR._labels_call(lb, gpu, g)
    got = labels.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    assert count == int((want == np.arange(n)).sum())
    extra = np.flatnonzero(got != np.arange(n))
    per_span = [int(((extra >= lo) & (extra < hi)).sum()) for lo, hi in spans]
    assert min(per_span) >= 3 and sum(per_span) == len(extra) and per_span[2] >= 10, per_span
    assert GR._check_extra(lb, gpu, got, len(extra) + 9) == len(extra)
    assert GR._check_extra(lb, gpu, got, per_span[0] + per_span[1] + per_span[2] // 2) == len(extra)


# ---- the ceiling is left at 0 ------------------------------------------------------------------------------------------------------
def test_the_ceiling_is_back_at_zero(lb, gpu):
    assert lb.debug_grid_ceiling()[0] == 0
