"""GPU tests of the batch recording scores and the batch recording top-K (LBAudioDetectiveCorpusRecordingPackedScoresBatchDevice,
LBAudioDetectiveCorpusQueryPackedRecordingTopKBatchKeysDevice, k_recording_batch.hip, StreamBank.identify_recordings).  Every
expected value is numpy (align_ref.align for EVERY recording and entry, the selection restated on those scores) or the output of a
call that existed before (recording_scores_device and query_packed_recording_topk_keys_device on one row of the block,
query_packed_topk_keys_device -- the scan -- on the whole block); scores are compared as bits, keys and lags exactly: nothing needs
a tolerance.  Output buffers are poison-filled before every call.  The corpus is built the way test_gpu_timeline_batch.py builds
its own (the helpers are copied, not imported): 2 x 64 + 5 entries, the last entry block partial -- 1 .. 40 sub-fingerprints, a
planted 17 and a planted 22, a duplicate of the 22 at a higher index, an all-zero entry and, as the LAST two, one entry of 150 and
one of 400: longer than the short windows, so that case A of the pair loop runs.  Because those two raise the call's tile bound
to 3 at every short window, the form W cases run against the whole corpus AND against its first 131 entries (1, 2 and 3 tiles);
an entry's score does not depend on the other entries, so one reference serves both.  The corpora, the blocks of recordings and
the reference are made once per module."""
import numpy as np
import pytest

from align_ref import align

pytestmark = pytest.mark.gpu

POISON = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
POISONF = -12345.0
L = 200
TILE, GROUP, WALK = 126, 504, 64
N_CASE = 2 * WALK + 5
N_SHORT = N_CASE - 2                     # without the two long entries: still a partial last block
E17, E22, EZERO, EDUP, E150, E400 = 7, 11, 29, 100, N_CASE - 2, N_CASE - 1
FORM_S, FORM_W = 0, 1
ONE = np.float32(1.0)
KS = (1, 3, 200)                         # 200: more than the corpus has entries, so more than score above 0


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
    counts[3], counts[5] = 1, 40                                 # the plan's shortest and (of the short corpus) longest entry
    counts[E150], counts[E400] = 150, 400
    e = _random(oracle, 4242, counts)
    pool = _random(oracle, 4343, [17, 22])
    e[E17], e[E22] = pool
    e[EDUP] = pool[1].copy()                                     # the 22 once more at a higher index: the tie goes to the lower
    e[EZERO] = np.zeros((10, L), np.uint8)                       # scores 0 against everything: never selected
    return e


# name: (form, recordings, sub-fingerprints each).  Form W: five recordings, so that the last group of four global tiles is partial
# and groups of four straddle recordings; form S: 5 tiles, two tile groups
CASES = {"w100": (FORM_W, 5, 100), "w129": (FORM_W, 5, 129), "w300": (FORM_W, 5, 300), "s525": (FORM_S, 3, 525)}
# name: [(recording, offset)] where the 22 / the 17 lie verbatim (cells of 1.0; the lag is minus the LOWEST offset of a recording)
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
        assert (_M["lengths"][:N_SHORT].min(), _M["lengths"][:N_SHORT].max(), len(e[E22]), len(e[E17])) == (1, 40, 22, 17)
        _M["corpus"] = {N_CASE: _ragged(lb, gpu, oracle, e), N_SHORT: _ragged(lb, gpu, oracle, e[:N_SHORT])}
        _M["dev"] = {name: gpu.from_numpy(_packed(oracle, b.reshape(-1, L))).cuda() for name, b in _M["blocks"].items()}
        _M["aligned"] = {}
    return _M


def _aligned(m, name, range_=0):
    """the reference's (scores float32 [R, N_CASE], lags int32 [R, N_CASE]) of every recording of a block against EVERY entry,
    made once"""
    if (name, range_) not in m["aligned"]:
        got = [[align(rec, ent, range_) for ent in m["entries"]] for rec in m["blocks"][name]]
        m["aligned"][(name, range_)] = (np.array([[g[0] for g in row] for row in got], np.float32),
                                        np.array([[g[1] for g in row] for row in got], np.int32))
    return m["aligned"][(name, range_)]


def _select(scores, lags, k, base=0):
    """the selection restated: per row the k largest keys score bits << 32 | 0xFFFFFFFF - (base + j) of the entries scoring above
    0, descending (so the lowest index first among equals), zero keys behind; the lag of the entry a key names, 0 for a zero key"""
    R, n = scores.shape
    keys = np.zeros((R, k), np.uint64)
    out = np.zeros((R, k), np.int32)
    for r in range(R):
        all_keys = (scores[r].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF - base) - np.arange(n, dtype=np.uint64))
        order = [j for j in np.argsort(all_keys, kind="stable")[::-1] if scores[r, j] > 0][:k]
        keys[r, :len(order)] = all_keys[order]
        out[r, :len(order)] = lags[r, order]
    return keys, out


def _scores(gpu, corpus, packed, R, per, range_=0, want_lags=True, stream=None):
    """one batch scores call into poison-filled buffers -> (scores float32 [R, n], lags int32 [R, n] or None)"""
    n = len(corpus)
    scores = gpu.full((R, max(1, n)), POISONF, dtype=gpu.float32, device="cuda")[:, :n].contiguous()
    lags = gpu.full((R, max(1, n)), POISON32, dtype=gpu.int32, device="cuda")[:, :n].contiguous() if want_lags else None
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = corpus.recording_scores_batch_device(packed, R, per, range_=range_, scores_out=scores, lags_out=lags, want_lags=want_lags,
                                               stream=stream)
    assert got[0] is scores and got[1] is lags
    (stream or gpu.cuda.current_stream()).synchronize()
    return scores.cpu().numpy(), lags.cpu().numpy() if want_lags else None


def _single_scores(gpu, corpus, packed, R, per, range_=0):
    """recording_scores_device on every row of the block in turn"""
    n = len(corpus)
    rows = packed.reshape(R, per, 32)
    scores = gpu.full((R, n), POISONF, dtype=gpu.float32, device="cuda")
    lags = gpu.full((R, n), POISON32, dtype=gpu.int32, device="cuda")
    for r in range(R):
        corpus.recording_scores_device(packed=rows[r], per_query=per, range_=range_, scores_out=scores[r], lags_out=lags[r])
    gpu.cuda.synchronize()
    return scores.cpu().numpy(), lags.cpu().numpy()


def _topk(gpu, corpus, packed, R, per, k, range_=0, base=0, want_lags=True, stream=None):
    """one batch top-K call into poison-filled buffers -> (keys uint64 [R, k], lags int32 [R, k] or None)"""
    keys = gpu.full((R, k), POISON, dtype=gpu.int64, device="cuda")
    lags = gpu.full((R, k), POISON32, dtype=gpu.int32, device="cuda") if want_lags else None
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = corpus.query_packed_recording_topk_batch_keys_device(packed, R, per, k, range_=range_, index_base=base, keys_out=keys,
                                                               lags_out=lags, aligned=want_lags, stream=stream)
    if want_lags:
        assert got[0] is keys and got[1] is lags
    else:
        assert got is keys
    (stream or gpu.cuda.current_stream()).synchronize()
    return keys.cpu().numpy().view(np.uint64), lags.cpu().numpy() if want_lags else None


def _single_topk(gpu, corpus, packed, R, per, k, range_=0, base=0):
    """query_packed_recording_topk_keys_device on every row of the block in turn"""
    rows = packed.reshape(R, per, 32)
    keys = gpu.full((R, k), POISON, dtype=gpu.int64, device="cuda")
    lags = gpu.full((R, k), POISON32, dtype=gpu.int32, device="cuda")
    for r in range(R):
        corpus.query_packed_recording_topk_keys_device(rows[r], per, k, range_=range_, index_base=base, keys_out=keys[r], lags_out=lags[r])
    gpu.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64), lags.cpu().numpy()


def _scan_topk(gpu, corpus, packed, R, per, k, range_=0, base=0):
    """the scan behind identify on the whole block"""
    keys = gpu.full((R, k), POISON, dtype=gpu.int64, device="cuda")
    lags = gpu.full((R, k), POISON32, dtype=gpu.int32, device="cuda")
    corpus.query_packed_topk_keys_device(packed, R, per, k, keys_out=keys, lags_out=lags, aligned=True, range_=range_, index_base=base)
    gpu.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64), lags.cpu().numpy()


def _same_scores(got, want):
    """scores as bits, lags exactly"""
    assert got[0].shape == want[0].shape
    assert np.array_equal(got[0].view(np.uint32), np.ascontiguousarray(want[0], np.float32).view(np.uint32))
    if got[1] is not None:
        assert np.array_equal(got[1], want[1])


def _same_keys(got, want):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    if got[1] is not None:
        assert np.array_equal(got[1], want[1])


def _plan(lb, m, n, R, per, limit=0, key_form=False):
    return lb.debug_recording_batch_plan(R, per, int(m["lengths"][:n].min()), int(m["lengths"][:n].max()), n, limit, key_form)


def _tiles(per, n):
    most = per                                                   # the shortest entry has one sub-fingerprint
    if n == N_CASE and per < 400:
        most = max(most, 400 - per + 1)
    return -(-most // TILE)


def _check(lb, gpu, m, name, n, range_=0, base=0, ks=KS, reference=True):
    """the whole contract for one block against the corpus of n entries: every score and lag against the reference and the single
    call, every key and lag row against the restated selection, the single top-K call and the scan"""
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"][n], m["dev"][name]
    got = _scores(gpu, corpus, packed, R, per, range_)
    single = _single_scores(gpu, corpus, packed, R, per, range_)
    _same_scores(got, single)
    want = single
    if reference:
        ref = _aligned(m, name, range_)
        want = (ref[0][:, :n], ref[1][:, :n])
        _same_scores(got, want)
    _same_scores(_scores(gpu, corpus, packed, R, per, range_, want_lags=False), (want[0], None))     # NULL lags: the same scores
    for k in ks:
        keys = _topk(gpu, corpus, packed, R, per, k, range_, base)
        _same_keys(keys, _select(np.ascontiguousarray(want[0]), want[1], k, base))
        _same_keys(keys, _single_topk(gpu, corpus, packed, R, per, k, range_, base))
        _same_keys(keys, _scan_topk(gpu, corpus, packed, R, per, k, range_, base))
        _same_keys(_topk(gpu, corpus, packed, R, per, k, range_, base, want_lags=False), (keys[0], None))
    return got


# ---- 1. forms and tiles, plants at the seams, case A, no leak from a neighbour ----------------------------------------------------------
@pytest.mark.parametrize("name,n", [("w100", N_SHORT), ("w129", N_SHORT), ("w300", N_SHORT), ("w100", N_CASE), ("w129", N_CASE),
                                    ("w300", N_CASE), ("s525", N_CASE)])
def test_rows_equal_the_reference_and_the_existing_calls(lb, gpu, oracle, name, n):
    m = _module(lb, gpu, oracle)
    form, R, per = CASES[name]
    for key_form in (False, True):
        plan = _plan(lb, m, n, R, per, key_form=key_form)
        assert plan["form"] == form and plan["tiles"] == _tiles(per, n) and plan["recordings_per_pass"] == R
        assert form == FORM_S or (R * plan["tiles"]) % 4 != 0     # form W: the last group of four global tiles is partial
    scores, lags = _check(lb, gpu, m, name, n)
    # the plants: a cell of 1.0, the lag minus the LOWEST offset of the piece in that recording
    for plants, entry in ((PLANTS_22, E22), (PLANTS_17, E17)):
        for r in range(R):
            at = [o for row, o in plants[name] if row == r]
            if at:
                assert scores[r, entry] == ONE and lags[r, entry] == -min(at), (name, r, entry)
    for r, _o in PLANTS_22[name]:
        assert scores[r, EDUP] == ONE and lags[r, EDUP] == lags[r, E22]
        keys = _topk(gpu, m["corpus"][n], m["dev"][name], R, per, 200)[0]
        order = [0xFFFFFFFF - int(key & np.uint64(0xFFFFFFFF)) for key in keys[r] if key]
        assert order.index(E22) + 1 == order.index(EDUP)          # the tie goes to the lower index, the duplicate follows
    assert not scores[:, EZERO].any() and not lags[:, EZERO].any()
    # the straddling 22: in the packed block it lies verbatim across the seam of r | r + 1; no recording holds it
    if name in STRADDLE:
        r = STRADDLE[name]
        assert scores[r, E22] < ONE and scores[r + 1, E22] < ONE and scores[r, EDUP] < ONE and scores[r + 1, EDUP] < ONE
    # case A: the recording lies verbatim inside a longer entry
    for entry, block, r, at in INSIDE:
        if block == name and n == N_CASE:
            assert scores[r, entry] == ONE and lags[r, entry] == at


def test_the_shapes_are_the_seams(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    assert len(m["entries"]) == 2 * WALK + 5 and N_SHORT % WALK != 0
    assert (0, TILE - 1) in PLANTS_22["w300"] and (1, TILE) in PLANTS_17["w300"]                       # offsets 125 | 126: the tile seam
    assert (1, GROUP - 1) in PLANTS_22["s525"] and (0, GROUP) in PLANTS_17["s525"]                     # 503 | 504: the group seam
    assert (0, TILE - 1) in PLANTS_22["s525"] and (1, TILE) in PLANTS_17["s525"]
    for name, (_form, _R, per) in CASES.items():                  # the last legal offset of recording r, offset 0 of r + 1
        last = [(r, o, 22) for r, o in PLANTS_22[name] if o == per - 22] + [(r, o, 17) for r, o in PLANTS_17[name] if o == per - 17]
        assert last, name
        assert all((r + 1, 0) in (PLANTS_22 if size == 22 else PLANTS_17)[name] for r, _o, size in last), name
    assert any(len([o for row, o in PLANTS_17[name] if row == r]) > 1 for name in CASES for r in range(5))   # the same piece twice
    # case A runs: offsets of the long entries at the short windows, in tile 0 and beyond it
    assert 150 - 100 + 1 < TILE < 400 - 129 + 1 and INSIDE[1][3] // TILE == 1
    assert [_tiles(per, N_SHORT) for per in (100, 129, 300)] == [1, 2, 3]


# ---- 2. options: a masked range, an index base -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w300", "s525"])
def test_a_masked_range(lb, gpu, oracle, name):
    """a range below the sub-fingerprint length: the non-FULL instances of both forms"""
    m = _module(lb, gpu, oracle)
    _check(lb, gpu, m, name, N_CASE, range_=64, ks=(3,))
    _check(lb, gpu, m, name, N_CASE, range_=199, ks=(3,), reference=False)


@pytest.mark.parametrize("name", ["w129", "s525"])
def test_an_index_base(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"][N_CASE], m["dev"][name]
    zero = _topk(gpu, corpus, packed, R, per, 3)
    for base in (1000, (1 << 32) - N_CASE):
        _check(lb, gpu, m, name, N_CASE, base=base, ks=(3, 200))
        got = _topk(gpu, corpus, packed, R, per, 3, base=base)
        assert np.array_equal(got[0][got[0] != 0] + np.uint64(base), zero[0][zero[0] != 0]) and np.array_equal(got[1], zero[1])
    with pytest.raises(lb.LBAudioDetectiveError) as err:
        _topk(gpu, corpus, packed, R, per, 3, base=(1 << 32) - N_CASE + 1)
    assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")


def test_the_form_changes_nothing(lb, gpu, oracle):
    """form S forced where the plan takes form W"""
    m = _module(lb, gpu, oracle)
    try:
        for name, n in (("w129", N_CASE), ("w129", N_SHORT), ("w300", N_SHORT)):
            _form, R, per = CASES[name]
            lb.debug_set_recording_batch_form(True)
            assert _plan(lb, m, n, R, per)["form"] == FORM_S
            _check(lb, gpu, m, name, n, ks=(3,))
            _check(lb, gpu, m, name, n, range_=64, ks=(3,))
            lb.debug_set_recording_batch_form(False)
            assert _plan(lb, m, n, R, per)["form"] == FORM_W
    finally:
        lb.debug_set_recording_batch_form(False)


# ---- 3. passes and chunks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w300", "s525"])
def test_passes_and_chunks_change_nothing(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"][N_CASE], m["dev"][name]
    tiles = _tiles(per, N_CASE)
    whole, block = 3 * WALK * tiles * 8, WALK * tiles * 8
    ref = _aligned(m, name)
    try:
        corpus.set_join_scratch_limit(0)
        # (a) several passes of recordings, the last one partial; (b) one recording per pass, several entry chunks, the last partial
        for limit, rpp, chunk in ((2 * whole + 3, 2, 3 * WALK), (whole, 1, 3 * WALK), (whole - 1, 1, 2 * WALK), (block, 1, WALK)):
            for key_form in (False, True):
                plan = _plan(lb, m, N_CASE, R, per, limit, key_form)
                assert (plan["recordings_per_pass"], plan["entries_per_chunk"]) == (rpp, chunk) and plan["scratch_bytes"] <= limit
            assert R % rpp != 0 or rpp == 1
            corpus.set_join_scratch_limit(limit)
            _same_scores(_scores(gpu, corpus, packed, R, per), ref)
            _same_scores(_scores(gpu, corpus, packed, R, per, want_lags=False), (ref[0], None))
            for k in (3, 200):
                _same_keys(_topk(gpu, corpus, packed, R, per, k), _select(ref[0], ref[1], k))
            _same_keys(_topk(gpu, corpus, packed, R, per, 3, want_lags=False), (_select(ref[0], ref[1], 3)[0], None))
        # a limit below one block of ONE recording
        corpus.set_join_scratch_limit(block - 1)
        for call in (lambda: _scores(gpu, corpus, packed, R, per), lambda: _topk(gpu, corpus, packed, R, per, 3)):
            with pytest.raises(lb.LBAudioDetectiveError) as err:
                call()
            assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    finally:
        corpus.set_join_scratch_limit(0)


# ---- 4. the second trip of both forms' grid-stride loops ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w300", "s525"])
def test_second_trips(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    form, R, per = CASES[name]
    tiles = _tiles(per, N_CASE)
    units = 3 * (-(-(R * tiles) // 4) if form == FORM_W else R * -(-tiles // 4))
    ref = _aligned(m, name)
    try:
        for ceiling in (1, 4):
            assert ceiling < units
            lb.debug_set_grid_ceiling(ceiling)
            before = lb.debug_grid_ceiling()[1]
            _same_scores(_scores(gpu, m["corpus"][N_CASE], m["dev"][name], R, per), ref)
            assert lb.debug_grid_ceiling()[1] > before
            _same_keys(_topk(gpu, m["corpus"][N_CASE], m["dev"][name], R, per, 3), _select(ref[0], ref[1], 3))
    finally:
        lb.debug_set_grid_ceiling(0)
    assert lb.debug_grid_ceiling()[0] == 0


# ---- 5. more tiles than the fold has lanes for an entry ----------------------------------------------------------------------------------------
def test_the_fold_takes_a_second_trip(lb, gpu, oracle):
    """two recordings of 8100 sub-fingerprints: 65 tiles, so that lanes of the fold read a second partial (tile += lanes); the
    plants lie in tile 64 of recording 0 and in tile 0 of recording 1.  Against the single calls and the scan."""
    m = _module(lb, gpu, oracle)
    R, per = 2, 8100
    corpus = m["corpus"][N_CASE]
    plan = _plan(lb, m, N_CASE, R, per)
    assert plan["tiles"] == 65 > 64 and plan["form"] == FORM_S and plan["recordings_per_pass"] == 2
    block = oracle.synth_ragged_entries(5150, 0, np.array([R * per], np.uint32), L).reshape(R, per, L).copy()
    block[0, 64 * TILE + 3:64 * TILE + 25] = m["entries"][E22]
    block[1, 5:22] = m["entries"][E17]
    packed = gpu.from_numpy(_packed(oracle, block.reshape(-1, L))).cuda()
    got = _scores(gpu, corpus, packed, R, per)
    _same_scores(got, _single_scores(gpu, corpus, packed, R, per))
    assert got[0][0, E22] == ONE and got[1][0, E22] == -(64 * TILE + 3) and got[0][1, E17] == ONE and got[1][1, E17] == -5
    for k in (1, 200):
        keys = _topk(gpu, corpus, packed, R, per, k)
        _same_keys(keys, _select(got[0], got[1], k))
        _same_keys(keys, _single_topk(gpu, corpus, packed, R, per, k))
        _same_keys(keys, _scan_topk(gpu, corpus, packed, R, per, k))


# ---- 6. one recording: the single call ------------------------------------------------------------------------------------------------------------
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
    got = _scores(gpu, corpus, packed, 1, per)
    _same_scores(got, _single_scores(gpu, corpus, packed, 1, per))
    want = [align(q, ent, 0) for ent in m["entries"]]
    _same_scores(got, (np.array([[w[0] for w in want]], np.float32), np.array([[w[1] for w in want]], np.int32)))
    for k in KS:
        keys = _topk(gpu, corpus, packed, 1, per, k)
        _same_keys(keys, _select(got[0], got[1], k))
        _same_keys(keys, _single_topk(gpu, corpus, packed, 1, per, k))
        _same_keys(keys, _scan_topk(gpu, corpus, packed, 1, per, k))
    if per == 700:
        assert got[0][0, E22] == ONE and got[1][0, E22] == -600
    if per == 17:
        assert got[0][0, E17] == ONE and got[1][0, E17] == 0


# ---- 7. the empty corpus; refusals that need the corpus ---------------------------------------------------------------------------------------------
def test_the_empty_corpus(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    empty = lb.Corpus.ragged(L, 4, 16)
    packed = m["dev"]["w100"]
    # the scores form writes nothing
    scores = gpu.full((5, 4), POISONF, dtype=gpu.float32, device="cuda")
    lags = gpu.full((5, 4), POISON32, dtype=gpu.int32, device="cuda")
    empty.recording_scores_batch_device(packed, 5, 100, scores_out=scores, lags_out=lags)
    gpu.cuda.synchronize()
    assert bool((scores == POISONF).all()) and bool((lags == POISON32).all())
    # the key form writes zeros
    for want_lags in (True, False):
        keys, klags = _topk(gpu, empty, packed, 5, 100, 3, want_lags=want_lags)
        assert not keys.any() and (klags is None or not klags.any())


def test_refusals(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    packed = m["dev"]["w100"]
    above = _ragged(lb, gpu, oracle, _random(oracle, 5, [3, 1024 + 1, 2]))
    for corpus in (lb.Corpus(L, 4, 8), above):                    # a uniform corpus; an entry above the cap
        keys = gpu.full((5, 3), POISON, dtype=gpu.int64, device="cuda")
        scores = gpu.full((5, 8), POISONF, dtype=gpu.float32, device="cuda")
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            corpus.query_packed_recording_topk_batch_keys_device(packed, 5, 100, 3, keys_out=keys)
        assert err.value.status == bad
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            corpus.recording_scores_batch_device(packed, 5, 100, scores_out=scores, want_lags=False)
        assert err.value.status == bad
        gpu.cuda.synchronize()
        assert bool((keys == POISON).all()) and bool((scores == POISONF).all())   # a refused call writes nothing


# ---- 8. two calls in a row on two streams ---------------------------------------------------------------------------------------------------------------
def test_two_streams_in_a_row(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"][N_CASE]
    names = ("s525", "w300", "w129")
    streams = [gpu.cuda.Stream(), gpu.cuda.Stream(), gpu.cuda.Stream()]
    outs = []
    for i, (s, name) in enumerate(zip(streams, names)):           # each call is made while the one before may still run
        _form, R, per = CASES[name]
        s.wait_stream(gpu.cuda.current_stream())
        if i == 1:                                                # the scores form between two key forms
            a = gpu.full((R, N_CASE), POISONF, dtype=gpu.float32, device="cuda")
            b = gpu.full((R, N_CASE), POISON32, dtype=gpu.int32, device="cuda")
            corpus.recording_scores_batch_device(m["dev"][name], R, per, scores_out=a, lags_out=b, stream=s)
        else:
            a = gpu.full((R, 3), POISON, dtype=gpu.int64, device="cuda")
            b = gpu.full((R, 3), POISON32, dtype=gpu.int32, device="cuda")
            corpus.query_packed_recording_topk_batch_keys_device(m["dev"][name], R, per, 3, keys_out=a, lags_out=b, stream=s)
        outs.append((a, b))
    for s in streams:
        s.synchronize()
    for i, ((a, b), name) in enumerate(zip(outs, names)):
        ref = _aligned(m, name)
        if i == 1:
            _same_scores((a.cpu().numpy(), b.cpu().numpy()), ref)
        else:
            _same_keys((a.cpu().numpy().view(np.uint64), b.cpu().numpy()), _select(ref[0], ref[1], 3))


# ---- 9. the stream bank ---------------------------------------------------------------------------------------------------------------------------------
def test_stream_bank_identify_recordings(lb, gpu, oracle):
    """three channels of test_gpu_stream_bank.py's pruned configuration; the corpus holds random entries and, per channel, rows
    [total - 15, total - 5) of its own sub-fingerprints: identify_recordings against identify(aligned=True) on the same window,
    and the planted spans win with 1.0 at offset 5 of a window of 20"""
    rate, window, stride, bands, length = 44100, 1024, 64, 32, 200
    hop, frames, n = 128 * stride, 23, 20
    cfg = oracle.Config(rate, window, stride, bands, length)
    sig = [oracle.synth_clip(0x53424B31, c, rate, window + frames * hop + 7) for c in range(3)]
    ref = [oracle.fingerprint_pcm(s, cfg) for s in sig]
    assert all(r.shape == (frames, length) and r.any(axis=1).all() for r in ref)
    det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
    bank = lb.StreamBank(det, 3, 24)
    counts = [s.size for s in sig]
    bank.push_device(gpu.from_numpy(np.concatenate(sig).astype(np.float32)).cuda(), counts)
    assert bank.totals().tolist() == [frames] * 3
    ent = _random(oracle, 61, np.random.default_rng(4).integers(1, 16, 30), length)
    ent.append(_random(oracle, 62, [31], length)[0])              # longer than the window: case A
    planted = {}
    for c in range(3):
        planted[c] = len(ent)
        ent.append(ref[c][frames - 15:frames - 5].copy())
    corpus = _ragged(lb, gpu, oracle, ent, length)
    channels = [2, 0, 1]
    stream = gpu.cuda.Stream()
    stream.wait_stream(gpu.cuda.current_stream())
    for k in (1, 4):
        keys, lags = bank.identify_recordings(corpus, channels, n, k=k, aligned=True, stream=stream)
        stream.synchronize()
        assert keys.shape == (3, k) and lags.shape == (3, k) and keys.dtype == gpu.int64 and lags.dtype == gpu.int32
        want = bank.identify(corpus, channels, n, k=k, aligned=True)
        gpu.cuda.synchronize()
        assert np.array_equal(keys.cpu().numpy(), want[0].cpu().numpy()) and np.array_equal(lags.cpu().numpy(), want[1].cpu().numpy())
        only = bank.identify_recordings(corpus, channels, n, k=k)
        gpu.cuda.synchronize()
        assert np.array_equal(only.cpu().numpy(), keys.cpu().numpy())
        got = keys.cpu().numpy().view(np.uint64)
        for j, c in enumerate(channels):
            assert got[j, 0] == (np.uint64(ONE.view(np.uint32)) << np.uint64(32)) | np.uint64(0xFFFFFFFF - planted[c])
            assert lags.cpu().numpy()[j, 0] == -5
    win = bank.window_device(channels, n)
    gpu.cuda.synchronize()
    rows = lb.unpack_packed(win.cpu().numpy(), length).reshape(3, n, length)
    want = [[align(rows[j], e, 0) for e in ent] for j in range(3)]
    scores, slags = corpus.recording_scores_batch_device(win, 3, n)
    gpu.cuda.synchronize()
    _same_scores((scores.cpu().numpy(), slags.cpu().numpy()),
                 (np.array([[w[0] for w in row] for row in want], np.float32), np.array([[w[1] for w in row] for row in want], np.int32)))
