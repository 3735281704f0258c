"""GPU tests of the batch recording timeline (LBAudioDetectiveCorpusRecordingPackedTimelineBatchKeysDevice, k_timeline_batch.hip,
StreamBank.timeline).  Every expected value is numpy (timeline_ref on align_ref.profile, recording by recording) or the
single-recording call on one row of the block; keys are compared as integers, lengths exactly: nothing needs a tolerance.  Output
buffers are poison-filled before every call.  The corpus is built the way test_gpu_timeline.py builds its own (the helpers are
copied, not imported): 2 x 128 + 5 entries of 1 .. 40 sub-fingerprints, the last entry block partial, a planted 22 and a planted
17; it, the blocks of recordings and the reference's profiles are made once per module."""
import numpy as np
import pytest

import timeline_ref

pytestmark = pytest.mark.gpu

POISON = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
L = 200
TILE, GROUP, WALK, FOLD_ROWS = 126, 504, 128, 32
N_CASE = 2 * WALK + 5
E17, E22 = 7, 11
T_HIGH, T_LOW = 0.7, 0.3
FORM_S, FORM_W = 0, 1
ONE = int(np.float32(1.0).view(np.uint32))


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
    counts[3], counts[5] = 1, 40                                 # the plan's shortest and longest entry, whatever the draw
    e = _random(oracle, 4242, counts)
    pool = _random(oracle, 4343, [17, 22])
    e[E17], e[E22] = pool
    return e


# name: (form, recordings, sub-fingerprints each).  Form W: five recordings, so that the last group of four global tiles is partial,
# at 1, 2 and 3 tiles (groups of four straddle recordings at 3); form S: 5 tiles, two tile groups
CASES = {"w100": (FORM_W, 5, 100), "w129": (FORM_W, 5, 129), "w300": (FORM_W, 5, 300), "s525": (FORM_S, 3, 525)}
# name: [(recording, offset)] where the 22 / the 17 lie verbatim and undisturbed (cells of 1.0), and the recording r whose end and
# whose successor's start hold the two halves of the 22
PLANTS_22 = {"w100": [(0, 0), (1, 100 - 22), (2, 0)], "w129": [(1, 129 - 22), (2, 0)],
             "w300": [(0, TILE - 1), (1, TILE), (2, 300 - 22), (3, 0)], "s525": [(0, TILE - 1), (1, TILE), (1, GROUP - 1), (2, 0)]}
PLANTS_17 = {"w100": [(3, 50)], "w129": [(4, 129 - 17)], "w300": [(4, 2 * TILE)], "s525": [(2, GROUP)]}
STRADDLE = {"w100": 3, "w129": 2, "w300": 3, "s525": 0}


def _block(oracle, e, name):
    """Booleans [recordings, per, L]"""
    _form, R, per = CASES[name]
    block = oracle.synth_ragged_entries(777 + per, 0, np.array([R * per], np.uint32), L).reshape(R, per, L).copy()
    for r, o in PLANTS_22[name]:
        block[r, o:o + 22] = e[E22]
    for r, o in PLANTS_17[name]:
        block[r, o:o + 17] = e[E17]
    r = STRADDLE[name]
    block[r, per - 11:] = e[E22][:11]                            # in the packed block the 22 lies verbatim across the seam
    block[r + 1, :11] = e[E22][11:]
    flat = block.reshape(R * per, L)
    assert np.array_equal(flat[(r + 1) * per - 11:(r + 1) * per + 11], e[E22])
    return block


_M = {}


def _module(lb, gpu, oracle):
    if not _M:
        e = _entries(oracle)
        _M["entries"] = e
        _M["lengths"] = np.array([len(x) for x in e], np.int64)
        assert (_M["lengths"].min(), _M["lengths"].max(), len(e[E22]), len(e[E17])) == (1, 40, 22, 17)
        _M["corpus"] = _ragged(lb, gpu, oracle, e)
        _M["blocks"] = {name: _block(oracle, e, name) for name in CASES}
        _M["dev"] = {name: gpu.from_numpy(_packed(oracle, b.reshape(-1, L))).cuda() for name, b in _M["blocks"].items()}
        _M["profiles"] = {}
    return _M


def _want(m, name, t, range_=0, base=0):
    """the reference's (keys uint64 [R, per], lengths uint32 [R, per]), recording by recording; the profiles of a (block, range)
    are made once"""
    block = m["blocks"][name]
    if (name, range_) not in m["profiles"]:
        m["profiles"][(name, range_)] = [timeline_ref.profiles(rec, m["entries"], range_) for rec in block]
    rows = [timeline_ref.fold(block.shape[1], p, t, base) for p in m["profiles"][(name, range_)]]
    return np.stack([k for k, _ in rows]), np.stack([n for _, n in rows])


def _batch(gpu, corpus, packed, R, per, t, range_=0, base=0, want_lengths=True, stream=None):
    """one batch call into poison-filled buffers -> (keys uint64 [R, per], lengths uint32 [R, per] or None)"""
    keys = gpu.full((R, per), POISON, dtype=gpu.int64, device="cuda")
    lengths = gpu.full((R, per), POISON32, dtype=gpu.int32, device="cuda") if want_lengths else None
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = corpus.recording_timeline_batch_keys_device(packed, R, per, t, range_=range_, index_base=base, keys_out=keys, lengths_out=lengths,
                                                      want_lengths=want_lengths, stream=stream)
    assert got[0] is keys and got[1] is lengths
    (stream or gpu.cuda.current_stream()).synchronize()
    return keys.cpu().numpy().view(np.uint64), lengths.cpu().numpy().view(np.uint32) if want_lengths else None


def _single(gpu, corpus, packed, R, per, t, range_=0, base=0):
    """the single-recording call on every row of the block in turn -> (keys uint64 [R, per], lengths uint32 [R, per])"""
    rows = packed.reshape(R, per, 32)
    keys = gpu.full((R, per), POISON, dtype=gpu.int64, device="cuda")
    lengths = gpu.full((R, per), POISON32, dtype=gpu.int32, device="cuda")
    for r in range(R):
        corpus.recording_timeline_keys_device(packed=rows[r], per_query=per, threshold=t, range_=range_, index_base=base, keys_out=keys[r],
                                              lengths_out=lengths[r])
    gpu.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64), lengths.cpu().numpy().view(np.uint32)


def _same(got, want):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    if got[1] is not None:
        assert np.array_equal(got[1], want[1])


def _plan(lb, m, R, per, limit=0):
    return lb.debug_timeline_batch_plan(R, per, int(m["lengths"].min()), int(m["lengths"].max()), N_CASE, limit)


def _scratch_bytes(entries, tiles):
    """the header's single-call formula"""
    return -(-entries // WALK) * tiles * 126 * 8


# ---- 1. forms and tiles, plants at the seams, no leak from a neighbour ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_rows_equal_the_reference_and_the_single_call(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    form, R, per = CASES[name]
    plan = _plan(lb, m, R, per)
    assert plan["form"] == form and plan["tiles"] == -(-per // TILE) and plan["recordings_per_pass"] == R
    assert form == FORM_S or (R * plan["tiles"]) % 4 != 0         # form W: the last group of four global tiles is partial
    for t in (T_HIGH, T_LOW):
        want = _want(m, name, t)
        got = _batch(gpu, m["corpus"], m["dev"][name], R, per, t)
        _same(got, want)
        _same(got, _single(gpu, m["corpus"], m["dev"][name], R, per, t))
        for plants, entry in ((PLANTS_22, E22), (PLANTS_17, E17)):
            for r, o in plants[name]:
                assert got[0][r, o] == (ONE << 32) | (0xFFFFFFFF - entry) and got[1][r, o] == len(m["entries"][entry]), (name, r, o)
        # the straddling 22: in the packed block it lies verbatim at the last 11 offsets of recording r and the first 11 of r + 1;
        # no recording holds it, the reference has no cell of 1.0 there, and neither has the device
        r = STRADDLE[name]
        for keys, lengths in (want, got):
            idx, sc = timeline_ref.decode(keys[r])
            tail = slice(per - 21, per)                           # where a 22 that read on into recording r + 1 would start
            assert E22 not in idx[tail] and not np.any((sc[tail] == 1.0) & (lengths[r, tail] > 11)), name
    low = _want(m, name, T_LOW)[0]
    assert 2 * np.count_nonzero(low) > low.size                   # at the low threshold most offsets have a noise winner


def test_the_shapes_are_the_seams(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    assert len(m["entries"]) == 2 * WALK + 5
    assert [o for _r, o in PLANTS_22["w300"][:2]] == [125, 126] and [o for _r, o in PLANTS_22["s525"][:3]] == [125, 126, 503]
    for name, (_form, R, per) in CASES.items():
        last = [(r, o) for r, o in PLANTS_22[name] if o == per - 22]
        assert last or name == "s525"
        for r, o in last:                                         # the last legal offset of recording r, offset 0 of r + 1
            assert (r + 1, 0) in PLANTS_22[name]
    assert PLANTS_22["s525"][2:] == [(1, GROUP - 1), (2, 0)] and PLANTS_17["s525"] == [(2, GROUP)]


# ---- 2. options -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w300", "s525"])
def test_options(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"], m["dev"][name]
    zero = _batch(gpu, corpus, packed, R, per, T_LOW)
    # a range below the sub-fingerprint length: the masked instances
    for range_ in (64, 199):
        _same(_batch(gpu, corpus, packed, R, per, T_LOW, range_=range_), _want(m, name, T_LOW, range_))
    # an index base
    for base in (1000, (1 << 32) - N_CASE):
        got = _batch(gpu, corpus, packed, R, per, T_LOW, base=base)
        _same(got, _want(m, name, T_LOW, base=base))
        assert np.array_equal(got[0][got[0] != 0] + np.uint64(base), zero[0][zero[0] != 0]) and np.array_equal(got[1], zero[1])
        idx, sc, ln = lb.decode_timeline_batch_keys(got[0].view(np.int64), got[1], base)
        assert idx.shape == sc.shape == ln.shape == (R, per)
        for r in range(R):
            one = lb.decode_timeline_keys(got[0][r].view(np.int64), got[1][r], base)
            assert all(np.array_equal(a, b) for a, b in zip((idx[r], sc[r].view(np.uint32), ln[r]), (one[0], one[1].view(np.uint32), one[2])))
            assert np.array_equal(idx[r], timeline_ref.decode(zero[0][r])[0])
    with pytest.raises(lb.LBAudioDetectiveError) as err:
        _batch(gpu, corpus, packed, R, per, T_LOW, base=(1 << 32) - N_CASE + 1)
    assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    # without lengths: the same keys
    _same(_batch(gpu, corpus, packed, R, per, T_LOW, want_lengths=False), (zero[0], None))
    # a threshold above 1 is legal and matches nothing
    above = _batch(gpu, corpus, packed, R, per, 1.5)
    assert not above[0].any() and not above[1].any()


def test_the_form_changes_nothing(lb, gpu, oracle):
    """form S forced where the plan takes form W"""
    m = _module(lb, gpu, oracle)
    try:
        for name in ("w100", "w129", "w300"):
            _form, R, per = CASES[name]
            lb.debug_set_timeline_batch_form(True)
            assert _plan(lb, m, R, per)["form"] == FORM_S
            _same(_batch(gpu, m["corpus"], m["dev"][name], R, per, T_LOW), _want(m, name, T_LOW))
            lb.debug_set_timeline_batch_form(False)
            assert _plan(lb, m, R, per)["form"] == FORM_W
    finally:
        lb.debug_set_timeline_batch_form(False)


# ---- 3. passes and chunks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w300", "s525"])
def test_passes_and_chunks_change_nothing(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    _form, R, per = CASES[name]
    corpus, packed = m["corpus"], m["dev"][name]
    tiles = -(-per // TILE)
    whole, block = _scratch_bytes(N_CASE, tiles), _scratch_bytes(WALK, tiles)
    assert whole == 3 * block
    try:
        corpus.set_join_scratch_limit(0)
        one = {t: _batch(gpu, corpus, packed, R, per, t) for t in (T_HIGH, T_LOW)}
        for t in one:
            _same(one[t], _want(m, name, t))
        # (a) several passes of recordings, the last one partial; (b) one recording per pass, several entry chunks, the last partial
        for limit, rpp, chunk in ((2 * whole + 3, 2, 3 * WALK), (whole, 1, 3 * WALK), (whole - 1, 1, 2 * WALK), (block, 1, WALK)):
            plan = _plan(lb, m, R, per, limit)
            assert (plan["recordings_per_pass"], plan["entries_per_chunk"]) == (rpp, chunk) and plan["scratch_bytes"] <= limit
            assert R % rpp != 0 or rpp == 1
            corpus.set_join_scratch_limit(limit)
            for t in one:
                _same(_batch(gpu, corpus, packed, R, per, t), one[t])
            _same(_batch(gpu, corpus, packed, R, per, T_LOW, want_lengths=False), (one[T_LOW][0], None))
        # a limit below one block of ONE recording
        corpus.set_join_scratch_limit(block - 1)
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            _batch(gpu, corpus, packed, R, per, T_LOW)
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    finally:
        corpus.set_join_scratch_limit(0)


# ---- 4. the second trip of both forms' grid-stride loops ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w300", "s525"])
def test_second_trips(lb, gpu, oracle, name):
    m = _module(lb, gpu, oracle)
    form, R, per = CASES[name]
    tiles = -(-per // TILE)
    units = 3 * (-(-(R * tiles) // 4) if form == FORM_W else R * -(-tiles // 4))
    want = _want(m, name, T_LOW)
    try:
        for ceiling in (1, 4):
            assert ceiling < units
            lb.debug_set_grid_ceiling(ceiling)
            before = lb.debug_grid_ceiling()[1]
            _same(_batch(gpu, m["corpus"], m["dev"][name], R, per, T_LOW), want)
            assert lb.debug_grid_ceiling()[1] > before
    finally:
        lb.debug_set_grid_ceiling(0)
    assert lb.debug_grid_ceiling()[0] == 0


# ---- 5. more entry blocks than one level of the fold takes ----------------------------------------------------------------------------------------------
def test_two_level_fold(lb, gpu, oracle):
    """33 x 128 + 5 entries of 1 .. 8 sub-fingerprints, two recordings, against the single call; form W, form S forced, and form S
    by shape"""
    n = (FOLD_ROWS + 1) * WALK + 5
    counts = np.random.default_rng(3).integers(1, 9, n)
    ent = _random(oracle, 515, counts)
    corpus = _ragged(lb, gpu, oracle, ent)
    for per, forms in ((300, (FORM_W, FORM_S)), (525, (FORM_S,))):
        block = oracle.synth_ragged_entries(516 + per, 0, np.array([2 * per], np.uint32), L).reshape(2, per, L).copy()
        block[0, 40:40 + len(ent[n - 2])] = ent[n - 2]            # a plant in the last, partial block
        block[1, TILE:TILE + len(ent[0])] = ent[0]
        packed = gpu.from_numpy(_packed(oracle, block.reshape(-1, L))).cuda()
        want = _single(gpu, corpus, packed, 2, per, T_LOW)
        idx0, sc0 = timeline_ref.decode(want[0][0])
        assert sc0[40] == 1.0 and timeline_ref.decode(want[0][1])[1][TILE] == 1.0 and idx0.max() > FOLD_ROWS * WALK
        try:
            for form in forms:
                lb.debug_set_timeline_batch_form(form == FORM_S)
                assert lb.debug_timeline_batch_plan(2, per, int(counts.min()), int(counts.max()), n)["form"] == form
                _same(_batch(gpu, corpus, packed, 2, per, T_LOW), want)
        finally:
            lb.debug_set_timeline_batch_form(False)


# ---- 6. one recording: the single call ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 17, 700])
def test_one_recording_is_the_single_call(lb, gpu, oracle, per):
    m = _module(lb, gpu, oracle)
    q = _random(oracle, 900 + per, [per])[0]
    if per == 700:
        q[600:622] = m["entries"][E22]
    elif per == 17:
        q[:] = m["entries"][E17]
    packed = gpu.from_numpy(_packed(oracle, q)).cuda()
    for t in (T_HIGH, T_LOW):
        got = _batch(gpu, m["corpus"], packed, 1, per, t)
        _same(got, _single(gpu, m["corpus"], packed, 1, per, t))
        want = timeline_ref.timeline(q, m["entries"], t)
        _same(got, (want[0][None], want[1][None]))
    if per == 700:
        assert got[0][0, 600] >> np.uint64(32) == ONE and got[1][0, 600] == 22
    if per == 17:
        assert got[0][0, 0] == (ONE << 32) | (0xFFFFFFFF - E17)


# ---- 7. nothing takes part; refusals that need the corpus ----------------------------------------------------------------------------------------------------
def test_nothing_takes_part(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    packed = m["dev"]["w100"]
    longer = _ragged(lb, gpu, oracle, _random(oracle, 31, [101, 130, 140]))
    empty = lb.Corpus.ragged(L, 4, 16)
    for corpus in (longer, empty):
        for want_lengths in (True, False):
            keys, lengths = _batch(gpu, corpus, packed, 5, 100, T_LOW, want_lengths=want_lengths)
            assert not keys.any() and (lengths is None or not lengths.any())


def test_refusals(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    packed = m["dev"]["w100"]
    cap = 1024
    above = _ragged(lb, gpu, oracle, _random(oracle, 5, [3, cap + 1, 2]))
    for corpus in (lb.Corpus(L, 4, 8), above):                    # a uniform corpus; an entry above the cap
        keys = gpu.full((5, 100), POISON, dtype=gpu.int64, device="cuda")
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            corpus.recording_timeline_batch_keys_device(packed, 5, 100, T_LOW, keys_out=keys, want_lengths=False)
        assert err.value.status == bad
        gpu.cuda.synchronize()
        assert bool((keys == POISON).all())                       # a refused call writes nothing


# ---- 8. two calls in a row on two streams --------------------------------------------------------------------------------------------------------------------
def test_two_streams_in_a_row(lb, gpu, oracle):
    m = _module(lb, gpu, oracle)
    corpus = m["corpus"]
    names = ("s525", "w300")
    streams = [gpu.cuda.Stream(), gpu.cuda.Stream()]
    outs = []
    for s, name in zip(streams, names):                           # the second call is made while the first may still run
        _form, R, per = CASES[name]
        keys = gpu.full((R, per), POISON, dtype=gpu.int64, device="cuda")
        lengths = gpu.full((R, per), POISON32, dtype=gpu.int32, device="cuda")
        s.wait_stream(gpu.cuda.current_stream())
        corpus.recording_timeline_batch_keys_device(m["dev"][name], R, per, T_LOW, keys_out=keys, lengths_out=lengths, stream=s)
        outs.append((keys, lengths))
    for s in streams:
        s.synchronize()
    for (keys, lengths), name in zip(outs, names):
        _same((keys.cpu().numpy().view(np.uint64), lengths.cpu().numpy().view(np.uint32)), _want(m, name, T_LOW))


# ---- 9. the stream bank's timeline -----------------------------------------------------------------------------------------------------------------------------
def test_stream_bank_timeline(lb, gpu, oracle):
    """three channels of test_gpu_stream_bank.py's pruned configuration (its generic one gives sub-fingerprints without a set
    Boolean, whose cells are 0); the corpus holds random entries and, per channel, rows [total - 15, total - 5) of its own
    sub-fingerprints: window_device then the single call per channel, and the planted spans score 1.0 at offset 5 of a window of 20"""
    rate, window, stride, bands, length = 44100, 1024, 64, 32, 200
    hop, frames, n = 128 * stride, 23, 20
    cfg = oracle.Config(rate, window, stride, bands, length)
    sig = [oracle.synth_clip(0x53424B31, c, rate, window + frames * hop + 7) for c in range(3)]
    ref = [oracle.fingerprint_pcm(s, cfg) for s in sig]
    assert all(r.shape == (frames, length) and r.any(axis=1).all() for r in ref)
    det =lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
    bank = lb.StreamBank(det, 3, 24)
    counts = [s.size for s in sig]
    bank.push_device(gpu.from_numpy(np.concatenate(sig).astype(np.float32)).cuda(), counts)
    assert bank.totals().tolist() == [frames] * 3
    ent = _random(oracle, 61, np.random.default_rng(4).integers(1, 16, 30), length)
    planted = {}
    for c in range(3):
        planted[c] = len(ent)
        ent.append(ref[c][frames - 15:frames - 5].copy())
    corpus = _ragged(lb, gpu, oracle, ent, length)
    channels = [2, 0, 1]
    stream = gpu.cuda.Stream()
    stream.wait_stream(gpu.cuda.current_stream())
    keys, lengths = bank.timeline(corpus, channels, n, T_LOW, stream=stream)
    stream.synchronize()
    assert keys.shape == (3, n) and lengths.shape == (3, n) and keys.dtype == gpu.int64 and lengths.dtype == gpu.int32
    got = (keys.cpu().numpy().view(np.uint64), lengths.cpu().numpy().view(np.uint32))
    win = bank.window_device(channels, n)
    gpu.cuda.synchronize()
    assert np.array_equal(lb.unpack_packed(win.cpu().numpy(), length).reshape(3, n, length), np.stack([ref[c][frames - n:] for c in channels]))
    _same(got, _single(gpu, corpus, win.reshape(3 * n, 32), 3, n, T_LOW))
    want = [timeline_ref.timeline(ref[c][frames - n:], ent, T_LOW) for c in channels]
    _same(got, (np.stack([k for k, _ in want]), np.stack([x for _, x in want])))
    for j, c in enumerate(channels):
        assert got[0][j, 5] == (ONE << 32) | (0xFFFFFFFF - planted[c]) and got[1][j, 5] == 10
    keys2, none = bank.timeline(corpus, channels, n, T_LOW, want_lengths=False)
    gpu.cuda.synchronize()
    assert none is None and np.array_equal(keys2.cpu().numpy().view(np.uint64), got[0])
