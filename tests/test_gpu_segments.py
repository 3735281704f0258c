"""GPU tests of the recording segments call (LBAudioDetectiveTimelineSegmentsFromKeysDevice, k_segments.hip,
timeline_segments_device, Corpus.recording_segments_batch_keys_device, StreamBank.segments).  Every output word -- starts, keys,
lengths, counts, the zeros behind the spans -- is compared with BOTH host statements of the greedy, row by row:
timeline_ref.segments and lbaudiodetective_amd.timeline_segments (which must agree with each other first); keys are compared as
integers, nothing needs a tolerance.  Output buffers are filled with 0xFF bytes before every call.

timeline_ref.segments takes every non-zero key as a candidate, also one of length 0, which the timeline calls never write; the
call's contract (and timeline_segments) leave such an offset out, so the reference is given the keys with those offsets zeroed.
Score words are drawn from the positive finite floats, as the timeline calls write them: timeline_segments orders by the decoded
score, the device by the key, and the two orders are the same exactly there."""
import numpy as np
import pytest

import timeline_ref

pytestmark = pytest.mark.gpu

L = 200
T_HIGH, T_LOW = 0.7, 0.3
ONE = int(np.float32(1.0).view(np.uint32))


def _key(score, index):
    return (int(np.float32(score).view(np.uint32)) << 32) | (0xFFFFFFFF - int(index))


def _random_keys(rng, n):
    """distinct-looking keys: score words of floats in [0.125, 1), entries 0 .. 999"""
    hi = rng.integers(0x3E000000, 0x3F800000, n).astype(np.uint64)
    return (hi << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - rng.integers(0, 1000, n).astype(np.uint64))


def _want(lb, keys, lengths, cap):
    """(starts uint32 [R, cap], keys uint64 [R, cap], lengths uint32 [R, cap], counts uint32 [R]) from the two host references"""
    keys = np.asarray(keys, np.uint64).reshape(-1, np.shape(keys)[-1])
    lengths = np.asarray(lengths, np.uint32).reshape(keys.shape)
    R = keys.shape[0]
    st, ks, ln = np.zeros((R, cap), np.uint32), np.zeros((R, cap), np.uint64), np.zeros((R, cap), np.uint32)
    counts = np.zeros(R, np.uint32)
    for r in range(R):
        a = timeline_ref.segments(np.where(lengths[r] != 0, keys[r], 0).astype(np.uint64), lengths[r])
        b = lb.timeline_segments(*lb.decode_timeline_keys(keys[r].view(np.int64), lengths[r]))
        assert [x[0] for x in a] == b[0].tolist() and [x[1] for x in a] == b[1].tolist() and [x[3] for x in a] == b[3].tolist()
        assert [int(np.float32(x[2]).view(np.uint32)) for x in a] == b[2].view(np.uint32).tolist()
        counts[r] = len(a)
        m = min(len(a), cap)
        st[r, :m] = b[0][:m]
        ks[r, :m] = keys[r][b[0][:m]]
        ln[r, :m] = b[3][:m]
    return st, ks, ln, counts


def _run(lb, gpu, keys, lengths, cap, want_lengths=True, stream=None):
    """one call into 0xFF-filled buffers -> (starts, keys, lengths or None, counts) as numpy, 2-D"""
    keys = np.asarray(keys, np.uint64).reshape(-1, np.shape(keys)[-1])
    lengths = np.asarray(lengths, np.uint32).reshape(keys.shape)
    R = keys.shape[0]
    dk = gpu.from_numpy(keys.view(np.int64).copy()).cuda()
    dl = gpu.from_numpy(lengths.view(np.int32).copy()).cuda()
    st = gpu.full((R, cap), -1, dtype=gpu.int32, device="cuda")
    ks = gpu.full((R, cap), -1, dtype=gpu.int64, device="cuda")
    ln = gpu.full((R, cap), -1, dtype=gpu.int32, device="cuda") if want_lengths else None
    cn = gpu.full((R,), -1, dtype=gpu.int32, device="cuda")
    if stream is not None:
        stream.wait_stream(gpu.cuda.current_stream())
    got = lb.timeline_segments_device(dk, dl, cap, starts_out=st, keys_out=ks, lengths_out=ln, counts_out=cn, want_lengths=want_lengths,
                                      stream=stream)
    assert got[0] is st and got[1] is ks and got[2] is ln and got[3] is cn
    (stream or gpu.cuda.current_stream()).synchronize()
    return (st.cpu().numpy().view(np.uint32), ks.cpu().numpy().view(np.uint64), ln.cpu().numpy().view(np.uint32) if want_lengths else None,
            cn.cpu().numpy().view(np.uint32))


def _same(got, want):
    assert np.array_equal(got[3], want[3]), (got[3], want[3])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if got[2] is not None:
        assert np.array_equal(got[2], want[2])


def _check(lb, gpu, keys, lengths, cap, **kw):
    want = _want(lb, keys, lengths, cap)
    _same(_run(lb, gpu, keys, lengths, cap, **kw), want)
    return want


def _row(per, spans):
    """a row of `per` offsets from (offset, score, entry, length) candidates"""
    keys, lengths = np.zeros(per, np.uint64), np.zeros(per, np.uint32)
    for o, score, entry, n in spans:
        keys[o], lengths[o] = _key(score, entry), n
    return keys, lengths


def _starts(want, r=0):
    return want[0][r, :min(int(want[3][r]), want[0].shape[1])].tolist()


# ---- 1. hand-made rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 2, 63, 64, 65, 127, 129, 1000])
def test_lengths_that_are_no_power_of_two(lb, gpu, per):
    rng = np.random.default_rng(per)
    # nothing
    want = _check(lb, gpu, np.zeros(per, np.uint64), rng.integers(0, 5, per).astype(np.uint32), 3)
    assert want[3][0] == 0
    # every offset a candidate of length 1: all of them are spans; the cut and the zero fill
    keys = _random_keys(rng, per)
    for cap in sorted({1, max(1, per - 1), per, per + 3}):
        want = _check(lb, gpu, keys, np.ones(per, np.uint32), cap)
        assert want[3][0] == per and _starts(want) == list(range(min(per, cap)))
    # a mix
    keys = np.where(rng.random(per) < 0.5, _random_keys(rng, per), 0).astype(np.uint64)
    _check(lb, gpu, keys, rng.integers(0, 9, per).astype(np.uint32), per)


def test_ties_go_to_the_lower_offset(lb, gpu):
    k = 0.5, 7
    keys, lengths = _row(100, [(10, *k, 5), (12, *k, 5), (14, *k, 5), (15, *k, 5), (40, *k, 5), (41, *k, 5), (99, *k, 5)])
    want = _check(lb, gpu, keys, lengths, 8)
    assert _starts(want) == [10, 15, 40, 99]
    keys, lengths = np.full(100, _key(*k), np.uint64), np.full(100, 3, np.uint32)
    want = _check(lb, gpu, keys, lengths, 100)
    assert _starts(want) == list(range(0, 100, 3))


def test_a_key_of_length_zero_is_no_segment(lb, gpu):
    keys, lengths = _row(50, [(5, 0.9, 1, 0), (4, 0.5, 2, 3), (20, 0.8, 3, 0), (49, 0.7, 4, 0)])
    want = _check(lb, gpu, keys, lengths, 4)
    assert _starts(want) == [4]
    keys, lengths = _row(50, [(o, 0.9, o, 0) for o in range(50)])
    assert _check(lb, gpu, keys, lengths, 4)[3][0] == 0


def test_spans_that_touch_or_cross_a_mask_word(lb, gpu):
    per = 130
    rows = [[(60, 0.5, 1, 4), (64, 0.6, 2, 6)],                       # 63 | 64: touch
            [(60, 0.6, 1, 5), (65, 0.5, 2, 5)],                       # 64 | 65: touch
            [(60, 0.5, 1, 5), (64, 0.6, 2, 6)],                       # one offset shared: the better one stays
            [(60, 0.9, 1, 11), (63, 0.8, 2, 1), (64, 0.8, 3, 1), (70, 0.8, 4, 2), (71, 0.7, 5, 1), (59, 0.6, 6, 1), (58, 0.5, 7, 3)],
            [(0, 0.5, 1, 64), (64, 0.5, 2, 64), (128, 0.5, 3, 64), (127, 0.9, 4, 1)]]
    built = [_row(per, r) for r in rows]
    keys, lengths = np.stack([k for k, _ in built]), np.stack([n for _, n in built])
    want = _check(lb, gpu, keys, lengths, 6)
    assert [_starts(want, r) for r in range(5)] == [[60, 64], [60, 65], [64], [59, 60, 71], [0, 127, 128]]
    # a span of 1 024 offsets in a row of 1 100
    keys, lengths = _row(1100, [(50, 0.9, 1, 1024), (10, 0.5, 2, 40), (11, 0.6, 3, 40), (1073, 0.8, 4, 1), (1074, 0.4, 5, 1),
                                (600, 0.8, 6, 2), (49, 0.3, 7, 1), (1080, 0.2, 8, 1000)])
    want = _check(lb, gpu, keys, lengths, 8)
    assert _starts(want) == [10, 50, 1074, 1080]


def test_the_end_of_the_recording(lb, gpu):
    per = 77
    rows = [[(per - 5, 0.5, 1, 5), (per - 10, 0.4, 2, 5)],            # ends exactly at per, and one that touches it
            [(per - 3, 0.9, 1, 10), (per - 5, 0.5, 2, 5), (per - 8, 0.5, 3, 5)],       # clipped: it still blocks what it covers
            [(per - 1, 0.5, 1, 70000), (0, 0.4, 2, 70000)]]           # lengths that do not fit 16 bits
    built = [_row(per, r) for r in rows]
    want = _check(lb, gpu, np.stack([k for k, _ in built]), np.stack([n for _, n in built]), 4)
    assert [_starts(want, r) for r in range(3)] == [[per - 10, per - 5], [per - 8, per - 3], [per - 1]]
    assert want[2][1, 1] == 10 and want[2][2, 0] == 70000           # the length as it came


@pytest.mark.parametrize("span", [2, 3, 64])
def test_chains_of_overlapping_spans(lb, gpu, span):
    """every offset of 200 a candidate that overlaps its neighbours, the keys rising / falling with the offset: each acceptance
    depends on the one before it, right through the batches of 64"""
    per = 200
    rising = np.array([_key(0.25 + o / 512.0, 5) for o in range(per)], np.uint64)
    keys = np.stack([rising, rising[::-1].copy()])
    want = _check(lb, gpu, keys, np.full((2, per), span, np.uint32), per)
    assert _starts(want, 1) == list(range(0, per, span))
    assert _starts(want, 0) == sorted(range(per - 1, -1, -span))


def test_a_better_span_between_two_neighbours(lb, gpu):
    rows = [[(10, 0.5, 1, 10), (15, 0.9, 2, 10), (20, 0.6, 3, 10)],
            [(10, 0.5, 1, 5), (15, 0.9, 2, 10), (25, 0.6, 3, 10)],    # the neighbours only touch it
            [(10, 0.5, 1, 10), (15, 0.9, 2, 10), (20, 0.95, 3, 10)]]  # the right neighbour is better still: the middle goes
    built = [_row(40, r) for r in rows]
    want = _check(lb, gpu, np.stack([k for k, _ in built]), np.stack([n for _, n in built]), 3)
    assert [_starts(want, r) for r in range(3)] == [[15], [10, 15, 25], [10, 20]]


def test_the_longest_recording(lb, gpu):
    """per = 8192, the cap: random candidates, and every offset a span of its own"""
    per = 8192
    rng = np.random.default_rng(8192)
    keys = np.stack([np.where(rng.random(per) < 0.5, _random_keys(rng, per), 0).astype(np.uint64), _random_keys(rng, per)])
    lengths = np.stack([rng.integers(1, 71, per).astype(np.uint32), np.ones(per, np.uint32)])
    want = _check(lb, gpu, keys, lengths, per + 3)
    assert 100 < want[3][0] < per and want[3][1] == per
    with pytest.raises(lb.LBAudioDetectiveError) as err:
        _run(lb, gpu, np.zeros((1, per + 1), np.uint64), np.zeros((1, per + 1), np.uint32), 4)
    assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")


# ---- 2. batches ---------------------------------------------------------------------------------------------------------------
def test_neighbouring_recordings_do_not_meet(lb, gpu):
    """the last span of row r ends at per (or would pass it), row r + 1 has a candidate at offset 0"""
    per = 100
    built = [_row(per, [(0, 0.4, r, 7), (per - 6, 0.9, 10 + r, 6 if r % 2 else 60), (50, 0.5, 20 + r, 3)]) for r in range(5)]
    want = _check(lb, gpu, np.stack([k for k, _ in built]), np.stack([n for _, n in built]), 5)
    assert all(_starts(want, r) == [0, 50, per - 6] for r in range(5))


def _sweep(seed, R, per, kinds, density):
    rng = np.random.default_rng(seed)
    if kinds:
        pool = _random_keys(rng, kinds)
        keys = pool[rng.integers(0, kinds, (R, per))]
    else:
        keys = _random_keys(rng, R * per).reshape(R, per)
    keys = np.where(rng.random((R, per)) < density, keys, 0).astype(np.uint64)
    return keys, rng.integers(1, 71, (R, per)).astype(np.uint32)


def test_the_grid_changes_nothing(lb, gpu):
    keys, lengths = _sweep(70, 70, 90, 0, 0.5)
    want = _want(lb, keys, lengths, 20)
    _same(_run(lb, gpu, keys, lengths, 20), want)
    try:
        for ceiling in (1, 4):
            lb.debug_set_grid_ceiling(ceiling)
            before = lb.debug_grid_ceiling()[1]
            _same(_run(lb, gpu, keys, lengths, 20), want)
            assert lb.debug_grid_ceiling()[1] > before
    finally:
        lb.debug_set_grid_ceiling(0)
    assert lb.debug_grid_ceiling()[0] == 0


def test_two_streams_and_no_lengths(lb, gpu):
    keys, lengths = _sweep(71, 9, 129, 6, 0.5)
    want = _want(lb, keys, lengths, 16)
    streams = [gpu.cuda.Stream(), gpu.cuda.Stream()]
    dk = gpu.from_numpy(keys.view(np.int64).copy()).cuda()
    dl = gpu.from_numpy(lengths.view(np.int32).copy()).cuda()
    outs = []
    for s in streams:                                             # the second call is made while the first may still run
        s.wait_stream(gpu.cuda.current_stream())
        outs.append(lb.timeline_segments_device(dk, dl, 16, stream=s))
    for s in streams:
        s.synchronize()
    for st, ks, ln, cn in outs:
        assert st.shape == (9, 16) and ks.dtype == gpu.int64 and ln.dtype == gpu.int32 and cn.shape == (9,)
        _same((st.cpu().numpy().view(np.uint32), ks.cpu().numpy().view(np.uint64), ln.cpu().numpy().view(np.uint32),
               cn.cpu().numpy().view(np.uint32)), want)
    # outLengths NULL: the other outputs are the same
    got = _run(lb, gpu, keys, lengths, 16, want_lengths=False)
    assert got[2] is None
    _same(got, want)
    # one recording as 1-D tensors, and the decoder
    one = lb.timeline_segments_device(dk[3], dl[3], 16)
    gpu.cuda.synchronize()
    assert one[0].shape == (16,) and one[3].dim() == 0 and int(one[3]) == want[3][3]
    dec = lb.decode_segments(*one)
    ref = lb.timeline_segments(*lb.decode_timeline_keys(keys[3].view(np.int64), lengths[3]))
    m = min(16, len(ref[0]))
    assert all(a.dtype == b.dtype and np.array_equal(a, b[:m]) for a, b in zip(dec, ref))
    # ... into rows the caller gives, as [capacity] or as [1, capacity]: the row comes back either way
    for shape in ((16,), (1, 16)):
        st, ks, ln = (gpu.full(shape, -1, dtype=dt, device="cuda") for dt in (gpu.int32, gpu.int64, gpu.int32))
        cn = gpu.full((1,), -1, dtype=gpu.int32, device="cuda")
        row = lb.timeline_segments_device(dk[3], dl[3], 16, starts_out=st, keys_out=ks, lengths_out=ln, counts_out=cn)
        gpu.cuda.synchronize()
        assert row[0].shape == row[1].shape == row[2].shape == (16,) and row[3].dim() == 0
        assert all(gpu.equal(a, b) for a, b in zip(row, one)) and gpu.equal(row[0], st.reshape(-1))
    # keys and lengths are integers of 64 and 32 bits, not merely words of that size
    for bad_k, bad_l in ((dk.double(), dl), (dk, dl.float()), (dk.int(), dl), (dk, dl.long())):
        with pytest.raises(ValueError):
            lb.timeline_segments_device(bad_k, bad_l, 16)


# ---- 3. random sweep ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [6, 0])
@pytest.mark.parametrize("density", [0.05, 0.5, 1.0])
def test_random_sweep(lb, gpu, kinds, density):
    keys, lengths = _sweep(1000 + kinds + int(100 * density), 64, 300, kinds, density)
    want = _check(lb, gpu, keys, lengths, 300)
    assert want[3].min() > 0 and want[3].max() < 300


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
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


def _host_segments(lb, keys, lengths, cap, base=0):
    """the host path on a timeline's keys and lengths (device tensors [R, per]): decode, then timeline_segments per row, laid out
    as the device call lays its rows out"""
    k = keys.cpu().numpy().view(np.uint64)
    idx, sc, ln = lb.decode_timeline_batch_keys(keys, lengths, base)
    R = k.shape[0]
    st, ks, lo = np.zeros((R, cap), np.uint32), np.zeros((R, cap), np.uint64), np.zeros((R, cap), np.uint32)
    counts = np.zeros(R, np.uint32)
    for r in range(R):
        s = lb.timeline_segments(idx[r], sc[r], ln[r])
        counts[r] = len(s[0])
        m = min(cap, len(s[0]))
        st[r, :m], ks[r, :m], lo[r, :m] = s[0][:m], k[r][s[0][:m]], s[3][:m]
    return st, ks, lo, counts


def _np(out):
    return (out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy().view(np.uint64), out[2].cpu().numpy().view(np.uint32),
            out[3].cpu().numpy().view(np.uint32))


def test_corpus_segments_end_to_end(lb, gpu, oracle):
    """300 entries of 20 .. 70 sub-fingerprints, 6 recordings of 256 with entries planted verbatim: the one call equals the
    timeline batch call followed by the host's timeline_segments per row, the planted entries are spans with score 1.0, and the
    key block goes into ids_from_keys_device as it is"""
    R, per, cap, base = 6, 256, 24, 1000
    counts = np.random.default_rng(5).integers(20, 71, 300)
    counts[0], counts[1] = 20, 70
    ent = _random(oracle, 2024, counts)
    corpus = _ragged(lb, gpu, oracle, ent)
    ids = (np.arange(300, dtype=np.uint64) * np.uint64(7)) + np.uint64(1 << 40)
    corpus.set_entry_ids(ids)
    block = oracle.synth_ragged_entries(99, 0, np.array([R * per], np.uint32), L).reshape(R, per, L).copy()
    plants = [(0, 0, 17), (0, 100, 1), (1, per - len(ent[33]), 33), (2, 0, 250), (2, len(ent[250]), 251), (4, 60, 0), (5, 130, 299)]
    for r, o, e in plants:
        assert o + len(ent[e]) <= per
        block[r, o:o + len(ent[e])] = ent[e]
    packed = gpu.from_numpy(_packed(oracle, block.reshape(-1, L))).cuda()
    stream = gpu.cuda.Stream()
    for t in (T_HIGH, T_LOW):
        keys, lengths = corpus.recording_timeline_batch_keys_device(packed, R, per, t, index_base=base)
        gpu.cuda.synchronize()
        want = _host_segments(lb, keys, lengths, cap, base)
        stream.wait_stream(gpu.cuda.current_stream())
        out = corpus.recording_segments_batch_keys_device(packed, R, per, t, cap, index_base=base, stream=stream)
        stream.synchronize()
        got = _np(out)
        _same(got, want)
        assert out[0].shape == (R, cap) and out[3].shape == (R,) and 0 < got[3].max() <= cap
        dec = lb.decode_segments(*out, index_base=base)
        for r, o, e in plants:
            st, idx, sc, ln = dec[r]
            at = st.tolist().index(o)
            assert (idx[at], sc[at], ln[at]) == (e, 1.0, len(ent[e])), (r, o, e)
        got_ids = corpus.ids_from_keys_device(out[1], index_base=base).cpu().numpy().view(np.uint64).reshape(R, cap)
        for r in range(R):
            m = int(got[3][r])
            assert np.array_equal(got_ids[r, :m], ids[dec[r][1]]) and not got_ids[r, m:].any()
    # the timeline's keys and lengths in between belong to the call's stream: blocks of their sizes made and filled on the
    # current stream straight behind the call, while the side stream still runs, are not theirs
    gpu.cuda.synchronize()
    out = corpus.recording_segments_batch_keys_device(packed, R, per, T_LOW, cap, index_base=base, stream=stream)
    junk = [gpu.full((R, per), -1, dtype=dt, device="cuda") for dt in (gpu.int64, gpu.int32) for _ in range(4)]
    stream.synchronize()
    gpu.cuda.synchronize()
    _same(_np(out), want)
    assert all(bool((j == -1).all()) for j in junk)


def test_stream_bank_segments(lb, gpu, oracle):
    """three channels of test_gpu_stream_bank.py's pruned configuration; the corpus holds random entries and, per channel, rows
    [total - 15, total - 5) of its own sub-fingerprints: StreamBank.segments equals window_device, the timeline batch call and the
    host's timeline_segments per row, and the planted span starts at offset 5 of a window of 20"""
    rate, window, stride, bands, length = 44100, 1024, 64, 32, 200
    hop, frames, n, cap = 128 * stride, 23, 20, 6
    cfg = oracle.Config(rate, window, stride, bands, length)
    sig = [oracle.synth_clip(0x53424B31, c, rate, window + frames * hop + 7) for c in range(3)]
    ref = [oracle.fingerprint_pcm(s, cfg) for s in sig]
    det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
    bank = lb.StreamBank(det, 3, 24)
    bank.push_device(gpu.from_numpy(np.concatenate(sig).astype(np.float32)).cuda(), [s.size for s in sig])
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
    out = bank.segments(corpus, channels, n, T_LOW, cap, stream=stream)
    stream.synchronize()
    win = bank.window_device(channels, n)
    keys, lengths = corpus.recording_timeline_batch_keys_device(win.reshape(3 * n, 32), 3, n, T_LOW)
    gpu.cuda.synchronize()
    _same(_np(out), _host_segments(lb, keys, lengths, cap))
    for j, (st, idx, sc, ln) in enumerate(lb.decode_segments(*out)):
        at = st.tolist().index(5)
        assert (idx[at], sc[at], ln[at]) == (planted[channels[j]], 1.0, 10)
