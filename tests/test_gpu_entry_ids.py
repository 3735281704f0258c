"""GPU tests of the entry ids (LBAudioDetectiveCorpusSetEntryIds[Device], ...GetEntryIds, ...HasEntryIds, ...IdsFromKeysDevice,
...KeysFromIdsDevice, and the ids' part in removal, save and load).  What is expected is always numpy on the test's own inputs:
the ids it set, compacted by the keep mask of a removal, looked up by position for keys and by "lowest index with that id" for
ids.  Everything is compared as integers.  Every device output is poison-filled before the call, with a poisoned pad behind what
the call may write that must still hold the poison afterwards."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"constexpr\s+uint32_t\s+kRemoveTileEntries\s*=\s*(\d+)\s*;",
                     open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_remove.hip")).read()).group(1))

POISON8 = 0xA5
POISON64 = -0x5A5A5A5A5A5A5A5B            # 0xA5A5A5A5A5A5A5A5 as int64
PAD = 9                                   # poisoned words behind what a call may write
SEED = 0x49445331
BASE = 1000003
L = 200
N_UNIFORM, N_SUB = 3000, 5
N_RAGGED = 700
ONE = np.uint64(0x3F800000) << np.uint64(32)          # the score word of KeysFromIds' keys: the bits of 1.0f
LOW = np.uint64(0xFFFFFFFF)
KINDS = ("uniform", "ragged")
COPY = 200                                # this entry is a copy of entry 7


# ---- the contract, restated ------------------------------------------------------------------------------------------------
def _make_ids(n, seed):
    """n ids from a fixed seed: distinct non-zero words (an odd multiplier permutes 64 bits), and then 1 and 2^64 - 1, a pair
    equal in the low and a pair equal in the high 32 bits, a run of sequential values, a run of multiples of 2^20, zeros, and
    duplicates at known indices.  Returns (ids, {duplicated id: its indices})."""
    rng = np.random.default_rng(seed)
    ids = (rng.permutation(n).astype(np.uint64) + np.uint64(1 << 33)) * np.uint64(0x9E3779B97F4A7C15)
    ids[0], ids[1] = 1, 0xFFFFFFFFFFFFFFFF
    ids[2], ids[3] = (7 << 32) | 0x12345678, (9 << 32) | 0x12345678
    ids[4], ids[5] = (0xDEADBEEF << 32) | 5, (0xDEADBEEF << 32) | 6
    ids[10:60] = 1000000 + np.arange(50, dtype=np.uint64)
    ids[60:110] = (np.arange(50, dtype=np.uint64) + np.uint64(1)) << np.uint64(20)
    ids[110:120] = 0
    ids[n - 3] = 0
    ids[130] = ids[131] = ids[20]
    ids[n - 1] = ids[70]
    ids[140] = ids[141] = 0x5555555555
    dups = {int(ids[20]): [20, 130, 131], int(ids[70]): [70, n - 1], 0x5555555555: [140, 141]}
    # the plan above is all there is: no other value occurs twice
    values, counts = np.unique(ids[ids != 0], return_counts=True)
    assert {int(v) for v in values[counts > 1]} == set(dups) and (ids == 0).sum() == 11
    return ids, dups


def _lowest(ids):
    """id -> the lowest index that has it (id 0 is no id)"""
    first = {}
    for e, v in enumerate(ids.tolist()):
        if v and v not in first:
            first[v] = e
    return first


def _expected_keys(wanted, ids, base):
    """KeysFromIds of the list `wanted` against a corpus whose entries have `ids`"""
    first = _lowest(ids)
    out = np.zeros(len(wanted), np.uint64)
    for i, v in enumerate(np.asarray(wanted, np.uint64).tolist()):
        if v in first:
            out[i] = ONE | (LOW - np.uint64(base + first[v]))
    return out


def _expected_ids(keys, ids, base):
    """IdsFromKeys of `keys` against a corpus whose entries have `ids` (None: a corpus without ids)"""
    keys = np.asarray(keys, np.uint64)
    out = np.zeros(len(keys), np.uint64)
    if ids is None:
        return out
    index = (LOW - (keys & LOW)).astype(np.int64) - base
    ok = (keys != 0) & (index >= 0) & (index < len(ids))
    out[ok] = ids[index[ok]]
    return out


def _keys_of(globals_, rng):
    """64-bit keys of a list of GLOBAL indices (-1: a zero key) with score words that must be ignored"""
    g = np.asarray(globals_, np.int64)
    score = rng.integers(1, 1 << 31, len(g)).astype(np.uint64) << np.uint64(32)
    keys = score | (LOW - np.where(g < 0, 0, g).astype(np.uint64))
    keys[g < 0] = 0
    return keys


def _dev64(gpu, a):
    return gpu.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def _call(gpu, fn, words, base):
    """one of the two list calls on `words` into a poisoned buffer -> the n words written; the pad behind them is checked here"""
    n = len(words)
    out = gpu.full((n + PAD,), POISON64, dtype=gpu.int64, device="cuda")
    got = fn(_dev64(gpu, words), index_base=base, out=out)
    assert got is out
    gpu.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[n:] == POISON64).all(), "words behind the output were written"
    return host[:n].view(np.uint64)


# ---- the two corpora -------------------------------------------------------------------------------------------------------
_MADE = {}


def _data(kind):
    """(bools of every sub-fingerprint, counts per entry, ids, duplicates), made once and left unchanged"""
    if kind not in _MADE:
        rng = np.random.default_rng(SEED + len(kind))
        if kind == "uniform":
            counts = np.full(N_UNIFORM, N_SUB, np.uint32)
        else:
            counts = rng.integers(1, 10, N_RAGGED).astype(np.uint32)
            counts[COPY] = counts[7]
        flat = rng.integers(0, 2, (int(counts.sum()), L), dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        flat[off[COPY]:off[COPY + 1]] = flat[off[7]:off[8]]           # a planted copy: a match besides the self-match
        ids, dups = _make_ids(len(counts), SEED)
        _MADE[kind] = (flat, counts, off, ids, dups)
    return _MADE[kind]


def _packed(oracle, bools):
    return np.ascontiguousarray(oracle.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _corpus(lb, gpu, oracle, kind, n=None, spare=40, with_ids=True):
    """the first n entries of the kind's data in a corpus with `spare` entries of room, their ids set (device form)"""
    flat, counts, off, ids, _ = _data(kind)
    n = len(counts) if n is None else n
    rows = gpu.from_numpy(_packed(oracle, flat[:off[n]])).cuda() if n else None
    if kind == "uniform":
        c = lb.Corpus(L, N_SUB, n + spare)
        if n:
            c.append_packed_device(rows.reshape(n, N_SUB, 32))
    else:
        c = lb.Corpus.ragged(L, n + spare, int(off[n]) + 9 * spare)
        if n:
            c.append_ragged_packed_device(rows, counts[:n])
    if with_ids and n:
        c.set_entry_ids(_dev64(gpu, ids[:n]))
    return c


def _rows(oracle, kind):
    flat, counts, off, _, _ = _data(kind)
    packed = _packed(oracle, flat)
    return [packed[off[e]:off[e + 1]] for e in range(len(counts))]


def _append_more(lb, gpu, oracle, c, kind, k):
    """k more entries (copies of the first k): an append knows nothing of ids"""
    flat, counts, off, _, _ = _data(kind)
    rows = gpu.from_numpy(_packed(oracle, flat[:off[k]])).cuda()
    if kind == "uniform":
        c.append_packed_device(rows.reshape(k, N_SUB, 32))
    else:
        c.append_ragged_packed_device(rows, counts[:k])


# ---- set / get -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_set_and_get(lb, gpu, oracle, kind):
    N = lb._native
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _, counts, _, ids, _ = _data(kind)
    n, spare = len(counts), 40
    c = _corpus(lb, gpu, oracle, kind, spare=spare, with_ids=False)
    gpu.cuda.synchronize()
    live = lb.debug_live_bytes()
    assert not c.has_entry_ids and not c.entry_ids().any() and len(c.entry_ids()) == n
    # an empty range does not turn ids on, in either form; a range beyond the count is refused and turns nothing on
    c.set_entry_ids(np.zeros(0, np.uint64))
    c.set_entry_ids(_dev64(gpu, ids[:0]), first=n)
    some = (N.UInt64 * 4)(1, 2, 3, 4)
    d_some = _dev64(gpu, [1, 2, 3, 4])
    assert c._L.LBAudioDetectiveCorpusSetEntryIds(c._ref, n - 3, 4, some) == bad
    assert c._L.LBAudioDetectiveCorpusSetEntryIdsDevice(c._ref, n - 3, 4, d_some.data_ptr(), None) == bad
    assert c._L.LBAudioDetectiveCorpusSetEntryIds(c._ref, n + 1, 0, None) == bad
    assert not c.has_entry_ids and lb.debug_live_bytes() == live
    # two disjoint ranges: the device form, then the host form
    cut = n // 3 + 1
    c.set_entry_ids(_dev64(gpu, ids[cut:]), first=cut)
    assert c.has_entry_ids
    got = c.entry_ids()
    assert not got[:cut].any() and np.array_equal(got[cut:], ids[cut:])
    c.set_entry_ids(ids[:cut])
    assert np.array_equal(c.entry_ids(), ids)
    assert np.array_equal(c.entry_ids(first=5, n=7), ids[5:12])
    gpu.cuda.synchronize()
    assert lb.debug_live_bytes() == (live[0] + 8 * (n + spare), live[1] + 8 * cut)      # the block of `capacity` words; the staging
    # refused with ids on: nothing changes
    assert c._L.LBAudioDetectiveCorpusSetEntryIds(c._ref, n - 3, 4, some) == bad
    assert c._L.LBAudioDetectiveCorpusSetEntryIdsDevice(c._ref, n - 3, 4, d_some.data_ptr(), None) == bad
    assert np.array_equal(c.entry_ids(), ids)
    # the words from the count to the capacity are zero, and so are the ids of entries appended later
    assert not c.entry_ids(first=n, n=spare).any()
    with pytest.raises(lb.LBAudioDetectiveError):
        c.entry_ids(first=n, n=spare + 1)
    _append_more(lb, gpu, oracle, c, kind, 11)
    assert len(c) == n + 11
    got = c.entry_ids()
    assert np.array_equal(got[:n], ids) and not got[n:].any()
    c.set_entry_ids([77, 78], first=n + 2)
    assert c.entry_ids(first=n, n=11).tolist() == [0, 0, 77, 78] + [0] * 7
    c.dispose()


# ---- the two lookups -------------------------------------------------------------------------------------------------------
def _hand_made_keys(n, base, rng):
    """a zero key, indices below and above the range, valid ones with score words that must be ignored"""
    inside = (rng.integers(0, n, 40) + base).tolist() + [base, base + n - 1, base + 110, base + 131]
    outside = [base + n, base + n + 1, 0xFFFFFFFF, 0xFFFFFFFE] + ([base - 1, 0, base // 2] if base else [])
    return _keys_of([-1] + outside[:2] + inside[:20] + [-1, -1] + outside[2:] + inside[20:] + [-1], rng)


def _check_ids_from_keys(lb, gpu, c, kind, fps):
    """-> everything the calls returned, for the comparison between grids"""
    _, counts, _, ids, _ = _data(kind)
    n = len(counts)
    rng = np.random.default_rng(5)
    seen = []
    for base in (0, BASE):
        # the key block of a real threshold batch, zero padded
        keys, cnt = c.query_batch_threshold_keys_device(fps, 0.95, 16, index_base=base)
        gpu.cuda.synchronize()
        block = keys.cpu().numpy().reshape(-1).view(np.uint64)
        assert (block == 0).any() and int(cnt.sum().item()) == (block != 0).sum() >= len(fps) + 1
        got = _call(gpu, c.ids_from_keys_device, block, base)
        assert np.array_equal(got, _expected_ids(block, ids, base)), (kind, base, "threshold keys")
        seen.append(got)
        made = _hand_made_keys(n, base, rng)
        got = _call(gpu, c.ids_from_keys_device, made, base)
        assert np.array_equal(got, _expected_ids(made, ids, base)), (kind, base, "hand-made keys")
        assert got.any() and not got.all()
        seen.append(got)
        # a key for every entry, shuffled, among keys of other entries: more than one workgroup's worth
        many = _keys_of(np.concatenate([rng.permutation(n) + base, [-1, base + n, -1]]), rng)
        got = _call(gpu, c.ids_from_keys_device, many, base)
        assert np.array_equal(got, _expected_ids(many, ids, base)), (kind, base, "a key for every entry")
        seen.append(got)
    assert len(_call(gpu, c.ids_from_keys_device, np.zeros(0, np.uint64), 0)) == 0
    return seen


def _wanted_lists(ids, rng):
    absent = np.array([3, 0xFFFFFFFFFFFFFFFE, (7 << 32) | 0x12345679, (8 << 32) | 0x12345678, 51 << 20, 1000050, 999999], np.uint64)
    assert not np.isin(absent, ids).any()

    def at(*where):                           # (a corpus emptied by a removal has no id to ask for)
        return ids[np.asarray(where) % len(ids)] if len(ids) else ids[:0]

    return {
        "every id, shuffled": ids[rng.permutation(len(ids))],
        "absent ids": absent,
        "zeros": np.zeros(5, np.uint64),
        "repeats": np.concatenate([at(20, 20, 130, 70, 70, 0, 1, 1), absent[:2], [np.uint64(0)], at(len(ids) - 1, 141, 140)]),
        "one": at(2),
        "none": ids[:0],
    }


def _check_keys_from_ids(gpu, c, ids, what, rows=None):
    """ids: the ids the corpus' entries have now -> everything the calls returned"""
    rng = np.random.default_rng(6)
    seen = []
    for base in (0, BASE):
        for name, wanted in _wanted_lists(ids, rng).items():
            got = _call(gpu, c.keys_from_ids_device, wanted, base)
            exp = _expected_keys(wanted, ids, base)
            assert np.array_equal(got, exp), (what, base, name, np.nonzero(got != exp)[0][:4])
            assert ((got == 0) | ((got >> np.uint64(32)) == np.uint64(0x3F800000))).all()
            seen.append(got)
    if rows is not None:                      # the output as it is names the entries for the gather
        wanted = _wanted_lists(ids, rng)["repeats"]
        keys = c.keys_from_ids_device(_dev64(gpu, wanted))
        packed, offsets = c.gather_keys_device(keys)
        first = _lowest(ids)
        picked = [rows[first[v]] if v in first else rows[0][:0] for v in wanted.tolist()]
        assert np.array_equal(offsets.cpu().numpy(), np.concatenate([[0], np.cumsum([len(p) for p in picked])]))
        assert np.array_equal(packed.cpu().numpy(), np.concatenate(picked))
    return seen


def _query_fps(lb, kind):
    flat, counts, off, _, _ = _data(kind)
    return [lb.Fingerprint.from_bools(flat[off[e]:off[e + 1]]) for e in (7, len(counts) // 2, len(counts) - 1)]


@pytest.mark.parametrize("kind", KINDS)
def test_ids_from_keys(lb, gpu, oracle, kind):
    c = _corpus(lb, gpu, oracle, kind)
    _check_ids_from_keys(lb, gpu, c, kind, _query_fps(lb, kind))
    c.dispose()


@pytest.mark.parametrize("kind", KINDS)
def test_keys_from_ids(lb, gpu, oracle, kind):
    _, _, _, ids, dups = _data(kind)
    c = _corpus(lb, gpu, oracle, kind)
    _check_keys_from_ids(gpu, c, ids, kind, rows=_rows(oracle, kind))
    # duplicates resolve to the lowest index, whichever of them is asked for
    for v, where in dups.items():
        got = _call(gpu, c.keys_from_ids_device, np.array([v], np.uint64), 0)
        assert int(LOW - (got[0] & LOW)) == min(where)
    c.dispose()


@pytest.mark.parametrize("kind", KINDS)
def test_counts_one_and_zero(lb, gpu, oracle, kind):
    _, _, _, ids, _ = _data(kind)
    one = _corpus(lb, gpu, oracle, kind, n=1)
    for base in (0, BASE):
        got = _call(gpu, one.keys_from_ids_device, np.array([ids[0], ids[1], 0, ids[0]], np.uint64), base)
        key = ONE | (LOW - np.uint64(base))
        assert got.tolist() == [key, 0, 0, key]
        got = _call(gpu, one.ids_from_keys_device, np.array([key, 0, key - np.uint64(1)], np.uint64), base)
        assert got.tolist() == [ids[0], 0, 0]
    one.dispose()
    empty = _corpus(lb, gpu, oracle, kind, n=0)
    assert not empty.has_entry_ids
    assert not _call(gpu, empty.keys_from_ids_device, ids[:9], 0).any()
    assert not _call(gpu, empty.ids_from_keys_device, _keys_of([0, 1, -1], np.random.default_rng(1)), 0).any()
    empty.dispose()


def _strided(lb):
    return lb.debug_grid_ceiling()[1]


@pytest.mark.parametrize("kind", KINDS)
def test_second_trips(lb, gpu, oracle, kind):
    """the lookups, the index build and the removal's id launches under a ceiling of 1 and of 4 workgroups: identical results,
    and every one of them really strode"""
    _, counts, _, ids, _ = _data(kind)
    n = len(counts)
    fps = _query_fps(lb, kind)
    gone = np.unique(list(range(3, n, 7)) + [0, 20, n - 1])
    keep = np.ones(n, bool)
    keep[gone] = False

    def run():
        c = _corpus(lb, gpu, oracle, kind)
        before = _strided(lb)
        seen = _check_ids_from_keys(lb, gpu, c, kind, fps)
        looked = _strided(lb) - before
        before = _strided(lb)
        seen += _check_keys_from_ids(gpu, c, ids, kind)           # (the first call builds the index)
        built = _strided(lb) - before
        before = _strided(lb)
        assert c.remove(gone) == len(gone)
        removed = _strided(lb) - before
        assert np.array_equal(c.entry_ids(), ids[keep]) and not c.entry_ids(first=len(c), n=len(gone)).any()
        seen += _check_keys_from_ids(gpu, c, ids[keep], (kind, "after the removal"))
        c.dispose()
        return seen, looked, built, removed

    plain, _, _, _ = run()
    for ceiling in (1, 4):
        try:
            lb.debug_set_grid_ceiling(ceiling)
            before = _strided(lb)
            capped, looked, built, removed = run()
            grown = _strided(lb) - before
        finally:
            lb.debug_set_grid_ceiling(0)
        assert len(capped) == len(plain) and all(np.array_equal(a, b) for a, b in zip(plain, capped)), (kind, ceiling)
        if n > 256 * ceiling:                 # more than `ceiling` workgroups of work: the key lists of every entry (one per index
            # base); init, insert and a list of every id; the removal's gather and scatter
            assert looked >= 2 and built >= 3 and removed >= 2 and grown >= looked + built + removed, (kind, ceiling, looked, built, removed, grown)
    assert n > 256


# ---- removal ---------------------------------------------------------------------------------------------------------------
def _removal_sets(n):
    rng = np.random.default_rng(9)
    scattered = np.unique(np.concatenate([rng.choice(n, n // 9, replace=False), [0, 20, 70, 110, 140, 141, n - 1]]))
    return {"scattered": scattered, "the last entries": np.arange(n - 37, n), "every entry": np.arange(n), "nothing valid": np.zeros(0, np.int64)}


@pytest.mark.parametrize("form", ("host indices", "device keys"))
@pytest.mark.parametrize("kind", KINDS)
def test_removal_moves_the_ids(lb, gpu, oracle, kind, form):
    _, counts, _, ids, _ = _data(kind)
    n = len(counts)
    rng = np.random.default_rng(10)
    for name, gone in _removal_sets(n).items():
        keep = np.ones(n, bool)
        keep[gone] = False
        results = []
        for limit in (0, "one tile"):
            c = _corpus(lb, gpu, oracle, kind)
            if limit:
                c.set_remove_scratch_limit(TILE * c.entry_stride_bytes)       # the smallest legal one: the moves run in several chunks
            if form == "host indices":
                removed = c.remove(np.concatenate([gone, gone[:5]]))
            else:
                junk = [-1, BASE + n, BASE + n + 5] + ([BASE - 1] if len(gone) else [])
                g = np.concatenate([gone + BASE, junk, gone[:5] + BASE]).astype(np.int64)
                removed = c.remove_keys_device(_dev64(gpu, _keys_of(g, rng)), index_base=BASE)
            what = (kind, form, name, limit)
            assert removed == len(gone) and len(c) == n - len(gone), what
            assert c.has_entry_ids
            got = c.entry_ids()
            assert np.array_equal(got, ids[keep]), (what, np.nonzero(got != ids[keep])[0][:4])
            assert not c.entry_ids(first=len(c), n=n + 40 - len(c)).any(), (what, "words from the new count on")
            # the ids now name the NEW indices; an id whose every entry went gives the zero key
            _check_keys_from_ids(gpu, c, ids[keep], what)
            all_gone = np.setdiff1d(ids[~keep], np.concatenate([ids[keep], [np.uint64(0)]]))
            if len(all_gone):
                assert not _call(gpu, c.keys_from_ids_device, all_gone, 0).any(), what
            back = _call(gpu, c.ids_from_keys_device, _keys_of(np.arange(len(c)), rng), 0)
            assert np.array_equal(back, ids[keep]), what
            _append_more(lb, gpu, oracle, c, kind, 6)
            tail = c.entry_ids(first=n - len(gone), n=6)
            assert not tail.any() and np.array_equal(c.entry_ids()[:n - len(gone)], ids[keep]), (what, "a later append")
            results.append(c.entry_ids(first=0, n=n + 40))
            c.dispose()
        assert np.array_equal(results[0], results[1]), (kind, form, name, "the scratch limit changed the result")


@pytest.mark.parametrize("kind", KINDS)
def test_remove_ids_and_gather_ids_equal_the_index_forms(lb, gpu, oracle, tmp_path, kind):
    _, counts, _, ids, dups = _data(kind)
    n = len(counts)
    rng = np.random.default_rng(11)
    where = np.concatenate([rng.choice(np.arange(150, n - 5), 60, replace=False), [0, 1, 20, 70, 140]])
    wanted = np.concatenate([ids[where], np.array([3, 0], np.uint64), ids[where[:4]]])       # an absent id, id 0, repeats
    a, b = _corpus(lb, gpu, oracle, kind), _corpus(lb, gpu, oracle, kind)
    packed, offsets = a.gather_ids(wanted)
    exp_packed, exp_offsets = b.gather(where)
    lens = np.diff(offsets.cpu().numpy())
    assert np.array_equal(lens[:len(where)], np.diff(exp_offsets.astype(np.int64))) and lens[len(where):].tolist()[:2] == [0, 0]
    assert np.array_equal(packed.cpu().numpy()[:len(exp_packed)], exp_packed)
    assert a.remove_ids(wanted) == len(where) == b.remove(where)
    assert np.array_equal(a.entry_ids(), b.entry_ids())
    a.save(str(tmp_path / "a.bin"))
    b.save(str(tmp_path / "b.bin"))
    assert open(tmp_path / "a.bin", "rb").read() == open(tmp_path / "b.bin", "rb").read()
    # of the entries that share an id the lowest went: the next one is now the lowest
    v = int(ids[20])
    got = _call(gpu, a.keys_from_ids_device, np.array([v], np.uint64), 0)
    keep = np.ones(n, bool)
    keep[where] = False
    assert int(LOW - (got[0] & LOW)) == int(np.cumsum(keep)[dups[v][1]] - 1)
    a.dispose()
    b.dispose()


# ---- save / load -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_save_and_load(lb, gpu, oracle, tmp_path, kind):
    _, counts, off, ids, _ = _data(kind)
    n = len(counts)
    per = N_SUB if kind == "uniform" else 0
    gpu.cuda.synchronize()
    live = lb.debug_live_bytes()
    plain = _corpus(lb, gpu, oracle, kind, with_ids=False)
    c = _corpus(lb, gpu, oracle, kind)
    plain.save(str(tmp_path / "plain.bin"))
    c.save(str(tmp_path / "ids.bin"))
    old = open(tmp_path / "plain.bin", "rb").read()
    new = open(tmp_path / "ids.bin", "rb").read()
    # without ids: exactly header + payload; with ids: the same bytes and the trailer behind them
    payload = n * plain.entry_stride_bytes if kind == "uniform" else 4 * n + 32 * int(off[n])
    assert len(old) == 32 + payload
    trailer = b"LBADIDS1" + np.uint64(n).tobytes() + ids.tobytes()
    assert new == old + trailer
    loaded = lb.Corpus.load(str(tmp_path / "ids.bin"), L, per, n + 10)
    assert loaded.has_entry_ids and len(loaded) == n and np.array_equal(loaded.entry_ids(), ids)
    assert not loaded.entry_ids(first=n, n=10).any()
    _check_keys_from_ids(gpu, loaded, ids, (kind, "loaded"))
    loaded.save(str(tmp_path / "again.bin"))
    assert open(tmp_path / "again.bin", "rb").read() == new
    loaded.dispose()
    # today's file loads without ids; so does one with other bytes behind the payload
    for name, data in (("plain.bin", old), ("junk.bin", old + b"LBADIDS2" + trailer[8:]), ("short.bin", old + b"LBAD")):
        with open(tmp_path / name, "wb") as f:
            f.write(data)
        again = lb.Corpus.load(str(tmp_path / name), L, per, n)
        assert not again.has_entry_ids and len(again) == n and not again.entry_ids().any()
        again.dispose()
    # a trailer that lies: cut inside the ids, cut inside the count, a count that is not the payload's
    gpu.cuda.synchronize()
    held = lb.debug_live_bytes()
    wrong = {"cut ids": new[:-8], "cut to one id": new[:len(old) + 24], "cut count": new[:len(old) + 12], "magic only": new[:len(old) + 8],
             "count + 1": old + b"LBADIDS1" + np.uint64(n + 1).tobytes() + ids.tobytes() + bytes(8),
             "count - 1": old + b"LBADIDS1" + np.uint64(n - 1).tobytes() + ids.tobytes()}
    for name, data in wrong.items():
        with open(tmp_path / "wrong.bin", "wb") as f:
            f.write(data)
        assert lb.lib().LBAudioDetectiveCorpusLoad(str(tmp_path / "wrong.bin").encode(), n) is None, name
        assert lb.debug_live_bytes() == held, (name, "a failed load leaked")
    plain.dispose()
    c.dispose()
    gpu.cuda.synchronize()
    assert lb.debug_live_bytes() == live


# ---- a corpus that never sets an id ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_no_footprint_without_ids(lb, gpu, oracle, tmp_path, kind):
    """Two corpora of the same entries go through a query and a removal.  One never meets an id call; the other is asked for ids
    and keys all along.  Neither gets an id block, the calls give zeros, and both hold the same bytes, launch the same strided
    launches and save the same file: the second one's calls added nothing to what the first one does -- the path from before
    ids existed."""
    _, counts, _, ids, _ = _data(kind)
    n = len(counts)
    fps = _query_fps(lb, kind)
    gone = list(range(5, n, 11))
    rng = np.random.default_rng(12)
    grown, files, strided = [], [], []
    try:
        lb.debug_set_grid_ceiling(1)
        for ask in (False, True):
            gpu.cuda.synchronize()
            c = _corpus(lb, gpu, oracle, kind, with_ids=False)
            live, launches = lb.debug_live_bytes(), _strided(lb)

            def asked():
                before = lb.debug_live_bytes(), _strided(lb)
                assert not c.has_entry_ids and not c.entry_ids().any()
                assert not _call(gpu, c.ids_from_keys_device, _keys_of(rng.integers(0, len(c), 700), rng), 0).any()
                assert not _call(gpu, c.keys_from_ids_device, ids[:700], 0).any()
                assert not c.has_entry_ids and (lb.debug_live_bytes(), _strided(lb)) == before

            if ask:
                asked()
            keys, _ = c.query_batch_threshold_keys_device(fps, 0.95, 16)
            gpu.cuda.synchronize()
            if ask:
                assert not c.ids_from_keys_device(keys.reshape(-1)).any().item()
            assert c.remove(gone) == len(gone)
            if ask:
                asked()
            grown.append(tuple(x - y for x, y in zip(lb.debug_live_bytes(), live)))
            strided.append(_strided(lb) - launches)
            c.save(str(tmp_path / "c.bin"))
            files.append(open(tmp_path / "c.bin", "rb").read())
            c.dispose()
    finally:
        lb.debug_set_grid_ceiling(0)
    assert grown[0] == grown[1] and strided[0] == strided[1] and files[0] == files[1]
    assert b"LBADIDS1" not in files[0][-(16 + 8 * n):]
