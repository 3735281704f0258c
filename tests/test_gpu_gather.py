"""GPU tests of the gather of corpus entries (LBAudioDetectiveCorpusGatherKeysDevice, LBAudioDetectiveCorpusGatherIndices,
LBAudioDetectiveCorpusCopyFingerprint).  What is expected is always the test's own input: the packed numpy rows it appended
(oracle.pack_bools: unused bits zero), concatenated in the order of the key list, and the cumulative row lengths.  Everything
is compared as integers.  Every output buffer is poison-filled before the call, and the bytes behind min(total, capacity)
sub-fingerprints -- and the words behind the offsets -- must still hold the poison afterwards."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON8 = 0xA5
POISON64 = -0x5A5A5A5A5A5A5A5B            # 0xA5A5A5A5A5A5A5A5 as int64
SEED = 0x47415448
PAD = 9                                   # poisoned sub-fingerprints / words behind what a call may write
BASE = 1000003


def _constant(name):
    src = open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_gather.hip")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))


T = _constant("kGatherTileKeys")


# ---- the contract, restated ------------------------------------------------------------------------------------------------
def _packed(oracle, bools):
    """[..., L] Booleans -> [..., 32] bytes of the packed layout, unused bits zero"""
    return np.ascontiguousarray(oracle.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _keys(globals_, rng):
    """64-bit keys of a list of GLOBAL indices (-1: a zero key) with score words that must be ignored"""
    g = np.asarray(globals_, np.int64)
    score = rng.integers(1, 1 << 31, len(g)).astype(np.uint64) << np.uint64(32)
    keys = score | (np.uint64(0xFFFFFFFF) - np.where(g < 0, 0, g).astype(np.uint64))
    keys[g < 0] = 0
    return keys


def _expected(rows, globals_, base):
    """rows: the corpus' entries as a list of [len, 32] byte arrays -> (offsets uint64 [n + 1], bytes [total, 32])"""
    n = len(rows)
    picked = [rows[g - base] if base <= g < base + n else rows[0][:0] for g in np.asarray(globals_, np.int64).tolist()]
    off = np.concatenate([[0], np.cumsum([len(p) for p in picked])]).astype(np.uint64)
    flat = np.concatenate(picked) if picked else np.zeros((0, 32), np.uint8)
    return off, flat.reshape(-1, 32)


def _gather_dev(gpu, c, keys, base, capacity, stream=None):
    """the device form into poisoned buffers -> (offsets uint64 [n + 1], packed bytes [capacity + PAD, 32]); the words behind the
    offsets are checked here"""
    n = len(keys)
    d_keys = gpu.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).cuda()
    d_off = gpu.full((n + 1 + PAD,), POISON64, dtype=gpu.int64, device="cuda")
    d_packed = gpu.full((capacity + PAD, 32), POISON8, dtype=gpu.uint8, device="cuda")
    if stream is not None:
        gpu.cuda.current_stream().synchronize()               # (the buffers above are ready)
    if capacity:
        packed, off = c.gather_keys_device(d_keys, index_base=base, packed_out=d_packed, offsets_out=d_off, capacity=capacity, stream=stream)
        assert packed is d_packed and off is d_off
    else:                                                     # the sizing call: 0 / NULL
        st = c._L.LBAudioDetectiveCorpusGatherKeysDevice(c._ref, d_keys.data_ptr() if n else None, n, base, None, 0, d_off.data_ptr(),
                                                         stream.cuda_stream if stream is not None else gpu.cuda.current_stream().cuda_stream)
        assert st == 0, st
    (stream or gpu.cuda.current_stream()).synchronize()
    off = d_off.cpu().numpy()
    assert (off[n + 1:] == POISON64).all(), "words behind the offsets were written"
    return off[:n + 1].view(np.uint64), d_packed.cpu().numpy()


def _check(gpu, c, rows, globals_, base, rng, what, capacity=None):
    """one device call: offsets, total, the prefix below the capacity and the poison behind it.  capacity None: the true total"""
    exp_off, exp = _expected(rows, globals_, base)
    total = int(exp_off[-1])
    cap = total if capacity is None else capacity
    off, packed = _gather_dev(gpu, c, _keys(globals_, rng), base, cap)
    assert np.array_equal(off, exp_off), (what, "offsets", np.nonzero(off != exp_off)[0][:4], off[-1], total)
    m = min(total, cap)
    bad = np.nonzero((packed[:m] != exp[:m]).any(axis=1))[0]
    assert len(bad) == 0, (what, "bytes of sub-fingerprints", bad[:4], packed[bad[0]].tolist(), exp[bad[0]].tolist())
    assert (packed[m:] == POISON8).all(), (what, "written behind min(total, capacity)", m)
    return off, packed


def _key_lists(n, rng):
    """name -> GLOBAL indices relative to base 0 (add the base to those >= 0 that are meant to be inside); -1: a zero key;
    'out' markers are made by the caller.  Every list the issue names."""
    lists = {
        "empty": [],
        "one": [n // 3],
        "first and last": [0, n - 1],
        "T - 1": rng.integers(0, n, T - 1),
        "T": rng.integers(0, n, T),
        "T + 1": rng.integers(0, n, T + 1),
        "2T + 3": rng.integers(0, n, 2 * T + 3),
        "shuffle of all": rng.permutation(n),
        "in order": np.arange(n),
        "duplicates": [3 % n, 3 % n, 3 % n, 7 % n, n - 1, 7 % n, n - 1, 0, 0],
    }
    some = rng.integers(0, n, 40).tolist()
    lists["zero keys"] = [-1, -1, -1] + some[:10] + [-1] + some[10:20] + [-1] * 5 + some[20:] + [-1, -1]
    lists["only zero keys"] = [-1] * 7
    return {k: np.asarray(v, np.int64) for k, v in lists.items()}


def _run_lists(gpu, c, rows, what, seed):
    n = len(rows)
    rng = np.random.default_rng(seed)
    for base in (0, BASE):
        for name, rel in _key_lists(n, rng).items():
            g = np.where(rel >= 0, rel + base, -1)
            _check(gpu, c, rows, g, base, rng, (what, base, name))
        # indices below the base and at or above base + count, among valid ones; 0xFFFFFFFF has a zero low word under a score
        inside = (rng.integers(0, n, 12) + base).tolist()
        outside = [base + n, base + n + 1, 0xFFFFFFFF, 0xFFFFFFFE] + ([base - 1, 0, base // 2] if base else [])
        mixed = np.asarray(outside[:2] + inside[:6] + outside[2:] + inside[6:] + [base + n], np.int64)
        _check(gpu, c, rows, mixed, base, rng, (what, base, "outside the range"))
        _check(gpu, c, rows, np.asarray(outside * 3, np.int64), base, rng, (what, base, "all keys invalid"))


def _capacities(gpu, c, rows, what, seed, inside_entry=False):
    """the sizing call, capacity = total, total - 1, above the total (and one that ends inside an entry): the offsets and the
    total never change, the prefix is equal, the poison is intact behind it"""
    n = len(rows)
    rng = np.random.default_rng(seed)
    g = np.concatenate([rng.permutation(n)[:T + 7], [-1, -1], rng.integers(0, n, 30)]).astype(np.int64)
    exp_off, _ = _expected(rows, g, 0)
    total = int(exp_off[-1])
    caps = [0, total, total - 1, total + 5, 1]
    if inside_entry:
        k = next(i for i in range(len(g)) if g[i] >= 0 and len(rows[g[i]]) >= 3)
        caps.append(int(exp_off[k]) + 1)                      # ends after the first sub-fingerprint of row k
        last = max(i for i in range(len(g)) if g[i] >= 0 and len(rows[g[i]]) >= 3)
        caps.append(int(exp_off[last + 1]) - 1)               # ... before the last one of a late row
    for cap in caps:
        _check(gpu, c, rows, g, 0, rng, (what, "capacity", cap), capacity=cap)


# ---- uniform corpora -------------------------------------------------------------------------------------------------------
UNIFORM = [(200, 5), (200, 1), (200, 8), (256, 2), (33, 3), (7, 1), (2, 1)]
_MADE = {}


def _uniform_bools(length, n_sub, n):
    """n entries of random Booleans (every bit below the length carries information), made once per shape"""
    key = (length, n_sub)
    if key not in _MADE:
        _MADE[key] = np.random.default_rng(SEED + length * 16 + n_sub).integers(0, 2, (2 * T + 3, n_sub, length), dtype=np.uint8)
    return _MADE[key][:n]


def _uniform(lb, gpu, oracle, bools, capacity):
    n, n_sub, length = bools.shape
    c = lb.Corpus(length, n_sub, capacity)
    if n:
        c.append_packed_device(gpu.from_numpy(_packed(oracle, bools)).cuda())
    return c


@pytest.mark.parametrize("shape", UNIFORM)
def test_uniform_key_lists(lb, gpu, oracle, shape):
    length, n_sub = shape
    n = 2 * T + 3
    bools = _uniform_bools(length, n_sub, n)
    rows = list(_packed(oracle, bools))
    c = _uniform(lb, gpu, oracle, bools, n + 5)               # (a plane stride that is not the count)
    _run_lists(gpu, c, rows, shape, length * 100 + n_sub)
    c.dispose()


@pytest.mark.parametrize("shape", [(200, 5), (33, 3), (256, 2)])
def test_uniform_capacities(lb, gpu, oracle, shape):
    length, n_sub = shape
    n = 2 * T + 3
    bools = _uniform_bools(length, n_sub, n)
    c = _uniform(lb, gpu, oracle, bools, n)
    _capacities(gpu, c, list(_packed(oracle, bools)), shape, 5, inside_entry=n_sub >= 3)
    c.dispose()


# ---- ragged corpora --------------------------------------------------------------------------------------------------------
def _ragged_counts(seed):
    """T + 5 entries of 1 .. 70 sub-fingerprints, among them one of 1 and one of 3000"""
    counts = np.random.default_rng(seed).integers(1, 71, T + 5).astype(np.uint32)
    counts[2], counts[T // 2] = 1, 3000
    return counts


def _ragged(lb, gpu, oracle, flat, counts, entry_capacity, record_capacity):
    c = lb.Corpus.ragged(flat.shape[1], entry_capacity, record_capacity)
    if len(counts):
        c.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, flat)).cuda(), np.asarray(counts, np.uint32))
    return c


def _ragged_rows(oracle, flat, counts):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    packed = _packed(oracle, flat)
    return [packed[off[e]:off[e + 1]] for e in range(len(counts))]


def _ragged_made(length):
    key = ("ragged", length)
    if key not in _MADE:
        counts = _ragged_counts(length)
        flat = np.random.default_rng(SEED + length).integers(0, 2, (int(counts.sum()), length), dtype=np.uint8)
        _MADE[key] = (flat, counts)
    return _MADE[key]


@pytest.mark.parametrize("length", [200, 199, 64])
def test_ragged_key_lists(lb, gpu, oracle, length):
    flat, counts = _ragged_made(length)
    rows = _ragged_rows(oracle, flat, counts)
    c = _ragged(lb, gpu, oracle, flat, counts, len(counts) + 3, int(counts.sum()) + 11)
    _run_lists(gpu, c, rows, ("ragged", length), length)
    c.dispose()


@pytest.mark.parametrize("length", [200, 199])
def test_ragged_capacities(lb, gpu, oracle, length):
    flat, counts = _ragged_made(length)
    c = _ragged(lb, gpu, oracle, flat, counts, len(counts), int(counts.sum()))
    _capacities(gpu, c, _ragged_rows(oracle, flat, counts), ("ragged", length), 6, inside_entry=True)
    c.dispose()


# ---- edge cases ------------------------------------------------------------------------------------------------------------
def test_empty_corpus_and_empty_list(lb, gpu, oracle):
    rng = np.random.default_rng(1)
    for c in (lb.Corpus(200, 5, 4), lb.Corpus.ragged(200, 4, 40)):
        off, packed = _gather_dev(gpu, c, _keys([0, 1, -1, 5], rng), 0, 8)
        assert np.array_equal(off, np.zeros(5, np.uint64)) and (packed == POISON8).all()
        off, packed = _gather_dev(gpu, c, _keys([], rng), 0, 8)
        assert np.array_equal(off, np.zeros(1, np.uint64)) and (packed == POISON8).all()
        off, _ = _gather_dev(gpu, c, _keys([], rng), 0, 0)
        assert np.array_equal(off, np.zeros(1, np.uint64))
        packed, offsets = c.gather([])
        assert packed.shape == (0, 32) and offsets.tolist() == [0]
        c.dispose()


def test_shards_merge_by_the_one_non_empty_copy(lb, gpu, oracle):
    """two corpora as the shards [0, n1) and [n1, n1 + n2) of one index space: each serves the keys of its own range"""
    n1, n2 = T + 3, 700
    bools = _uniform_bools(200, 5, n1 + n2)
    rows = list(_packed(oracle, bools))
    a, b = _uniform(lb, gpu, oracle, bools[:n1], n1), _uniform(lb, gpu, oracle, bools[n1:], n2)
    rng = np.random.default_rng(2)
    g = np.concatenate([rng.permutation(n1 + n2)[:T + 50], [-1, n1 + n2, n1 - 1, n1]]).astype(np.int64)
    keys = _keys(g, rng)
    off_a, pk_a = _gather_dev(gpu, a, keys, 0, len(g) * 5)
    off_b, pk_b = _gather_dev(gpu, b, keys, n1, len(g) * 5)
    len_a, len_b = np.diff(off_a.astype(np.int64)), np.diff(off_b.astype(np.int64))
    assert not ((len_a > 0) & (len_b > 0)).any()
    exp_off, exp = _expected(rows, g, 0)
    assert np.array_equal(len_a + len_b, np.diff(exp_off.astype(np.int64)))
    merged = [(pk_a[off_a[i]:off_a[i + 1]] if len_a[i] else pk_b[off_b[i]:off_b[i + 1]]) for i in range(len(g))]
    assert np.array_equal(np.concatenate(merged), exp)
    a.dispose()
    b.dispose()


# ---- keys from the producers -----------------------------------------------------------------------------------------------
def _planted(oracle, n, n_sub, seed):
    """a synthetic corpus with near copies of other entries planted: 0, 1, 5, 20 and 60 flipped Booleans, eight of each"""
    b = oracle.synth_corpus(seed, 0, n, n_sub, 200).copy()
    rng = np.random.default_rng(seed)
    free = rng.permutation(n).tolist()
    for flips in (0, 1, 5, 20, 60) * 8:
        src, dst = free.pop(), free.pop()
        b[dst] = b[src]
        flat = b[dst].reshape(-1)
        flat[rng.choice(n_sub * 200, flips, replace=False)] ^= 1
    return b


def _gather_produced(gpu, c, rows, keys, base, what):
    """device keys exactly as a producer left them -> gathered unchanged; expected from the indices the keys decode to"""
    flat = keys.reshape(-1).contiguous()
    host = flat.cpu().numpy().view(np.uint64)
    g = np.where(host == 0, -1, 0xFFFFFFFF - (host & np.uint64(0xFFFFFFFF)).astype(np.int64))
    exp_off, exp = _expected(rows, g, base)
    total = int(exp_off[-1])
    d_off = gpu.full((len(host) + 1 + PAD,), POISON64, dtype=gpu.int64, device="cuda")
    d_packed = gpu.full((total + PAD, 32), POISON8, dtype=gpu.uint8, device="cuda")
    c.gather_keys_device(flat, index_base=base, packed_out=d_packed, offsets_out=d_off, capacity=total)
    gpu.cuda.synchronize()
    off, packed = d_off.cpu().numpy(), d_packed.cpu().numpy()
    assert np.array_equal(off[:len(host) + 1].view(np.uint64), exp_off) and (off[len(host) + 1:] == POISON64).all(), what
    assert np.array_equal(packed[:total], exp) and (packed[total:] == POISON8).all(), what
    return g


def test_keys_of_topk_threshold_and_join_are_gathered_unchanged(lb, gpu, oracle):
    n = T + 300
    bools = _planted(oracle, n, 5, 93)
    rows = list(_packed(oracle, bools))
    c = _uniform(lb, gpu, oracle, bools, n)
    fps = [lb.Fingerprint.from_bools(bools[i]) for i in (5, n // 2, n - 1)]
    keys = gpu.full((3, 8), POISON64, dtype=gpu.int64, device="cuda")
    c.query_batch_topk_keys_device(fps, 8, keys, index_base=BASE)
    g = _gather_produced(gpu, c, rows, keys, BASE, "top-K")
    assert (g >= 0).sum() >= 3
    keys, counts = c.query_batch_threshold_keys_device(fps, 0.6, 64, index_base=BASE)
    g = _gather_produced(gpu, c, rows, keys, BASE, "threshold")
    assert (g < 0).any() and (g >= 0).sum() == int(counts.sum().item()) >= 3, "zero padding and matches are both wanted"
    keys, offsets = c.join_threshold_keys_device(0.8, 4096)
    g = _gather_produced(gpu, c, rows, keys, 0, "join")
    assert 0 < (g >= 0).sum() == int(offsets[-1].item()) < 4096
    c.dispose()


# ---- round trip ------------------------------------------------------------------------------------------------------------
def _saved(c, path):
    c.save(str(path))
    with open(path, "rb") as f:
        return f.read()


def _in_order(gpu, n):
    return gpu.from_numpy((np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64)).view(np.int64)).cuda()


@pytest.mark.parametrize("shape", [(200, 5), (33, 3)])
def test_uniform_round_trip_and_removal(lb, gpu, oracle, tmp_path, shape):
    length, n_sub = shape
    n = 2 * T + 3
    bools = _uniform_bools(length, n_sub, n)
    c = _uniform(lb, gpu, oracle, bools, n)
    packed, offsets = c.gather_keys_device(_in_order(gpu, n))             # (sizes itself)
    assert packed.shape == (n * n_sub, 32) and int(offsets[-1].item()) == n * n_sub
    fresh = lb.Corpus(length, n_sub, n)
    fresh.append_packed_device(packed.reshape(n, n_sub, 32))
    assert _saved(fresh, tmp_path / "b.bin") == _saved(c, tmp_path / "a.bin")
    gone = list(range(3, n, 7)) + [0, n - 1]
    keep = np.ones(n, bool)
    keep[gone] = False
    assert c.remove(gone) == int((~keep).sum())
    kept = len(c)
    packed, offsets = c.gather_keys_device(_in_order(gpu, kept))
    assert np.array_equal(packed.cpu().numpy(), _packed(oracle, bools[keep]).reshape(-1, 32))
    assert np.array_equal(offsets.cpu().numpy(), np.arange(kept + 1) * n_sub)
    fresh.dispose()
    c.dispose()


def test_ragged_round_trip_and_removal(lb, gpu, oracle, tmp_path):
    flat, counts = _ragged_made(199)
    n, total = len(counts), int(counts.sum())
    rows = _ragged_rows(oracle, flat, counts)
    c = _ragged(lb, gpu, oracle, flat, counts, n, total)
    packed, offsets = c.gather_keys_device(_in_order(gpu, n))
    assert packed.shape == (total, 32)
    got_counts = np.diff(offsets.cpu().numpy())
    assert np.array_equal(got_counts, counts)
    fresh = lb.Corpus.ragged(199, n, total)
    fresh.append_ragged_packed_device(packed, got_counts.astype(np.uint32))
    assert _saved(fresh, tmp_path / "b.bin") == _saved(c, tmp_path / "a.bin")
    gone = list(range(1, n, 5)) + [0, n - 1, T // 2]
    keep = np.ones(n, bool)
    keep[gone] = False
    assert c.remove(gone) == int((~keep).sum())
    kept = np.nonzero(keep)[0]
    packed, offsets = c.gather_keys_device(_in_order(gpu, len(kept)))
    assert np.array_equal(packed.cpu().numpy(), np.concatenate([rows[e] for e in kept]))
    assert np.array_equal(np.diff(offsets.cpu().numpy()), counts[keep])
    fresh.dispose()
    c.dispose()


# ---- the route this opens: a ragged corpus queried with its own entries ----------------------------------------------------
def test_gathered_entries_as_packed_threshold_queries_of_a_ragged_corpus(lb, gpu, oracle):
    L = 12
    counts = np.random.default_rng(7).integers(1, 41, 300).astype(np.uint32)
    same = [4, 50, 51, 177, 299]
    counts[same] = L
    flat = oracle.synth_ragged_entries(SEED, 0, counts, 200)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    flat[off[51]:off[52]] = flat[off[4]:off[5]]               # a planted copy: a match besides the self-match
    c = _ragged(lb, gpu, oracle, flat, counts, len(counts), int(counts.sum()))
    ids = [e for e in range(len(counts)) if counts[e] == L]
    assert set(same) <= set(ids)
    keys = gpu.from_numpy((np.uint64(0xFFFFFFFF) - np.asarray(ids, np.uint64)).view(np.int64)).cuda()
    packed, offsets = c.gather_keys_device(keys)
    assert packed.shape == (len(ids) * L, 32)
    capacity = 64
    for threshold in (0.3, 0.999):
        got_keys, got_counts = c.query_packed_threshold_keys_device(packed, len(ids), L, threshold, capacity)
        fps = [lb.Fingerprint.from_bools(flat[off[e]:off[e + 1]]) for e in ids]
        exp_keys, exp_counts = c.query_batch_threshold_keys_device(fps, threshold, capacity)
        gpu.cuda.synchronize()
        assert gpu.equal(got_counts, exp_counts) and gpu.equal(got_keys, exp_keys), threshold
        assert int(exp_counts.min().item()) >= 1 and int(exp_counts[ids.index(4)].item()) >= 2
    c.dispose()


# ---- ordering --------------------------------------------------------------------------------------------------------------
def test_gather_on_another_stream_waits_for_the_append(lb, gpu, oracle):
    """an append on stream A, then at once -- no host synchronisation -- a gather on stream B: the new entries come back"""
    n_old, n_new = 1000, 100000
    rng = np.random.default_rng(11)
    old = _uniform_bools(200, 5, n_old)
    new_packed = rng.integers(0, 256, (n_new, 5, 32), dtype=np.uint8)
    new_packed[:, :, 25:] = 0                                 # (bits 200 .. 255: the packed contract)
    c = _uniform(lb, gpu, oracle, old, n_old + n_new)
    d_new = gpu.from_numpy(new_packed).cuda()
    want = n_old + np.concatenate([np.arange(n_new - 500, n_new), [0, n_new // 2]])
    keys = gpu.from_numpy((np.uint64(0xFFFFFFFF) - want.astype(np.uint64)).view(np.int64)).cuda()
    d_off = gpu.full((len(want) + 1,), POISON64, dtype=gpu.int64, device="cuda")
    d_packed = gpu.full((len(want) * 5, 32), POISON8, dtype=gpu.uint8, device="cuda")
    gpu.cuda.synchronize()
    a, b = gpu.cuda.Stream(), gpu.cuda.Stream()
    c.append_packed_device(d_new, stream=a)
    c.gather_keys_device(keys, packed_out=d_packed, offsets_out=d_off, capacity=len(want) * 5, stream=b)
    b.synchronize()
    assert np.array_equal(d_off.cpu().numpy(), np.arange(len(want) + 1) * 5)
    assert np.array_equal(d_packed.cpu().numpy(), new_packed[want - n_old].reshape(-1, 32))
    gpu.cuda.synchronize()
    c.dispose()


# ---- host forms ------------------------------------------------------------------------------------------------------------
def test_host_forms(lb, gpu, oracle):
    N = lb._native
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    rng = np.random.default_rng(3)
    n = T + 9
    ub = _uniform_bools(33, 3, n)
    flat, counts = _ragged_made(199)
    cases = ((_uniform(lb, gpu, oracle, ub, n), list(_packed(oracle, ub))),
             (_ragged(lb, gpu, oracle, flat, counts, len(counts), int(counts.sum())), _ragged_rows(oracle, flat, counts)))
    for c, rows in cases:
        m = len(rows)
        idx = np.concatenate([rng.permutation(m)[:T + 2], [0, m - 1, 5, 5]]).astype(np.int64)
        exp_off, exp = _expected(rows, idx, 0)
        packed, offsets = c.gather(idx)
        assert np.array_equal(offsets, exp_off) and np.array_equal(packed, exp)
        d_off, d_packed = _gather_dev(gpu, c, _keys(idx, rng), 0, int(exp_off[-1]))
        assert np.array_equal(d_off, offsets) and np.array_equal(d_packed[:len(packed)], packed)
        # cut by the capacity: the true total, the prefix, nothing behind it
        cap = int(exp_off[-1]) - 3
        out = np.full((cap + PAD, 32), POISON8, np.uint8)
        off = np.full(len(idx) + 1 + PAD, 0xDEAD, np.uint64)
        ip, op = idx.astype(np.uint64), off.ctypes.data_as(C.POINTER(N.UInt64))
        st = c._L.LBAudioDetectiveCorpusGatherIndices(c._ref, ip.ctypes.data_as(C.POINTER(N.UInt64)), len(ip), out.ctypes.data, cap, op)
        assert st == 0 and np.array_equal(off[:len(idx) + 1], exp_off) and (off[len(idx) + 1:] == 0xDEAD).all()
        assert np.array_equal(out[:cap], exp[:cap]) and (out[cap:] == POISON8).all()
        # an index = the count: refused, nothing written
        out[:] = POISON8
        off[:] = 0xDEAD
        for wrong in ([m], [0, 1, m], [1 << 40]):
            ip = np.asarray(wrong, np.uint64)
            st = c._L.LBAudioDetectiveCorpusGatherIndices(c._ref, ip.ctypes.data_as(C.POINTER(N.UInt64)), len(ip), out.ctypes.data, cap, op)
            assert st == bad and (out == POISON8).all() and (off == 0xDEAD).all(), wrong
        with pytest.raises(lb.LBAudioDetectiveError):
            c.gather([m])
        c.dispose()


def test_fingerprint_of_an_entry(lb, gpu, oracle):
    rng = np.random.default_rng(4)
    for c, lens, length in ((lb.Corpus(33, 3, 8), [3, 3, 3, 3], 33), (lb.Corpus(200, 5, 8), [5, 5], 200),
                            (lb.Corpus.ragged(199, 8, 400), [1, 70, 7, 200], 199)):
        fps = [lb.Fingerprint.from_bools(rng.integers(0, 2, (k, length), dtype=np.uint8)) for k in lens]
        for fp in fps:
            c.append_fingerprint(fp)
        for i in reversed(range(len(fps))):
            got = c.fingerprint(i)
            assert got.subfingerprint_length == length and got.number_of_subfingerprints == lens[i]
            assert got.equal_to_fingerprint(fps[i]) and np.array_equal(got.to_bools(), fps[i].to_bools()), i
            got.dispose()
        with pytest.raises(IndexError):
            c.fingerprint(len(fps))
        assert c._L.LBAudioDetectiveCorpusCopyFingerprint(c._ref, len(fps)) is None
        assert c._L.LBAudioDetectiveCorpusCopyFingerprint(c._ref, 1 << 40) is None
        c.dispose()


# ---- live bytes ------------------------------------------------------------------------------------------------------------
def test_scratch_is_counted_and_goes_with_the_corpus(lb, gpu, oracle):
    gpu.cuda.synchronize()
    live = lb.debug_live_bytes()
    n = 2 * T + 3
    bools = _uniform_bools(200, 5, n)
    flat, counts = _ragged_made(64)
    for c in (_uniform(lb, gpu, oracle, bools, n), _ragged(lb, gpu, oracle, flat, counts, len(counts), int(counts.sum()))):
        before = lb.debug_live_bytes()
        keys = _in_order(gpu, len(c))
        c.gather_keys_device(keys)
        tiles = (len(c) + T - 1) // T
        assert lb.debug_live_bytes() == (before[0] + 8 * tiles, before[1])        # the header's formula
        c.gather(np.arange(10))                                   # (the host form's block is its own and is gone again)
        c.gather_keys_device(keys[:T])
        assert lb.debug_live_bytes() == (before[0] + 8 * tiles, before[1])        # (a smaller call keeps the block)
        c.dispose()
    gpu.cuda.synchronize()
    assert lb.debug_live_bytes() == live
