"""CPU checks of the threshold query: the merge of several shards' key lists (a concatenation in rank order), the
gather-and-merge over a world-size-2 gloo group (the CPU oracle's per-entry scores standing in for the scan), the six symbols
and their declared signatures, the argument checks that need no device, and the compiled selection kernels of k_threshold.hip
(no scratch memory, no register spilled)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from lbaudiodetective_amd import sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

SYMBOLS = ("LBAudioDetectiveCorpusQueryThreshold", "LBAudioDetectiveCorpusQueryBatchThreshold",
           "LBAudioDetectiveCorpusQueryBatchThresholdAligned", "LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice",
           "LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice", "LBAudioDetectiveThresholdKeysFromScoresDevice")


def _has_gpu():
    return torch.cuda.is_available()


def host_threshold_keys(scores, t, capacity, index_base=0):
    """The contract: entries with score >= t (a float32 compare) in ascending index, cut at the capacity, as 0-padded keys;
    and the true count."""
    scores = np.asarray(scores, np.float32)
    with np.errstate(invalid="ignore"):
        at = np.nonzero(scores >= np.float32(t))[0]
    keys = (scores[at].view(np.uint32).astype(np.int64) << 32) | (0xFFFFFFFF - (index_base + at.astype(np.int64)))
    keys = keys[:capacity]
    return np.concatenate([keys, np.zeros(capacity - len(keys), np.int64)]), len(at)


@pytest.mark.parametrize("seed", range(8))
def test_merge_threshold_keys_is_the_concatenation_of_everything(seed):
    rng = np.random.default_rng(seed)
    ranks, queries = int(rng.integers(1, 5)), int(rng.integers(1, 4))
    sizes = rng.integers(0, 60, ranks)
    sizes[rng.integers(0, ranks)] = 0 if seed % 2 else sizes[0]          # a rank without entries now and then
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    total = int(bounds[-1])
    # capacities that cut nothing, that cut inside a rank, and 1
    for capacity in (max(1, total), max(1, total // 3), 1, total + 5):
        gathered = np.zeros((ranks, queries, capacity), np.int64)
        counts = np.zeros((ranks, queries), np.int64)
        want = np.zeros((queries, capacity), np.int64)
        want_n = np.zeros(queries, np.int64)
        for q in range(queries):
            scores = rng.choice(np.float32([0.0, 0.25, 0.5, 0.5, 0.75, 1.0]), total).astype(np.float32)
            t = np.float32([0.5, 0.75, 2.0][q % 3])                      # 2.0: no rank matches anything
            for r in range(ranks):
                gathered[r, q], counts[r, q] = host_threshold_keys(scores[bounds[r]:bounds[r + 1]], t, capacity, int(bounds[r]))
            want[q], want_n[q] = host_threshold_keys(scores, t, capacity)
        got, got_n = sharded.merge_threshold_keys(torch.from_numpy(gathered), torch.from_numpy(counts), capacity)
        assert np.array_equal(got.numpy(), want), (capacity, ranks)
        assert np.array_equal(got_n.numpy(), want_n)


def test_merge_threshold_keys_keeps_rank_order_and_true_totals():
    bits = int(np.float32(0.8).view(np.uint32))
    key = lambda i: (bits << 32) | (0xFFFFFFFF - i)   # noqa: E731
    # rank 0 holds 2 of its 5 matches' worth of room (cut), rank 1 one match, rank 2 none
    keys = torch.tensor([[[key(1), key(3)]], [[key(10), 0]], [[0, 0]]], dtype=torch.int64)
    counts = torch.tensor([[5], [1], [0]], dtype=torch.int64)
    got, total = sharded.merge_threshold_keys(keys, counts, 2)
    assert got.tolist() == [[key(1), key(3)]] and total.tolist() == [6]
    keys = torch.tensor([[[key(1), 0, 0]], [[key(10), key(11), key(12)]], [[key(20), 0, 0]]], dtype=torch.int64)
    counts = torch.tensor([[1], [3], [1]], dtype=torch.int64)
    got, total = sharded.merge_threshold_keys(keys, counts, 3)
    assert got.tolist() == [[key(1), key(10), key(11)]] and total.tolist() == [5]


def _worker(rank, world, port, n_entries, planted, q, t, capacity, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import oracle as O
    import lbaudiodetective_amd as lb
    begin, end = sharded.shard_range(n_entries, rank, world)
    corpus = O.synth_corpus(77, begin, end - begin, 5, 200)
    for g in planted:
        if begin <= g < end:
            corpus[g - begin] = q
    _, _, scores = O.corpus_best_ragged(q, (corpus.reshape(-1, 200), np.full(end - begin, 5, np.uint32)), 200, want_scores=True)
    keys, count = host_threshold_keys(scores, t, capacity, begin)
    merged, totals = sharded.gather_threshold_keys(torch.from_numpy(keys).reshape(1, capacity), torch.tensor([count]), capacity)
    ret[rank] = [(list(i), [float(x) for x in s], int(n)) for (i, s), n in
                 ((lb.decode_threshold_keys(row, n), n) for row, n in zip(merged, totals))]
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("planted,t,capacity", [([1500, 300, 1700, 999, 1000], 0.9, 8), ([1500, 300, 1700, 999, 1000], 0.9, 4),
                                                ([], 0.9, 8), ([300, 1700], None, 2000)])
def test_gather_and_merge_two_ranks(oracle, planted, t, capacity):
    n_entries, world = 2000, 2
    q = oracle.synth_entry(5, 123456, 5, 200)
    corpus = oracle.synth_corpus(77, 0, n_entries, 5, 200)
    for g in planted:
        corpus[g] = q
    _, _, scores = oracle.corpus_best_ragged(q, (corpus.reshape(-1, 200), np.full(n_entries, 5, np.uint32)), 200, want_scores=True)
    if t is None:
        t = float(np.median(scores))                       # a threshold that is a score: about half of either shard, with ties
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 35500 + (os.getpid() + len(planted) + capacity) % 2000
    mp.spawn(_worker, args=(world, port, n_entries, planted, q, t, capacity, ret), nprocs=world, join=True)
    at = np.nonzero(scores >= np.float32(t))[0]
    want = [(list(at[:capacity]), [float(x) for x in scores[at[:capacity]]], len(at))]
    assert ret[0] == ret[1] == want
    if planted and capacity == 8:
        assert want[0][0] == sorted(planted) and want[0][2] == len(planted)
    if capacity == 4:
        assert want[0][2] == 5 and want[0][0] == sorted(planted)[:4]       # the list was cut inside shard 1, the count was not


def test_threshold_kernels_use_no_scratch(tmp_path):
    """k_threshold.hip compiles for gfx950 with the Makefile's flags; the three kernels report 0 bytes of private segment and
    no spilled register (the metadata only)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_threshold.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_threshold.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-x", "hip", "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"),
           src, "-o", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    for kernel in ("threshold_count_kernel", "threshold_offsets_kernel", "threshold_scatter_kernel"):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == 1, (kernel, sorted(meta))
        assert list(hits.values())[0] == (0, 0), hits
    assert len(meta) == 3, sorted(meta)


def _prototype(name):
    """the parameter types of `name` as include/lbaudiodetective.h declares it, comments removed"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lbaudiodetective.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return m.group(1), [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(2).split(",")]


def test_symbols_exist_with_the_declared_signatures(lb):
    N = lb._native
    raw = C.CDLL(lb.LIB_PATH)
    ctype = {"LBAudioDetectiveCorpusRef": N.Ref, "LBAudioDetectiveFingerprintRef": N.Ref,
             "const LBAudioDetectiveFingerprintRef*": C.POINTER(N.Ref), "const void*": C.c_void_p, "void*": C.c_void_p,
             "const Float32*": C.c_void_p, "UInt32": N.UInt32, "UInt64": N.UInt64, "Float32": N.Float32,
             "SInt64*": C.POINTER(N.SInt64), "Float32*": C.POINTER(N.Float32), "SInt32*": C.POINTER(N.SInt32),
             "UInt64*": C.POINTER(N.UInt64)}
    ref, refs, dev = "LBAudioDetectiveCorpusRef", "const LBAudioDetectiveFingerprintRef*", "void*"
    want = {
        SYMBOLS[0]: [ref, "LBAudioDetectiveFingerprintRef", "UInt32", "Float32", "UInt64", "SInt64*", "Float32*", "UInt64*"],
        SYMBOLS[1]: [ref, refs, "UInt32", "UInt32", "Float32", "UInt64", "SInt64*", "Float32*", "UInt64*"],
        SYMBOLS[2]: [ref, refs, "UInt32", "UInt32", "Float32", "UInt64", "SInt64*", "Float32*", "SInt32*", "UInt64*"],
        SYMBOLS[3]: [ref, refs, "UInt32", "UInt32", "Float32", "UInt64", "UInt64", dev, dev, dev],
        SYMBOLS[4]: [ref, "const void*", "UInt32", "UInt32", "UInt32", "Float32", "UInt64", "UInt64", dev, dev, dev, dev],
        SYMBOLS[5]: ["const Float32*", "UInt64", "UInt32", "Float32", "UInt64", "UInt64", dev, dev, dev],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [ctype[p] for p in params], (name, args)
    for attr in ("query_threshold", "query_threshold_batch", "query_batch_threshold_keys_device", "query_packed_threshold_keys_device"):
        assert callable(getattr(lb.Corpus, attr))
    assert callable(lb.ShardedCorpus.query_threshold)
    for fn in ("decode_threshold_keys", "threshold_keys_from_scores_device", "merge_threshold_keys", "gather_threshold_keys"):
        assert callable(getattr(lb, fn)) and fn in lb.__all__
    # no status constant was added for a cut list: it is no error
    assert len(lb._native.declared_symbols()[1]) == 10


def test_decode_threshold_keys(lb):
    keys, n = host_threshold_keys(np.float32([0.1, 0.9, np.nan, 0.7, np.inf, -1.0, 0.7]), 0.7, 6, 100)
    idx, sc = lb.decode_threshold_keys(keys, n)
    assert n == 4 and idx.tolist() == [101, 103, 104, 106] and sc.tolist() == [np.float32(0.9), np.float32(0.7), np.inf, np.float32(0.7)]
    idx2, _ = lb.decode_threshold_keys(keys)               # without a count: up to the zero padding
    assert idx2.tolist() == idx.tolist()
    idx3, _ = lb.decode_threshold_keys(keys[:3], n)        # a cut row
    assert idx3.tolist() == [101, 103, 104]


def test_bad_arguments_are_refused_before_any_device_work(lb):
    """Every refusal below is decided before anything touches a device or a handle: the calls return on a machine without a
    GPU, and with a corpus handle that is never read."""
    L = lb.lib()
    N = lb._native
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    fp = lb.Fingerprint.from_bools(np.ones((3, 200), np.uint8))
    one = (N.Ref * 1)(fp._ref)
    empty = lb.Fingerprint(200)
    none = (N.Ref * 1)(empty._ref)
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    fake = C.c_void_p(p)                  # ... and for a corpus handle
    idx, sc, lag, cnt = (N.SInt64 * 4)(), (N.Float32 * 4)(), (N.SInt32 * 4)(), (N.UInt64 * 1)()
    single, batch, aligned = L.LBAudioDetectiveCorpusQueryThreshold, L.LBAudioDetectiveCorpusQueryBatchThreshold, L.LBAudioDetectiveCorpusQueryBatchThresholdAligned
    keysdev, packed, select = (L.LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice, L.LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice,
                               L.LBAudioDetectiveThresholdKeysFromScoresDevice)
    for t in (0.0, -1.0, float("nan"), float("inf"), -0.0):
        assert single(fake, fp._ref, 0, t, 4, idx, sc, cnt) == bad, t
        assert batch(fake, one, 1, 0, t, 4, idx, sc, cnt) == bad, t
        assert aligned(fake, one, 1, 0, t, 4, idx, sc, lag, cnt) == bad, t
        assert keysdev(fake, one, 1, 0, t, 4, 0, p, p, None) == bad, t
        assert packed(fake, p, 1, 5, 0, t, 4, 0, p, p, p, None) == bad, t
        assert select(p, 100, 1, t, 4, 0, p, p, None) == bad, t
    # capacity 0; inCount x inCapacity above 2^31
    for cap, n in ((0, 1), ((1 << 31) + 1, 1), (1 << 30, 3)):
        refs = (N.Ref * n)(*[fp._ref] * n)
        assert batch(fake, refs, n, 0, 0.7, cap, idx, sc, cnt) == bad
        assert aligned(fake, refs, n, 0, 0.7, cap, idx, sc, lag, cnt) == bad
        assert keysdev(fake, refs, n, 0, 0.7, cap, 0, p, p, None) == bad
        assert packed(fake, p, n, 5, 0, 0.7, cap, 0, p, p, None, None) == bad
        assert select(p, 100, n, 0.7, cap, 0, p, p, None) == bad
    assert single(fake, fp._ref, 0, 0.7, 0, idx, sc, cnt) == bad
    # NULL pointers, no queries, a query without sub-fingerprints
    assert single(fake, None, 0, 0.7, 4, idx, sc, cnt) == bad
    assert single(fake, fp._ref, 0, 0.7, 4, None, sc, cnt) == bad
    assert single(fake, fp._ref, 0, 0.7, 4, idx, None, cnt) == bad
    assert single(fake, fp._ref, 0, 0.7, 4, idx, sc, None) == bad
    assert single(fake, empty._ref, 0, 0.7, 4, idx, sc, cnt) == bad
    assert batch(fake, None, 1, 0, 0.7, 4, idx, sc, cnt) == bad
    assert batch(fake, one, 0, 0, 0.7, 4, idx, sc, cnt) == bad
    assert batch(fake, none, 1, 0, 0.7, 4, idx, sc, cnt) == bad
    assert aligned(fake, one, 1, 0, 0.7, 4, idx, sc, None, cnt) == bad
    assert keysdev(fake, one, 1, 0, 0.7, 4, 0, None, p, None) == bad
    assert keysdev(fake, one, 1, 0, 0.7, 4, 0, p, None, None) == bad
    assert packed(fake, None, 1, 5, 0, 0.7, 4, 0, p, p, None, None) == bad
    assert packed(fake, p, 1, 5, 0, 0.7, 4, 0, None, p, None, None) == bad
    assert packed(fake, p, 1, 5, 0, 0.7, 4, 0, p, None, None, None) == bad
    assert packed(fake, p, 0, 5, 0, 0.7, 4, 0, p, p, None, None) == bad
    assert packed(fake, p, 1, 0, 0, 0.7, 4, 0, p, p, None, None) == bad
    assert select(None, 100, 1, 0.7, 4, 0, p, p, None) == bad
    assert select(p, 100, 1, 0.7, 4, 0, None, p, None) == bad
    assert select(p, 100, 1, 0.7, 4, 0, p, None, None) == bad
    assert select(p, 100, 0, 0.7, 4, 0, p, p, None) == bad
    assert select(p, 100, 1, 0.7, 4, (1 << 32) - 99, p, p, None) == bad        # index_base + count > 2^32
    assert select(p, (1 << 32) + 1, 1, 0.7, 4, 0, p, p, None) == bad


@pytest.mark.skipif(_has_gpu(), reason="the no-device statuses need a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks every call reports kLBAudioDetectiveDeviceUnavailable."""
    L = lb.lib()
    N = lb._native
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    fp = lb.Fingerprint.from_bools(np.ones((3, 200), np.uint8))
    one = (N.Ref * 1)(fp._ref)
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    idx, sc, lag, cnt = (N.SInt64 * 4)(), (N.Float32 * 4)(), (N.SInt32 * 4)(), (N.UInt64 * 1)()
    assert L.LBAudioDetectiveCorpusQueryThreshold(None, fp._ref, 0, 0.7, 4, idx, sc, cnt) == nogp
    assert L.LBAudioDetectiveCorpusQueryBatchThreshold(None, one, 1, 0, 0.7, 4, idx, sc, cnt) == nogp
    assert L.LBAudioDetectiveCorpusQueryBatchThresholdAligned(None, one, 1, 0, 0.7, 4, idx, sc, lag, cnt) == nogp
    assert L.LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice(None, one, 1, 0, 1.5, 4, 0, p, p, None) == nogp      # (t > 1 is legal)
    assert L.LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice(None, p, 1, 5, 0, 0.7, 4, 0, p, p, None, None) == nogp
    assert L.LBAudioDetectiveThresholdKeysFromScoresDevice(p, 100, 1, 0.7, 4, 0, p, p, None) == nogp
