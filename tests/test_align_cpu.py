"""CPU checks of the alignment feature: the numpy restatement of the contract (tests/align_ref.py) against the oracle's compare,
the argument checks and the missing-device status of the new C entry points, the gather-and-merge of
ShardedCorpus.query_topk_aligned over a world-size-2 gloo group (oracle scores and restated lags standing in for the device), and
the compiled kernels of k_align.hip (no register spilled, no scratch)."""
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

import align_ref
from lbaudiodetective_amd import sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _has_gpu():
    try:
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.parametrize("seed", range(4))
def test_restatement_matches_the_oracle_compare(oracle, seed):
    """Score of the restatement == lbo_compare_fp, bit for bit, on a few hundred pairs (odd lengths, odd ranges, all-zero
    sub-fingerprints, planted matches), and the lag points at an offset that reaches it."""
    rng = np.random.default_rng(seed)
    for _ in range(80):
        L = int(rng.choice([200, 199, 57, 31, 2, 3]))
        rg = int(rng.choice([0, 1, 2, L // 2 | 1, L - 1, L, L + 5])) if L > 2 else int(rng.choice([0, 1, 2]))
        nq, ne = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        q = (rng.random((nq, L)) < rng.choice([0.5, 0.1, 0.0])).astype(np.uint8)
        e = (rng.random((ne, L)) < rng.choice([0.5, 0.9])).astype(np.uint8)
        if rng.random() < 0.4:                     # plant the shorter inside the longer
            if nq < ne:
                o = int(rng.integers(0, ne - nq + 1))
                e[o:o + nq] = q
            else:
                o = int(rng.integers(0, nq - ne + 1))
                q[o:o + ne] = e
        score, lag = align_ref.align(q, e, rg)
        want = np.float32(oracle.compare_fp(q, e, rg if rg else L, L))
        assert score.view(np.uint32) == want.view(np.uint32), (L, rg, nq, ne, score, want)
        prof, entry_long = align_ref.profile(q, e, rg)
        assert entry_long == (nq < ne)
        off = lag if entry_long else -lag
        assert off >= 0 and prof[off] == score and not (prof[:off] == score).any()


def test_restatement_on_a_planted_match():
    rng = np.random.default_rng(5)
    q = (rng.random((7, 200)) < 0.5).astype(np.uint8)
    e = (rng.random((40, 200)) < 0.5).astype(np.uint8)
    e[23:30] = q
    assert align_ref.align(q, e, 0) == (np.float32(1.0), 23)
    # the entry inside a longer query: case B, negative lag
    assert align_ref.align(e, q, 0) == (np.float32(1.0), -23)
    # two identical plants: the lower offset wins
    e[5:12] = q
    assert align_ref.align(q, e, 0)[1] == 5


@pytest.mark.skipif(_has_gpu(), reason="the no-device statuses need a machine without a GPU")
def test_new_entry_points_validate_and_fail_without_gpu(lb):
    L = lb.lib()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    fp = lb.Fingerprint.from_bools(np.ones((3, 200), np.uint8))
    one = (lb._native.Ref * 1)(fp._ref)
    empty = lb.Fingerprint(200)                        # no sub-fingerprints: not a query
    none = (lb._native.Ref * 1)(empty._ref)
    idx, sc, lag, cnt = (lb._native.SInt64 * 4)(), (lb._native.Float32 * 4)(), (lb._native.SInt32 * 4)(), (lb._native.UInt32 * 1)()
    keys = C.c_void_p(0x1000)                           # never dereferenced: the call stops before any device work
    # AlignKeysDevice: k out of range, no queries, NULL keys / lags, an empty query
    assert L.LBAudioDetectiveCorpusAlignKeysDevice(None, one, 1, 0, 0, keys, 0, keys, None, None) == bad
    assert L.LBAudioDetectiveCorpusAlignKeysDevice(None, one, 1, 0, 1025, keys, 0, keys, None, None) == bad
    assert L.LBAudioDetectiveCorpusAlignKeysDevice(None, one, 0, 0, 1, keys, 0, keys, None, None) == bad
    assert L.LBAudioDetectiveCorpusAlignKeysDevice(None, None, 1, 0, 1, keys, 0, keys, None, None) == bad
    assert L.LBAudioDetectiveCorpusAlignKeysDevice(None, one, 1, 0, 1, None, 0, keys, None, None) == bad
    assert L.LBAudioDetectiveCorpusAlignKeysDevice(None, one, 1, 0, 1, keys, 0, None, None, None) == bad
    assert L.LBAudioDetectiveCorpusAlignKeysDevice(None, none, 1, 0, 1, keys, 0, keys, None, None) == bad
    assert L.LBAudioDetectiveCorpusAlignKeysDevice(None, one, 1, 0, 4, keys, 0, keys, None, None) == nogp
    # QueryBatchTopKAligned
    assert L.LBAudioDetectiveCorpusQueryBatchTopKAligned(None, one, 1, 0, 0, idx, sc, lag, cnt) == bad
    assert L.LBAudioDetectiveCorpusQueryBatchTopKAligned(None, one, 1, 0, 4, idx, sc, None, cnt) == bad
    assert L.LBAudioDetectiveCorpusQueryBatchTopKAligned(None, one, 1, 0, 4, None, sc, lag, cnt) == bad
    assert L.LBAudioDetectiveCorpusQueryBatchTopKAligned(None, one, 1, 0, 4, idx, sc, lag, cnt) == nogp
    # QueryAligned
    assert L.LBAudioDetectiveCorpusQueryAligned(None, None, 0, idx, sc, lag) == bad
    assert L.LBAudioDetectiveCorpusQueryAligned(None, fp._ref, 0, idx, sc, None) == bad
    assert L.LBAudioDetectiveCorpusQueryAligned(None, empty._ref, 0, idx, sc, lag) == bad
    assert L.LBAudioDetectiveCorpusQueryAligned(None, fp._ref, 0, idx, sc, lag) == nogp
    # MatchProfile: NULL count / first lag, a buffer without capacity... and no device
    n, first = lb._native.UInt64(0), lb._native.SInt32(0)
    out = (lb._native.Float32 * 4)()
    assert L.LBAudioDetectiveCorpusMatchProfile(None, fp._ref, 0, 0, out, 4, None, C.byref(first)) == bad
    assert L.LBAudioDetectiveCorpusMatchProfile(None, fp._ref, 0, 0, out, 4, C.byref(n), None) == bad
    assert L.LBAudioDetectiveCorpusMatchProfile(None, fp._ref, 0, 0, None, 4, C.byref(n), C.byref(first)) == bad
    assert L.LBAudioDetectiveCorpusMatchProfile(None, fp._ref, 0, 0, out, 4, C.byref(n), C.byref(first)) == nogp
    assert L.LBAudioDetectiveCorpusMatchProfile(None, fp._ref, 0, 0, None, 0, C.byref(n), C.byref(first)) == nogp


def _key(score, index):
    return (int(np.float32(score).view(np.uint32)) << 32) | (0xFFFFFFFF - index)


def test_merge_carries_lags_with_their_keys():
    # rank 0: entries 0..2, rank 1: entries 3..5; ties on score go to the lower index, padding keeps lag 0
    a = [[_key(0.9, 2), 17], [_key(0.5, 0), -3], [0, 0]]
    b = [[_key(0.9, 4), -8], [_key(0.7, 3), 2], [_key(0.5, 5), 11]]
    gathered = torch.tensor([[a], [b]], dtype=torch.int64)
    keys, lags = sharded.merge_topk_aligned(gathered, 4)
    assert torch.equal(keys, sharded.merge_topk_keys(gathered[..., 0], 4))
    assert [0xFFFFFFFF - (int(k) & 0xFFFFFFFF) for k in keys[0]] == [2, 4, 3, 0]
    assert lags[0].tolist() == [17, -8, 2, -3]
    keys, lags = sharded.merge_topk_aligned(torch.tensor([[a]], dtype=torch.int64), 3)
    assert lags[0].tolist() == [17, -3, 0] and int(keys[0, 2]) == 0


def _entries(n_entries, planted, q):
    """A seeded ragged corpus of 1..29 sub-fingerprints per entry, q planted into entry g at offset off for (g, off) in planted."""
    rng = np.random.default_rng(9)
    counts = rng.integers(1, 30, n_entries)
    entries = [(rng.random((int(c), 200)) < 0.5).astype(np.uint8) for c in counts]
    for g, off in planted:
        e = np.zeros((max(entries[g].shape[0], q.shape[0] + off), 200), np.uint8)
        e[:entries[g].shape[0]] = entries[g]
        e[off:off + q.shape[0]] = q
        entries[g] = e
    return entries


def _shard_pairs(oracle, entries, q, k, begin, end):
    """This shard's top-k keys (oracle scores) and lags (restatement) as [1, k, 2]."""
    local = entries[begin:end]
    _, _, scores = oracle.corpus_best_ragged(q, local, 200, want_scores=True)
    order = np.lexsort((np.arange(len(local)), -scores))
    order = order[scores[order] > 0][:k]
    pairs = np.zeros((1, k, 2), np.int64)
    for j, e in enumerate(order):
        pairs[0, j, 0] = _key(scores[e], begin + int(e))
        pairs[0, j, 1] = align_ref.align(q, local[e], 200)[1]
    return pairs


def _worker(rank, world, port, n_entries, planted, q, k, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import oracle as O
    import lbaudiodetective_amd as lb
    begin, end = sharded.shard_range(n_entries, rank, world)
    pairs = _shard_pairs(O, _entries(n_entries, planted, q), q, k, begin, end)
    keys, lags = sharded.gather_topk_aligned(torch.from_numpy(pairs), k)
    idx, sc = lb.decode_topk_keys(keys[0])
    ret[rank] = (list(idx), list(sc), lags[0, :len(idx)].tolist())
    dist.barrier()
    dist.destroy_process_group()


def test_gather_and_merge_aligned_two_ranks(oracle):
    n_entries, world, k = 300, 2, 8
    q = (np.random.default_rng(77).random((6, 200)) < 0.5).astype(np.uint8)
    planted = [(210, 4), (40, 0), (149, 9)]
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 35600 + os.getpid() % 2000
    mp.spawn(_worker, args=(world, port, n_entries, planted, q, k, ret), nprocs=world, join=True)
    entries = _entries(n_entries, planted, q)
    _, _, scores = oracle.corpus_best_ragged(q, entries, 200, want_scores=True)
    order = np.lexsort((np.arange(n_entries), -scores))[:k]
    want = (list(order), list(scores[order]), [align_ref.align(q, entries[e], 200)[1] for e in order])
    assert ret[0] == ret[1] == want
    assert want[0][:3] == [40, 149, 210] and want[2][:3] == [0, 9, 4]


def test_align_kernels_spill_nothing(tmp_path):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_align.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_align.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-x", "hip", "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"),
           src, "-o", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    kernels = {k: v for k, v in meta.items() if "align_" in k}
    # keys, finish and profile kernels, one instance per corpus layout
    assert len(kernels) == 6, sorted(kernels)
    assert {k: v for k, v in kernels.items() if v != (0, 0, 0)} == {}
    assert "scratch_" not in isa.replace("SCRATCH_EN", "")
