"""CPU checks of the top-K query: the merge of several shards' key lists, the gather-and-merge of ShardedCorpus.query_topk
over a world-size-2 gloo group (the CPU oracle's per-entry scores standing in for the scan), and the compiled selection
kernels of k_topk.hip (no register spilled)."""
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


def host_topk_keys(scores, k, index_base=0):
    """The contract: entries with score > 0, score descending then index ascending, cut at k, as 0-padded keys."""
    scores = np.asarray(scores, np.float32)
    idx = np.arange(len(scores), dtype=np.int64)
    keep = scores > 0
    s, i = scores[keep], idx[keep]
    order = np.lexsort((i, -s))[:k]
    keys = (s[order].view(np.uint32).astype(np.int64) << 32) | (0xFFFFFFFF - (index_base + i[order]))
    return np.concatenate([keys, np.zeros(k - len(keys), np.int64)])


@pytest.mark.parametrize("seed", range(6))
def test_merge_topk_keys_matches_a_sort_of_everything(seed):
    rng = np.random.default_rng(seed)
    ranks, queries, k = int(rng.integers(1, 5)), int(rng.integers(1, 4)), int(rng.integers(1, 40))
    sizes = rng.integers(0, 60, ranks)
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    for q in range(queries):
        # few distinct values: ties across ranks; zeros: entries that do not enter the list
        scores = rng.choice(np.float32([0.0, 0.25, 0.5, 0.5, 0.75, 1.0]), int(bounds[-1])).astype(np.float32)
        local = np.stack([host_topk_keys(scores[bounds[r]:bounds[r + 1]], k, int(bounds[r])) for r in range(ranks)])
        if q == 0:
            gathered = np.zeros((ranks, queries, k), np.int64)
            want = np.zeros((queries, k), np.int64)
        gathered[:, q] = local
        want[q] = host_topk_keys(scores, k)
    got = sharded.merge_topk_keys(torch.from_numpy(gathered), k).numpy()
    assert np.array_equal(got, want)


def test_merge_topk_keys_lowest_index_wins_across_ranks():
    bits = int(np.float32(0.8).view(np.uint32))
    a = [(bits << 32) | (0xFFFFFFFF - 9), 0]
    b = [(bits << 32) | (0xFFFFFFFF - 4), (bits << 32) | (0xFFFFFFFF - 5)]
    got = sharded.merge_topk_keys(torch.tensor([[a], [b]], dtype=torch.int64), 3)[0].tolist()
    assert [0xFFFFFFFF - (x & 0xFFFFFFFF) for x in got] == [4, 5, 9]


def _worker(rank, world, port, n_entries, planted, q, k, ret):
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
    local = torch.from_numpy(host_topk_keys(scores, k, begin)).reshape(1, k)
    merged = sharded.gather_topk_keys(local, k)
    ret[rank] = [(list(i), list(s)) for i, s in (lb.decode_topk_keys(row) for row in merged)]
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("planted", [[1500, 300, 1700, 999, 1000], []])
def test_gather_and_merge_two_ranks(oracle, planted):
    n_entries, world, k = 2000, 2, 10
    q = oracle.synth_entry(5, 123456, 5, 200)
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 33500 + (os.getpid() + len(planted)) % 2000
    mp.spawn(_worker, args=(world, port, n_entries, planted, q, k, ret), nprocs=world, join=True)
    corpus = oracle.synth_corpus(77, 0, n_entries, 5, 200)
    for g in planted:
        corpus[g] = q
    _, _, scores = oracle.corpus_best_ragged(q, (corpus.reshape(-1, 200), np.full(n_entries, 5, np.uint32)), 200, want_scores=True)
    order = np.lexsort((np.arange(n_entries), -scores))[:k]
    want = [(list(order), list(scores[order]))]
    assert ret[0] == ret[1] == want
    if planted:
        assert want[0][0][:len(planted)] == sorted(planted)


def test_topk_kernels_spill_nothing(tmp_path):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_topk.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_topk.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-x", "hip", "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"),
           src, "-o", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    kernels = {k: v for k, v in meta.items() if "topk_" in k}
    # init, gather, sort and six instances each of the histogram and scan passes
    assert len(kernels) == 3 + 6 + 6, sorted(kernels)
    assert {k: v for k, v in kernels.items() if v != (0, 0)} == {}
