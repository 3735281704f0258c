"""Corpus sharded across the GPUs of one node (one process per GPU, torch.distributed).

Each rank holds a contiguous index range of the reference-fingerprint database and scans only
that.  The single exchange step is a MAX all-reduce of one int64 per query:
``key = float_bits(best score) << 32 | (0xFFFFFFFF - global index)``.  Scores are >= 0, so their
IEEE bit patterns order like the values, and the complemented index makes the LOWEST index win
ties -- the strict '<' of the upstream best-match loop (LBAudioDetectiveTests.m:80-83).  With the
"nccl" backend (RCCL on ROCm) the 8-byte message travels over xGMI; "gloo" is used by the CPU
tests of this reduction logic.
"""
from __future__ import annotations

# True: the helpers below run their collectives whenever torch.distributed is initialised, also in a group of ONE rank
# (bench.py --force-dist: the N > 1 code paths executed on a single GPU); False: a lone rank skips them.
FORCE_COLLECTIVES = False


def _collective(group=None) -> bool:
    """Is there a process group this call should talk to?"""
    try:
        import torch.distributed as dist
    except ImportError:                 # a torch built without distributed support: one rank, no group
        return False
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return FORCE_COLLECTIVES or dist.get_world_size(group) > 1


def shard_range(n_entries: int, rank: int, world_size: int):
    """Contiguous [begin, end) of rank's shard; sizes differ by at most one."""
    base, extra = divmod(n_entries, world_size)
    begin = rank * base + min(rank, extra)
    return begin, begin + base + (1 if rank < extra else 0)


def make_key(score_bits: int, global_index: int) -> int:
    return (score_bits << 32) | (0xFFFFFFFF - global_index)


def decode_key(key: int):
    """(index, score) from a reduced key; index -1 when nothing scored above 0."""
    import struct
    key &= 0xFFFFFFFFFFFFFFFF
    score = struct.unpack("<f", struct.pack("<I", key >> 32))[0]
    if key == 0 or not score > 0.0:
        return -1, score
    return 0xFFFFFFFF - (key & 0xFFFFFFFF), score


def allreduce_best(key_tensor, group=None):
    """In-place MAX all-reduce of an int64 key tensor (any device the backend supports)."""
    import torch.distributed as dist
    if _collective(group):
        dist.all_reduce(key_tensor, op=dist.ReduceOp.MAX, group=group)
    return key_tensor


def merge_topk_keys(gathered, k: int):
    """[R, Q, K] int64 top-K keys of R shards (rows descending, 0-padded) -> [Q, k]: the k largest of each query's R * K keys.
    The keys are non-negative as int64 (score bits <= 0x7F800000) and distinct apart from the zero padding (shards never
    share an index), so the k largest are the global top-k in the library's order: score descending, lowest index first."""
    import torch
    r, q, kk = gathered.shape
    flat = gathered.permute(1, 0, 2).reshape(q, r * kk)
    return torch.sort(flat, dim=1, descending=True).values[:, :k].contiguous()


def gather_topk_keys(local_keys, k: int, group=None):
    """Collective: this rank's [Q, K] top-K keys -> the merged [Q, k] of every rank (one all_gather_into_tensor)."""
    import torch
    import torch.distributed as dist
    if not _collective(group):
        return merge_topk_keys(local_keys.unsqueeze(0), k)
    world = dist.get_world_size(group)
    q, kk = local_keys.shape
    out = torch.empty((world * q, kk), dtype=local_keys.dtype, device=local_keys.device)   # (rank-major; gloo wants it flat)
    dist.all_gather_into_tensor(out, local_keys.contiguous(), group=group)
    return merge_topk_keys(out.view(world, q, kk), k)


def merge_topk_aligned(gathered, k: int):
    """[R, Q, K, 2] int64 (key, lag) pairs of R shards -> ([Q, k] keys, [Q, k] lags): merge_topk_keys' keys in its order, each
    lag carried with its key (the zero padding, the only keys that repeat, has lag 0)."""
    import torch
    r, q, kk, _ = gathered.shape
    flat = gathered.permute(1, 0, 2, 3).reshape(q, r * kk, 2)
    order = torch.sort(flat[..., 0], dim=1, descending=True).indices[:, :k]
    return torch.gather(flat[..., 0], 1, order).contiguous(), torch.gather(flat[..., 1], 1, order).contiguous()


def gather_topk_aligned(local_pairs, k: int, group=None):
    """Collective: this rank's [Q, K, 2] (key, lag) pairs -> the merged ([Q, k] keys, [Q, k] lags) of every rank (one
    all_gather_into_tensor: keys and lags travel together)."""
    import torch
    import torch.distributed as dist
    if not _collective(group):
        return merge_topk_aligned(local_pairs.unsqueeze(0), k)
    world = dist.get_world_size(group)
    q, kk, two = local_pairs.shape
    out = torch.empty((world * q, kk, two), dtype=local_pairs.dtype, device=local_pairs.device)
    dist.all_gather_into_tensor(out, local_pairs.contiguous(), group=group)
    return merge_topk_aligned(out.view(world, q, kk, two), k)


def merge_threshold_keys(gathered_keys, gathered_counts, capacity: int):
    """[R, Q, C] int64 threshold keys of R shards (rows in ascending index, 0-padded) and their [R, Q] counts -> ([Q, capacity]
    keys, [Q] totals).  Row q is rank 0's first min(count, C) keys, then rank 1's, and so on, cut at `capacity` and 0-padded: the
    shards hold contiguous index ranges in rank order, so the concatenation IS the global list in ascending index.  The total
    is the sum over the ranks -- the true number of matches, also where a rank's list or the merged one was cut (with
    capacity <= C a rank whose list was cut fills the merged row by itself, so the row is always the global list's head)."""
    import torch
    r, q, c = gathered_keys.shape
    counts = gathered_counts.to(torch.int64)
    held = counts.clamp(max=c)                                           # keys a rank's row really holds
    start = torch.cumsum(held, dim=0) - held                             # [R, Q]: where a rank's keys begin in the merged row
    slot = start.unsqueeze(2) + torch.arange(c, device=gathered_keys.device).view(1, 1, c)
    live = (torch.arange(c, device=gathered_keys.device).view(1, 1, c) < held.unsqueeze(2)) & (slot < capacity)
    out = torch.zeros((q, capacity), dtype=gathered_keys.dtype, device=gathered_keys.device)
    rows = torch.arange(q, device=gathered_keys.device).view(1, q, 1).expand(r, q, c)
    out[rows[live], slot[live]] = gathered_keys[live]
    return out, counts.sum(dim=0)


def gather_threshold_keys(local_keys, local_counts, capacity: int, group=None):
    """Collective: this rank's [Q, C] threshold keys and [Q] counts -> merge_threshold_keys of every rank's (one
    all_gather_into_tensor of the keys, one of the counts)."""
    import torch
    import torch.distributed as dist
    if not _collective(group):
        return merge_threshold_keys(local_keys.unsqueeze(0), local_counts.unsqueeze(0), capacity)
    world = dist.get_world_size(group)
    q, c = local_keys.shape
    keys = torch.empty((world * q, c), dtype=local_keys.dtype, device=local_keys.device)
    counts = torch.empty(world * q, dtype=torch.int64, device=local_keys.device)
    dist.all_gather_into_tensor(keys, local_keys.contiguous(), group=group)
    dist.all_gather_into_tensor(counts, local_counts.to(torch.int64).contiguous(), group=group)
    return merge_threshold_keys(keys.view(world, q, c), counts.view(world, q), capacity)


def gather_packed(local_packed, group=None):
    """Optional last step of sharded fingerprinting: every rank contributes its [n_local, count, 32]
    packed sub-fingerprints (160 B per one-second clip) and receives all of them in rank order.  Ranks
    may hold different numbers of clips.  The fingerprint path itself needs no collective."""
    import torch
    import torch.distributed as dist
    if not _collective(group):
        return local_packed
    world = dist.get_world_size(group)
    n = torch.tensor([local_packed.shape[0]], dtype=torch.int64, device=local_packed.device)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n, group=group)
    counts = [int(c.item()) for c in counts]
    biggest = max(counts)
    padded = torch.zeros((biggest,) + tuple(local_packed.shape[1:]), dtype=local_packed.dtype, device=local_packed.device)
    padded[: local_packed.shape[0]] = local_packed
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded, group=group)
    return torch.cat([p[:c] for p, c in zip(parts, counts)], dim=0)


def broadcast_fingerprint(fp, src: int = 0, group=None, device=None):
    """Send rank `src`'s query fingerprint to every rank (the 160-byte "query broadcast" of the sharded
    compare).  `fp` is a Fingerprint on the source rank and may be None elsewhere; returns a Fingerprint
    on every rank.  Two small collectives: the shape, then the Booleans."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from .api import Fingerprint
    if not _collective(group):
        return fp
    if device is None:
        device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
    shape = torch.zeros(2, dtype=torch.int64, device=device)
    if dist.get_rank(group) == src:
        bools = fp.to_bools()
        shape[0], shape[1] = bools.shape[0], bools.shape[1]
    dist.broadcast(shape, src=src, group=group)
    n, length = int(shape[0]), int(shape[1])
    data = torch.zeros(max(1, n * length), dtype=torch.uint8, device=device)
    if dist.get_rank(group) == src and n * length:
        data[: n * length] = torch.from_numpy(np.ascontiguousarray(bools).reshape(-1)).to(device)
    dist.broadcast(data, src=src, group=group)
    if dist.get_rank(group) == src:
        return fp
    out = Fingerprint(length)
    rows = data[: n * length].cpu().numpy().reshape(n, length)
    for row in rows:
        out.add_subfingerprint(row)
    return out


def make_comm(rank: int = 0, world_size: int = 1, group=None):
    """The library's own RCCL communicator for the sharded query (LBAudioDetectiveCommInitRank).  Rank 0 obtains
    the 128-byte id; torch.distributed -- plumbing, whatever backend it runs on -- carries it to the other ranks.
    The current CUDA/HIP device must already be this rank's."""
    from .api import Comm
    uid, err = [None], None
    if rank == 0:
        try:
            uid[0] = Comm.unique_id()
        except Exception as e:          # noqa: BLE001 -- the other ranks are waiting in the broadcast: tell them
            err = e
    if world_size > 1 or _collective(group):
        # (one rank without FORCE_COLLECTIVES never touches torch.distributed; FORCE_COLLECTIVES must be set identically on
        # every rank BEFORE any helper of this module is called, or the ranks' broadcast calls do not pair up)
        import torch.distributed as dist
        dist.broadcast_object_list(uid, src=0, group=group)
    if uid[0] is None:
        raise err if err is not None else RuntimeError("rank 0 could not obtain an RCCL unique id")
    return Comm(world_size, uid[0], rank)


class ShardedCorpus:
    """This rank's shard of a global corpus plus the collective top-1 query.  With `comm` (make_comm) the
    exchange step runs inside the library (ncclAllReduce of the uint64 keys, LBAudioDetectiveCorpusQuerySharded);
    without it the keys are reduced through torch.distributed (the CPU tests use gloo).

    Packed queries (fingerprints already on the device) need nothing here: `local.query_packed_keys_device` /
    `local.query_packed_topk_keys_device` with index_base = `begin` write the very keys (and lags) that a max-reduction,
    gather_topk_keys and gather_topk_aligned take."""

    def __init__(self, subfingerprint_length: int, subfingerprints_per_entry: int, n_entries_global: int,
                 rank: int = 0, world_size: int = 1, group=None, comm=None):
        from .api import Corpus
        self.rank, self.world_size, self.group, self.comm = rank, world_size, group, comm
        self.n_entries_global = n_entries_global
        self.begin, self.end = shard_range(n_entries_global, rank, world_size)
        self.local = Corpus(subfingerprint_length, subfingerprints_per_entry, max(1, self.end - self.begin))

    def append_packed_device(self, packed, stream=None):
        self.local.append_packed_device(packed, stream)

    def query_batch(self, fps, range_: int = 0, keys_out=None):
        """Collective: several queries, one pass over every shard, one all-reduce of len(fps) int64 keys."""
        if self.comm is not None:
            return self.local.query_batch_sharded(fps, self.comm, self.begin, range_)
        import torch
        if keys_out is None:
            keys_out = torch.zeros(len(fps), dtype=torch.int64, device="cuda")
        self.local.query_batch_keys_device(fps, keys_out, range_, index_base=self.begin)
        allreduce_best(keys_out, self.group)
        return [decode_key(int(k)) for k in keys_out.tolist()]

    def query_topk(self, fps, k: int, range_: int = 0):
        """Collective: the k best matches of every query over all shards -> list of (global indices, scores).  This rank's
        keys (index_base = its first global index), one all-gather of the [Q, k] keys through torch.distributed, the merge."""
        import torch
        from .api import decode_topk_keys
        keys = torch.zeros((len(fps), k), dtype=torch.int64, device="cuda")
        self.local.query_batch_topk_keys_device(fps, k, keys, range_, index_base=self.begin)
        merged = gather_topk_keys(keys, k, self.group).cpu()
        return [decode_topk_keys(row) for row in merged]

    def query_topk_aligned(self, fps, k: int, range_: int = 0):
        """Collective: query_topk with the lag of every match -> list of (global indices, scores, lags).  Each rank aligns
        its own keys on the device (index_base = its first global index) before the exchange; keys and lags then travel as one
        [Q, k, 2] all-gather and merge together."""
        import numpy as np
        import torch
        from .api import decode_topk_keys
        keys = torch.zeros((len(fps), k), dtype=torch.int64, device="cuda")
        self.local.query_batch_topk_keys_device(fps, k, keys, range_, index_base=self.begin)
        lags = self.local.align_keys_device(fps, keys, k, index_base=self.begin, range_=range_)
        merged, merged_lags = gather_topk_aligned(torch.stack([keys, lags.to(torch.int64)], dim=2), k, self.group)
        out = []
        for row, lrow in zip(merged.cpu(), merged_lags.cpu()):
            idx, sc = decode_topk_keys(row)
            out.append((idx, sc, lrow[: len(idx)].numpy().astype(np.int32)))
        return out

    def query_threshold(self, fps, threshold: float, capacity: int, range_: int = 0):
        """Collective: every entry of every shard whose score is >= threshold -> list of (global indices, scores, total) per
        query, indices ascending, cut at `capacity`; total is the true number of matches over all shards.  This rank's keys
        and counts (index_base = its first global index), one all-gather of each through torch.distributed, the concatenation."""
        from .api import decode_threshold_keys
        keys, counts = self.local.query_batch_threshold_keys_device(fps, threshold, capacity, range_=range_, index_base=self.begin)
        merged, totals = gather_threshold_keys(keys, counts, capacity, self.group)
        return [decode_threshold_keys(row, t) + (int(t),) for row, t in zip(merged.cpu(), totals.cpu())]

    def query(self, fp, range_: int = 0, key_out=None):
        """Collective: every rank calls it with the same query; returns (global index, score)."""
        if self.comm is not None:
            return self.local.query_sharded(fp, self.comm, self.begin, range_)
        import torch
        if key_out is None:
            key_out = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.local.query_key_device(fp, key_out, range_, index_base=self.begin)
        allreduce_best(key_out, self.group)
        return decode_key(int(key_out.item()))
