"""GPU test of the three families of the occurrences pass against EACH OTHER on one corpus handle: occurrences, recording scores
and the recording timeline share the corpus' events, the staged query and a join scratch each of them carves its own way
(csrc/recording_pass.cpp), so calls of different families issued back to back on two streams must leave each other's results
alone.  Every expected value is numpy (align_ref's profiles and alignment, timeline_ref) and every comparison is of integers and
bit patterns: nothing needs a tolerance.  Output buffers are poison-filled.  The helpers are test_gpu_timeline.py's, copied."""
import os
import re

import numpy as np
import pytest

import timeline_ref
from align_ref import align, profile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
POISONF = -12345.0
L = 200
N = 200                                                  # entries: above the occurrences block and the timeline walk
N_QUERY = 300
E22 = 150                                                # where the planted entry lies: in the last block of either family
T_TIMELINE = 0.3


def _source(name):
    return open(os.path.join(ROOT, name)).read()


def _constant(name, file):
    return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name,
                         _source(os.path.join("lbaudiodetective_amd", "csrc", file))).group(1))


TILE = _constant("kOcKeep", "k_occurrences.hip")        # offsets of a tile
BLOCK = _constant("kOcBlock", "k_occurrences.hip")      # entries an occurrences or scores chunk is a multiple of
WALK = _constant("kTlEntries", "k_timeline.hip")        # entries a timeline chunk is a multiple of


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
    c.append_ragged_packed_device(gpu.from_numpy(_packed(oracle, np.concatenate(entries))).cuda(), counts)
    return c


def _expected_occurrences(profiles, t):
    """(keys uint64, lags int32) of every cell at or above t that is a peak of its profile, entries and offsets ascending
    (test_gpu_occurrences.py's)"""
    keys, lags = [], []
    for j, (q, entry_long) in enumerate(profiles):
        m = q >= np.float32(t)
        left = np.ones(len(q), bool)
        right = np.ones(len(q), bool)
        left[1:] = q[1:] > q[:-1]
        right[:-1] = q[:-1] >= q[1:]
        o = np.flatnonzero(m & left & right)
        keys.append((q[o].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - j))
        lags.append(o if entry_long else -o)
    return np.concatenate(keys).astype(np.uint64), np.concatenate(lags).astype(np.int32)


def _chunks(limit, tiles):
    """entries per chunk of (occurrences, scores, timeline) under a scratch limit: the header's per-chunk formulas"""
    occurrences = (limit - 24) // (BLOCK * (16 + 8 * tiles) + -(-tiles // 4) * 4) * BLOCK
    scores = limit // (BLOCK * tiles * 8) * BLOCK
    timeline = limit // (tiles * 126 * 8) * WALK
    return occurrences, scores, timeline


class _Call:
    """one device form into poison-filled buffers of its own; result(): its outputs as numpy, once its stream is synchronised"""

    def __init__(self, gpu, corpus, family, stream, fp=None, packed=None, t=None, capacity=0):
        self.family = family
        i64 = lambda n: gpu.full((n,), POISON, dtype=gpu.int64, device="cuda")            # noqa: E731
        i32 = lambda n: gpu.full((n,), POISON32, dtype=gpu.int32, device="cuda")          # noqa: E731
        if family == "occurrences":
            self.out = (i64(capacity), i32(capacity), i64(1))
            if packed is None:
                corpus.query_occurrences_keys_device(fp, float(t), capacity, peaks=True, keys_out=self.out[0], lags_out=self.out[1],
                                                     count_out=self.out[2], stream=stream)
            else:
                corpus.query_packed_occurrences_keys_device(packed, N_QUERY, float(t), capacity, peaks=True, keys_out=self.out[0],
                                                            lags_out=self.out[1], count_out=self.out[2], stream=stream)
        elif family == "scores":
            self.out = (gpu.full((N,), POISONF, dtype=gpu.float32, device="cuda"), i32(N))
            corpus.recording_scores_device(fp=fp, packed=packed, per_query=N_QUERY if packed is not None else 0, scores_out=self.out[0],
                                           lags_out=self.out[1], stream=stream)
        else:
            self.out = (i64(N_QUERY), i32(N_QUERY))
            corpus.recording_timeline_keys_device(fp=fp, packed=packed, per_query=N_QUERY if packed is not None else 0,
                                                  threshold=T_TIMELINE, keys_out=self.out[0], lengths_out=self.out[1], stream=stream)

    def result(self):
        """integers throughout: keys uint64, scores as their bits, lags / lengths / count as they are"""
        out = [x.cpu().numpy() for x in self.out]
        if self.family == "scores":
            return out[0].view(np.uint32), out[1]
        return tuple([out[0].view(np.uint64)] + [x.view(np.uint32 if self.family == "timeline" else x.dtype) for x in out[1:]])


def _equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_the_three_families_interleaved_on_one_handle(lb, gpu, oracle):
    rng = np.random.default_rng(23)
    counts = rng.integers(1, 41, N)
    counts[0], counts[1], counts[E22] = 1, 40, 22
    entries = _random(oracle, 2121, counts)
    query = _random(oracle, 2222, [N_QUERY])[0]
    query[TILE - 1:TILE + 21] = entries[E22]                     # offset 125: the last cell of tile 0
    query[2 * TILE:2 * TILE + 22] = entries[E22]                 # offset 252: the first cell of tile 2
    assert N > WALK > BLOCK and (TILE, E22 // WALK, E22 // BLOCK) == (126, 1, 2)
    fp = lb.Fingerprint.from_bools(query)
    packed = gpu.from_numpy(_packed(oracle, query)).cuda()

    # the references, each family's own
    profiles = [profile(query, e, 0) for e in entries]
    cells = np.sort(np.concatenate([p for p, _ in profiles]))
    t_occ = np.float32(cells[len(cells) // 2])                   # the median cell: a list of many entries
    want_occ = _expected_occurrences(profiles, t_occ)
    capacity = len(want_occ[0]) + 5
    aligned = [align(query, e, 0) for e in entries]
    want_scores = (np.array([a[0] for a in aligned], np.float32).view(np.uint32), np.array([a[1] for a in aligned], np.int32))
    want_timeline = timeline_ref.timeline(query, entries, T_TIMELINE)
    assert len(want_occ[0]) > N and np.count_nonzero(want_timeline[0]) > N_QUERY // 2
    one = int(np.float32(1.0).view(np.uint32))
    for o in (TILE - 1, 2 * TILE):
        assert want_timeline[0][o] == (one << 32) | (0xFFFFFFFF - E22) and want_timeline[1][o] == 22
        assert (one << 32) | (0xFFFFFFFF - E22) in want_occ[0][want_occ[1] == -o]
    assert want_scores[0][E22] == one and want_scores[1][E22] == -(TILE - 1)

    # a scratch limit under which every family takes at least two chunks
    tiles = -(-(N_QUERY - int(counts.min()) + 1) // TILE)
    assert tiles == 3 == -(-int((np.abs(counts - N_QUERY) + 1).max()) // TILE)
    limit = max(24 + BLOCK * (16 + 8 * tiles) + -(-tiles // 4) * 4, BLOCK * tiles * 8, tiles * 126 * 8) + 7
    assert all(0 < chunk < N for chunk in _chunks(limit, tiles)), _chunks(limit, tiles)

    forms = [("occurrences", dict(fp=fp, t=t_occ, capacity=capacity)), ("scores", dict(packed=packed)), ("timeline", dict(packed=packed)),
             ("occurrences", dict(packed=packed, t=t_occ, capacity=capacity)), ("scores", dict(fp=fp)), ("timeline", dict(fp=fp))]

    # each form alone on a fresh handle, against its reference
    alone_corpus = _ragged(lb, gpu, oracle, entries)
    alone_corpus.set_join_scratch_limit(limit)
    alone = []
    for family, kw in forms:
        call = _Call(gpu, alone_corpus, family, None, **kw)
        gpu.cuda.synchronize()
        alone.append(call.result())
        if family == "occurrences":
            keys, lags, count = alone[-1]
            m = len(want_occ[0])
            assert count.view(np.uint64)[0] == m and np.array_equal(keys[:m], want_occ[0]) and np.array_equal(lags[:m], want_occ[1])
            assert not keys[m:].any() and not lags[m:].any()
        else:
            assert _equal(alone[-1], want_scores if family == "scores" else want_timeline), family

    # the six interleaved on ONE fresh handle (its scratch grows on the way) and two streams, no host synchronisation between them
    corpus = _ragged(lb, gpu, oracle, entries)
    corpus.set_join_scratch_limit(limit)
    streams = [gpu.cuda.Stream(), gpu.cuda.Stream()]
    gpu.cuda.synchronize()                                        # (the append and the poison fills below are the current stream's)
    calls = []
    for i, (family, kw) in enumerate(forms):
        streams[i % 2].wait_stream(gpu.cuda.current_stream())
        calls.append(_Call(gpu, corpus, family, streams[i % 2], **kw))
    for s in streams:
        s.synchronize()
    for (family, _kw), call, want in zip(forms, calls, alone):
        assert _equal(call.result(), want), family

    # the host-returning forms in a row on the same handle, against the decoded device results
    idx, sc, lags, count = corpus.query_occurrences(fp, float(t_occ), capacity, peaks=True)
    want_idx, want_sc, want_lags = lb.decode_occurrence_keys(alone[0][0], alone[0][1], int(alone[0][2].view(np.uint64)[0]))
    assert count == len(want_occ[0]) and np.array_equal(idx, want_idx) and np.array_equal(lags, want_lags)
    assert np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))
    idx, sc, lags = corpus.query_recording_topk(fp, 5)
    bits, entry_lags = alone[4]
    best = np.argsort(-((bits.astype(np.int64) << 32) | (0xFFFFFFFF - np.arange(N, dtype=np.int64))), kind="stable")[:5]
    assert bits[best[4]] > 0 and best[0] == E22
    assert np.array_equal(idx, best) and np.array_equal(sc.view(np.uint32), bits[best]) and np.array_equal(lags, entry_lags[best])
    idx, sc, lengths = corpus.recording_timeline(fp, T_TIMELINE)
    want_idx, want_sc, want_lengths = lb.decode_timeline_keys(alone[5][0].view(np.int64), alone[5][1])
    assert np.array_equal(idx, want_idx) and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))
    assert np.array_equal(lengths, want_lengths)
