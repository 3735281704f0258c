"""numpy restatement of the tail occurrences contract (LBAudioDetectiveCorpusQueryPackedOccurrencesTailBatchKeysDevice), for the tests.

Recording r of n_q sub-fingerprints with d_r = min(new count, max_new, n_q) new ones, against the entries of a ragged corpus: entry
j of n_j sub-fingerprints takes part when n_j <= n_q (the recording is fingerprint1), its cells are the offsets max(0, n_q - n_j -
d_r + 1) .. n_q - n_j, a cell's value is align_ref.profile's q_o, and it matches when q_o >= threshold as float32.  A row is the
matches in (entry ascending, offset ascending) order: key = q_o bits << 32 | 0xFFFFFFFF - (index_base + j), lag = -o."""
import numpy as np

from align_ref import profile


def clamp_new(new, max_new, n_q):
    return min(int(new), int(max_new), int(n_q))


def tail_range(n_q, n_j, d):
    """the offsets of (recording of n_q, entry of n_j) a push of d new sub-fingerprints completed: range(first, last + 1)"""
    if n_j > n_q or n_j == 0 or d <= 0:
        return range(0)
    return range(max(0, n_q - n_j - d + 1), n_q - n_j + 1)


def tail_cells(recording, entries, d, range_=0):
    """every cell of the recording's row, matching or not: [(entry j, offset o, q_o float32)] in the row's order"""
    recording = np.asarray(recording, np.uint8)
    n_q = recording.shape[0]
    cells = []
    for j, entry in enumerate(entries):
        offsets = tail_range(n_q, len(entry), d)
        if len(offsets) == 0:
            continue
        q, entry_long = profile(recording, entry, range_)
        assert not entry_long and len(q) == n_q - len(entry) + 1
        cells.extend((j, o, q[o]) for o in offsets)
    return cells


def key_of(q, j, index_base=0):
    return (int(np.float32(q).view(np.uint32)) << 32) | (0xFFFFFFFF - (index_base + j))


def tail_row(cells, threshold, capacity, index_base=0):
    """(keys uint64 [capacity], lags int32 [capacity], true count) of one recording from its cells"""
    t = np.float32(threshold)
    hits = [(j, o, q) for (j, o, q) in cells if q >= t]
    keys = np.zeros(capacity, np.uint64)
    lags = np.zeros(capacity, np.int32)
    for slot, (j, o, q) in enumerate(hits[:capacity]):
        keys[slot] = key_of(q, j, index_base)
        lags[slot] = -o
    return keys, lags, len(hits)


def tail_rows(recordings, entries, new_counts, max_new, threshold, capacity, range_=0, index_base=0):
    """(keys uint64 [R, capacity], lags int32 [R, capacity], counts int64 [R]) of a whole call"""
    R = len(recordings)
    keys = np.zeros((R, capacity), np.uint64)
    lags = np.zeros((R, capacity), np.int32)
    counts = np.zeros(R, np.int64)
    for r, rec in enumerate(recordings):
        d = clamp_new(new_counts[r], max_new, len(rec))
        keys[r], lags[r], counts[r] = tail_row(tail_cells(rec, entries, d, range_), threshold, capacity, index_base)
    return keys, lags, counts


def filter_batch_row(keys, lags, count, entry_lengths, n_q, d, capacity, index_base=0):
    """one row of the batch occurrences call (peaks off, NOT cut: count <= len(keys)) with only the tail cells kept, as tail_row
    gives it"""
    assert count <= len(keys), "the batch row must hold every match for the filter to be exact"
    out_k = np.zeros(capacity, np.uint64)
    out_l = np.zeros(capacity, np.int32)
    kept = 0
    for k, lag in zip(np.asarray(keys, np.uint64)[:count], np.asarray(lags, np.int32)[:count]):
        j = 0xFFFFFFFF - (int(k) & 0xFFFFFFFF) - index_base
        n_j = int(entry_lengths[j])
        if n_j <= n_q and -int(lag) in tail_range(n_q, n_j, d) and lag <= 0:
            if kept < capacity:
                out_k[kept], out_l[kept] = k, lag
            kept += 1
    return out_k, out_l, kept


def full_cells(recording, entries, longest, range_=0):
    """every cell (j, absolute position, q) of the whole recording for the entries of at most `longest` sub-fingerprints: what the
    union of the tail calls must be, each once"""
    out = []
    recording = np.asarray(recording, np.uint8)
    for j, entry in enumerate(entries):
        if len(entry) > min(longest, recording.shape[0]) or len(entry) == 0:
            continue
        q, _ = profile(recording, entry, range_)
        out.extend((j, o, q[o]) for o in range(len(q)))
    return out
