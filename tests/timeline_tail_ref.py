"""numpy restatement of the timeline tail contract (LBAudioDetectiveCorpusRecordingPackedTimelineTailBatchKeysDevice), for the tests.

A window of n sub-fingerprints after a push of `new` of them: shift = min(new, n), cells = min(new, max_new, n).  The STRIP T[o] is the
unsigned maximum of  q_o bits << 32 | 0xFFFFFFFF - (index_base + j)  over the tail occurrences' cells (occurrences_tail_ref.tail_cells
at `cells`) with q_o >= threshold as float32, 0 where there is none.  The ROLL is max(T[o], prev[o + shift]) with prev read as 0
beyond its row.  The lengths are looked up from the entries' lengths by the index a key names: 0 for a zero key or an index outside
the corpus."""
import numpy as np

from occurrences_tail_ref import clamp_new, key_of, tail_cells


def strip_of_cells(n, cells, threshold, index_base=0):
    """T uint64 [n] from tail_cells' list [(entry, offset, q)]"""
    t = np.float32(threshold)
    out = np.zeros(n, np.uint64)
    for (j, o, q) in cells:
        if q >= t:
            k = np.uint64(key_of(q, j, index_base))
            if k > out[o]:
                out[o] = k
    return out


def strip(window, entries, cells, threshold, range_=0, index_base=0):
    """T uint64 [n] of one window whose newest `cells` sub-fingerprints (already clamped) are new"""
    return strip_of_cells(len(window), tail_cells(window, entries, cells, range_), threshold, index_base)


def roll(prev, shift, strip_):
    """max(strip, prev shifted left by `shift` (already clamped to the row), zeros behind it); prev None: the strip"""
    strip_ = np.asarray(strip_, np.uint64)
    n = len(strip_)
    moved = np.zeros(n, np.uint64)
    if prev is not None and shift < n:
        moved[:n - shift] = np.asarray(prev, np.uint64)[shift:]
    return np.maximum(moved, strip_)


def lengths_of(keys, entry_lengths, index_base=0):
    """uint32, the shape of keys: the length of the entry a key names, 0 for a zero key or an index outside the corpus"""
    keys = np.asarray(keys, np.uint64)
    idx = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64) - index_base
    idx %= 1 << 32                                                   # (the device's 32-bit arithmetic)
    el = np.asarray(entry_lengths, np.uint32)
    ok = (keys != 0) & (idx < len(el))
    out = np.zeros(keys.shape, np.uint32)
    out[ok] = el[idx[ok]]
    return out


def update(prev, window, entries, new, max_new, threshold, range_=0, index_base=0):
    """(keys uint64 [n], lengths uint32 [n]) of one row of the call"""
    n = len(window)
    keys = roll(prev, min(int(new), n), strip(window, entries, clamp_new(new, max_new, n), threshold, range_, index_base))
    return keys, lengths_of(keys, [len(e) for e in entries], index_base)
