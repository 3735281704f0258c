"""numpy restatement of the tail peaks contract (LBAudioDetectiveCorpusQueryPackedOccurrencesTailPeaksBatchKeysDevice), for the tests.

Recording r of n_q sub-fingerprints with d_r = min(new count, max_new, n_q) new ones, against the entries of a ragged corpus: entry
j of 1 <= n_j <= n_q sub-fingerprints takes part, last = n_q - n_j.  Its JUDGED cells are the offsets max(0, last - d_r) .. last - 1
-- each judged one sub-fingerprint late, when its right neighbour exists -- and with `final` the newest cell `last` too.  A judged
cell matches when q_o >= threshold as float32, (o == 0 or q_o > q_(o-1)) and (o == last or q_o >= q_(o+1)), q being
align_ref.profile's values of the WINDOW.  A row is the matches in (entry ascending, offset ascending) order: key = q_o bits << 32 |
0xFFFFFFFF - (index_base + j), lag = -o.  The rule is written out here cell by cell; recording_ref's vector form is what
test_occurrences_tail_peaks_cpu.py holds it against."""
import numpy as np

from align_ref import profile
from occurrences_tail_ref import clamp_new, key_of  # noqa: F401  (clamp_new: the tests')


def judged_range(n_q, n_j, d, final):
    """the offsets of (recording of n_q, entry of n_j) that a call behind a push of d new sub-fingerprints judges"""
    if n_j > n_q or n_j == 0:
        return range(0)
    last = n_q - n_j
    return range(max(0, last - max(int(d), 0)), last + 1 if final else last)


def profiles(recording, entries, range_=0):
    """the costly half, once per (recording, range): [(entry j, q float32 [n_q - n_j + 1])] for the entries that take part"""
    recording = np.asarray(recording, np.uint8)
    n_q = recording.shape[0]
    out = []
    for j, entry in enumerate(entries):
        if len(entry) == 0 or len(entry) > n_q:
            continue
        q, entry_long = profile(recording, entry, range_)
        assert not entry_long and len(q) == n_q - len(entry) + 1 and q.dtype == np.float32
        out.append((j, q))
    return out


def is_peak(q, o):
    """the occurrences' peak rule at offset o of one profile: the first cell of a plateau"""
    left = o == 0 or q[o] > q[o - 1]
    right = o == len(q) - 1 or q[o] >= q[o + 1]
    return bool(left and right)


def judged_cells(profs, n_q, d, final):
    """every judged cell of a recording's row, matching or not: [(entry j, offset o, q_o float32, peak)] in the row's order"""
    cells = []
    for j, q in profs:
        for o in judged_range(n_q, n_q - len(q) + 1, d, final):
            cells.append((j, o, q[o], is_peak(q, o)))
    return cells


def peaks_row(cells, threshold, capacity, index_base=0):
    """(keys uint64 [capacity], lags int32 [capacity], true count) of one recording from its judged cells"""
    t = np.float32(threshold)
    hits = [(j, o, q) for (j, o, q, peak) in cells if peak and q >= t]
    keys = np.zeros(capacity, np.uint64)
    lags = np.zeros(capacity, np.int32)
    for slot, (j, o, q) in enumerate(hits[:capacity]):
        keys[slot] = key_of(q, j, index_base)
        lags[slot] = -o
    return keys, lags, len(hits)


def peaks_rows(recordings, entries, new_counts, max_new, final, threshold, capacity, range_=0, index_base=0):
    """(keys uint64 [R, capacity], lags int32 [R, capacity], counts int64 [R]) of a whole call"""
    R = len(recordings)
    keys = np.zeros((R, capacity), np.uint64)
    lags = np.zeros((R, capacity), np.int32)
    counts = np.zeros(R, np.int64)
    for r, rec in enumerate(recordings):
        d = clamp_new(new_counts[r], max_new, len(rec))
        cells = judged_cells(profiles(rec, entries, range_), len(rec), d, final)
        keys[r], lags[r], counts[r] = peaks_row(cells, threshold, capacity, index_base)
    return keys, lags, counts


def filter_batch_row(keys, lags, count, entry_lengths, n_q, d, final, capacity, index_base=0):
    """one row of the batch occurrences call with peaks ON (NOT cut: count <= len(keys)) with only the judged cells kept, as
    peaks_row gives it"""
    assert count <= len(keys), "the batch row must hold every match for the filter to be exact"
    out_k = np.zeros(capacity, np.uint64)
    out_l = np.zeros(capacity, np.int32)
    kept = 0
    for k, lag in zip(np.asarray(keys, np.uint64)[:count], np.asarray(lags, np.int32)[:count]):
        j = 0xFFFFFFFF - (int(k) & 0xFFFFFFFF) - index_base
        n_j = int(entry_lengths[j])
        if n_j <= n_q and lag <= 0 and -int(lag) in judged_range(n_q, n_j, d, final):
            if kept < capacity:
                out_k[kept], out_l[kept] = k, lag
            kept += 1
    return out_k, out_l, kept


def life_calls(pushes, window):
    """a channel's life as calls: fed in `pushes`, a call with final off behind every push on a window of min(total so far,
    window(total, d)) sub-fingerprints, and one final call with new count 0 on the last window -> [(total, n, d, final)]"""
    calls, fed = [], 0
    for d, final in [(int(d), False) for d in pushes] + [(0, True)]:
        fed += d
        if fed:
            calls.append((fed, min(fed, int(window(fed, d))), d, final))
    return calls


def life_cells(recording, entries, pushes, window, range_=0):
    """every judged cell of every call of a channel's life, matching or not: [(call k, entry j, absolute position, q_o, peak)]"""
    recording = np.asarray(recording, np.uint8)
    assert sum(pushes) == recording.shape[0]
    out = []
    for k, (fed, n, d, final) in enumerate(life_calls(pushes, window)):
        profs = profiles(recording[fed - n:fed], entries, range_)
        out.extend((k, j, fed - n + o, q, peak) for (j, o, q, peak) in judged_cells(profs, n, min(d, n), final))
    return out


def life(cells, threshold):
    """[(entry j, absolute position, q bits)] of every match of every call, in call order, from life_cells' list"""
    t = np.float32(threshold)
    return [(j, at, int(np.float32(q).view(np.uint32))) for (_k, j, at, q, peak) in cells if peak and q >= t]
