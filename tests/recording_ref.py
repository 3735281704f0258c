"""numpy restatement of every output of the recording family (the occurrences, the recording scores, top-K and threshold, the
timeline and the segments, single and batch), for the tests and tools/fuzz_recording.py, on align_ref.profile and timeline_ref.

cells(recording, entries, range) is the costly half: per entry (q float32 [n_off], entry_long), every cell of the pair.  Make it once
per (recording, range); every call of the family is a fold of it:

  occurrences   the cells q_o >= float32(t) -- with peaks only those with (o == 0 or q_o > q_(o-1)) and (o == last or q_o >= q_(o+1))
                -- in (entry, offset) order: key  q_o bits << 32 | 0xFFFFFFFF - (index base + entry), lag +o where the entry is the
                longer and -o otherwise; the true count, the list cut at the capacity, zeros behind it
  scores        max(0, max q_o) per entry and the lag of the LOWEST offset that reaches it
  top-K         the entries scoring above 0, score descending then index ascending, the first k; rows 0-padded, lag 0 for a zero key
  threshold     the entries whose score is >= float32(t) in ascending index, their lags, the true count, cut at the capacity
  timeline      timeline_ref.fold over the entries not longer than the recording
  segments      timeline_ref.segments as rows of `capacity` slots in start order, the true count

The batch forms are these row by row (batch()).  Each rule is a function of its own so that a test can replace exactly one."""
import numpy as np

import timeline_ref
from align_ref import profile

LOW = 0xFFFFFFFF


def cells(recording, entries, range_=0):
    """[(q float32 [n_off], entry_long)] per entry"""
    return [profile(recording, entry, range_) for entry in entries]


# ---- the rules, one function each ------------------------------------------------------------------------------------------------
def reaches(q, t):
    return q >= np.float32(t)


def peak_left(q):
    m = np.ones(len(q), bool)
    m[1:] = q[1:] > q[:-1]
    return m


def peak_right(q):
    m = np.ones(len(q), bool)
    m[:-1] = q[:-1] >= q[1:]
    return m


def best_offset(q, best):
    """the lowest offset that reaches the score (0 where no cell does: a score of 0 over negative or absent cells)"""
    at = np.flatnonzero(q == best)
    return int(at[0]) if len(at) else 0


def lag_of(offset, entry_long):
    return offset if entry_long else -offset


def occurrence_order(entry, offset):
    """the order of the list: entries ascending, offsets ascending inside an entry"""
    return np.lexsort((offset, entry))


def topk_order(scores):
    """score descending, then index ascending"""
    idx = np.arange(len(scores))
    return np.lexsort((idx, -scores.astype(np.float64)))


def fold(nq, profs, threshold, index_base=0):
    return timeline_ref.fold(nq, profs, threshold, index_base)


def greedy(keys, lengths):
    return timeline_ref.segments(keys, lengths)


# ---- the folds -------------------------------------------------------------------------------------------------------------------
def make_keys(values, index, index_base=0):
    """score bits << 32 | 0xFFFFFFFF - (index base + index)"""
    v = np.asarray(values, np.float32).reshape(-1)
    i = np.asarray(index, np.int64).reshape(-1) + int(index_base)
    return (v.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(LOW) - i.astype(np.uint64))


def _cut(capacity, *arrays):
    out = []
    for a in arrays:
        row = np.zeros(capacity, a.dtype)
        m = min(len(a), capacity)
        row[:m] = a[:m]
        out.append(row)
    return out


def occurrences_all(cs, t, peaks, index_base=0):
    """(keys uint64 [count], lags int32 [count]): the whole list"""
    entry, offset, value, lag = [], [], [], []
    for j, (q, entry_long) in enumerate(cs):
        m = reaches(q, t)
        if peaks:
            m = m & peak_left(q) & peak_right(q)
        o = np.flatnonzero(m)
        entry.append(np.full(len(o), j, np.int64))
        offset.append(o.astype(np.int64))
        value.append(q[o])
        lag.append(np.array([lag_of(int(x), entry_long) for x in o], np.int64))
    if not entry:
        return np.zeros(0, np.uint64), np.zeros(0, np.int32)
    entry, offset, value, lag = (np.concatenate(x) for x in (entry, offset, value, lag))
    order = occurrence_order(entry, offset)
    return make_keys(value[order], entry[order], index_base), lag[order].astype(np.int32)


def occurrences(cs, t, peaks, capacity, index_base=0):
    """(keys uint64 [capacity], lags int32 [capacity], count)"""
    keys, lags = occurrences_all(cs, t, peaks, index_base)
    return (*_cut(capacity, keys, lags), len(keys))


def scores(cs):
    """(scores float32 [n], lags int32 [n])"""
    sc = np.zeros(len(cs), np.float32)
    lags = np.zeros(len(cs), np.int32)
    for j, (q, entry_long) in enumerate(cs):
        sc[j] = max(np.float32(0.0), q.max())
        lags[j] = lag_of(best_offset(q, sc[j]), entry_long)
    return sc, lags


def topk(cs, k, index_base=0):
    """(keys uint64 [k], lags int32 [k])"""
    sc, lags = scores(cs)
    order = topk_order(sc)
    order = order[sc[order] > 0][:k]
    return tuple(_cut(k, make_keys(sc[order], order, index_base), lags[order]))


def threshold(cs, t, capacity, index_base=0):
    """(keys uint64 [capacity], lags int32 [capacity], count)"""
    sc, lags = scores(cs)
    at = np.flatnonzero(reaches(sc, t))
    return (*_cut(capacity, make_keys(sc[at], at, index_base), lags[at]), len(at))


def timeline(cs, nq, t, index_base=0):
    """(keys uint64 [nq], lengths uint32 [nq]); an entry takes part when it is not longer than the recording"""
    profs = [None if entry_long else (nq - len(q) + 1, q) for q, entry_long in cs]
    return fold(nq, profs, t, index_base)


def segments(keys, lengths, capacity):
    """(starts int32 [capacity], keys uint64 [capacity], lengths uint32 [capacity], count) of one timeline"""
    keys = np.asarray(keys).astype(np.uint64)
    spans = greedy(keys, lengths)
    starts = np.array([s[0] for s in spans], np.int32)
    return (*_cut(capacity, starts, keys[starts.astype(np.int64)], np.array([s[3] for s in spans], np.uint32)), len(spans))


def batch(rows):
    """the single results row by row: a list of tuples -> a tuple of stacked arrays (counts as an int64 vector)"""
    return tuple(np.stack([np.asarray(r[i]) for r in rows]) for i in range(len(rows[0])))
