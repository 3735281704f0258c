"""numpy restatement of the recording tail contract (LBAudioDetectiveCorpusRecordingPackedScoresTailBatchDevice and the two key forms
behind it), for the tests: the fold over occurrences_tail_ref.tail_cells -- the cells a push has completed -- built from
recording_ref's rules.

For recording r and entry j:  score = max(+0, the largest q_o of the pair's tail cells) as float32, +0 where the pair has none;
lag = -(the LOWEST tail offset whose q_o equals the score) -- recording_ref.best_offset / lag_of restricted to the tail cells, the
entry never the longer --, 0 where no tail cell equals it.  The key forms are recording_ref's selections over a row of scores: the
top-K (score above 0, descending, the lowest index first, zeros behind) and the threshold row (ascending index, the true count, cut
at the capacity, zeros behind)."""
import numpy as np

import occurrences_tail_ref as tail
import recording_ref as rr


def fold_cells(cells, n_entries):
    """(scores float32 [n_entries], lags int32 [n_entries]) of one recording from its tail cells [(j, o, q)]"""
    sc = np.zeros(n_entries, np.float32)
    lags = np.zeros(n_entries, np.int32)
    per_entry = {}
    for j, o, q in cells:
        per_entry.setdefault(j, []).append((o, q))
    for j, lst in per_entry.items():
        offs = np.array([o for (o, _q) in lst], np.int64)
        q = np.array([v for (_o, v) in lst], np.float32)
        assert (np.diff(offs) == 1).all()                 # a pair's tail cells are consecutive offsets, ascending
        sc[j] = max(np.float32(0.0), q.max())
        at = np.flatnonzero(q == sc[j])                   # best_offset's rule on the tail cells alone
        lags[j] = rr.lag_of(int(offs[at[0]]), False) if len(at) else 0
    return sc, lags


def scores(recording, entries, d, range_=0):
    """(scores, lags) of one recording with d new sub-fingerprints (already clamped)"""
    return fold_cells(tail.tail_cells(recording, entries, d, range_), len(entries))


def topk_row(sc, lags, k, index_base=0):
    """(keys uint64 [k], lags int32 [k]): recording_ref.topk's selection over a row of scores"""
    order = rr.topk_order(sc)
    order = order[sc[order] > 0][:k]
    return tuple(rr._cut(k, rr.make_keys(sc[order], order, index_base), lags[order].astype(np.int32)))


def threshold_row(sc, lags, t, capacity, index_base=0):
    """(keys uint64 [capacity], lags int32 [capacity], true count): recording_ref.threshold's selection over a row of scores"""
    at = np.flatnonzero(rr.reaches(sc, t))
    return (*rr._cut(capacity, rr.make_keys(sc[at], at, index_base), lags[at].astype(np.int32)), len(at))


def fold_occurrence_row(keys, lags, count, capacity):
    """a row of the tail OCCURRENCES call (not cut: count <= len(keys)) folded to the threshold row: per distinct entry the key of its
    largest cell and the lag of the lowest offset that reaches it, in ascending index"""
    assert count <= len(keys), "the occurrences row must hold every match for the fold to be exact"
    k = np.asarray(keys, np.uint64)[:count]
    lg = np.asarray(lags, np.int32)[:count]
    best = {}
    for key, lag in zip(k.tolist(), lg.tolist()):         # (entry ascending, offset ascending): the first of equal keys is the lowest offset
        j = 0xFFFFFFFF - (key & 0xFFFFFFFF)
        if j not in best or key > best[j][0]:
            best[j] = (key, lag)
    order = sorted(best)
    out_k = np.array([best[j][0] for j in order], np.uint64)
    out_l = np.array([best[j][1] for j in order], np.int32)
    return (*rr._cut(capacity, out_k, out_l), len(order))


def rows(recordings, entries, new_counts, max_new, range_=0):
    """(scores float32 [R, n], lags int32 [R, n]) of a whole call"""
    out = [scores(rec, entries, tail.clamp_new(new_counts[r], max_new, len(rec)), range_) for r, rec in enumerate(recordings)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
