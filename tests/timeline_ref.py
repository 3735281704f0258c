"""numpy restatement of the recording timeline (LBAudioDetectiveCorpusRecordingTimelineKeysDevice and kin), for the tests, on
align_ref.profile: for every entry not longer than the query the profile's cells below the threshold become 0, the others the
key  cell bits << 32 | 0xFFFFFFFF - (index base + entry) ; out[o] is the running element-wise maximum over the entries (0 where
no cell counts), lengths[o] the winning entry's sub-fingerprints.  And the greedy segments over the per-offset winners."""
import numpy as np

from align_ref import profile


def profiles(query, entries, range_=0):
    """per entry: (sub-fingerprints, cells float32 [n_q - n_e + 1]) of an entry that takes part, None of one longer than the
    query.  The costly half of the reference: make it once per (query, range) and fold it at every threshold."""
    query = np.asarray(query, np.uint8)
    out = []
    for entry in entries:
        ne = len(entry)
        if ne > query.shape[0] or ne == 0:
            out.append(None)
            continue
        cells, entry_long = profile(query, entry, range_)
        assert not entry_long and len(cells) == query.shape[0] - ne + 1
        out.append((ne, cells))
    return out


def timeline(query, entries, threshold, range_=0, index_base=0):
    """(keys uint64 [n_q], lengths uint32 [n_q])"""
    return fold(len(query), profiles(query, entries, range_), threshold, index_base)


def fold(nq, profs, threshold, index_base=0):
    """(keys uint64 [n_q], lengths uint32 [n_q]) from profiles()"""
    keys = np.zeros(nq, np.uint64)
    lengths = np.zeros(nq, np.uint32)
    t = np.float32(threshold)
    for j, p in enumerate(profs):
        if p is None:
            continue
        ne, cells = p
        low = np.uint64(0xFFFFFFFF - (index_base + j))
        k = np.where(cells >= t, (cells.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low, np.uint64(0)).astype(np.uint64)
        better = k > keys[:len(k)]
        keys[:len(k)][better] = k[better]
        lengths[:len(k)][better] = ne
    return keys, lengths


def decode(keys, index_base=0):
    """(indices int64, scores float32): -1 / 0 for a zero key"""
    k = np.asarray(keys).astype(np.uint64)
    idx = np.where(k != 0, (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64) - index_base, -1)
    return idx.astype(np.int64), (k >> np.uint64(32)).astype(np.uint32).view(np.float32)


def segments(keys, lengths):
    """Greedy over the winners: descending key, ties to the lower offset; a winner is accepted when its span [o, o + length)
    meets no accepted span.  -> list of (start, index, score, length) sorted by start (index as the key holds it)."""
    keys = np.asarray(keys).astype(np.uint64)
    taken = set()
    out = []
    for o in sorted(range(len(keys)), key=lambda o: (-int(keys[o]), o)):
        if keys[o] == 0:
            break
        span = range(o, o + int(lengths[o]))
        if any(x in taken for x in span):
            continue
        taken.update(span)
        out.append((o, 0xFFFFFFFF - (int(keys[o]) & 0xFFFFFFFF), np.uint32(int(keys[o]) >> 32).view(np.float32), int(lengths[o])))
    return sorted(out)
