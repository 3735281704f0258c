"""Brute-force reference of the occurrence segments call (LBAudioDetectiveOccurrenceSegmentsFromKeysDevice): plain Python over a set
of taken offsets, independent of lbaudiodetective_amd.occurrence_segments (numpy, lexsort, a boolean mask) and of the kernel (a
bitonic sort, bit masks).  The contract is restated here from the header, not taken from either."""

INT32_MIN = -(1 << 31)


def span(lag, length, per):
    """[s, e) of a slot in the recording's offsets, or None when the slot is no candidate by its geometry"""
    lag, length, per = int(lag), int(length), int(per)
    at = -lag                                  # Python integers: any 32-bit lag word is harmless
    s = at if at > 0 else 0
    e = at + length if at + length < per else per
    if length == 0 or s >= per or e <= s:
        return None
    return s, e


def segments(keys, lags, lengths, per, count=None):
    """The accepted spans of ONE row as a list of (start, key, lag, length, slot) in ascending start order.  keys: unsigned 64-bit
    values, lags: signed 32-bit, lengths: unsigned 32-bit, one per slot; count: the row's count as the occurrences call wrote it
    (slots from min(count, slots) on are ignored), None for every slot."""
    slots = len(keys)
    m = slots if count is None else min(int(count), slots)
    cand = []
    for p in range(m):
        k = int(keys[p])
        if k == 0:
            continue
        se = span(lags[p], lengths[p], per)
        if se is None:
            continue
        cand.append((-k, se[0], p, se[1]))
    cand.sort()                                # (-key, start, slot): descending key, then lower start, then lower slot
    taken = set()
    kept = []
    for nk, s, p, e in cand:
        if any(o in taken for o in range(s, e)):
            continue
        taken.update(range(s, e))
        kept.append((s, -nk, int(lags[p]), int(lengths[p]), p))
    kept.sort()
    return kept


def rows(keys, lags, lengths, per, out_capacity, counts=None):
    """The call's output blocks for a batch as nested lists: (starts, keys, lags, lengths) each [recordings][out_capacity] with zeros
    behind the spans, and the true counts [recordings]."""
    st, ks, lg, ln, cn = [], [], [], [], []
    for r in range(len(keys)):
        kept = segments(keys[r], lags[r], lengths[r], per, None if counts is None else counts[r])
        cn.append(len(kept))
        kept = kept[:out_capacity]
        pad = [0] * (out_capacity - len(kept))
        st.append([x[0] for x in kept] + pad)
        ks.append([x[1] for x in kept] + pad)
        lg.append([x[2] for x in kept] + pad)
        ln.append([x[3] for x in kept] + pad)
    return st, ks, lg, ln, cn
