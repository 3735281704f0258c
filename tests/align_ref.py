"""numpy restatement of the alignment contract (LBAudioDetectiveCorpusQueryAligned and kin), for the tests.

For a query of n_q sub-fingerprints against an entry of n_e, fingerprint1 is the entry when n_q < n_e (case A, lag +offset) and
the query otherwise (case B, lag -offset).  q_o = float32 sum over i, in order, of ratio(fp1[i + o], fp2[i]) / n2, where a ratio
takes `possible` from fingerprint1's pairs inside the range (oracle/lbad_oracle.c: lbo_compare_sub, a missing Boolean of an odd
length counts as 0) and is np.float32(hits) / np.float32(possible), correctly rounded.  The score is max(0, max q_o), the offset
the first o that reaches it."""
import numpy as np


def _pair_words(bools, range_):
    """[n, L] Booleans -> P, N, NZ as [n, 2] uint64 pair masks (pair p at bit p & 63 of word p >> 6), NZ inside the range."""
    b = np.asarray(bools, np.uint8)
    n, L = b.shape
    lim = min(range_ if range_ else L, L)
    pairs = (L + 1) // 2
    padded = np.zeros((n, 2 * pairs), np.uint8)
    padded[:, :L] = b
    first, second = padded[:, 0::2], padded[:, 1::2]
    width = 128
    def words(bits):
        full = np.zeros((n, width), np.uint8)
        full[:, :pairs] = bits
        return np.packbits(full.reshape(n, 2, 64), axis=2, bitorder="little").view(np.uint64).reshape(n, 2)
    inside = np.zeros((1, width), np.uint8)
    inside[0, :(lim + 1) // 2] = 1
    P, N = words(first), words(second)
    rm = np.packbits(inside.reshape(1, 2, 64), axis=2, bitorder="little").view(np.uint64).reshape(1, 2)
    return P, N, (P | N) & rm


def profile(query, entry, range_):
    """Every q_o (float32, offset order) and the case ("A": the entry is fingerprint1) of query against entry."""
    query, entry = np.asarray(query, np.uint8), np.asarray(entry, np.uint8)
    entry_long = query.shape[0] < entry.shape[0]
    fp1, fp2 = (entry, query) if entry_long else (query, entry)
    n1, n2 = fp1.shape[0], fp2.shape[0]
    n_off = n1 - n2 + 1
    P1, N1, NZ1 = _pair_words(fp1, range_)
    P2, N2, _ = _pair_words(fp2, range_)
    possible = np.bitwise_count(NZ1).sum(axis=1).astype(np.float32)
    s = np.zeros(n_off, np.float32)
    for i in range(n2):
        rows = slice(i, i + n_off)
        d = (P1[rows] ^ P2[i]) | (N1[rows] ^ N2[i])
        hits = np.bitwise_count(NZ1[rows] & ~d).sum(axis=1).astype(np.float32)
        poss = possible[rows]
        r = np.zeros(n_off, np.float32)
        np.divide(hits, poss, out=r, where=poss > 0)
        s = s + r
    return s / np.float32(n2), entry_long


def align(query, entry, range_):
    """(score float32, lag) of query against entry."""
    q, entry_long = profile(query, entry, range_)
    best = np.float32(max(np.float32(0.0), q.max()))
    offset = int(np.flatnonzero(q == best)[0]) if q.max() == best else 0
    return best, (offset if entry_long else -offset)
