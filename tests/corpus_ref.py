"""numpy model of a corpus handle and of every corpus call outside the recording family (queries, joins, groups, removal, gather,
entry ids), for the tests and tools/fuzz_corpus.py.  No GPU, no torch, no call into the library or the C oracle: the contract is
include/lbaudiodetective.h as it words it.

A Model holds the corpus as a list of (uid, Booleans [n_e, L]) entries, an optional id per entry, L, and n_sub for a uniform
corpus (0: ragged).  It is mutated in step with a device corpus (append, remove, remove_keys, set_ids) and every read is a fold
of its entries' scores:

  scores      score and lag of a query against an entry: align_ref's rule (the shorter slides along the longer, fingerprint1 is the
              entry when the query is shorter and the query otherwise, q_o = float32 sum in order of hits / possible, / steps; score =
              max(0, max q_o), offset = the LOWEST o that reaches it).  A uniform corpus queried at its own n_sub is the equal-length
              case.  score_block() is that rule vectorised over all entries of one length (the ratio of every pair of sub-fingerprints
              once, then an in-order float32 cumulative sum along every diagonal); the CPU test holds it to align_ref.align bit for
              bit.  The model caches (query id, uid) -> (score, first offset, last offset, entry longer), so a step recomputes only
              entries that are new.
  top-1       the highest key  score bits << 32 | 0xFFFFFFFF - (base + index)  over all entries: the lowest index wins ties; a best
              score of 0 gives index -1, score 0 on the host and, as a key, score word 0 over the lowest index; an empty corpus 0
  top-K       entries with score > 0, score descending, lowest index first, cut at K; zero keys, -1 / 0 and lag 0 behind them
  threshold   score >= t as float32, ascending index, cut at the capacity; the count is the true total, zeros behind the matches
  joins       ordered pairs (row, entry) at the threshold as CSR: rows ascending, entries ascending inside a row; offsets never cut,
              keys (and a ragged join's lags) cut at the capacity
  labels      the lowest index of the connected component over pairs matching in EITHER direction; dedup keeps each group's first
  removal     the kept entries close up in order, ids move with their entries, the map is the new index or 0xFFFFFFFF
  keys        a zero key, a key outside [base, base + count) and a repeated key name nothing (more)
  gather      packed entries and offsets in LIST order, an empty row for a key that names nothing
  ids         0 = none; appended entries have id 0; keys_from_ids gives score word 1.0f and the LOWEST index with that id

Each rule is a function of its own so that a test can replace exactly one."""
import numpy as np

from align_ref import _pair_words

LOW = 0xFFFFFFFF
GONE = 0xFFFFFFFF
ONE_BITS = 0x3F800000


# ---- the rules, one function each ------------------------------------------------------------------------------------------------
def low_word(index, index_base):
    """the low word of a key: 0xFFFFFFFF - (index base + index)"""
    return np.uint64(LOW) - (np.asarray(index, np.int64) + int(index_base)).astype(np.uint64)


def reaches(scores, t):
    return scores >= np.float32(t)


def admitted(scores):
    """top-K takes scores above 0 only"""
    return scores > 0


def topk_order(scores):
    """score descending, then index ascending"""
    return np.lexsort((np.arange(len(scores)), -scores.astype(np.float64)))


def threshold_order(at):
    """ascending index"""
    return np.sort(at)


def best_offset(first, last):
    """the LOWEST offset that reaches the score"""
    return first


def lag_of(offset, entry_long):
    return np.where(entry_long, offset, -offset).astype(np.int32)


def kept_after(n, indices):
    """the keep mask of a removal of `indices` (valid, duplicates allowed) from n entries"""
    keep = np.ones(n, bool)
    keep[np.asarray(indices, np.int64)] = False
    return keep


def moved_ids(ids, keep):
    """ids move with their entries"""
    return [i for i, k in zip(ids, keep) if k]


def appended_id(stale, position):
    """the id of an entry appended at `position`: none, whatever stood there before a removal"""
    return 0


def pair_skipped(row, entry, skip_same_index):
    return bool(skip_same_index) and row == entry


def edges_of(pairs):
    """the undirected edges of ordered matching pairs: a match in either direction joins two entries"""
    return pairs


def group_keeper(members):
    """the entry of a group that a dedup keeps: the first"""
    return members[0]


def gather_rows(named):
    """the rows of a gather: list order"""
    return named


# ---- scores -----------------------------------------------------------------------------------------------------------------------
def _ratios(W1, W2):
    """R[a, b] = float32 ratio of fingerprint1's sub-fingerprint a against fingerprint2's b (possible from fingerprint1's pairs)"""
    P1, N1, NZ1 = W1
    P2, N2, _ = W2
    hits = np.zeros((len(P1), len(P2)), np.uint16)
    for w in range(P1.shape[1]):
        d = (P1[:, None, w] ^ P2[None, :, w]) | (N1[:, None, w] ^ N2[None, :, w])
        hits += np.bitwise_count(NZ1[:, None, w] & ~d)
    hits = hits.astype(np.float32)
    poss = np.broadcast_to(np.bitwise_count(NZ1).sum(axis=1).astype(np.float32)[:, None], hits.shape)
    r = np.zeros(hits.shape, np.float32)
    np.divide(hits, poss, out=r, where=poss > 0)
    return r


def score_block(query, entries, range_):
    """(scores float32 [n], first offset, last offset, entry longer [n]) of one query against entries of ANY lengths: one pass per
    distinct length"""
    n = len(entries)
    sc, first, last = np.zeros(n, np.float32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    longer = np.zeros(n, bool)
    if n == 0:
        return sc, first, last, longer
    nq = len(query)
    lens = np.array([len(e) for e in entries], np.int64)
    longer = lens > nq
    starts = np.zeros(n, np.int64)                                           # (of an entry's records inside its own side's block)
    for side in (longer, ~longer):
        starts[side] = np.concatenate([[0], np.cumsum(lens[side])])[:-1]
    WQ = _pair_words(query, range_)
    words = lambda side: _pair_words(np.concatenate([e for e, s in zip(entries, side) if s]), range_)
    RA = _ratios(words(longer), WQ) if longer.any() else None                # fingerprint1 = the entry
    RB = _ratios(WQ, words(~longer)) if (~longer).any() else None            # fingerprint1 = the query
    for m in np.unique(lens):
        g = np.flatnonzero(lens == m)
        S = starts[g][:, None, None]
        if m > nq:
            o, i = np.arange(m - nq + 1)[None, :, None], np.arange(nq)[None, None, :]
            D, steps = RA[S + o + i, i], nq
        else:
            o, i = np.arange(nq - m + 1)[None, :, None], np.arange(m)[None, None, :]
            D, steps = RB[o + i, S + i], int(m)
        q = np.cumsum(D, axis=2, dtype=np.float32)[:, :, -1] / np.float32(steps)
        best = np.maximum(np.float32(0.0), q.max(axis=1))
        hit = q == best[:, None]
        sc[g] = best
        first[g] = np.where(hit.any(axis=1), hit.argmax(axis=1), 0)
        last[g] = np.where(hit.any(axis=1), hit.shape[1] - 1 - hit[:, ::-1].argmax(axis=1), 0)
    return sc, first, last, longer


def bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


def make_keys(scores, index, index_base=0):
    """score bits << 32 | low word"""
    return (bits(scores).astype(np.uint64) << np.uint64(32)) | low_word(np.asarray(index).reshape(-1), index_base)


def key_indices(keys, index_base, count):
    """the entries a key list names, as the removal, the gather and the ids read it: -1 for a zero key and for an index outside
    [base, base + count)"""
    keys = np.asarray(keys).astype(np.uint64).reshape(-1)
    idx = (np.int64(LOW) - (keys & np.uint64(LOW)).astype(np.int64)) - int(index_base)
    ok = (keys != 0) & (idx >= 0) & (idx < count)
    return np.where(ok, idx, -1)


def pack(bools):
    """[n, L] Booleans -> [n, 32] bytes, Boolean b at bit b & 31 of word b >> 5"""
    b = np.asarray(bools, np.uint8)
    full = np.zeros((b.shape[0], 256), np.uint8)
    full[:, :b.shape[1]] = b
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little"))


def _cut(capacity, a):
    row = np.zeros(capacity, a.dtype)
    m = min(len(a), capacity)
    row[:m] = a[:m]
    return row


# ---- the model --------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, L, n_sub, range_=0):
        self.L, self.n_sub, self.range = L, n_sub, range_
        self.entries, self.ids, self.stale = [], None, {}                      # [(uid, bools)], ids or None, position -> an old id
        self.uid, self.cache, self.version, self.whole = 0, {}, 0, {}          # (whole: qid -> the arrays at this version)

    def __len__(self):
        return len(self.entries)

    @property
    def ragged(self):
        return self.n_sub == 0

    @property
    def total(self):
        return sum(len(e) for _, e in self.entries)

    def bools(self):
        return [e for _, e in self.entries]

    # -- mutations
    def append(self, new):
        self.version += 1
        for e in new:
            if self.ids is not None:
                self.ids.append(appended_id(self.stale, len(self.entries)))
            self.entries.append((self.uid, np.asarray(e, np.uint8)))
            self.uid += 1

    def set_ids(self, first, ids):
        if len(ids) == 0:
            return
        if self.ids is None:
            self.ids = [0] * len(self.entries)
        self.ids[first:first + len(ids)] = [int(x) for x in ids]

    def remove(self, indices):
        """-> (removed, map uint32 [old count])"""
        n = len(self.entries)
        self.version += 1
        keep = kept_after(n, indices)
        new = np.where(keep, np.cumsum(keep) - 1, GONE).astype(np.uint32)
        if self.ids is not None:
            moved = moved_ids(self.ids, keep)
            kept = int(keep.sum())
            moved = (moved + [0] * n)[:kept] if len(moved) < kept else moved[:kept]
            self.stale = {p: self.ids[p] for p in range(kept, n)}
            self.ids = moved
        self.entries = [e for e, k in zip(self.entries, keep) if k]
        return int(n - keep.sum()), new

    def remove_keys(self, keys, index_base=0):
        at = key_indices(keys, index_base, len(self.entries))
        return self.remove(np.unique(at[at >= 0]))

    # -- scores
    def scores(self, qid, query):
        """(scores float32 [n], lags int32 [n]) of the query against every entry, through the cache"""
        if self.whole.get(qid, (None,))[0] == self.version:
            sc, first, last, longer = self.whole[qid][1:]
            return sc, lag_of(best_offset(first, last), longer)
        mine = self.cache.setdefault(qid, {})
        new = [(u, e) for u, e in self.entries if u not in mine]
        if new:
            sc, first, last, longer = score_block(query, [e for _, e in new], self.range)
            for k, (u, _) in enumerate(new):
                mine[u] = (sc[k], first[k], last[k], longer[k])
        n = len(self.entries)
        got = [mine[u] for u, _ in self.entries]
        sc = np.array([g[0] for g in got], np.float32).reshape(n)
        first, last = np.array([g[1] for g in got], np.int64).reshape(n), np.array([g[2] for g in got], np.int64).reshape(n)
        longer = np.array([g[3] for g in got], bool).reshape(n)
        self.whole[qid] = (self.version, sc, first, last, longer)
        return sc, lag_of(best_offset(first, last), longer)

    # -- queries
    def topk(self, sc, lags, k, index_base=0):
        """(keys uint64 [k], lags int32 [k], indices int64 [m], scores float32 [m])"""
        order = topk_order(sc)
        order = order[admitted(sc[order])][:k]
        return _cut(k, make_keys(sc[order], order, index_base)), _cut(k, lags[order]), order.astype(np.int64), sc[order]

    def top1(self, sc, index_base=0):
        """(key, index, score): the key is the highest over ALL entries (an empty corpus: 0) -- over entries that all score 0 that
        is score word 0 and the lowest index --, the host answer of a best score of 0 is index -1, score 0"""
        if len(sc) == 0:
            return np.uint64(0), -1, np.float32(0.0)
        j = int(topk_order(sc)[0])
        return make_keys(sc[j], j, index_base)[0], (j if sc[j] > 0 else -1), sc[j]

    def threshold(self, sc, lags, t, capacity, index_base=0):
        """(keys uint64 [capacity], lags int32 [capacity], count, indices [m], scores [m])"""
        at = threshold_order(np.flatnonzero(reaches(sc, t)))
        m = min(len(at), capacity)
        return _cut(capacity, make_keys(sc[at], at, index_base)), _cut(capacity, lags[at]), len(at), at[:m].astype(np.int64), sc[at][:m]

    # -- joins
    def join(self, rows, t, capacity, skip_same_index, index_base=0):
        """rows: [(row index, qid, bools)] -> (keys uint64 [capacity], lags int32 [capacity], offsets int64 [rows + 1], pairs)"""
        keys, lags, offsets, pairs = [], [], [0], []
        for r, qid, q in rows:
            sc, lg = self.scores(qid, q)
            at = [j for j in np.flatnonzero(reaches(sc, t)) if not pair_skipped(r, int(j), skip_same_index)]
            at = np.array(at, np.int64)
            keys.append(make_keys(sc[at], at, index_base))
            lags.append(lg[at])
            pairs += [(r, int(j)) for j in at]
            offsets.append(offsets[-1] + len(at))
        keys = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
        lags = np.concatenate(lags) if lags else np.zeros(0, np.int32)
        return _cut(capacity, keys), _cut(capacity, lags.astype(np.int32)), np.array(offsets, np.int64), pairs

    def self_rows(self, first, count):
        return [(i, ("e", self.entries[i][0]), self.entries[i][1]) for i in range(first, first + count)]

    def labels(self, t):
        """(labels int32 [n], groups): the lowest index of every entry's component of the self-join's match graph"""
        n = len(self.entries)
        pairs = self.join(self.self_rows(0, n), t, 1, True)[3]
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for a, b in edges_of(pairs):
            a, b = find(a), find(b)
            if a != b:
                parent[max(a, b)] = min(a, b)
        lab = np.array([find(i) for i in range(n)], np.int32).reshape(n)
        return lab, len(set(lab.tolist()))

    def dedup(self, t):
        """-> (removed, labels before)"""
        lab, _ = self.labels(t)
        groups = {}
        for i, g in enumerate(lab.tolist()):
            groups.setdefault(g, []).append(i)
        keepers = {group_keeper(m) for m in groups.values()}
        removed, _ = self.remove([i for i in range(len(lab)) if i not in keepers])
        return removed, lab

    # -- gather and ids
    def gather(self, named, capacity=None):
        """named: entry indices, -1 for an empty row -> (packed uint8 [capacity, 32] -- None: the total --, offsets int64 [n + 1])"""
        named = gather_rows(np.asarray(named, np.int64))
        sizes = [len(self.entries[i][1]) if i >= 0 else 0 for i in named]
        rows = [self.entries[i][1] for i in named if i >= 0]
        flat = pack(np.concatenate(rows)) if rows else np.zeros((0, 32), np.uint8)
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        return flat if capacity is None else flat[:capacity], offsets

    def entry_ids(self):
        return np.array(self.ids if self.ids is not None else [0] * len(self.entries), np.uint64).reshape(len(self.entries))

    def ids_from_keys(self, keys, index_base=0):
        at = key_indices(keys, index_base, len(self.entries))
        ids = self.entry_ids()
        return np.array([int(ids[i]) if i >= 0 else 0 for i in at], np.uint64).reshape(len(at))

    def keys_from_ids(self, ids, index_base=0):
        """score word 1.0f, the LOWEST index with that id; the zero key for id 0, an unknown id, a corpus without ids"""
        mine = {}
        for i, x in enumerate(self.entry_ids().tolist()):
            if x and self.ids is not None:
                mine.setdefault(x, i)
        out = [(ONE_BITS << 32) | int(low_word(mine[int(x)], index_base)) if int(x) in mine else 0 for x in ids]
        return np.array(out, np.uint64).reshape(len(out))
