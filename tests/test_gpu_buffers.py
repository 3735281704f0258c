"""GPU tests of who owns the device and pinned memory behind a detective and a corpus (csrc/buffers.hpp).

1. Every owner is released: LBAudioDetectiveDebugLiveBytes reads the same after a handle that went through every entry point
   with scratch of its own has been disposed as it did before the handle was made, and more while it is alive.
2. The scratch of the handle-taking corpus calls regrows under queued work: a small call, a larger one on a second stream, the
   small one again, nothing awaited in between.

Every result on the way is compared with the oracle: per-entry scores from oracle.corpus_best_ragged (a uniform corpus is a
ragged one of equal counts), the lists they imply (score descending, lowest index first, scores above 0) and, for lags, the
restatement in tests/align_ref.py, whose score is pinned to the oracle's for every pair that is used."""
import os

import numpy as np
import pytest

import align_ref

pytestmark = pytest.mark.gpu

SEED = 0x4C424148
L = 200
N_UNIFORM, N_SUB = 3000, 5
N_RAGGED = 500
BIRDS = os.path.join(os.path.dirname(__file__), "golden", "birds")


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _packed(oracle, bools):
    """[..., L] Booleans -> the library's 32-byte packed rows (uint8)"""
    return np.ascontiguousarray(oracle.pack_bools(bools)).view(np.uint8).reshape(bools.shape[:-1] + (32,))


def _near(rng, base, flips):
    q = base.copy()
    for _ in range(flips):
        q[rng.integers(0, q.shape[0]), rng.integers(0, q.shape[1])] ^= 1
    return q


class Reference:
    """A corpus on the host and what the oracle says about queries against it; computed once per query, never changed."""

    def __init__(self, oracle, flat, counts):
        self.oracle, self.flat, self.counts = oracle, flat, np.asarray(counts, np.uint32)
        self.off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.cache = {}

    def entry(self, e):
        return self.flat[self.off[e]:self.off[e + 1]]

    def scores(self, q):
        key = q.tobytes()
        if key not in self.cache:
            s = self.oracle.corpus_best_ragged(q, (self.flat, self.counts), L, nthreads=16, want_scores=True)[2]
            s = np.array(s, np.float32)
            s.setflags(write=False)
            self.cache[key] = s
        return self.cache[key]

    def topk(self, q, k):
        """(indices, scores) of the k best entries scoring above 0: score descending, equal scores lowest index first"""
        s = self.scores(q)
        order = np.lexsort((np.arange(len(s)), -s))
        order = order[s[order] > 0][:k]
        return order.astype(np.int64), s[order]

    def top1(self, q):
        idx, sc = self.topk(q, 1)
        return (int(idx[0]), float(sc[0])) if len(idx) else (-1, 0.0)

    def lag(self, q, e):
        score, lag = align_ref.align(q, self.entry(e), 0)
        assert _bits(score) == _bits(self.scores(q)[e]), "the restatement disagrees with the oracle"
        return lag

    def check_keys(self, lb, q, keys_row, k, what, lags_row=None):
        """one row of top-K keys (and its lags) against the oracle"""
        idx, sc = lb.decode_topk_keys(keys_row)
        wi, ws = self.topk(q, k)
        assert np.array_equal(idx, wi) and np.array_equal(_bits(sc), _bits(ws)), (what, idx, wi)
        if lags_row is not None:
            want = [self.lag(q, int(e)) for e in wi]
            assert list(lags_row[:len(wi)]) == want and not np.any(lags_row[len(wi):]), (what, lags_row, want)

    def check_key(self, lb, q, key, what):
        """a top-1 key as LBAudioDetectiveCorpusDecodeKey reads it"""
        idx, sc = lb.Corpus.decode_key(int(key))
        wi, ws = self.top1(q)
        assert idx == wi and (idx < 0 or _bits(sc) == _bits(ws)), (what, idx, sc, wi, ws)


@pytest.fixture(scope="module")
def uniform_ref(oracle):
    host = oracle.synth_corpus(SEED, 0, N_UNIFORM, N_SUB, L)
    host[1700] = host[23]                                     # a duplicate: the lower index wins
    host[9] = 0                                               # an all-zero entry
    return Reference(oracle, host.reshape(-1, L), np.full(N_UNIFORM, N_SUB, np.uint32))


@pytest.fixture(scope="module")
def ragged_ref(oracle):
    counts = np.random.default_rng(11).integers(4, 41, N_RAGGED).astype(np.uint32)
    return Reference(oracle, oracle.synth_ragged_entries(SEED + 1, 0, counts, L), counts)


def _corpus(lb, gpu, oracle, ref, ragged):
    rows = gpu.from_numpy(_packed(oracle, ref.flat)).cuda()
    if ragged:
        c = lb.Corpus.ragged(L, len(ref.counts), int(ref.counts.sum()))
        c.append_ragged_packed_device(rows, ref.counts)
    else:
        c = lb.Corpus(L, N_SUB, len(ref.counts))
        c.append_packed_device(rows.reshape(len(ref.counts), N_SUB, 32))
    gpu.cuda.synchronize()
    return c


def _warm_up(lb):
    """the process-wide contexts that are never freed (the pair compare's, the Frame API's) exist before a reading is taken"""
    a = lb.Fingerprint.from_bools(np.ones((2, L), np.uint8))
    assert a.compare_to_fingerprint(a, L) == 1.0
    f = lb.Frame(4)
    for i in range(4):
        f.set_row(np.arange(4, dtype=np.float32) + i, i)
    f.decompose()
    return lb.debug_live_bytes()


# ---- 1. every owner is released ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_corpus_releases_everything_it_owned(lb, gpu, oracle, uniform_ref, ragged_ref, tmp_path, ragged):
    ref = ragged_ref if ragged else uniform_ref
    rng = np.random.default_rng(21 + ragged)
    before = _warm_up(lb)
    c = _corpus(lb, gpu, oracle, ref, ragged)
    made = lb.debug_live_bytes()
    assert made[0] > before[0] and made[1] > before[1]        # the entries and the key block of the sharded query

    per = 21 if ragged else N_SUB
    src = [int(e) for e in np.flatnonzero(ref.counts >= per)[[0, 5, 20]]] if ragged else [23, 1700, 2999]
    qs = [_near(rng, ref.entry(e)[:per], f) for e, f in zip(src, (0, 12, 40))]
    qs.append((rng.random((per, L)) < 0.5).astype(np.uint8))
    fps = [lb.Fingerprint.from_bools(q) for q in qs]
    k = 4

    for q, fq in zip(qs, fps):                                # the polled query (uniform: the pinned, mapped result word)
        assert c.query(fq) == ref.top1(q)
    key = gpu.empty(1, dtype=gpu.int64, device="cuda")
    c.set_kernel_variant(1)                                   # uniform: the generic scan and its staging pair
    c.query_key_device(fps[1], key)
    ref.check_key(lb, qs[1], key.cpu().numpy()[0], "generic scan")
    c.set_kernel_variant(0)
    assert c.query_batch(fps) == [ref.top1(q) for q in qs]
    for q, (idx, sc) in zip(qs, c.query_batch_topk(fps, k)):
        wi, ws = ref.topk(q, k)
        assert np.array_equal(idx, wi) and np.array_equal(_bits(sc), _bits(ws))
    for q, (idx, sc, lags) in zip(qs, c.query_batch_topk_aligned(fps, k)):
        wi, ws = ref.topk(q, k)
        assert np.array_equal(idx, wi) and np.array_equal(_bits(sc), _bits(ws))
        assert list(lags) == [ref.lag(q, int(e)) for e in wi]
    wi, ws = ref.top1(qs[1])
    assert c.query_aligned(fps[1]) == (wi, ws, ref.lag(qs[1], wi))
    prof, first = c.match_profile(fps[1], src[2])
    want_prof, _ = align_ref.profile(qs[1], ref.entry(src[2]), 0)
    assert first == 0 and np.array_equal(_bits(prof), _bits(want_prof))
    assert _bits(max(np.float32(0), want_prof.max())) == _bits(ref.scores(qs[1])[src[2]])
    assert np.array_equal(_bits(c.scores_device(fps[1]).cpu().numpy()), _bits(ref.scores(qs[1])))
    d_rows = gpu.from_numpy(_packed(oracle, np.stack(qs))).cuda()
    keys = c.query_packed_keys_device(d_rows, len(qs), per).cpu().numpy()
    tk, tl = c.query_packed_topk_keys_device(d_rows, len(qs), per, k, aligned=True)
    tk, tl = tk.cpu().numpy(), tl.cpu().numpy()
    for i, q in enumerate(qs):
        ref.check_key(lb, q, keys[i], ("packed", i))
        ref.check_keys(lb, q, tk[i], k, ("packed top-K", i), tl[i])
    grown = lb.debug_live_bytes()
    assert grown[0] > made[0] and grown[1] > made[1]          # the scratch of those calls

    path = str(tmp_path / "corpus.lbad")
    c.save(path)
    c2 = lb.Corpus.load(path, L, 0 if ragged else N_SUB)
    assert len(c2) == len(ref.counts) and lb.debug_live_bytes()[0] > grown[0]
    assert c2.query_batch(fps) == [ref.top1(q) for q in qs]
    c2.dispose()
    assert lb.debug_live_bytes() == grown
    c.dispose()
    assert lb.debug_live_bytes() == before


def test_detective_releases_everything_it_owned(lb, gpu, oracle):
    before = _warm_up(lb)
    det = lb.Detective()
    assert lb.debug_live_bytes() == before                    # a detective owns nothing until it is used
    cfg = oracle.Config()
    rng = np.random.default_rng(31)
    pcm = (rng.standard_normal(2048 + 64 * 128 * 2 + 5) * 0.3).astype(np.float32)
    assert np.array_equal(det.process_pcm(pcm).to_bools(), oracle.fingerprint_pcm(pcm, cfg))         # a one-off host call
    clips = lb.synth_clips_device(SEED, 0, 3, 5512, 2048 + 64 * 128)
    got = lb.unpack_packed(det.fingerprint_clips_device(clips).cpu().numpy(), L).reshape(3, -1, L)
    assert np.array_equal(got, oracle.fingerprint_batch(clips.cpu().numpy(), cfg))
    paths = sorted(os.path.join(BIRDS, f) for f in os.listdir(BIRDS) if f.endswith(".caf"))[:4]
    want = [oracle.fingerprint_file(p, cfg, 1, 1, 0) for p in paths]
    for pipeline in (True, False):                            # a file batch, two slots in flight and one
        det.set_file_pipeline(pipeline)
        for fp, w in zip(det.process_audio_urls(paths), want):
            assert np.array_equal(fp.to_bools(), w), pipeline
    # two rate pairs and both sinc models: a phase table per pair and model, both converter tables
    x, rate = oracle.decode_audio_file(paths[0])
    for out_rate in (5512, 48000):
        det.configure(sample_rate=out_rate)
        for mode in (0, 1):
            det.set_resampler_mode(mode)
            conv = det.convert_audio_url(paths[0])[0]
            assert np.array_equal(conv.view(np.uint32), oracle.resample(x, rate, float(out_rate), mode).view(np.uint32)), (out_rate, mode)
    alive = lb.debug_live_bytes()
    assert alive[0] > before[0] and alive[1] > before[1]
    det.dispose()
    assert lb.debug_live_bytes() == before


# ---- 2. the scratch regrows under queued work -------------------------------------------------------------------------------
def _run_calls(gpu, corpus, streams, groups, k):
    """per group of fingerprints, on the streams in turn and with nothing awaited: top-1 keys, top-K keys, their lags"""
    out = []
    for i, fps in enumerate(groups):
        s = streams[i % 2]
        with gpu.cuda.stream(s):
            top1 = gpu.empty(len(fps), dtype=gpu.int64, device="cuda")
            topk = gpu.empty((len(fps), k), dtype=gpu.int64, device="cuda")
            if len(fps) == 1:
                corpus.query_key_device(fps[0], top1, stream=s)
            else:
                corpus.query_batch_keys_device(fps, top1, stream=s)
            corpus.query_batch_topk_keys_device(fps, k, topk, stream=s)
            out.append((top1, topk))
    lags = []
    for i, (fps, (_, topk)) in enumerate(zip(groups, out)):   # ... then the alignment of those keys, likewise
        s = streams[i % 2]
        with gpu.cuda.stream(s):
            lags.append(corpus.align_keys_device(fps, topk, k, stream=s))
    gpu.cuda.synchronize()
    return [(a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()) for (a, b), c in zip(out, lags)]


def _check_calls(lb, ref, groups_q, results, k, what):
    for g, (qs, (top1, topk, lags)) in enumerate(zip(groups_q, results)):
        for i, q in enumerate(qs):
            ref.check_key(lb, q, top1[i], (what, g, i))
            ref.check_keys(lb, q, topk[i], k, (what, g, i), lags[i])


def test_uniform_scratch_regrows_under_queued_work(lb, gpu, oracle, uniform_ref):
    """3, 17 and 3 queries: across kQueryBatchMax = 8 twice; the query blocks, the score rows and the selection's scratch regrow"""
    ref = uniform_ref
    rng = np.random.default_rng(41)
    c = _corpus(lb, gpu, oracle, ref, False)
    picks = rng.integers(0, N_UNIFORM, 23)
    picks[:3] = (23, 1700, 9)
    qs = [_near(rng, ref.entry(int(e)), int(f)) for e, f in zip(picks, rng.integers(0, 60, 23))]
    groups_q = [qs[:3], qs[3:20], qs[20:]]
    groups = [[lb.Fingerprint.from_bools(q) for q in g] for g in groups_q]
    gpu.cuda.synchronize()
    results = _run_calls(gpu, c, (gpu.cuda.Stream(), gpu.cuda.Stream()), groups, 4)
    _check_calls(lb, ref, groups_q, results, 4, "uniform")
    c.dispose()


def test_ragged_scratch_regrows_under_queued_work(lb, gpu, oracle, ragged_ref):
    """single queries of 5, 60 and 5 sub-fingerprints -- the ring's slots grow, and 60 is too long to travel in the kernel's
    arguments -- then batches of 3 and 9 queries of 21"""
    ref = ragged_ref
    rng = np.random.default_rng(43)
    c = _corpus(lb, gpu, oracle, ref, True)
    long_e = int(np.argmax(ref.counts))
    def cut(per, flips):
        e = int(rng.choice(np.flatnonzero(ref.counts >= min(per, 40))))
        base = ref.entry(e)[:per]
        if base.shape[0] < per:                               # longer than any entry: an entry inside random rows
            pad = (rng.random((per, L)) < 0.5).astype(np.uint8)
            pad[7:7 + base.shape[0]] = base
            base = pad
        return _near(rng, base, flips)
    singles = [[cut(5, 3)], [cut(60, 20)], [_near(rng, ref.entry(long_e)[2:7], 0)]]
    batches = [[cut(21, int(f)) for f in rng.integers(0, 40, 3)], [cut(21, int(f)) for f in rng.integers(0, 40, 9)]]
    streams = (gpu.cuda.Stream(), gpu.cuda.Stream())
    for groups_q, what in ((singles, "ragged singles"), (batches, "ragged batches")):
        groups = [[lb.Fingerprint.from_bools(q) for q in g] for g in groups_q]
        gpu.cuda.synchronize()
        results = _run_calls(gpu, c, streams, groups, 4)
        _check_calls(lb, ref, groups_q, results, 4, what)
    c.dispose()
