"""GPU tests of the stream bank (LBAudioDetectiveStreamBank*, k_stream_bank.hip): many live channels fingerprinted on the device
per push.

Expected values are the CPU oracle's: a channel that has received L samples, in whatever chunking, has the sub-fingerprints
oracle.fingerprint_pcm gives for those L samples (oracle.synth_clip signals).  The oracle runs ONCE per configuration on each
channel's whole signal; since frame f reads samples [f * hop, f * hop + W + hop) and nothing else, the first
subfingerprint_count(L) rows of that result are the rows of the first L samples.  A push's outNewPacked must hold rows
[total before, total after) of every channel in channel order, the ring the last min(total, H) rows.  Every comparison is exact
(Booleans, counts, keys and lags as integers), and every output block is poison-filled before the call that writes it.

One case of the issue cannot exist and is replaced: "a frame lying wholly inside the carried samples".  A channel carries
p < W + hop samples (otherwise it would have completed a frame), and a frame reads W + hop, so every frame reads at least one new
sample.  The chunking schedule instead has the extreme, p = W + hop - 1 followed by one new sample, and frames whose first
W + hop - 1 - k samples are carried."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x53424B31
POISON = 0xA5
# name: (sample rate, window, stride, bands, sub-fingerprint length) -- the pruned stage 1, rows_stream2, a generic configuration
CONFIGS = {"pruned": (44100, 1024, 64, 32, 200), "stream2": (5512, 2048, 64, 32, 200), "generic": (8000, 64, 8, 16, 100)}
N_SIGNALS = 6
_cache = {}


def _case(lb, oracle, name, frames=14):
    """the detective, the channels' whole signals and their oracle rows, once per configuration and length"""
    key = (name, frames)
    if key not in _cache:
        rate, window, stride, bands, length = CONFIGS[name]
        cfg = oracle.Config(rate, window, stride, bands, length)
        hop = 128 * stride
        n = window + frames * hop + 7
        sig = [oracle.synth_clip(SEED, c, rate, n) for c in range(N_SIGNALS)]
        ref = [oracle.fingerprint_pcm(s, cfg) for s in sig]
        assert all(r.shape == (frames, length) for r in ref)
        det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
        _cache[key] = dict(det=det, cfg=cfg, window=window, stride=stride, hop=hop, length=length, sig=sig, ref=ref, rate=rate)
    return _cache[key]


class Model:
    """what the bank must hold: per channel the samples received since its (re)start and the rows they give"""

    def __init__(self, case, n_channels, history):
        self.case, self.n, self.history = case, n_channels, history
        self.start = [0] * n_channels        # where in its signal the channel (re)started
        self.at = [0] * n_channels           # samples of its signal handed over so far
        self.rows = [case["ref"][c] for c in range(n_channels)]     # rows of the samples from `start` on

    def count(self, c, at=None):
        got = (self.at[c] if at is None else at) - self.start[c]
        w, s = self.case["window"], self.case["stride"]
        return 0 if got < w else ((got - w) // s) // 128

    def pending(self, c):
        return self.at[c] - self.start[c] - self.count(c) * self.case["hop"]

    def resolve(self, tokens):
        """a push's counts: an integer, or ("to", x): as many as make carried + new equal x"""
        return [t if isinstance(t, int) else t[1] - self.pending(c) for c, t in enumerate(tokens)]

    def take(self, counts):
        """the samples of a push (one array per channel) and the rows it must produce, channel by channel"""
        chunks, new = [], []
        for c, n in enumerate(counts):
            assert n >= 0 and self.at[c] + n <= self.case["sig"][c].size, "the schedule outruns the signal"
            chunks.append(self.case["sig"][c][self.at[c]:self.at[c] + n])
            before = self.count(c)
            self.at[c] += n
            new.append(self.rows[c][before:self.count(c)])
        return chunks, new

    def reset(self, oracle, c):
        self.start[c] = self.at[c]
        tail = self.case["sig"][c][self.at[c]:]
        self.rows[c] = oracle.fingerprint_pcm(tail, self.case["cfg"]) if tail.size >= self.case["window"] else np.zeros((0, self.case["length"]), np.uint8)

    def history_rows(self, c):
        t = self.count(c)
        return self.rows[c][max(0, t - self.history):t]


def _device_samples(gpu, chunks, shift):
    """the chunks one after the other on the device, the block `shift` floats off a 256-byte boundary"""
    flat = np.concatenate([np.zeros(shift, np.float32)] + [np.asarray(c, np.float32) for c in chunks])
    return gpu.from_numpy(flat).cuda()[shift:]


def _push(lb, gpu, bank, model, counts, host=False, shift=0, stream=None, slack=2):
    """one push, everything it reports checked against the model; returns the packed rows as bytes"""
    chunks, new = model.take(counts)
    want = np.concatenate(new) if new else np.zeros((0, model.case["length"]), np.uint8)
    total = want.shape[0]
    out = gpu.full((total + slack, 32), POISON, dtype=gpu.uint8, device="cuda")
    if host:
        got_counts, got = bank.push([c if c.size else None for c in chunks], new_out=out, stream=stream)
    else:
        samples = _device_samples(gpu, chunks, shift)
        gpu.cuda.synchronize()
        got_counts, got = bank.push_device(samples, counts, new_out=out, stream=stream)
    (stream.synchronize() if stream is not None else gpu.cuda.synchronize())
    assert got_counts.tolist() == [r.shape[0] for r in new]
    assert got.shape == (total, 32)
    raw = out.cpu().numpy()
    assert np.all(raw[total:] == POISON), "the push wrote behind its total"
    assert np.array_equal(lb.unpack_packed(raw[:total], model.case["length"]), want)
    assert bank.totals().tolist() == [model.count(c) for c in range(model.n)]
    assert bank.pending().tolist() == [model.pending(c) for c in range(model.n)]
    return raw[:total].copy()


def _check_history(bank, model):
    for c in range(model.n):
        got = bank.fingerprint(c)
        want = model.history_rows(c)
        assert got.number_of_subfingerprints == want.shape[0]
        if want.shape[0]:
            assert np.array_equal(got.to_bools(), want), f"history of channel {c}"


def _schedule(window, hop):
    """eight pushes of six channels: channel 0 silent; counts of 0, 1, hop - 1, hop and those that bring carried + new to
    W + hop - 1, W + hop and W + 3 hop + 5; three frames in one push (channel 1, push 0); p > hop with two frames (channel 2,
    push 2); p = W + hop - 1 and one new sample (channels 1 and 2)"""
    full = window + hop
    per_channel = [
        [0] * 8,
        [full + 2 * hop + 5, 1, hop - 1, hop, ("to", full - 1), 1, 0, ("to", full + 2 * hop + 5)],
        [1, ("to", full - 1), hop + 1, hop - 1, hop, 0, ("to", full), 1],
        [hop - 1, hop, 1, ("to", full), 0, hop, ("to", full + 2 * hop + 5), hop - 1],
        [hop, hop, hop, hop + 2, hop, hop, hop - 2, hop],
        [("to", full), 1, 1, ("to", full), hop - 1, ("to", full + 2 * hop + 5), 1, hop],
    ]
    return [[per_channel[c][i] for c in range(6)] for i in range(8)]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_chunking(lb, gpu, oracle, name):
    case = _case(lb, oracle, name)
    model = Model(case, 6, 16)
    bank = lb.StreamBank(case["det"], 6, 16)
    streams = [lb.Stream(case["det"]) for _ in range(6)]
    seam_offsets, most_frames, carried_max = set(), 0, 0
    for i, tokens in enumerate(_schedule(case["window"], case["hop"])):
        counts = model.resolve(tokens)
        pend = [model.pending(c) for c in range(6)]
        shift = i % 3                       # the block itself starts 0, 4 or 8 bytes off a 16-byte boundary
        before = [model.count(c) for c in range(6)]
        _push(lb, gpu, bank, model, counts, shift=shift)
        at = shift
        for c in range(6):
            ready = model.count(c) - before[c]
            if ready and pend[c]:           # a frame across the seam: where its new run starts, in samples
                seam_offsets.add(at % 4)
                carried_max = max(carried_max, pend[c])
            if ready >= 2 and pend[c] > case["hop"]:
                most_frames = max(most_frames, ready)
            at += counts[c]
            streams[c].push(case["sig"][c][model.at[c] - counts[c]:model.at[c]])
    # the schedule did what its description says
    assert {o % 2 for o in seam_offsets} == {0, 1} and 0 in seam_offsets, seam_offsets
    assert most_frames >= 2 and carried_max == case["window"] + case["hop"] - 1
    assert bank.totals()[0] == 0 and bank.pending()[0] == 0
    assert max(bank.totals()) >= 6
    _check_history(bank, model)
    for c in range(6):
        want = streams[c].fingerprint()
        got = bank.fingerprint(c)
        assert got.number_of_subfingerprints == want.number_of_subfingerprints
        if got.number_of_subfingerprints:
            assert np.array_equal(got.to_bools(), want.to_bools())


def _window(lb, gpu, bank, model, channels, n):
    out = gpu.full((len(channels), n, 32), POISON, dtype=gpu.uint8, device="cuda")
    bank.window_device(channels, n, out=out)
    gpu.cuda.synchronize()
    got = lb.unpack_packed(out.cpu().numpy(), model.case["length"]).reshape(len(channels), n, -1)
    for j, c in enumerate(channels):
        t = model.count(c)
        assert np.array_equal(got[j], model.rows[c][t - n:t]), (channels, n, j)


@pytest.mark.parametrize("history", [3, 1])
def test_ring(lb, gpu, oracle, history):
    case = _case(lb, oracle, "pruned")
    W, hop = case["window"], case["hop"]
    model = Model(case, 3, history)
    bank = lb.StreamBank(case["det"], 3, history)
    pushes = [[W + 5 * hop, W + hop, 0], [hop, 2 * hop, W + hop - 1], [2 * hop, hop, 1], [3 * hop, 3 * hop, 2 * hop], [hop, 0, hop]]
    for i, counts in enumerate(pushes):
        new = _push(lb, gpu, bank, model, counts)
        if i == 0:
            assert new.shape[0] == 6 and bank.totals().tolist() == [5, 1, 0]       # five frames of one channel, more than H
        _check_history(bank, model)
        for n in range(1, history + 1):
            able = [c for c in (2, 1, 1, 0) if model.count(c) >= n]               # descending, one channel twice
            if able:
                _window(lb, gpu, bank, model, able, n)
        # a window longer than a channel's total, or than the history: refused, nothing written
        short = [c for c in range(3) if model.count(c) < history]
        out = gpu.full((3, history + 1, 32), POISON, dtype=gpu.uint8, device="cuda")
        for channels, n in ([([0] + short[:1], history)] if short else []) + [([0], history + 1), ([0, 3], 1)]:
            with pytest.raises(lb.LBAudioDetectiveError) as err:
                bank.window_device(channels, n, out=out)
            assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
        gpu.cuda.synchronize()
        assert bool((out == POISON).all())
        assert bank.totals().tolist() == [model.count(c) for c in range(3)]
    assert bank.totals().tolist() == [12, 7, 4]                                    # the ring was crossed several times
    _check_history(bank, model)


@pytest.fixture(params=[0, 1, 4], ids=["ceiling0", "ceiling1", "ceiling4"])
def ceiling(request, lb):
    """the grid ceiling of the test, 0 again whatever the test did"""
    lb.debug_set_grid_ceiling(request.param)
    try:
        yield request.param
    finally:
        lb.debug_set_grid_ceiling(0)


# name -> (configuration, frames of the signals, channels, frames per pass, history, pushes, window rows, listed channels): seven
# frames in passes of two, six channels (more rows than a ceiling of 4); 140 frames in passes of 64 with a window of 129 rows --
# more than one trip of the 256 lanes of the rows and window launches
PASS_CASES = {
    "seven": ("pruned", 14, 6, 2, 4, lambda W, hop: [[W + 2 * hop] + [W + hop] * 5, [hop, hop + 1] * 3, [hop - 1, 3 * hop] * 3], 3, (5, 0)),
    "many": ("generic", 150, 2, 64, 140, lambda W, hop: [[W + 130 * hop, W + 10 * hop], [hop, hop + 1], [7 * hop - 1, 5 * hop]], 129, (0, 0)),
}
_unconstrained = {}


@pytest.mark.parametrize("which", list(PASS_CASES))
def test_passes_and_second_trips(lb, gpu, oracle, ceiling, which):
    name, frames, n_channels, per_pass, history, pushes, rows, listed = PASS_CASES[which]
    case = _case(lb, oracle, name, frames)
    model = Model(case, n_channels, history)
    bank = lb.StreamBank(case["det"], n_channels, history, frames_per_pass=per_pass)
    strided = lb.debug_grid_ceiling()[1]
    got = [_push(lb, gpu, bank, model, counts, shift=1) for counts in pushes(case["window"], case["hop"])]
    assert got[0].shape[0] == (7 if which == "seven" else 140)
    out = gpu.full((2, rows, 32), POISON, dtype=gpu.uint8, device="cuda")
    bank.window_device(listed, rows, out=out)
    gpu.cuda.synchronize()
    got.append(out.cpu().numpy())
    for j, c in enumerate(listed):
        t = model.count(c)
        assert np.array_equal(lb.unpack_packed(got[-1][j], case["length"]), model.rows[c][t - rows:t])
    _check_history(bank, model)
    if ceiling:
        assert lb.debug_grid_ceiling()[1] > strided, "no launch in here had a grid below its work"
        if which in _unconstrained:         # (the unconstrained case runs first; alone, a ceiling case still has the oracle)
            assert all(np.array_equal(a, b) for a, b in zip(got, _unconstrained[which]))
    else:
        _unconstrained[which] = got


def test_refused_push_leaves_the_state_alone(lb, gpu, oracle):
    case = _case(lb, oracle, "pruned")
    W, hop = case["window"], case["hop"]
    model = Model(case, 3, 4)
    bank = lb.StreamBank(case["det"], 3, 4)
    _push(lb, gpu, bank, model, [hop + 5, W + hop, 0])
    counts = [W + hop, hop, W + 2 * hop]                       # five frames
    chunks = [case["sig"][c][model.at[c]:model.at[c] + counts[c]] for c in range(3)]
    samples = _device_samples(gpu, chunks, 0)
    small = gpu.full((2, 32), POISON, dtype=gpu.uint8, device="cuda")
    totals, pending = bank.totals(), bank.pending()
    for push in (lambda: bank.push_device(samples, counts, new_out=small), lambda: bank.push(chunks, new_out=small)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            push()
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    gpu.cuda.synchronize()
    assert bool((small == POISON).all())
    assert np.array_equal(bank.totals(), totals) and np.array_equal(bank.pending(), pending)
    _check_history(bank, model)
    _push(lb, gpu, bank, model, counts)                        # the same push with room: what it would have given
    _push(lb, gpu, bank, model, [hop, hop, hop])
    _check_history(bank, model)


def test_push_after_a_changed_setting_is_refused(lb, gpu, oracle):
    """the bank takes window, stride, bands and sub-fingerprint length from the detective when it is made: a push after any of
    them changed is refused and changes nothing; with the setting back the bank goes on where it was"""
    case = _case(lb, oracle, "pruned")
    W, hop = case["window"], case["hop"]
    rate, window, stride, bands, length = CONFIGS["pruned"]
    det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
    model = Model(case, 2, 3)
    bank = lb.StreamBank(det, 2, 3)
    _push(lb, gpu, bank, model, [W + hop + 3, hop - 1])
    for changed in (dict(window=2048), dict(stride=32), dict(bands=16), dict(subfp_len=100)):
        det.configure(**changed)
        counts = [hop, hop]
        chunks = [case["sig"][c][model.at[c]:model.at[c] + counts[c]] for c in range(2)]
        out = gpu.full((4, 32), POISON, dtype=gpu.uint8, device="cuda")
        totals, pending = bank.totals(), bank.pending()
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            bank.push_device(_device_samples(gpu, chunks, 0), counts, new_out=out)
        assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid"), changed
        gpu.cuda.synchronize()
        assert bool((out == POISON).all())
        assert np.array_equal(bank.totals(), totals) and np.array_equal(bank.pending(), pending)
        det.configure(window=window, stride=stride, bands=bands, subfp_len=length)
        _push(lb, gpu, bank, model, counts)
        _check_history(bank, model)


def test_reset(lb, gpu, oracle):
    case = _case(lb, oracle, "stream2")
    W, hop = case["window"], case["hop"]
    model = Model(case, 3, 3)
    bank = lb.StreamBank(case["det"], 3, 3)
    _push(lb, gpu, bank, model, [W + hop + 9, W + 2 * hop - 1, hop])
    _push(lb, gpu, bank, model, [hop, 1, hop])
    with pytest.raises(lb.LBAudioDetectiveError):
        bank.reset([1, 3])                                     # a channel out of range: nothing is reset
    assert bank.totals().tolist() == [model.count(c) for c in range(3)]
    bank.reset([1])
    model.reset(oracle, 1)
    assert bank.totals().tolist() == [model.count(0), 0, model.count(2)] and bank.pending()[1] == 0 and model.count(0) == 2
    assert bank.fingerprint(1).number_of_subfingerprints == 0
    with pytest.raises(lb.LBAudioDetectiveError):
        bank.window_device([1], 1)
    _push(lb, gpu, bank, model, [hop - 1, W + hop - 1, hop])
    _push(lb, gpu, bank, model, [1, 2 * hop + 1, W])
    assert bank.totals()[1] == 3 and min(bank.totals()) >= 2
    _check_history(bank, model)
    _window(lb, gpu, bank, model, [1, 0, 2], 2)


def test_host_and_device_pushes_agree(lb, gpu, oracle):
    case = _case(lb, oracle, "generic")
    W, hop = case["window"], case["hop"]
    pushes = [[W + 3 * hop + 5, hop - 1, 0, 1], [hop, W + 1, 0, W + hop - 2], [1, 4 * hop, 0, 1], [hop - 1, 1, 0, 2 * hop]]
    results = []
    for host in (False, True):
        model = Model(case, 4, 3)
        bank = lb.StreamBank(case["det"], 4, 3)
        new = [_push(lb, gpu, bank, model, counts, host=host, shift=3) for counts in pushes]
        able = [c for c in range(4) if model.count(c) >= 3]
        assert able
        ring = bank.window_device(able, 3)
        gpu.cuda.synchronize()
        results.append((new, ring.cpu().numpy(), bank.totals(), bank.pending()))
        _check_history(bank, model)
    for a, b in zip(*[r[0] for r in results]):
        assert np.array_equal(a, b)
    assert all(np.array_equal(results[0][i], results[1][i]) for i in (1, 2, 3))


def _ragged_corpus(lb, gpu, oracle, case, channels, ends):
    """about 40 entries: random ones, and pieces of the channels' oracle fingerprints -- the first three from inside the window
    the test asks about (rows [end - 15, end - 5) of each channel)"""
    counts = oracle.synth_ragged_counts(SEED, 0, 25, 1, 40)
    corpus = lb.Corpus.ragged(200, 64, int(counts.sum()) + 400)
    corpus.append_ragged_packed_device(lb.synth_ragged_corpus_device(SEED, 0, counts, 200), counts)
    rng = np.random.default_rng(SEED)
    for i in range(15):
        rows = case["ref"][channels[i % len(channels)]]
        a = int(rng.integers(0, rows.shape[0] - 2))
        b = int(rng.integers(a + 1, min(rows.shape[0], a + 30) + 1))
        if i < len(channels):
            a, b = ends[channels[i]] - 15, ends[channels[i]] - 5
        corpus.append_fingerprint(lb.Fingerprint.from_bools(rows[a:b]))
    return corpus


def _expected_keys(lb, gpu, corpus, model, channels, n, k):
    fps = [lb.Fingerprint.from_bools(model.rows[c][model.count(c) - n:model.count(c)]) for c in channels]
    keys = gpu.zeros((len(fps), k), dtype=gpu.int64, device="cuda")
    corpus.query_batch_topk_keys_device(fps, k, keys)
    lags = corpus.align_keys_device(fps, keys, k)
    gpu.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64), lags.cpu().numpy()


def test_end_to_end_and_asynchrony(lb, gpu, oracle):
    """identify against a ragged corpus; then the same chain -- push, window, packed top-K query -- on ONE non-default stream
    with one synchronise at the end, and two pushes on two streams with no host wait between them: the serial results"""
    case = _case(lb, oracle, "pruned", 26)
    W, hop = case["window"], case["hop"]
    channels = [2, 0, 1]
    corpus = _ragged_corpus(lb, gpu, oracle, case, channels, [23, 23, 25])
    assert len(corpus) == 40
    first, second = [W + 20 * hop + 3, W + 22 * hop, W + 21 * hop - 1], [3 * hop, hop, 4 * hop + 1]
    # serial, on the current stream
    model = Model(case, 3, 24)
    bank = lb.StreamBank(case["det"], 3, 24, frames_per_pass=32)
    _push(lb, gpu, bank, model, first)
    _push(lb, gpu, bank, model, second)                        # totals 23, 23, 25: channel 2 has wrapped
    assert bank.totals().tolist() == [23, 23, 25]
    keys, lags = bank.identify(corpus, channels, n=21, k=3, aligned=True)
    gpu.cuda.synchronize()
    want_keys, want_lags = _expected_keys(lb, gpu, corpus, model, channels, 21, 3)
    assert keys.shape == (3, 3) and lags.shape == (3, 3)
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), want_keys) and np.array_equal(lags.cpu().numpy(), want_lags)
    assert (want_keys[:, 0] >> np.uint64(32)).min() == np.float32(1.0).view(np.uint32), "every channel has a piece of itself in the corpus"
    # one non-default stream, one synchronise
    chunks = [[case["sig"][c][a:a + n] for c, (a, n) in enumerate(zip(at, counts))] for at, counts in (([0, 0, 0], first), (first, second))]
    blocks = [_device_samples(gpu, ch, 1) for ch in chunks]
    s1, s2 = gpu.cuda.Stream(), gpu.cuda.Stream()
    bank2 = lb.StreamBank(case["det"], 3, 24, frames_per_pass=32)
    new = [gpu.full((80, 32), POISON, dtype=gpu.uint8, device="cuda") for _ in range(2)]
    win = gpu.full((3, 21, 32), POISON, dtype=gpu.uint8, device="cuda")
    k2 = gpu.zeros((3, 3), dtype=gpu.int64, device="cuda")
    l2 = gpu.zeros((3, 3), dtype=gpu.int32, device="cuda")
    gpu.cuda.synchronize()
    c1, n1 = bank2.push_device(blocks[0], first, new_out=new[0], stream=s1)
    c2, n2 = bank2.push_device(blocks[1], second, new_out=new[1], stream=s1)
    bank2.window_device(channels, 21, out=win, stream=s1)
    corpus.query_packed_topk_keys_device(win, 3, 21, 3, keys_out=k2, lags_out=l2, stream=s1)
    s1.synchronize()
    assert c1.tolist() == [20, 22, 20] and c2.tolist() == [3, 1, 5]
    assert np.array_equal(k2.cpu().numpy().view(np.uint64), want_keys) and np.array_equal(l2.cpu().numpy(), want_lags)
    for got, counts_, base in ((n1, c1, [0, 0, 0]), (n2, c2, c1.tolist())):
        want = np.concatenate([case["ref"][c][base[c]:base[c] + int(counts_[c])] for c in range(3)])
        assert np.array_equal(lb.unpack_packed(got.cpu().numpy(), 200), want)
    # two pushes on two streams, no host wait in between: the second waits for the first on the device
    bank3 = lb.StreamBank(case["det"], 3, 24, frames_per_pass=32)
    win3 = gpu.full((3, 21, 32), POISON, dtype=gpu.uint8, device="cuda")
    gpu.cuda.synchronize()
    bank3.push_device(blocks[0], first, stream=s1)
    bank3.push_device(blocks[1], second, stream=s2)
    bank3.window_device(channels, 21, out=win3, stream=s1)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(win3.cpu().numpy(), win.cpu().numpy())
    assert bank3.totals().tolist() == [23, 23, 25]
    for c in range(3):
        assert np.array_equal(bank3.fingerprint(c).to_bools(), model.history_rows(c))
