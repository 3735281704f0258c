"""GPU tests of the resampler bank (LBAudioDetectiveResamplerBank*, k_resample_bank.hip): many live channels rate-converted on
the device per push.

Expected values are the CPU oracle's: a channel that has received L samples since it started, in whatever chunking, has emitted the
first emitted(L) = max(0, ceil((L - m_hi) q / p)) samples of oracle.resample on its signal (oracle.synth_clip signals), and a
finished one all of oracle.resample(x[:L]).  The oracle runs ONCE per rate pair on each channel's whole signal (and once more for a
channel that starts again).  A push's outSamples must hold samples [emitted before, emitted after) of every channel in channel
order.  Every comparison is exact (bit patterns, counts), and every output block is poison-filled before the call that writes it."""
from math import gcd

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x52534232
POISON = -0x5A5A5A5B                      # 0xA5A5A5A5 as int32: a NaN no conversion produces
# name: (rate in, rate out, mode, samples of a signal): p mod q = 1; a gather; upsampling with 49 taps; the short kernel
PAIRS = {"44k": (44100, 5512, 0, 30000), "48k": (48000, 5512, 0, 30000), "up": (8000, 44100, 0, 12000), "short": (44100, 5512, 1, 30000)}
N_SIGNALS = 6
_cache = {}


def _case(lb, oracle, name):
    """the channels' whole signals and their oracle conversions, once per rate pair"""
    if name not in _cache:
        rate_in, rate_out, mode, n = PAIRS[name]
        g = gcd(rate_in, rate_out)
        sig = [oracle.synth_clip(SEED, c, rate_in, n + 11 * c) for c in range(N_SIGNALS)]
        ref = [oracle.resample(s, rate_in, rate_out, mode) for s in sig]
        _, _, m_lo, m_hi = lb.debug_resampler_bank_plan(rate_in, rate_out, mode, [0], [0], [0])
        _cache[name] = dict(rate_in=rate_in, rate_out=rate_out, mode=mode, p=rate_in // g, q=rate_out // g, m_lo=m_lo, m_hi=m_hi,
                            span=m_hi - m_lo + 1, sig=sig, ref=ref)
    return _cache[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Model:
    """what the bank must have done: per channel the samples received since its (re)start and what they convert to"""

    def __init__(self, oracle, case, n_channels, sig=None, ref=None):
        self.oracle, self.case, self.n = oracle, case, n_channels
        self.sig = sig if sig is not None else case["sig"]
        self.start = [0] * n_channels        # where in its signal the channel (re)started
        self.at = [0] * n_channels           # samples of its signal handed over so far
        self.ref = list(ref if ref is not None else case["ref"])[:n_channels]      # the conversion of the samples from `start` on
        self.got = [[] for _ in range(n_channels)]                                 # what the bank emitted since `start`

    def length(self, c):
        return self.at[c] - self.start[c]

    def emitted(self, c, more=0):
        L, k = self.length(c) + more, self.case
        return 0 if L <= k["m_hi"] else -((L - k["m_hi"]) * k["q"] // -k["p"])

    def need(self, c, outputs):
        """the fewest new samples with which the channel emits at least `outputs` samples"""
        n = 0
        while self.emitted(c, n) - self.emitted(c) < outputs:
            n += 1
        return n

    def resolve(self, tokens):
        """a push's counts: an integer; "quiet": the most samples that emit nothing; ("out", k): the fewest that emit k or more;
        ("to", L): as many as bring the channel's total to L"""
        counts = []
        for c, t in enumerate(tokens):
            if t == "quiet":
                t = max(0, self.need(c, 1) - 1)
            elif isinstance(t, tuple) and t[0] == "out":
                t = self.need(c, t[1])
            elif isinstance(t, tuple) and t[0] == "to":
                t = t[1] - self.length(c)
            counts.append(int(t))
        return counts

    def take(self, counts):
        """the samples of a push (one array per channel) and the samples it must emit, channel by channel"""
        chunks, new = [], []
        for c, n in enumerate(counts):
            assert n >= 0 and self.at[c] + n <= self.sig[c].size, "the schedule outruns the signal"
            chunks.append(self.sig[c][self.at[c]:self.at[c] + n])
            before = self.emitted(c)
            self.at[c] += n
            assert self.emitted(c) <= self.ref[c].size
            new.append(self.ref[c][before:self.emitted(c)])
        return chunks, new

    def restart(self, c):
        self.start[c] = self.at[c]
        k = self.case
        self.ref[c] = self.oracle.resample(self.sig[c][self.at[c]:], k["rate_in"], k["rate_out"], k["mode"])
        self.got[c] = []

    def finish(self, c):
        """what finishing the channel must emit: the rest of the conversion of exactly the samples it has"""
        k = self.case
        whole = self.oracle.resample(self.sig[c][self.start[c]:self.at[c]], k["rate_in"], k["rate_out"], k["mode"])
        return whole, whole[self.emitted(c):]

    def totals(self):
        return [self.length(c) for c in range(self.n)], [self.emitted(c) for c in range(self.n)]


def _poisoned(gpu, n):
    return gpu.full((n,), POISON, dtype=gpu.int32, device="cuda").view(gpu.float32)


def _device_samples(gpu, chunks, shift, dtype=np.float32):
    """the chunks one after the other on the device, the block `shift` samples off a 256-byte boundary"""
    flat = np.concatenate([np.zeros(shift, dtype)] + [np.asarray(c, dtype) for c in chunks])
    return gpu.from_numpy(flat).cuda()[shift:]


def _check_block(gpu, bank, model, out, got_counts, got, new, stream=None):
    (stream.synchronize() if stream is not None else gpu.cuda.synchronize())
    want = np.concatenate(new) if new else np.zeros(0, np.float32)
    assert got_counts.tolist() == [r.size for r in new]
    assert got.shape == (want.size,)
    raw = out.cpu().numpy()
    assert np.all(raw[want.size:].view(np.int32) == POISON), "the call wrote behind its total"
    assert np.array_equal(_bits(raw[:want.size]), _bits(want))
    for c, r in enumerate(new):
        model.got[c].append(r)
    totals = bank.totals()
    assert [totals[0].tolist(), totals[1].tolist()] == list(model.totals())
    return raw[:want.size].copy()


def _push(gpu, bank, model, counts, host=False, shift=0, stream=None, slack=3, dtype=np.float32, quant=None):
    """one push, everything it reports checked against the model; returns the emitted samples.  quant: the int16 samples
    themselves, channel by channel, for a push in that format (the model's signals are then s / 32768)"""
    at = list(model.at)
    chunks, new = model.take(counts)
    if quant is not None:
        chunks = [quant[c][at[c]:at[c] + n] for c, n in enumerate(counts)]
    out = _poisoned(gpu, sum(r.size for r in new) + slack)
    if host:
        got_counts, got = bank.push([c if c.size else None for c in chunks], out=out, stream=stream)
    else:
        samples = _device_samples(gpu, chunks, shift, dtype)
        gpu.cuda.synchronize()
        got_counts, got = bank.push_device(samples, counts, out=out, stream=stream)
    return _check_block(gpu, bank, model, out, got_counts, got, new, stream)


def _schedule(case):
    """Pushes of six channels, different channels doing different things in the same push.  Channel 0 is silent.  Channel 1 walks
    one sample at a time across L = m_hi - 1 .. m_hi + 2, so its first output must appear with sample m_hi + 1.  Channel 2 appends
    chunks shorter than the tap span that emit nothing, then takes chunks that emit as few outputs as a chunk can (exactly one where
    the rate goes down).  Channel 3 emits more than 600 outputs in one push (several workgroups, a run boundary), then 1 500: more
    than a period of q <= 1 378 outputs, so lanes take two outputs q apart with one set of weights.  Channels 4 and 5 take odd
    counts, so the runs behind them start off 16-byte boundaries."""
    hi = case["m_hi"]
    return [
        [0, hi - 1, 7, ("out", 650), 1, hi + 5],
        [0, 1, "quiet", 1, 3, 3],
        [0, 1, ("out", 1), "quiet", 1, ("out", 1)],
        [0, 1, "quiet", ("out", 1), ("out", 300), 0],
        [0, 1, ("out", 1), 0, "quiet", ("out", 257)],
        [0, 0, "quiet", ("out", 1500), ("out", 1), "quiet"],
        [0, ("out", 256), ("out", 1), 1, 0, ("out", 513)],
        [0, "quiet", 0, 0, ("out", 2), 1],
    ]


@pytest.mark.parametrize("name", list(PAIRS))
def test_chunking(lb, gpu, oracle, name):
    case = _case(lb, oracle, name)
    hi, down = case["m_hi"], case["p"] > case["q"]
    results = []
    for host in (False, True):
        model = Model(oracle, case, 6)
        bank = lb.ResamplerBank(case["rate_in"], case["rate_out"], 6, case["mode"])
        seen = dict(append=0, one=0, big=0, offsets=set(), first=None)
        blocks = []
        for i, tokens in enumerate(_schedule(case)):
            counts = model.resolve(tokens)
            before = [model.emitted(c) for c in range(6)]
            carried = [model.length(c) for c in range(6)]
            shift = i % 4                       # the block itself starts 0, 4, 8 or 12 bytes off a 16-byte boundary
            blocks.append(_push(gpu, bank, model, counts, host=host, shift=shift))
            at = shift
            for c in range(6):
                new = model.emitted(c) - before[c]
                if counts[c] and new == 0 and carried[c]:
                    seen["append"] += 1
                    assert counts[c] < case["span"]
                seen["one"] += new == 1
                seen["big"] += new > 600
                if counts[c]:
                    seen["offsets"].add(at % 4)
                if c == 1 and new and seen["first"] is None:
                    seen["first"] = (model.length(1), new)
                at += counts[c]
        # the schedule did what its description says: the first output of channel 1 came with sample m_hi + 1
        assert seen["first"] == (hi + 1, -(case["q"] // -case["p"]))
        assert seen["append"] >= 4 and seen["big"] >= 2 and seen["offsets"] == {0, 1, 2, 3}
        assert seen["one"] >= 3 if down else seen["one"] == 0
        li, lo = bank.totals()
        assert li[0] == 0 and lo[0] == 0 and lo.max() > 1300
        results.append(blocks)
        bank.dispose()
    for a, b in zip(*results):                  # the host form against the device form
        assert np.array_equal(_bits(a), _bits(b))


# Rate pairs at which the units take their other shapes (name: rate in, rate out, mode, samples of a signal, pushes).  A workgroup
# stages at most 2 816 input samples, so a run has min(256, floor((2 816 - span - 1) q / p) + 1) outputs; positions inside the period
# in several periods are taken where q >= 2 runs, consecutive outputs otherwise.
#   steep1    48 kHz -> 1 kHz: span 2 305, runs of 11, q = 1: consecutive outputs, 25 of them are three runs
#   steep4001 48 kHz -> 4 001 Hz: span 576, runs of 187 < 256, q = 4 001: 22 runs a period, 4 500 outputs are two periods side by
#             side (with runs of 256 a run's range would be 3 636 samples: nothing would be written)
#   whole     48 kHz -> 8 kHz, mode 1: q = 1, every output has the same phase; 700 outputs are three runs of consecutive outputs
SHAPES = {
    "steep1": (48000, 1000, 0, 40000, [[("out", 25), 100], [1, ("out", 1)], [("out", 11), ("out", 12)], ["quiet", ("out", 300)]]),
    "steep4001": (48000, 4001, 0, 70000, [[("out", 4500), 100], [1, ("out", 1)], [("out", 200), ("out", 400)], ["quiet", ("out", 4100)]]),
    "whole": (48000, 8000, 1, 20000, [[("out", 700), 30], [1, ("out", 1)], [("out", 300), ("out", 600)], ["quiet", ("out", 1)]]),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_unit_shapes(lb, gpu, oracle, name):
    rate_in, rate_out, mode, n, pushes = SHAPES[name]
    g = gcd(rate_in, rate_out)
    sig = [oracle.synth_clip(SEED + 2, c, rate_in, n) for c in range(2)]
    ref = [oracle.resample(s, rate_in, rate_out, mode) for s in sig]
    _, _, m_lo, m_hi = lb.debug_resampler_bank_plan(rate_in, rate_out, mode, [0], [0], [0])
    assert m_hi - m_lo + 1 == {"steep1": 2305, "steep4001": 576, "whole": 49}[name]
    case = dict(rate_in=rate_in, rate_out=rate_out, mode=mode, p=rate_in // g, q=rate_out // g, m_lo=m_lo, m_hi=m_hi, span=m_hi - m_lo + 1)
    model = Model(oracle, case, 2, sig=sig, ref=ref)
    bank = lb.ResamplerBank(rate_in, rate_out, 2, mode)
    for i, tokens in enumerate(pushes):
        _push(gpu, bank, model, model.resolve(tokens), shift=i)
    _finish(gpu, bank, model, [0, 1])


def test_int16_input_equals_the_float_path(lb, gpu, oracle):
    """int16 samples are read as (float)s * (1.0f / 32768.0f): the bank's output on them is its output on those floats, and the
    oracle's"""
    case = _case(lb, oracle, "48k")
    quant = [np.round(s[:9000] * 32767.0).astype(np.int16) for s in case["sig"][:3]]
    assert min(int(v.min()) for v in quant) < -1000 and max(int(v.max()) for v in quant) > 1000
    sig = [v.astype(np.float32) * np.float32(1.0 / 32768.0) for v in quant]
    ref = [oracle.resample(s, case["rate_in"], case["rate_out"], case["mode"]) for s in sig]
    pushes = [[case["m_hi"] + 1, 3, ("out", 300)], [1, "quiet", 1], [("out", 2), ("out", 1), 0], [("out", 520), 77, ("out", 3)]]
    results = []
    for which in ("int16 device", "int16 host", "float32"):
        model = Model(oracle, case, 3, sig=sig, ref=ref)
        bank = lb.ResamplerBank(case["rate_in"], case["rate_out"], 3, case["mode"])
        as_int = which != "float32"
        results.append([_push(gpu, bank, model, model.resolve(t), host=which == "int16 host", shift=1 + i, dtype=np.int16 if as_int else np.float32,
                              quant=quant if as_int else None) for i, t in enumerate(pushes)])
        assert bank.totals()[1].max() > 500
    for a, b, c in zip(*results):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    # one push has one format: int16 chunks beside float32 ones are refused, not read value for value
    totals = bank.totals()
    with pytest.raises(ValueError):
        bank.push([quant[0][:10], sig[1][:10], None])
    assert all(np.array_equal(a, b) for a, b in zip(bank.totals(), totals))


def _finish(gpu, bank, model, channels, stream=None):
    """finish the listed channels: counts, layout and the channels' whole outputs against the oracle, lengths included"""
    wholes = {c: model.finish(c) for c in sorted(set(channels))}
    new = [wholes[c][1] if c in wholes else np.zeros(0, np.float32) for c in range(model.n)]
    out = _poisoned(gpu, sum(r.size for r in new) + 3)
    got_counts, got = bank.finish(channels, out=out, stream=stream)
    for c, (whole, rest) in wholes.items():
        so_far = np.concatenate(model.got[c] + [rest]) if model.got[c] else rest
        assert so_far.size == whole.size == int(model.oracle.lib().lbo_resample_count(model.length(c), float(model.case["rate_in"]), float(model.case["rate_out"])))
        assert np.array_equal(_bits(so_far), _bits(whole)), "what the channel emitted before is not a prefix of its conversion"
    for c in wholes:
        model.restart(c)
    block = _check_block(gpu, bank, model, out, got_counts, got, new, stream)
    for c in wholes:
        model.got[c] = []
    return block


@pytest.mark.parametrize("name", ["44k", "up"])
def test_finish(lb, gpu, oracle, name):
    case = _case(lb, oracle, name)
    model = Model(oracle, case, 4)
    bank = lb.ResamplerBank(case["rate_in"], case["rate_out"], 4, case["mode"])
    _push(gpu, bank, model, model.resolve([("out", 300), 5, ("out", 40), ("out", 3)]))
    _push(gpu, bank, model, model.resolve([77, "quiet", 0, ("out", 270)]))
    with pytest.raises(lb.LBAudioDetectiveError) as err:
        bank.finish([1, 4])                                    # a channel out of range: nothing is finished
    assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    with pytest.raises(lb.LBAudioDetectiveError):
        bank.finish([2, 2])                                    # a channel listed twice
    assert [t.tolist() for t in bank.totals()] == list(model.totals())
    # channel 0 mid-signal, channel 1 before its first output (m_hi samples), in list order 1, 0
    assert model.length(1) == case["m_hi"] and model.emitted(1) == 0
    rest = _finish(gpu, bank, model, [1, 0])
    assert rest.size > 0 and bank.totals()[0].tolist()[:2] == [0, 0]
    # the next push to them starts a new signal; the others are undisturbed
    _push(gpu, bank, model, model.resolve([("out", 260), case["m_hi"] + 2, ("out", 5), 1]), shift=1)
    _push(gpu, bank, model, model.resolve([1, ("out", 2), "quiet", ("out", 1)]), shift=2)
    _finish(gpu, bank, model, [3])
    _finish(gpu, bank, model, [0, 1, 2, 3])                    # channel 3 has nothing: finishing it emits nothing
    assert [t.tolist() for t in bank.totals()] == [[0] * 4, [0] * 4]
    _push(gpu, bank, model, model.resolve([0, ("out", 1), 9, ("out", 30)]))


def test_reset(lb, gpu, oracle):
    case = _case(lb, oracle, "short")
    model = Model(oracle, case, 3)
    bank = lb.ResamplerBank(case["rate_in"], case["rate_out"], 3, case["mode"])
    _push(gpu, bank, model, model.resolve([("out", 100), ("out", 280), 11]))
    _push(gpu, bank, model, model.resolve([("out", 1), 1, "quiet"]))
    with pytest.raises(lb.LBAudioDetectiveError):
        bank.reset([1, 3])                                     # a channel out of range: nothing is reset
    assert [t.tolist() for t in bank.totals()] == list(model.totals())
    bank.reset([1, 2])
    model.restart(1)
    model.restart(2)
    assert [t.tolist() for t in bank.totals()] == list(model.totals()) and bank.totals()[0].tolist()[1:] == [0, 0]
    # a restarted channel has nothing carried: its first taps reach below index 0 and must read nothing of the old signal
    _push(gpu, bank, model, model.resolve([("out", 2), case["m_hi"] + 1, 5]), shift=3)
    _push(gpu, bank, model, model.resolve([0, ("out", 300), ("out", 1)]))
    assert bank.totals()[1].min() >= 1


def test_refused_push_leaves_the_state_alone(lb, gpu, oracle):
    import ctypes as C
    case = _case(lb, oracle, "44k")
    model = Model(oracle, case, 3)
    bank = lb.ResamplerBank(case["rate_in"], case["rate_out"], 3, case["mode"])
    _push(gpu, bank, model, model.resolve([("out", 20), 9, 0]))
    counts = model.resolve([("out", 5), ("out", 1), ("out", 270)])
    chunks = [model.sig[c][model.at[c]:model.at[c] + counts[c]] for c in range(3)]
    total = sum(model.emitted(c, counts[c]) - model.emitted(c) for c in range(3))
    samples = _device_samples(gpu, chunks, 0)
    small = _poisoned(gpu, total - 1)                          # capacity one short
    totals = bank.totals()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    for push in (lambda: bank.push_device(samples, counts, out=small), lambda: bank.push(chunks, out=small)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            push()
        assert err.value.status == bad
    # a NULL sample pointer with a non-zero count, both forms
    N = lb._native
    room = _poisoned(gpu, total + 3)
    c_counts, c_new, c_total = (N.UInt32 * 3)(*counts), (N.UInt32 * 3)(7, 7, 7), N.UInt64(7)
    for fn in (lb.lib().LBAudioDetectiveResamplerBankPushDevice, lb.lib().LBAudioDetectiveResamplerBankPush):
        assert fn(bank._ref, None, 0, c_counts, c_new, C.c_void_p(room.data_ptr()), room.numel(), C.byref(c_total), None) == bad
    assert list(c_new) == [7, 7, 7] and c_total.value == 7
    gpu.cuda.synchronize()
    assert bool((small.view(gpu.int32) == POISON).all()) and bool((room.view(gpu.int32) == POISON).all())
    assert all(np.array_equal(a, b) for a, b in zip(bank.totals(), totals))
    _push(gpu, bank, model, counts)                            # the same push with room: what it would have given
    _push(gpu, bank, model, model.resolve([("out", 1), "quiet", 3]))


def test_second_trips(lb, gpu, oracle):
    """Under a ceiling of 1 and of 4 workgroups every launch in here -- convert and commit of three pushes with five or six rows
    and seven or more units each (1 100 outputs at q = 689 are three runs of two periods), convert of a finish of six rows -- has
    a grid below its work: workgroups take several units, restaging their LDS blocks in between, with the results of one unit per
    workgroup (ceiling 0, run first in this same test) and of the oracle"""
    case = _case(lb, oracle, "48k")
    pushes = [[("out", 600), ("out", 1), 5, ("out", 257), ("out", 300), ("out", 2)], [("out", 300), "quiet", ("out", 1), ("out", 1100), 0, ("out", 2)],
              [("out", 3), ("out", 2), ("out", 700), 1, ("out", 1), ("out", 1)]]
    results = {}
    try:
        for ceiling in (0, 1, 4):
            lb.debug_set_grid_ceiling(ceiling)
            model = Model(oracle, case, 6)
            bank = lb.ResamplerBank(case["rate_in"], case["rate_out"], 6, case["mode"])
            strided = lb.debug_grid_ceiling()[1]
            got = [_push(gpu, bank, model, model.resolve(t), shift=1) for t in pushes]
            got.append(_finish(gpu, bank, model, [5, 0, 2, 3, 1, 4]))
            assert got[0].size >= 1160
            if ceiling:
                assert lb.debug_grid_ceiling()[1] >= strided + 7, "the launches in here did not have grids below their work"
                assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, results[0]))
            results[ceiling] = got
    finally:
        lb.debug_set_grid_ceiling(0)


def test_end_to_end_feeds_a_stream_bank(lb, gpu, oracle):
    """three 44.1 kHz channels through ResamplerBank.feed into a StreamBank at 5512 Hz / 2048 / 64, both pushes of every feed on
    one non-default stream with one synchronise at the end: each channel's sub-fingerprints are the oracle's for the oracle's
    conversion of its signal, as far as the samples it has emitted complete frames"""
    rate_in, rate, window, stride, bands, length = 44100, 5512, 2048, 64, 32, 200
    cfg = oracle.Config(rate, window, stride, bands, length)
    sig = [oracle.synth_clip(SEED + 1, c, rate_in, 150000 + 4000 * c) for c in range(3)]
    converted = [oracle.resample(s, rate_in, rate) for s in sig]
    rows = [oracle.fingerprint_pcm(v, cfg) for v in converted]
    assert [r.shape[0] for r in rows] == [2, 2, 2]
    det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
    stream_bank = lb.StreamBank(det, 3, 4)
    bank = lb.ResamplerBank(rate_in, rate, 3)
    rng = np.random.default_rng(SEED)
    at, feeds = [0, 0, 0], []
    while any(at[c] < sig[c].size for c in range(3)):
        counts = [min(int(rng.integers(0, 40000)) if rng.integers(0, 5) else 0, sig[c].size - at[c]) for c in range(3)]
        feeds.append((list(at), counts))
        at = [a + n for a, n in zip(at, counts)]
    assert 8 <= len(feeds) <= 60
    blocks = [_device_samples(gpu, [sig[c][a:a + n] for c, (a, n) in enumerate(zip(start, counts))], i % 4) for i, (start, counts) in enumerate(feeds)]
    outs = [gpu.full((4, 32), 0xA5, dtype=gpu.uint8, device="cuda") for _ in feeds]
    s1 = gpu.cuda.Stream()
    gpu.cuda.synchronize()
    results = [bank.feed(stream_bank, block, counts, new_out=out, stream=s1) for block, (_, counts), out in zip(blocks, feeds, outs)]
    s1.synchronize()
    _, m_lo, m_hi = lb.debug_resampler_bank_plan(rate_in, rate, 0, [0], [0], [0])[1:]
    g = gcd(rate_in, rate)
    emitted = [0 if s.size <= m_hi else -((s.size - m_hi) * (rate // g) // -(rate_in // g)) for s in sig]
    want_counts = [0 if e < window else ((e - window) // stride) // 128 for e in emitted]
    assert want_counts == [2, 2, 2] and bank.totals()[1].tolist() == emitted and bank.totals()[0].tolist() == [s.size for s in sig]
    assert stream_bank.totals().tolist() == want_counts
    got = [[] for _ in range(3)]
    for (new_counts, packed), out in zip(results, outs):
        raw = out.cpu().numpy()
        assert packed.shape[0] == int(new_counts.sum()) and np.all(raw[packed.shape[0]:] == 0xA5)
        unpacked, i = lb.unpack_packed(raw[:packed.shape[0]], length), 0
        for c in range(3):
            got[c].append(unpacked[i:i + int(new_counts[c])])
            i += int(new_counts[c])
    for c in range(3):
        assert np.array_equal(np.concatenate(got[c]), rows[c][:want_counts[c]]), f"channel {c}"
        assert np.array_equal(stream_bank.fingerprint(c).to_bools(), rows[c][:want_counts[c]])
