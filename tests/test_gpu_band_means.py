"""GPU parity of the band means of the pruned stage 1 (k_rows_pruned.hip), whose quotient p / divisor is the short form
of const_div.hpp behind a guard: every band mean (as a bit pattern) and every packed sub-fingerprint against the CPU oracle,
on the fast path and on every way into the fallback.

Plans (all 1024-sample windows, hop 64, 32 bands -- what rows_pruned_supported accepts):
  * 44.1 kHz, the headline: divisors 1..63, all proven;
  * 48 kHz: another divisor set, with a ZERO divisor (two equal band edges) -- never proven, its waves always divide;
  * 96 kHz: divisors up to 74.
Inputs: ordinary audio (fast path); silence (every sum +0, fast path); amplitudes that put the band sums below the
guard's lower bound 2^-100, into the denormals and to zero; amplitudes around the point where a band sum overflows to
+inf; NaN / inf samples (skipped terms).  The raw frames come from the tap (full rows); without the tap the headline
plan runs the compact rows, checked through the packed bits."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANS = {"headline_44k": 44100, "zero_divisor_48k": 48000, "wide_96k": 96000}
WINDOW, STRIDE, BANDS = 1024, 64, 32
N = WINDOW + STRIDE * 128 * 2          # two frames per clip


def _divisors(rate):
    """LBAudioDetective.m:362-371, as lbaudiodetective_amd/csrc/plan.cpp computes it; also the highest bin a band reads."""
    bottom = 318.0
    base = math.exp(math.log(rate / 2.0 / bottom) / BANDS)
    coef = WINDOW / rate * bottom
    u = lambda v: int(v) if v > 0 else 0
    idx = [u((base ** j - 1.0) * coef) + u(coef) for j in range(BANDS + 1)]
    bin_hz = rate / WINDOW
    edges = [min(u(2 * i / bin_hz - 1.0), WINDOW // 2) for i in idx]
    kmax = max([edges[b + 1] for b in range(BANDS) if edges[b] < edges[b + 1]] or [0])
    return [idx[b + 1] - idx[b] for b in range(BANDS)], kmax


def _cases(rate):
    rng = np.random.default_rng(7)
    t = np.arange(N) / rate
    audio = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t) + 0.05 * rng.standard_normal(N)).astype(np.float32)
    noise = rng.standard_normal(N).astype(np.float32)
    cases = {"audio": audio, "noise": (0.1 * noise).astype(np.float32), "silence": np.zeros(N, np.float32)}
    # a band sum of noise of amplitude a lies between 0.03 a^2 and 3e4 a^2: the first sums fall below 2^-100 = 7.9e-31
    # near a = 3e-15, all of them from 1e-18 on; the first denormal sums come at 3e-19, the first zeros at 1e-21
    for a in (1e-13, 1e-14, 3e-15, 1e-16, 1e-18, 3e-19, 1e-19, 1e-20, 1e-21, 1e-23):
        cases["tiny_%g" % a] = (a * noise).astype(np.float32)
    # ... and the sums pass 3.4e38 from a = 1e18 on; above 1e20 most single terms overflow and are skipped
    for a in (1e18, 5e18, 1e19, 2e19, 4e19, 8e19, 1.5e20, 1e21):
        cases["huge_%g" % a] = (a * noise).astype(np.float32)
    half = audio.copy()
    half[N // 2:] = 0.0                 # silence and audio in one clip: waves of both kinds in one launch
    cases["half_silent"] = half
    nan_burst = (0.1 * noise).astype(np.float32)
    nan_burst[3000:3003] = np.nan
    cases["nan_burst"] = nan_burst
    infs = (0.1 * noise).astype(np.float32)
    infs[5001] = np.inf
    infs[12000] = -np.inf
    cases["inf_samples"] = infs
    return cases


def _same_bits(got, want):
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return bool(((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all())


def _bits(lb, packed, length):
    p = packed.cpu().numpy()
    return lb.unpack_packed(p, length).reshape(p.shape[0], p.shape[1], length)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_band_means_and_bits_match_the_oracle(lb, gpu, oracle, name):
    rate = PLANS[name]
    divisors, kmax = _divisors(rate)
    assert kmax <= 22, "this plan would not run the pruned kernel"
    if name == "zero_divisor_48k":
        assert 0 in divisors
    if name == "wide_96k":
        assert max(divisors) > 63
    cfg = oracle.Config(sample_rate=rate, window=WINDOW)
    cases = _cases(rate)
    pcm = np.stack(list(cases.values()))
    clips = gpu.from_numpy(pcm).cuda()
    want = [oracle.fingerprint_pcm(pcm[i], cfg, taps=True) for i in range(len(cases))]
    # the inputs do what they are there for (44.1 kHz: the sums of the widest band, 63 terms)
    if name == "headline_44k":
        sums = {c: want[i][1][..., 31].astype(np.float64) * divisors[31] for i, c in enumerate(cases)}
        assert (sums["audio"] > 2.0 ** -100).all() and np.isfinite(sums["audio"]).all()
        assert any(((s > 0) & (s < 2.0 ** -100)).any() for c, s in sums.items() if c.startswith("tiny"))
        assert any(((s > 0) & (s < 2.0 ** -126)).any() for c, s in sums.items() if c.startswith("tiny"))
        assert any(np.isinf(s).any() for c, s in sums.items() if c.startswith("huge"))
    for variant in (0, 2):                                   # 2: specialised kernels or an error
        det = lb.Detective().configure(sample_rate=rate, window=WINDOW)
        det.set_kernel_variant(variant)
        for rep in range(2):                                 # twice: the claim counters are left at zero by the kernel itself
            packed, raw, _ = det.fingerprint_clips_device(clips, taps=True)
            plain = det.fingerprint_clips_device(clips)      # no tap: compact rows where the plan has them
            gpu.cuda.synchronize()
            bits, bits_plain, raw = _bits(lb, packed, cfg.subfp_len), _bits(lb, plain, cfg.subfp_len), raw.cpu().numpy()
            for i, cname in enumerate(cases):
                obits, oraw, _ = want[i]
                assert _same_bits(raw[i], oraw), f"{name}/{cname}: band means differ (variant {variant}, call {rep})"
                assert np.array_equal(bits[i], obits), f"{name}/{cname}: sub-fingerprints differ (variant {variant}, call {rep})"
                assert np.array_equal(bits_plain[i], obits), f"{name}/{cname}: sub-fingerprints without tap differ (variant {variant}, call {rep})"


@pytest.mark.parametrize("dtype", ["int16", "int32"])
def test_integer_input_band_means(lb, gpu, oracle, dtype):
    """The converting span loaders feed the same loop: int16 / int32 clips against the oracle on their float values."""
    # (a batch of clips goes through oracle.fingerprint_batch: [clips, sub-fingerprints, length] Booleans)
    rate = 44100
    cfg = oracle.Config(sample_rate=rate, window=WINDOW)
    rng = np.random.default_rng(11)
    if dtype == "int16":
        ints = rng.integers(-2000, 2000, (6, N)).astype(np.int16)
        ints[1] = 0
        ints[2, : N // 2] = 0
        as_float = (ints.astype(np.float64) / 32768.0).astype(np.float32)
    else:
        ints = rng.integers(-2 ** 31, 2 ** 31 - 1, (6, N), dtype=np.int64).astype(np.int32)
        ints[1] = 0
        ints[2] = rng.integers(-3, 4, N).astype(np.int32)       # 1e-9 of full scale: sums near 1e-20
        as_float = (ints.astype(np.float64) / 2.0 ** 31).astype(np.float32)
    want = oracle.fingerprint_batch(as_float, cfg)
    dev = gpu.from_numpy(ints).cuda()
    # the tap of the band means takes float32 only: integer clips are checked through the packed bits, on compact rows
    # (variant 0) and on full rows (variant 4), and their float values through the tap
    for variant in (0, 4):
        det = lb.Detective().configure(sample_rate=rate, window=WINDOW)
        det.set_kernel_variant(variant)
        got = _bits(lb, det.fingerprint_clips_device(dev), cfg.subfp_len)
        gpu.cuda.synchronize()
        assert np.array_equal(got, want), (dtype, variant)
    det = lb.Detective().configure(sample_rate=rate, window=WINDOW)
    _, raw, _ = det.fingerprint_clips_device(gpu.from_numpy(as_float).cuda(), taps=True)
    gpu.cuda.synchronize()
    raw = raw.cpu().numpy()
    for i in range(ints.shape[0]):
        assert _same_bits(raw[i], oracle.fingerprint_pcm(as_float[i], cfg, taps=True)[1]), (dtype, i)


def test_claim_counters_survive_many_launches(lb, gpu, oracle):
    """More frames than the persistent workgroups take statically, several times on one detective and on two streams:
    every launch must find the claim counters at zero (the last workgroup of the launch before it reset them)."""
    rate = 44100
    cfg = oracle.Config(sample_rate=rate, window=WINDOW)
    n_clips = 1200                                            # 2400 frames > 512 workgroups
    clips = lb.synth_clips_device(0x4C424144, 0, n_clips, rate, N)
    det = lb.Detective().configure(sample_rate=rate, window=WINDOW)
    first = det.fingerprint_clips_device(clips).cpu().numpy()
    host = clips[:8].cpu().numpy()
    assert np.array_equal(lb.unpack_packed(first[:8], cfg.subfp_len).reshape(8, -1, cfg.subfp_len), oracle.fingerprint_batch(host, cfg))
    side = gpu.cuda.Stream()
    for rep in range(4):
        if rep % 2:
            with gpu.cuda.stream(side):
                again = det.fingerprint_clips_device(clips)
            side.synchronize()
        else:
            again = det.fingerprint_clips_device(clips)
            gpu.cuda.synchronize()
        assert np.array_equal(again.cpu().numpy(), first), rep
    # a launch with fewer frames than workgroups (some exit at once) between two full ones
    small = det.fingerprint_clips_device(clips[:3]).cpu().numpy()
    assert np.array_equal(small, first[:3])
    assert np.array_equal(det.fingerprint_clips_device(clips).cpu().numpy(), first)
