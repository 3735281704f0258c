"""GPU parity of the two band-sum forms of the pruned stage 1 (k_rows_pruned.hip) on the plan 44.1 kHz / 1024 / 64 / 32 bands:
form 1 adds a band's power terms through LDS (frame_rows_pruned_kernel), form 2 in the lane that computed them
(frame_rows_lanes_kernel), form 0 (automatic) must take form 2.  Every case runs under all three: with the tap (full rows)
every band mean against the CPU oracle as a bit pattern, without it (compact rows) the packed bits, and the forms against
each other.

Shapes, the smallest at which the kernel can go wrong: one clip of exactly one frame; 3 clips of 2 frames (fewer frames than
XCDs: some workgroups leave at once through the ticket); 330 clips of 2 frames (more frames than the 512 persistent workgroups:
frames are claimed from the counters, the late store crosses units and frames); a clip with samples left over behind its last
frame.  Inputs as in tests/test_gpu_band_means.py: audio, noise, silence, half-silent; amplitudes 1e-13 .. 1e-23 (sums below
2^-100, denormal, zero: the fallback); 1e18 .. 1e21 (sums that overflow to +inf, single terms that are skipped); a NaN burst;
+-inf samples; int16 and int32 input.  On the 48 kHz and 96 kHz plans form 2 is an error and form 0 still equals the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATE, WINDOW, STRIDE, BANDS = 44100, 1024, 64, 32
ONE = WINDOW + STRIDE * 128            # exactly one frame: 9216 samples (see test_one_clip_of_one_frame)
N = WINDOW + STRIDE * 128 * 2          # two frames per clip
FORMS = (1, 2, 0)


def _inputs(rate, n):
    rng = np.random.default_rng(7)
    t = np.arange(n) / rate
    audio = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    noise = rng.standard_normal(n).astype(np.float32)
    cases = {"audio": audio, "noise": (0.1 * noise).astype(np.float32), "silence": np.zeros(n, np.float32)}
    half = audio.copy()
    half[n // 2:] = 0.0
    cases["half_silent"] = half
    # a band sum of noise of amplitude a lies between 0.03 a^2 and 3e4 a^2: the first sums fall below 2^-100 = 7.9e-31 near
    # a = 3e-15, the first denormal sums come at 3e-19, the first zeros at 1e-21
    for a in (1e-13, 1e-14, 3e-15, 1e-16, 1e-18, 3e-19, 1e-19, 1e-20, 1e-21, 1e-23):
        cases["tiny_%g" % a] = (a * noise).astype(np.float32)
    # ... and the sums pass 3.4e38 from a = 1e18 on; above 1e20 most single terms overflow and are skipped
    for a in (1e18, 5e18, 1e19, 2e19, 4e19, 8e19, 1.5e20, 1e21):
        cases["huge_%g" % a] = (a * noise).astype(np.float32)
    nan_burst = (0.1 * noise).astype(np.float32)
    nan_burst[3000:3003] = np.nan
    cases["nan_burst"] = nan_burst
    infs = (0.1 * noise).astype(np.float32)
    infs[5001] = np.inf
    infs[n - 4000] = -np.inf
    cases["inf_samples"] = infs
    return cases


def _same_bits(got, want):
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return bool(((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all())


def _bits(lb, packed, length):
    p = packed.cpu().numpy()
    return lb.unpack_packed(p, length).reshape(p.shape[0], p.shape[1], length)


def _det(lb, rate, form):
    det = lb.Detective().configure(sample_rate=rate, window=WINDOW, stride=STRIDE, bands=BANDS)
    det.set_band_sum_form(form)
    return det


@pytest.fixture(scope="module")
def reference(oracle):
    """The two-frame inputs and the oracle's (bits, band means) of each, computed once and left unchanged."""
    cfg = oracle.Config(sample_rate=RATE, window=WINDOW)
    cases = _inputs(RATE, N)
    pcm = np.stack(list(cases.values()))
    want = [oracle.fingerprint_pcm(pcm[i], cfg, taps=True) for i in range(len(cases))]
    pcm.setflags(write=False)
    return cfg, list(cases), pcm, np.stack([w[0] for w in want]), np.stack([w[1] for w in want])


def _check_forms(lb, gpu, cfg, pcm, want_bits, want_raw, what):
    """pcm [clips, samples] under the three forms, with and without the tap, against the oracle and each other."""
    clips = gpu.from_numpy(np.array(pcm, np.float32)).cuda()            # a writable copy: the reference stays untouched
    raws = {}
    for form in FORMS:
        det = _det(lb, RATE, form)
        assert det.band_sum_form() == (1 if form == 1 else 2), form        # automatic takes the lanes form
        for rep in range(2):                                               # twice: the kernel leaves its own counters at zero
            packed, raw, _ = det.fingerprint_clips_device(clips, taps=True)
            plain = det.fingerprint_clips_device(clips)                    # no tap: compact rows
            gpu.cuda.synchronize()
            raw = raw.cpu().numpy()
            assert _same_bits(raw, want_raw), f"{what}: band means differ from the oracle (form {form}, call {rep})"
            assert np.array_equal(_bits(lb, packed, cfg.subfp_len), want_bits), f"{what}: bits with tap (form {form}, call {rep})"
            assert np.array_equal(_bits(lb, plain, cfg.subfp_len), want_bits), f"{what}: bits on compact rows (form {form}, call {rep})"
        raws[form] = raw
    assert np.array_equal(raws[1].view(np.uint32), raws[2].view(np.uint32)), f"{what}: the two forms differ"
    assert np.array_equal(raws[0].view(np.uint32), raws[2].view(np.uint32)), f"{what}: automatic is not the lanes form"


def test_every_input_two_frames(lb, gpu, reference):
    cfg, names, pcm, want_bits, want_raw = reference
    # the inputs do what they are there for: sums of the widest live band (three terms) below the guard, denormal, +inf
    sums = want_raw[..., BANDS - 1].astype(np.float64) * 63.0           # the band's divisor at 44.1 kHz
    tiny = [i for i, c in enumerate(names) if c.startswith("tiny")]
    assert ((sums[tiny] > 0) & (sums[tiny] < 2.0 ** -100)).any() and ((sums[tiny] > 0) & (sums[tiny] < 2.0 ** -126)).any()
    assert np.isinf(sums[[i for i, c in enumerate(names) if c.startswith("huge")]]).any()
    _check_forms(lb, gpu, cfg, pcm, want_bits, want_raw, "all inputs")


def test_three_clips_of_two_frames(lb, gpu, reference):
    cfg, names, pcm, want_bits, want_raw = reference
    pick = [names.index("audio"), names.index("tiny_1e-18"), names.index("huge_2e+19")]
    _check_forms(lb, gpu, cfg, pcm[pick], want_bits[pick], want_raw[pick], "3 clips")


def test_more_frames_than_workgroups(lb, gpu, reference):
    cfg, names, pcm, want_bits, want_raw = reference
    pick = np.arange(330) % len(names)                                     # 660 frames > 512 workgroups
    _check_forms(lb, gpu, cfg, pcm[pick], want_bits[pick], want_raw[pick], "330 clips")


def test_one_clip_of_one_frame(lb, gpu, oracle, reference):
    """The shortest clip that holds a frame.  Its 128 windows end at sample 1024 + 127 * 64 = 9152, but the frame count is
    ((samples - window) / hop) / 128 as upstream computes it: 9152 samples make no frame (nothing is launched for them), 9216
    make one."""
    cfg, names, pcm, _, _ = reference
    clip = pcm[names.index("audio")][:ONE]
    bits, raw, _ = oracle.fingerprint_pcm(clip, cfg, taps=True)
    assert bits.shape[0] == 1 and oracle.fingerprint_pcm(clip[:ONE - STRIDE], cfg).shape[0] == 0
    _check_forms(lb, gpu, cfg, clip[None], bits[None], raw[None], "one frame")


def test_samples_left_over_behind_the_last_frame(lb, gpu, oracle, reference):
    cfg, names, pcm, _, _ = reference
    pick = [names.index("noise"), names.index("half_silent"), names.index("inf_samples")]
    clips = np.ascontiguousarray(pcm[pick][:, :ONE + STRIDE * 128 + 37])   # two frames and 37 samples
    want = [oracle.fingerprint_pcm(c, cfg, taps=True) for c in clips]
    assert want[0][0].shape[0] == 2
    _check_forms(lb, gpu, cfg, clips, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), "left-over samples")


@pytest.mark.parametrize("dtype", ["int16", "int32"])
def test_integer_input(lb, gpu, oracle, dtype):
    """The converting span loaders feed the same loop: the packed bits on compact rows (variant 0) and on full rows (variant 4;
    the tap takes float32 only), under every form."""
    cfg = oracle.Config(sample_rate=RATE, window=WINDOW)
    rng = np.random.default_rng(11)
    if dtype == "int16":
        ints = rng.integers(-2000, 2000, (6, N)).astype(np.int16)
        ints[1] = 0
        ints[2, : N // 2] = 0
        as_float = (ints.astype(np.float64) / 32768.0).astype(np.float32)
    else:
        ints = rng.integers(-2 ** 31, 2 ** 31 - 1, (6, N), dtype=np.int64).astype(np.int32)
        ints[1] = 0
        ints[2] = rng.integers(-3, 4, N).astype(np.int32)                  # 1e-9 of full scale: sums near 1e-20
        as_float = (ints.astype(np.float64) / 2.0 ** 31).astype(np.float32)
    want = oracle.fingerprint_batch(as_float, cfg)
    dev = gpu.from_numpy(ints).cuda()
    for form in FORMS:
        for variant in (0, 4):
            det = _det(lb, RATE, form)
            det.set_kernel_variant(variant)
            got = _bits(lb, det.fingerprint_clips_device(dev), cfg.subfp_len)
            gpu.cuda.synchronize()
            assert np.array_equal(got, want), (dtype, form, variant)


@pytest.mark.parametrize("rate", [48000, 96000])
def test_other_tables_refuse_the_lanes_form(lb, gpu, oracle, rate):
    cfg = oracle.Config(sample_rate=rate, window=WINDOW)
    cases = _inputs(rate, N)
    pick = ["audio", "tiny_1e-18", "huge_2e+19", "nan_burst"]
    pcm = np.stack([cases[c] for c in pick])
    det = lb.Detective().configure(sample_rate=rate, window=WINDOW, stride=STRIDE, bands=BANDS)
    with pytest.raises(lb.LBAudioDetectiveError):
        det.set_band_sum_form(2)
    det.set_band_sum_form(0)
    assert det.band_sum_form() == 1
    packed, raw, _ = det.fingerprint_clips_device(gpu.from_numpy(pcm).cuda(), taps=True)
    gpu.cuda.synchronize()
    raw = raw.cpu().numpy()
    for i, c in enumerate(pick):
        bits, oraw, _ = oracle.fingerprint_pcm(pcm[i], cfg, taps=True)
        assert _same_bits(raw[i], oraw), (rate, c)
        assert np.array_equal(_bits(lb, packed, cfg.subfp_len)[i], bits), (rate, c)
