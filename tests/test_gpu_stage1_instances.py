"""Every template instance of the stage-1 kernels (PCM windows -> 128 x bands frame rows) against the CPU oracle, one named case
at a time.

Stage 1 is some seventy instances chosen at run time by window, stride, band table, sample format, clip alignment, variant
and tuning.  Every kernel returns the same bits, so a configuration that silently moves to another kernel still passes a
parity test -- and the test that was meant to cover an instance stops covering it.  Each case below therefore NAMES the
instance it is there for, by hand, and asserts three things:

  1. routing: LBAudioDetectiveDebugStage1Choice for exactly this call (settings, variant, tuning, format, clip count and length,
     the tensor's address modulo 8, tap on and off) answers the instance the case names;
  2. band means: every float of the raw tap equals the oracle's as a bit pattern (test_gpu_band_means._same_bits: NaN equals
     NaN, nothing else is forgiven) -- integer PCM included, against the oracle on the float32 values the integers convert to
     (/ 32768, / 2^31: exact up to the one rounding of an int32 to float32);
  3. the Haar frame and the packed bits equal the oracle's; the bits a second time WITHOUT the tap, which is where the pruned
     kernel writes compact rows and where a batch walks in chunks.

INVENTORY is the full list of instances; test_every_instance_has_a_case fails when one of them has no case, and
tests/test_stage1_choice_cpu.py (no GPU) shows that the public settings reach every one of them, so none is excused.  The
same file checks the routing of every case on the CPU.

No live band: at 16- and 32-sample windows no sample rate from 650 Hz to 100 kHz gives a band a bin (the edges of every band
fall on one bin), so the rows of those cases are 0 / divisor -- +0 or NaN; what is observable (the rows, the Haar frame, the
bits) is still compared.  The other generic cases use rates at which their window has live bands."""
import collections

import numpy as np
import pytest

from test_gpu_band_means import _same_bits

pytestmark = pytest.mark.gpu

SEED = 0x4C424144
FMT_NAMES = ("f32", "i16", "i32")

# ---- the instances ---------------------------------------------------------------------------------------------------------
# fft_bands_kernel<LOG2W, WPB, CACHED>: the workgroup sizes launch_one lists per window size, with and without the twiddle cache
_GENERIC_WPB = {11: (12, 8, 4, 2, 1), 12: (7, 6, 4, 2, 1), 13: (2, 1)}
INVENTORY = {("generic", log2w, wpb, cached) for log2w in range(4, 14) for wpb in _GENERIC_WPB.get(log2w, (4,)) for cached in (0, 1)}
# frame_rows_pruned_kernel<FMT> (full or compact rows: a run-time argument), rows_stream_kernel<FMT>
INVENTORY |= {("pruned", fmt) for fmt in range(3)} | {("stream", fmt) for fmt in range(3)}
# rows_stream2_kernel<FMT, 2, 24> and <FMT, 0, 32>
INVENTORY |= {("stream2", fmt, qlo, qhi) for fmt in range(3) for qlo, qhi in ((2, 24), (0, 32))}
# rows_full_kernel<LOG2L, FMT, S64, lean>: 12 at stride 64, 4 float ones at other strides, 2 lean ones for 2048-sample windows
INVENTORY |= {("full", log2l, fmt, 1, 0) for log2l in range(1, 5) for fmt in range(3)}
INVENTORY |= {("full", log2l, 0, 0, 0) for log2l in range(1, 5)} | {("full", 4, 0, 1, 1), ("full", 4, 0, 0, 1)}
# instances the public settings cannot reach (tests/test_stage1_choice_cpu.py decides): none
UNREACHABLE = {}

# ---- the cases -------------------------------------------------------------------------------------------------------------
# cfg: (sample rate, window, stride, bands, sub-fingerprint length).  shape: "default" 3 clips of window + stride * (128 * 2 + 17)
# samples (two frames and a ragged tail); "one_frame" 1 clip of exactly one frame; "odd" 3 clips of an odd length (integer clips
# then start on 2-byte boundaries only); "offset" 1 clip whose tensor starts one sample into an allocation; "claimed" 600 clips of
# one frame (more frames than persistent workgroups: frames are claimed); "chunked" 5 clips of one frame, the scratch limit set
# so that the untapped call takes chunks of 2, 2 and 1.  want: the instance, BY HAND.  compact: the untapped call's rows.
Case = collections.namedtuple("Case", "name cfg fmt shape variant waves cache want fell_back compact")
CASES = []


def _case(name, cfg, want, fmt=0, shape="default", variant=0, waves=0, cache=True, fell_back=False, compact=False):
    CASES.append(Case("%s-%s-%s" % (name, FMT_NAMES[fmt], shape), cfg, fmt, shape, variant, waves, cache, tuple(want), fell_back,
                      compact))


SHAPES = ("default", "one_frame", "odd", "offset")
ALIGNED = ("default", "one_frame")            # shapes whose clips all start on sample-pair boundaries

# the generic kernel: one case per window size at automatic tuning, configurations without a specialised kernel ...
# (small windows have live bands only at low sample rates: 2 of 7 at 950 Hz / 64, 7 of 16 at 1150 Hz / 128, 26 of 64 at 1300 Hz / 256)
GENERIC = {4: (8000, 16, 16, 7, 33), 5: (8000, 32, 5, 32, 200), 6: (950, 64, 16, 7, 33), 7: (1150, 128, 100, 16, 200),
           8: (1300, 256, 100, 64, 256), 9: (8000, 512, 7, 20, 150), 10: (44100, 1024, 63, 32, 200),
           11: (44100, 2048, 63, 32, 200), 12: (44100, 4096, 65, 32, 200), 13: (44100, 8192, 64, 32, 200)}
_AUTO_WPB = {11: 12, 12: 7, 13: 1}
for _l, _cfg in GENERIC.items():
    _case("generic%d_auto" % _l, _cfg, ("generic", _l, _AUTO_WPB.get(_l, 4), 1))
    if _l <= 10:                              # ... and without the cache (the only other instance of these window sizes)
        _case("generic%d_nocache" % _l, _cfg, ("generic", _l, 4, 0), cache=False)
# window 8192 at 96 kHz with 64 bands, and where the cache does not fit beside one wave's 8192 samples and the table's bins: the
# uncached instance is taken AUTOMATICALLY (11 025 Hz reads more than 3000 bins)
_case("generic13_96k_64", (96000, 8192, 64, 64, 256), ("generic", 13, 1, 1))
_case("generic13_auto_uncached", (11025, 8192, 64, 32, 200), ("generic", 13, 1, 0), fell_back=True)
# every workgroup size launch_one lists for 2048, 4096 and 8192 samples, cache on and off, through set_kernel_tuning
for _l in (11, 12):
    for _w in _GENERIC_WPB[_l]:
        for _c in (1, 0):
            _case("generic%d_w%d_c%d" % (_l, _w, _c), GENERIC[_l], ("generic", _l, _w, _c), waves=_w, cache=bool(_c))
_case("generic13_w1_c1", GENERIC[13], ("generic", 13, 1, 1), waves=1)
_case("generic13_w1_c0", GENERIC[13], ("generic", 13, 1, 0), waves=1, cache=False)
_case("generic13_w2_c0", GENERIC[13], ("generic", 13, 2, 0), waves=2, cache=False)
# two waves AND the cache do not fit beside the 1500 bins 44.1 kHz reads: reported as falling back to one wave without the cache
_case("generic13_w2_c1_falls_back", GENERIC[13], ("generic", 13, 1, 0), waves=2, fell_back=True)
# ... they fit where the table reads few bins (3300 Hz: some 180)
_case("generic13_w2_c1_narrow", (3300, 8192, 64, 32, 200), ("generic", 13, 2, 1), waves=2)
_case("generic13_auto_narrow", (3300, 8192, 64, 32, 200), ("generic", 13, 2, 1))            # ... and are then the automatic choice
# a workgroup size the window has no instance for falls back as well
_case("generic11_w3_falls_back", GENERIC[11], ("generic", 11, 4, 0), waves=3, fell_back=True)
# the generic kernel reads the format at run time: integer PCM and every shape at a small and at a large window
for _fmt in range(3):
    for _shape in SHAPES:
        if _fmt or _shape != "default":
            _case("generic7", GENERIC[7], ("generic", 7, 4, 1), fmt=_fmt, shape=_shape)
    if _fmt:
        _case("generic13", GENERIC[13], ("generic", 13, 1, 1), fmt=_fmt)
        _case("generic13", GENERIC[13], ("generic", 13, 1, 1), fmt=_fmt, shape="odd")

# the pruned kernel (1024 samples, bins 0..21): alignment does not matter to it; compact rows without the tap
PRUNED = (44100, 1024, 64, 32, 200)
for _fmt in range(3):
    for _shape in SHAPES + ("chunked",):
        if _shape != "chunked" or _fmt < 2:
            _case("pruned", PRUNED, ("pruned", _fmt), fmt=_fmt, shape=_shape, compact=True)
_case("pruned_48k_zero_divisor", (48000, 1024, 64, 32, 200), ("pruned", 1), fmt=1)      # no sparse form: full rows
_case("pruned_full_rows", PRUNED, ("pruned", 2), fmt=2, variant=4)

# the streaming kernel of 2048-sample windows: q 2..23 at the default table, q 0..31 elsewhere; clips that do not start on pair
# boundaries go to rows_full_kernel<4> (float32 at the default table: its lean instance)
STREAM2 = (5512, 2048, 64, 32, 200)
STREAM2_WIDE = (11025, 2048, 64, 32, 200)
for _fmt in range(3):
    for _shape in ALIGNED + (("chunked",) if _fmt < 2 else ()):
        _case("stream2", STREAM2, ("stream2", _fmt, 2, 24), fmt=_fmt, shape=_shape)
    _case("stream2_wide", STREAM2_WIDE, ("stream2", _fmt, 0, 32), fmt=_fmt)
    _case("stream2_wide", STREAM2_WIDE, ("stream2", _fmt, 0, 32), fmt=_fmt, shape="one_frame")
    for _shape in ("odd", "offset"):
        _case("stream2_steps_aside", STREAM2, ("full", 4, _fmt, 1, 1 if _fmt == 0 else 0), fmt=_fmt, shape=_shape)
        _case("stream2_wide_steps_aside", STREAM2_WIDE, ("full", 4, _fmt, 1, 0), fmt=_fmt, shape=_shape)

# the streaming kernel of 4096-sample windows; there is no other specialised kernel of that size: unaligned clips go generic
STREAM = (48000, 4096, 64, 32, 200)
for _fmt in range(3):
    for _shape in ALIGNED + (("chunked",) if _fmt < 2 else ()):
        _case("stream", STREAM, ("stream", _fmt), fmt=_fmt, shape=_shape)
    for _shape in ("odd", "offset"):
        _case("stream_steps_aside", STREAM, ("generic", 12, 7, 1), fmt=_fmt, shape=_shape)

# rows_full_kernel at stride 64: LOG2L 1..4 (256 .. 2048 samples) x three formats, every shape (alignment does not matter)
FULL64 = {1: (8000, 256, 64, 32, 200), 2: (11025, 512, 64, 2, 20), 3: (22050, 1024, 64, 32, 200), 4: (22050, 2048, 64, 64, 256)}
for _l, _cfg in FULL64.items():
    for _fmt in range(3):
        for _shape in SHAPES:
            _case("full%d" % _l, _cfg, ("full", _l, _fmt, 1, 0), fmt=_fmt, shape=_shape)
# more than 512 frames: the persistent workgroups claim frames; and the chunked run
_case("full3", FULL64[3], ("full", 3, 0, 1, 0), shape="claimed")
_case("full3", FULL64[3], ("full", 3, 0, 1, 0), shape="chunked")
_case("full3", FULL64[3], ("full", 3, 1, 1, 0), fmt=1, shape="chunked")
# ... at other even strides: float32 only, the general span loader; integer PCM runs on the generic kernel
FULL_OTHER = {1: (8000, 256, 2, 32, 200), 2: (8000, 512, 6, 20, 150), 3: (11025, 1024, 32, 32, 200), 4: (22050, 2048, 128, 48, 256)}
for _l, _cfg in FULL_OTHER.items():
    for _shape in SHAPES:
        _case("full%d_stride%d" % (_l, _cfg[2]), _cfg, ("full", _l, 0, 0, 0), shape=_shape)
    _case("full%d_stride%d_integer_goes_generic" % (_l, _cfg[2]), _cfg, ("generic", _l + 7, 12 if _l == 4 else 4, 1), fmt=1)
# the lean instances of 2048-sample windows (a table that reads no more terms than the default's): the file hop of 8, and
# stride 64 where the streaming kernel is not taken (variant 3)
_case("full4_lean_hop8", (5512, 2048, 8, 32, 200), ("full", 4, 0, 0, 1))
_case("full4_lean_hop8", (5512, 2048, 8, 32, 200), ("full", 4, 0, 0, 1), shape="odd")
_case("full4_lean_variant3", STREAM2, ("full", 4, 0, 1, 1), variant=3)

assert len({c.name for c in CASES}) == len(CASES)


def test_every_instance_has_a_case():
    """(needs no GPU itself; tests/test_stage1_choice_cpu.py repeats it)"""
    covered = {c.want for c in CASES}
    assert not (INVENTORY - set(UNREACHABLE) - covered), sorted(INVENTORY - set(UNREACHABLE) - covered)
    assert covered <= INVENTORY and set(UNREACHABLE) <= INVENTORY


# ---- inputs and the oracle's answers, made once per (configuration, format, shape) ----------------------------------------------
def case_shape(case):
    """(clips, samples per clip, the tensor's address modulo 8)"""
    _, window, stride, _, _ = case.cfg
    n = window + stride * (128 * 2 + 17)
    elem = 2 if case.fmt == 1 else 4
    return {"default": (3, n, 0), "one_frame": (1, window + stride * 128, 0), "odd": (3, n | 1, 0), "offset": (1, n, elem),
            "claimed": (600, window + stride * 128, 0), "chunked": (5, window + stride * (128 + 17), 0)}[case.shape]


_REFERENCE = {}


def _reference(oracle, case):
    """(the clips as the device gets them, per clip the oracle's (bits, raw frames, Haar frames)); read-only once made"""
    key = (case.cfg, case.fmt, case.shape)
    if key in _REFERENCE:
        return _REFERENCE[key]
    n_clips, spc, _ = case_shape(case)
    rate = case.cfg[0]
    pcm = oracle.synth_clips(SEED, 100, n_clips, rate, spc)
    if n_clips >= 3:
        pcm[1, : spc // 2] = 0.0                            # silence in the first half
    if case.fmt == 0:
        clips, as_float = pcm, pcm
    else:
        rng = np.random.default_rng(spc)
        lo, hi, scale = (-32768, 32767, 32768.0) if case.fmt == 1 else (-2 ** 31, 2 ** 31 - 1, 2.0 ** 31)
        ints = np.rint(pcm.astype(np.float64) * (0.9 * scale))
        if case.fmt == 2:
            ints += rng.integers(-100, 101, ints.shape)     # low bits that the conversion to float32 has to round
        ints[pcm == 0.0] = 0
        if n_clips >= 3:                                    # full-scale extremes: a loader that converts through the wrong width
            pick = rng.integers(0, 4, spc)
            ints[2] = np.where(pick == 0, lo, np.where(pick == 1, hi, ints[2]))
        else:
            ints[0, 5::97] = lo
            ints[0, 50::97] = hi
        clips = np.clip(ints, lo, hi).astype(np.int16 if case.fmt == 1 else np.int32)
        as_float = (clips.astype(np.float64) / scale).astype(np.float32)
    cfg = oracle.Config(*case.cfg)
    want = [oracle.fingerprint_pcm(as_float[c], cfg, taps=True) for c in range(n_clips)]
    for a in (clips,) + tuple(x for w in want for x in w):
        a.setflags(write=False)
    _REFERENCE[key] = (clips, want)
    return _REFERENCE[key]


def check_routing(lb, det, case, address):
    """Assertion 1; needs no GPU (det: a Detective with the case's settings)"""
    n_clips, spc, _ = case_shape(case)
    for taps in (True, False):
        ch = det.stage1_choice(case.fmt, n_clips, spc, address, taps=taps, variant=case.variant, waves=case.waves, cache=case.cache)
        assert ch.status == 0 and ch.launches, (case.name, ch)
        assert (ch.family,) + ch.args == case.want, (case.name, taps, ch)
        assert ch.fell_back == case.fell_back, (case.name, ch)
        assert ch.compact == (case.compact and not taps), (case.name, taps, ch)


def _run(lb, gpu, oracle, case):
    rate, window, stride, bands, subfp_len = case.cfg
    n_clips, spc, address = case_shape(case)
    clips_host, want = _reference(oracle, case)
    det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=subfp_len)
    det.set_kernel_variant(case.variant)
    det.set_kernel_tuning(case.waves, case.cache)
    if case.shape == "offset":                              # the clip starts one sample into an allocation
        block = gpu.empty(spc + 1, dtype=(gpu.float32, gpu.int16, gpu.int32)[case.fmt], device="cuda")
        block[1:] = gpu.from_numpy(np.array(clips_host).reshape(-1)).cuda()
        clips = block[1:].view(1, spc)
    else:
        clips = gpu.from_numpy(np.array(clips_host)).cuda()      # (a copy: the shared reference stays read-only)
    assert clips.is_contiguous() and clips.data_ptr() % 8 == address
    check_routing(lb, det, case, clips.data_ptr())
    packed, raw, haar = det.fingerprint_clips_device(clips, taps=True)
    per = packed.shape[1]
    if case.shape == "chunked":                             # chunks of 2, 2 and 1 clips (one frame each)
        assert per == 1 and n_clips == 5
        det.set_scratch_limit(2 * 128 * bands * 4)
    plain = det.fingerprint_clips_device(clips)
    gpu.cuda.synchronize()
    raw, haar = raw.cpu().numpy(), haar.cpu().numpy()
    bits = lb.unpack_packed(packed.cpu().numpy(), subfp_len).reshape(n_clips, per, subfp_len)
    bits_plain = lb.unpack_packed(plain.cpu().numpy(), subfp_len).reshape(n_clips, per, subfp_len)
    for c in range(n_clips):
        obits, oraw, ohaar = want[c]
        assert oraw.shape == raw[c].shape == (per, 128, bands)
        assert _same_bits(raw[c], oraw), f"{case.name}: band means differ (clip {c})"
        assert np.array_equal(haar[c], ohaar, equal_nan=True), f"{case.name}: Haar coefficients differ (clip {c})"
        assert np.array_equal(bits[c], obits), f"{case.name}: sub-fingerprint bits differ (clip {c})"
        assert np.array_equal(bits_plain[c], obits), f"{case.name}: sub-fingerprint bits without the tap differ (clip {c})"


def _group(family):
    """the cases that are there for an instance of `family`"""
    return [pytest.param(c, id=c.name) for c in CASES if c.want[0] == family]


@pytest.mark.parametrize("case", _group("generic"))
def test_generic_instances(lb, gpu, oracle, case):
    _run(lb, gpu, oracle, case)


@pytest.mark.parametrize("case", _group("pruned"))
def test_pruned_instances(lb, gpu, oracle, case):
    _run(lb, gpu, oracle, case)


@pytest.mark.parametrize("case", _group("stream2"))
def test_stream2_instances(lb, gpu, oracle, case):
    _run(lb, gpu, oracle, case)


@pytest.mark.parametrize("case", _group("full"))
def test_full_instances(lb, gpu, oracle, case):
    _run(lb, gpu, oracle, case)


@pytest.mark.parametrize("case", _group("stream"))
def test_stream_instances(lb, gpu, oracle, case):
    _run(lb, gpu, oracle, case)
