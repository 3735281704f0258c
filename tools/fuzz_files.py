#!/usr/bin/env python3
"""Randomized sweep of the file entry points (not part of the test suite): tools/fuzz_files.py [trials] [seed].
Random WAV and CAF files (rate, 1-3 channels, 8 / 16 / 24 / 32-bit integer or 32 / 64-bit float samples of either
byte order, IMA4 packets with and without a packet table, any length) through LBAudioDetectiveProcessAudioURL --
decode and conversion to the processing rate on the DEVICE, then upstream's file loop -- against the ORACLE's own
file front end (oracle/lbad_file_oracle.c: container, IMA4 / LPCM decode, converter models, file loop; no code shared
with the library): the two must agree bit for bit for every payload format, rate ratio (decimating and
interpolating), converter model, hop mode and end-of-file treatment.  The library's HOST functions
(LBAudioDetectiveReadAudioURL) are checked against the oracle's decode + conversion on the way.
Before the fingerprints the SAMPLES are compared: LBAudioDetectiveConvertAudioURL (decode + conversion on the device)
against the oracle's decode + conversion, on bit patterns (tools/converter_paths.py: -0.0 is not +0.0, a NaN of the
oracle must be a NaN of the device), for every trial whose file the oracle accepts.  The processing rate and, for CAF
files, the file rate are also drawn from fractional and large-q rates (5512.5, 22254.54545, 22051, ...), which take
the converter's double-position path; the last line counts the trials per converter path as the branch model of
tools/converter_paths.py names them, and a run must have reached all of them.  One float file in four carries NaN
bursts, infinities and negative zeros; such a trial is redrawn when more than a tenth of the oracle's output is NaN
(fewer than 5 % of the trials may be, asserted), and when it holds a NaN or an infinity it is compared at the sample
level only: which of two NaN wavelet magnitudes is the larger is not defined by the fingerprint stage.
Round 2, decode and conversion on the device: 60 000 trials (seed 13), 0 mismatches, 423 s on one MI355X (34 570 of the
files long enough for at least one sub-fingerprint: 9 793 IMA4, 12 483 CAF LPCM, 12 294 WAV).
With the sample-level comparison and the wider rate lists: 300 trials (seed 20261002, the suite's run), 0 mismatches,
5.7 s on one MI355X against 4.8 s for the same run of the version before (the oracle's conversion was already part of
every trial, the device's ConvertAudioURL is what was added), every converter path reached: linear 97, rational-staged
122, plain 56, rational-unstaged 18, rational-q1 20, tiled-staged 35, tiled-ragged-taps 19, tiled-unstaged-input 5,
copy 2; no trial redrawn.  The drawn file lengths are unchanged (up to three seconds).  Long run: 20 000 trials
(seed 13), 0 mismatches, 281 s on one MI355X, all compared at the sample level, 4 930 with special values, 5 redrawn;
trials per path: rational-staged 7 830, linear 6 677, plain 3 461, tiled-staged 2 667, rational-unstaged 1 779,
tiled-ragged-taps 1 772, rational-q1 1 435, tiled-unstaged-input 629, copy 145."""
import os, struct, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collections
import numpy as np
import converter_paths as fp
import lbaudiodetective_amd as lb
from oracle import oracle as O

trials = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
bad = 0
redraws = 0
sample_checks = 0
special_trials = 0
paths_seen = collections.Counter()
rejected = {}
nonempty = {}
t0 = time.time()
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "f.wav")


specials = {"on": False, "nonfinite": False}


def with_specials(a):
    """Now and then: a NaN burst, single infinities and runs of negative zeros in a float payload (in place)."""
    specials["nonfinite"] = False
    if not specials["on"] or a.shape[0] < 8:
        return a
    n = a.shape[0]
    for _ in range(int(rng.integers(1, 4))):
        what, at = int(rng.integers(0, 4)), int(rng.integers(0, n))
        if what == 0:
            a[at:at + int(rng.integers(1, 9))] = np.nan
        elif what == 1:
            a[at, int(rng.integers(0, a.shape[1]))] = np.inf if rng.integers(0, 2) else -np.inf
        else:
            a[at:at + int(rng.integers(1, 2000))] = -0.0
        specials["nonfinite"] = specials["nonfinite"] or what < 2
    return a


def write_wav(x, rate, channels, kind):
    """x: float64 [frames, channels] in [-1, 1)."""
    if kind == "f32":
        data, tag, bits = with_specials(x.astype("<f4")).tobytes(), 3, 32
    elif kind == "u8":
        data, tag, bits = (np.clip(np.round(x * 128) + 128, 0, 255)).astype(np.uint8).tobytes(), 1, 8
    elif kind == "i16":
        data, tag, bits = np.clip(np.round(x * 32768), -32768, 32767).astype("<i2").tobytes(), 1, 16
    elif kind == "i24":
        v = np.clip(np.round(x * 8388608), -8388608, 8388607).astype("<i4")
        data, tag, bits = v.view(np.uint8).reshape(-1, 4)[:, :3].tobytes(), 1, 24
    else:
        data, tag, bits = np.clip(np.round(x * 2147483648.0), -2**31, 2**31 - 1).astype("<i4").tobytes(), 1, 32
    block = channels * bits // 8
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, tag, channels, rate, rate * block, block, bits)
    open(path, "wb").write(hdr + b"data" + struct.pack("<I", len(data)) + data)


def write_caf(rate, fourcc, flags, bytes_per_packet, frames_per_packet, channels, bits, payload, pakt=None):
    desc = struct.pack(">d4sIIIII", float(rate), fourcc, flags, bytes_per_packet, frames_per_packet, channels, bits)
    out = b"caff" + struct.pack(">HH", 1, 0) + b"desc" + struct.pack(">q", len(desc)) + desc
    if pakt is not None:
        body = struct.pack(">qqii", pakt[0], pakt[1], pakt[2], 0)
        out += b"pakt" + struct.pack(">q", len(body)) + body
    out += b"data" + struct.pack(">q", 4 + len(payload)) + struct.pack(">I", 0) + payload
    open(path, "wb").write(out)


def write_caf_lpcm(x, rate, channels, kind, little):
    """x: float64 [frames, channels]; kind: i8 / i16 / i24 / i32 / f32 / f64."""
    e = "<" if little else ">"
    if kind == "f32":
        data, bits, fl = with_specials(x.astype(e + "f4")).tobytes(), 32, 1
    elif kind == "f64":
        data, bits, fl = with_specials(x.astype(e + "f8")).tobytes(), 64, 1
    elif kind == "i8":
        data, bits, fl = np.clip(np.round(x * 128), -128, 127).astype(np.int8).tobytes(), 8, 0
    elif kind == "i16":
        data, bits, fl = np.clip(np.round(x * 32768), -32768, 32767).astype(e + "i2").tobytes(), 16, 0
    elif kind == "i24":
        v = np.clip(np.round(x * 8388608), -8388608, 8388607).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]
        data, bits, fl = (v if little else v[:, ::-1]).tobytes(), 24, 0
    else:
        data, bits, fl = np.clip(np.round(x * 2147483648.0), -2**31, 2**31 - 1).astype(e + "i4").tobytes(), 32, 0
    write_caf(rate, b"lpcm", fl | (2 if little else 0), channels * bits // 8, 1, channels, bits, data)


BIRD = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "birds", "BlackBird.caf"), "rb").read()
_at = BIRD.index(b"data") + 12 + 4
IMA_PACKETS = np.frombuffer(BIRD[_at: _at + 34 * ((len(BIRD) - _at) // 34)], np.uint8).reshape(-1, 34)


def write_caf_ima4(rate, channels, n_packets):
    """Any 34-byte packet is a valid IMA4 packet: interleave packets of a bird fixture as `channels` channels."""
    pick = rng.integers(0, IMA_PACKETS.shape[0], size=n_packets * channels)
    payload = IMA_PACKETS[pick].tobytes()
    pakt = None
    if rng.integers(0, 2):
        priming = int(rng.choice([0, 0, 7, 64, 100]))
        valid = int(rng.integers(0, n_packets * 64 + 1))
        pakt = (n_packets, valid, priming)
    write_caf(rate, b"ima4", 0, 34 * channels, 64, channels, 0, payload, pakt)


RATES = [4000, 8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000]
CAF_RATES = RATES + [22254.54545, 44100.5]
PROCESSING_RATES = [5512, 8000, 11025, 44100, 5512.5, 5000.5, 8000.5, 11025.5, 22051, 44100.5]


# rate pairs of converter paths that the two lists above reach too seldom for a run of a few hundred trials (the input
# span of a tiled block too long to stage, ragged tap counts, q = 1, rational ranges too long to stage): one trial in
# three takes one of them
RARE_PAIRS = [(96000, 8000.5), (44100, 44100.5), (5512, 5512.5), (48000, 8000), (44100, 11025), (64000, 5512), (96000, 5512)]


def draw_file(pair):
    """One random file at `path`: (file rate, channels, container, frames)."""
    container = rng.integers(0, 3)
    file_rate = float(rng.choice(CAF_RATES)) if container else int(rng.choice(RATES))
    if pair is not None:
        file_rate = pair[0]
    channels = int(rng.choice([1, 1, 2, 3]))
    frames = int(rng.integers(0, 3 * int(file_rate)))
    specials["on"] = rng.integers(0, 4) == 0
    specials["nonfinite"] = False
    if container == 2:
        write_caf_ima4(file_rate, channels, frames // 64)
    else:
        x = O.synth_clip(int(rng.integers(0, 2**31)), 3, 44100, max(frames * channels, 1))[: frames * channels].astype(np.float64).reshape(frames, channels)
        if container == 0:
            write_wav(x, file_rate, channels, str(rng.choice(["f32", "u8", "i16", "i24", "i32"])))
        else:
            write_caf_lpcm(x, file_rate, channels, str(rng.choice(["f32", "f64", "i8", "i16", "i24", "i32"])), bool(rng.integers(0, 2)))
    return file_rate, channels, container, frames


for t in range(trials):
    pair = RARE_PAIRS[int(rng.integers(0, len(RARE_PAIRS)))] if rng.integers(0, 3) == 0 else None
    file_rate, channels, container, frames = draw_file(pair)
    if rng.integers(0, 3) == 0:
        cfg = O.Config(float(rng.choice(PROCESSING_RATES)), int(2 ** rng.integers(7, 12)), int(rng.choice([32, 64, 100])),
                       int(rng.integers(1, 65)), 1)
        cfg.subfp_len = int(rng.integers(1, min(256, 128 * cfg.bands) + 1))
    else:
        cfg = O.Config()
    if pair is not None:
        cfg.sample_rate = pair[1]
    hop_mode, tail_mode, resampler = int(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
    det = lb.Detective().configure(sample_rate=cfg.sample_rate, window=cfg.window, stride=cfg.stride, bands=cfg.bands,
                                   subfp_len=cfg.subfp_len)
    det.set_file_hop_mode(hop_mode).set_file_tail_mode(tail_mode)
    det.set_resampler_mode(resampler)
    while True:                                                  # (a file whose conversion is mostly NaN compares nothing: redraw it)
        try:
            xs, rate = O.decode_audio_file(path)
            ys = O.resample(xs, rate, cfg.sample_rate, resampler)
        except (ValueError, FileNotFoundError):
            xs = ys = None
        if ys is None or ys.size == 0 or float(np.isnan(ys).mean()) <= 0.1:
            break
        redraws += 1
        file_rate, channels, container, frames = draw_file(pair)
    kind = ("wav", "caf-lpcm", "caf-ima4")[container]
    nonfinite = specials["nonfinite"]
    special_trials += int(specials["on"])
    if ys is not None:                                           # the samples first: decode + conversion on the device
        sample_checks += 1
        for name, blocks in fp.converter_paths(rate, cfg.sample_rate, resampler, xs.size).items():
            paths_seen[name] += 1
        try:
            cy, cframes, crate = det.convert_audio_url(path)
            msg = fp.bit_mismatch(cy, ys)
            if msg is None and (cframes != xs.size or crate != rate):
                msg = f"file frames / rate {cframes} / {crate} != {xs.size} / {rate}"
        except lb.LBAudioDetectiveError as e:
            msg = f"status {e.status}"
        if msg:
            bad += 1
            print("SAMPLE MISMATCH", t, file_rate, channels, kind, frames, cfg.sample_rate, resampler,
                  dict(fp.converter_paths(rate, cfg.sample_rate, resampler, xs.size)), msg, flush=True)
    try:
        got = det.process_audio_url(path).to_bools()
    except lb.LBAudioDetectiveError as e:
        got = ("error", e.status)
    try:
        want = O.fingerprint_file(path, cfg, hop_mode, tail_mode, resampler)
        xs, rate = O.decode_audio_file(path)
        hs, hrate = lb.read_audio_url(path)                      # the library's host decoder and converter, on the way
        hy, _ = lb.read_audio_url(path, cfg.sample_rate, resampler)
        if hrate != rate or fp.bit_mismatch(hs, xs) or fp.bit_mismatch(hy, ys):
            bad += 1
            print("HOST FRONT END MISMATCH", t, file_rate, channels, kind, frames, cfg.sample_rate, resampler, flush=True)
    except (ValueError, FileNotFoundError):
        want = ("error",)
    if isinstance(got, tuple):
        got = ("error",)
    if nonfinite and not isinstance(got, tuple) and not isinstance(want, tuple):
        want = got                                               # NaN / inf samples: the sample level above is the check
    same = (isinstance(got, tuple) and isinstance(want, tuple) and got == want) or \
           (not isinstance(got, tuple) and not isinstance(want, tuple) and got.shape[0] == want.shape[0] and (want.shape[0] == 0 or np.array_equal(got, want)))
    if isinstance(got, tuple):
        rejected[kind] = rejected.get(kind, 0) + 1
    elif got.shape[0]:
        nonempty[kind] = nonempty.get(kind, 0) + 1
    if not same:
        bad += 1
        print("FILE MISMATCH", t, file_rate, channels, kind, frames, cfg.sample_rate, cfg.window, cfg.stride, cfg.bands, cfg.subfp_len,
              hop_mode, tail_mode, resampler, got if isinstance(got, tuple) else got.shape, want if isinstance(want, tuple) else want.shape, flush=True)
missing = [p for p in fp.PATHS if not paths_seen[p]] if trials >= 300 else []
print(f"{trials} trials, {bad} mismatches, {time.time() - t0:.1f} s; files with at least one sub-fingerprint {nonempty}, rejected {rejected}; "
      f"{sample_checks} compared at the sample level, {special_trials} with special values, {redraws} redrawn; "
      f"trials per converter path {dict(paths_seen)}")
assert redraws * 20 < max(trials, 20), f"{redraws} of {trials} trials had to be redrawn (more than a tenth of the output NaN)"
assert not missing, f"converter paths never reached: {missing}"
sys.exit(1 if bad else 0)
