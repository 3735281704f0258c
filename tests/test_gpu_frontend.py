"""The device decoder (k_decode.hip) and converter (k_resample.hip) against the independent file oracle
(oracle/lbad_file_oracle.c), sample by sample, on every code path.

Expected samples come from the oracle alone (decode_audio_file + resample); got is Detective.convert_audio_url.  The
comparison is on bit patterns (frontend_paths.bit_mismatch): -0.0 differs from +0.0, a NaN of the oracle must be a NaN
of the device, everything else must be the same 32 bits; no tolerance, every output sample of every case.  Which path
of the converter a case takes is said by the branch model of tests/frontend_paths.py, which every grid case asserts
before the device runs (the model's own tests are in tests/test_frontend.py and need no GPU)."""
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

import frontend_paths as fp

pytestmark = pytest.mark.gpu

BIRDS = os.path.join(os.path.dirname(__file__), "golden", "birds")
_DETS = {}


def _detective(lb, rate_out, mode):
    if rate_out not in _DETS:
        _DETS[rate_out] = lb.Detective().configure(sample_rate=rate_out)
    return _DETS[rate_out].set_resampler_mode(mode)


def _check(lb, oracle, path, rate_out, mode, what, nan_share=0.0):
    """One file through the device front end against the oracle; returns the expected samples."""
    x, rate = oracle.decode_audio_file(path)
    want = oracle.resample(x, rate, rate_out, mode)
    if want.size:
        share = float(np.isnan(want).mean())
        assert share <= nan_share, f"{what}: {share:.3f} of the oracle's samples are NaN, the case compares too little"
    got, file_frames, file_rate = _detective(lb, rate_out, mode).convert_audio_url(path)
    assert file_frames == x.size and file_rate == rate, (what, file_frames, x.size, file_rate, rate)
    fp.assert_same_bits(got, want, what)
    return want


# ---- the converter grid ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", range(len(fp.GRID)), ids=[f"{a:g}-{b:g}" for a, b, _, _ in fp.GRID])
def test_converter_grid(lb, gpu, oracle, tmp_path, row):
    """Every row of the table in DESIGN.md section 2 (rational: staged / unstaged / q = 1; double position: tiled and
    staged, tiled with the input unstaged, ragged tap counts, plain; copy; linear), modes 0 and 1 (2 where the row says
    so), float32 CAF files (the desc chunk's rate is a double: fractional file rates), several thousand outputs with
    n_out % 256 neither 0 nor 1; the first and last `half` outputs (taps left and right of the file) are compared like
    all others.  Rows of EDGE_PAIRS also run the edge lengths: 0, 1, 2 frames, just under / over one kernel half-width,
    exactly 1 / 256 / 257 outputs, a last period group with one and with two of its periods active."""
    rate_in, rate_out, want, kind = fp.GRID[row]
    path = str(tmp_path / "x.caf")
    n_in = fp.grid_frames(rate_in, rate_out)
    for mode, paths in want.items():
        got = fp.converter_paths(rate_in, rate_out, mode, n_in)
        assert (set(got) == paths) if kind == "only" else (paths <= set(got)), (rate_in, rate_out, mode, dict(got))
    fp.write_f32_caf(path, rate_in, fp.signal(n_in, 1000 + row)[:, 0])
    for mode in want:
        _check(lb, oracle, path, rate_out, mode, f"{rate_in} -> {rate_out} mode {mode} frames {n_in}")
    if (rate_in, rate_out) in fp.EDGE_PAIRS:
        for mode in (0, 1):
            for n_edge in fp.edge_frames(rate_in, rate_out, mode):
                fp.write_f32_caf(path, rate_in, fp.signal(n_edge, 2000 + row)[:, 0])
                _check(lb, oracle, path, rate_out, mode, f"{rate_in} -> {rate_out} mode {mode} frames {n_edge} (edge)")


# ---- special values ---------------------------------------------------------------------------------------------
def _special_signal(kind):
    """60 000 frames with, far apart: a NaN burst, one +inf, one -inf, runs of -0.0, denormals, FLT_MAX; float64 files
    also hold values that overflow float32 (1e39), underflow it (1e-46) and sit on a rounding tie."""
    x = fp.signal(60000, 77)[:, 0].astype(np.float32).astype(np.float64 if kind == "f64" else np.float32)
    x[9000:9008] = np.nan
    x[21000] = np.inf
    x[33000] = -np.inf
    x[12000:12600] = -0.0                                   # longer than the long kernel at 44.1 kHz -> 5512 Hz (385 taps)
    x[15000:15003] = -0.0
    x[40000:40400] = np.float32(1e-41) * np.where(np.arange(400) % 3 == 0, -1, 1)      # float32 denormals
    x[45000] = np.finfo(np.float32).max
    x[47000] = -np.finfo(np.float32).max
    if kind == "f64":
        x[50000] = 1e39                                     # +inf as float32
        x[52000:52300] = 1e-46 * np.where(np.arange(300) % 2 == 0, -1, 1)              # +-0.0 as float32
        x[54000] = 1.0 + 2.0 ** -24                         # tie: to even, 1.0
        x[54001] = 1.0 + 3.0 * 2.0 ** -24                   # tie: to even, 1 + 2^-22
        x[54002] = -(1.0 + 2.0 ** -24 + 2.0 ** -50)         # just past the tie
        x[54003] = np.float64(np.finfo(np.float32).max) * (1.0 + 2.0 ** -25)           # rounds to FLT_MAX, not to inf
    return x


@pytest.mark.parametrize("kind,little", [("f32", False), ("f32", True), ("f64", False), ("f64", True)])
def test_special_values_through_decoder_and_converter(lb, gpu, oracle, tmp_path, kind, little):
    """Non-finite samples, negative zeros, denormals and the float64 -> float32 narrowing cases, through one rational
    pair, one double-position pair (sinc_sample's `an uncovered tap must not meet an inf / NaN sample`) and the copy path,
    the three models.  At most a tenth of the oracle's output may be NaN (asserted), so the comparison keeps its
    meaning.  The copy path returns the decoded bits unchanged, -0.0 and the NaN positions included; for float32 files
    that is the file's own bit patterns, NaN payloads included."""
    x = _special_signal(kind)
    path = str(tmp_path / "s.caf")
    open(path, "wb").write(fp.caf_lpcm_bytes(44100.0, x, kind, little))
    for rate_out in (5512.0, 5512.5, 48000.0, 44100.5):
        for mode in (0, 1, 2):
            want = _check(lb, oracle, path, rate_out, mode, f"{kind} special values -> {rate_out} mode {mode}", nan_share=0.1)
            assert np.isnan(want).any() and np.isfinite(want).mean() > 0.8
    want = _check(lb, oracle, path, 44100.0, 0, f"{kind} special values, copy", nan_share=0.1)
    assert np.isnan(want).sum() == 8 and np.signbit(want[12000:12600]).all() and not want[12000:12600].any()
    if kind == "f32":
        x = x.copy()
        x.view(np.uint32)[9000:9008] = [0x7FC00000, 0xFFC00000, 0x7FC01234, 0xFFFFFFFF, 0x7FE00001, 0x7FC00001, 0xFFC12345, 0x7FFFFFFF]
        open(path, "wb").write(fp.caf_lpcm_bytes(44100.0, x, kind, little))
        got, _, _ = _detective(lb, 44100.0, 0).convert_audio_url(path)
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32)), "copy path changed the bits of a float32 file"


# ---- the decoder grid -------------------------------------------------------------------------------------------
_CAF_FORMS = [("i8", False)] + [(k, e) for k in ("i16", "i24", "i32", "f32", "f64") for e in (True, False)]
_WAV_FORMS = ["u8", "i16", "i24", "i32", "f32"]


def _raw(kind, frames, channels, seed):
    """Random samples of the form with its extremes in front: INT_MIN, INT_MAX, -1, 0, 1; for int32 values whose quotient
    by 2^31 rounds when it is narrowed to float32."""
    rng = np.random.default_rng(seed)
    if kind[0] == "f":
        x = rng.standard_normal((frames, channels)) * 0.3
        special = [-0.0, 0.0, 1.0, -1.0, 1e-40, 0.1, 1.0 + 2.0 ** -24 if kind == "f64" else 1.0 + 2.0 ** -23, 3.5]
        x = x.astype(np.float32 if kind == "f32" else np.float64)
    elif kind == "u8":
        x = rng.integers(0, 256, (frames, channels), dtype=np.int64)
        special = [0, 255, 128, 127, 129]
    else:
        bits = int(kind[1:])
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        x = rng.integers(lo, hi + 1, (frames, channels), dtype=np.int64)
        special = [lo, hi, -1, 0, 1, lo + 1, hi - 1]
        if bits == 32:
            special += [(1 << 24) + 1, -(1 << 24) - 1, (1 << 25) + 3, 0x7FFFFF80, 0x7FFFFFBF, 0x7FFFFFC0, -0x7FFFFFC1, 0x12345679]
    flat = x.reshape(-1)
    k = min(flat.size, len(special))
    flat[:k] = special[:k]
    if flat.size >= 3 * len(special):                         # and once more at the end (last frames of the last block)
        flat[-len(special):] = special
    return x


def _form_bytes(container, kind, little, rate, frames, channels, seed, pad=None):
    raw = _raw(kind, frames, channels, seed)
    if container == "wav":
        return fp.wav_bytes(rate, raw, kind)
    return fp.caf_lpcm_bytes(rate, raw, kind, little, pad=pad)


def _all_forms():
    return [("caf", k, e) for k, e in _CAF_FORMS] + [("wav", k, True) for k in _WAV_FORMS]


@pytest.mark.parametrize("container,kind,little", _all_forms(), ids=[f"{c}-{k}-{'le' if e else 'be'}" for c, k, e in _all_forms()])
def test_decoder_grid_at_equal_rates(lb, gpu, oracle, tmp_path, container, kind, little):
    """Every PCM form of k_decode.hip against the oracle's decode, bit for bit, at equal rates (decode_batch_kernel and the
    copy loop only): 1, 2, 3 and 6 channels; 1, 255, 256, 257 and 3001 frames; the extremes of each width next to
    random samples; the multi-byte CAF forms once more behind a `free` chunk of odd length (payload at an odd file
    offset); then decode and conversion chained, at a double-position and a rational pair."""
    path = str(tmp_path / ("x." + container))
    seed = 0
    for channels in (1, 2, 3, 6):
        for frames in (1, 255, 256, 257, 3001):
            seed += 1
            open(path, "wb").write(_form_bytes(container, kind, little, 22050, frames, channels, seed))
            want = _check(lb, oracle, path, 22050.0, 0, f"{container} {kind} le={little} ch={channels} frames={frames}")
            assert want.size == frames
    if container == "caf" and kind != "i8":
        for pad in (7, 1):
            open(path, "wb").write(_form_bytes(container, kind, little, 22050, 3001, 2, 99, pad=pad))
            assert _check(lb, oracle, path, 22050.0, 0, f"{kind} le={little} behind a free chunk of {pad} bytes").size == 3001
    for channels in (1, 2):
        open(path, "wb").write(_form_bytes(container, kind, little, 44100, 30011, channels, 200 + channels))
        for rate_out, mode in ((5512.5, 0), (5512.0, 0), (5512.5, 1), (48000.0, 2)):
            _check(lb, oracle, path, rate_out, mode, f"{container} {kind} le={little} ch={channels} -> {rate_out} mode {mode}")


def _ima_packets():
    bird = open(os.path.join(BIRDS, "Wren.caf"), "rb").read()
    at = bird.index(b"data") + 16
    return np.frombuffer(bird[at:at + 34 * ((len(bird) - at) // 34)], np.uint8).reshape(-1, 34)


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_ima4_decoder_grid(lb, gpu, oracle, tmp_path, channels):
    """IMA4 with 1, 2 and 3 channels, without a packet table and with one (priming 0 / 7 / 64, valid frames cut short), at
    even and odd payload offsets, at equal rates and chained with a conversion."""
    packets = _ima_packets()
    path = str(tmp_path / "i.caf")
    for n_packets in (1, 4, 300):
        payload = packets[37:37 + n_packets * channels].tobytes()
        tables = [None] + [(n_packets, valid, priming) for priming in (0, 7, 64)
                           for valid in sorted({max(n_packets * 64 - priming - 13, 0), max(n_packets * 64 - priming, 0), 1})]
        for pakt in tables:
            for pad in (None, 3):
                open(path, "wb").write(fp.caf_bytes(44100.0, b"ima4", 0, 34 * channels, 64, channels, 0, payload, pakt=pakt, pad=pad))
                what = f"ima4 ch={channels} packets={n_packets} pakt={pakt} pad={pad}"
                want = _check(lb, oracle, path, 44100.0, 0, what)
                if pakt is None:
                    assert want.size == n_packets * 64
                else:
                    assert want.size == min(pakt[1], n_packets * 64 - min(pakt[2], n_packets * 64)), what
                if n_packets == 300:
                    _check(lb, oracle, path, 5512.5, 0, what + " -> 5512.5")
                    _check(lb, oracle, path, 5512.0, 1, what + " -> 5512")


# ---- grid-stride loops ------------------------------------------------------------------------------------------
def test_decode_and_copy_loops_stride_on_a_17_million_frame_file(lb, gpu, oracle, tmp_path):
    """decode_batch_kernel caps its grid at 4096 blocks and resample_batch_kernel at 65535: an int8 CAF file of 17 000 000
    frames has more than 4096 x 256 decode units and more than 65535 x 256 copy outputs, compared in full."""
    n = 17_000_000
    assert n > 4096 * 256 and n > fp.K["grid_max"] * fp.K["kThreads"]
    rng = np.random.default_rng(5)
    raw = rng.integers(-128, 128, n, dtype=np.int8)
    raw[:4] = [-128, 127, -1, 0]
    raw[-4:] = [1, -128, 127, -1]
    path = str(tmp_path / "big.caf")
    open(path, "wb").write(fp.caf_bytes(8000.0, b"lpcm", 0, 1, 1, 1, 8, raw.tobytes()))
    want = _check(lb, oracle, path, 8000.0, 0, "17 000 000 int8 frames at equal rates")
    assert want.size == n and np.array_equal(want[:2], np.float32([-1.0, 127 / 128]))


def test_ima4_decode_loop_strides_above_a_million_packets(lb, gpu, oracle, tmp_path):
    """More than 4096 x 256 = 1 048 576 IMA4 packets (a fixture's packets repeated, 36 MB): every decoded frame."""
    packets = _ima_packets()
    n_packets = 4096 * 256 + 2500
    reps = -(-n_packets // packets.shape[0])
    payload = np.tile(packets, (reps, 1))[:n_packets].tobytes()
    path = str(tmp_path / "big_ima.caf")
    open(path, "wb").write(fp.caf_bytes(44100.0, b"ima4", 0, 34, 64, 1, 0, payload, pakt=(n_packets, n_packets * 64 - 100, 7)))
    want = _check(lb, oracle, path, 44100.0, 0, "1 051 076 IMA4 packets at equal rates")
    assert want.size == n_packets * 64 - 100


def test_double_position_loop_strides_above_65535_blocks(lb, gpu, oracle, tmp_path):
    """8000 -> 16000.5 Hz, short kernel, 16 777 260 outputs: more than 65535 x 256, so the double-position loop of
    resample_batch_kernel strides (plain sinc_sample in every block, by the branch model).  The oracle converts this
    in 0.6 s on eight cores (measured; nine taps per output), so the case is affordable and compared in full."""
    rate_in, rate_out = 8000.0, 16000.5
    n_in = fp.frames_for_outputs(fp.K["grid_max"] * fp.K["kThreads"] + 300, rate_in, rate_out)
    assert fp.output_count(n_in, rate_in, rate_out) > fp.K["grid_max"] * fp.K["kThreads"] and fp.is_double_position(rate_in, rate_out, 1)
    path = str(tmp_path / "long.caf")
    fp.write_f32_caf(path, rate_in, fp.signal(n_in, 8)[:, 0])
    t0 = time.time()
    _check(lb, oracle, path, rate_out, 1, "16.8 million double-position outputs")
    print(f"16.8 million outputs: oracle + device + comparison {time.time() - t0:.1f} s")


# ---- several files in one launch --------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_out", [5512.5, 5512.0])
def test_mixed_paths_in_one_batch_launch(lb, gpu, oracle, tmp_path, rate_out):
    """process_audio_urls on one list that mixes a copy file, rational-staged / rational-unstaged files (at 5512 Hz),
    tiled and plain files, a zero-length file and an IMA4 fixture: one descriptor each, ONE resample_batch_kernel launch
    for all, so this is the per-file dispatch inside a launch.  The batch call returns fingerprints only, so the level
    is oracle.fingerprint_file (the samples are covered above): hop modes 0 / 1, the three tail modes, models 0 / 1."""
    files = [(5512.5, 4.0), (5512.0, 4.0), (44100.0, 4.0), (96000.0, 3.0), (22254.54545, 4.0), (11025.0, 5.0), (44100.0, 0.0),
             (64000.0, 3.0), (44100.5, 3.0)]
    paths, union = [], set()
    for k, (rate_in, seconds) in enumerate(files):
        n_in = int(rate_in * seconds)
        p = str(tmp_path / f"m{k}.caf")
        fp.write_f32_caf(p, rate_in, fp.signal(n_in, 300 + k)[:, 0])
        paths.append(p)
        for mode in (0, 1):
            union |= set(fp.converter_paths(rate_in, rate_out, mode, n_in))
    paths.append(os.path.join(BIRDS, "Crow.caf"))
    if rate_out == 5512.5:
        assert {"copy", "tiled-staged", "tiled-ragged-taps", "plain"} <= union
    else:
        assert {"copy", "rational-staged", "rational-unstaged", "plain", "tiled-staged"} <= union
    det = lb.Detective().configure(sample_rate=rate_out)
    cfg = oracle.Config(sample_rate=rate_out)
    n_sub = 0
    for hop_mode in (0, 1):
        for tail_mode in (0, 1, 2):
            for res in (0, 1):
                det.set_file_hop_mode(hop_mode).set_file_tail_mode(tail_mode).set_resampler_mode(res)
                fps, sts = det.process_audio_urls(paths, statuses=True)
                for p, f, st in zip(paths, fps, sts):
                    try:
                        want = oracle.fingerprint_file(p, cfg, hop_mode, tail_mode, res)
                    except ValueError:
                        assert st != 0 and f is None, (p, st)
                        continue
                    assert st == 0, (p, st)
                    got = f.to_bools()
                    assert got.shape[0] == want.shape[0] and (want.shape[0] == 0 or np.array_equal(got.reshape(want.shape), want)), \
                        (p, rate_out, hop_mode, tail_mode, res)
                    n_sub += want.shape[0]
    assert n_sub > 12 * 8                                   # the files are long enough to have fingerprints at all


# ---- the forced variants ----------------------------------------------------------------------------------------
def _double_position_cases():
    return [(ri, ro, mode) for ri, ro, want, _ in fp.GRID for mode in (0, 1) if fp.is_double_position(ri, ro, mode)]


def run_double_position_rows(tmp):
    """Child process of the test below (python tests/test_gpu_frontend.py <dir>): the double-position rows of the grid
    through whichever library LBAD_LIB names; one line per case, exit status 1 on the first mismatch."""
    import lbaudiodetective_amd as lb
    from oracle import oracle as O
    path = os.path.join(tmp, "v.caf")
    for rate_in, rate_out, mode in _double_position_cases():
        n_in = fp.grid_frames(rate_in, rate_out)
        x = fp.signal(n_in, 4000)[:, 0].astype(np.float32)
        fp.write_f32_caf(path, rate_in, x)
        got, frames, _ = lb.Detective().configure(sample_rate=rate_out).set_resampler_mode(mode).convert_audio_url(path)
        msg = fp.bit_mismatch(got, O.resample(x, rate_in, rate_out, mode))
        print(f"{rate_in:g} -> {rate_out:g} mode {mode} frames {n_in}: {msg or 'equal'}", flush=True)
        if msg or frames != n_in:
            return 1
    return 0


@pytest.mark.parametrize("switch", ["LBAD_EXP_FORCE_TILED", "LBAD_EXP_FORCE_PLAIN"])
def test_forced_variants_of_the_double_position_path(lb, gpu, oracle, tmp_path, switch):
    """k_resample.hip's two compile-time switches.  Forced tiling on pairs whose phases are spread wide (44100 -> 5000.5)
    is the only way to make lanes leave the staged table rows: general_tap's direct table read and the `worst >=
    kRowLen - 1` re-computation.  (Both are bounds-safe as written: the row index is clamped before the LDS read, the
    table index is guarded by `ok`, a lane past the end repeats the block's last active output.)  The file is compiled
    alone with the switch by the Makefile's own rule (FLAGS_k_resample, objects under tmp_path), linked with the objects
    of the regular build, and the double-position rows of the grid run in a fresh child process with LBAD_LIB pointing at
    the variant; the regular outputs are untouched."""
    csrc = os.path.join(fp.ROOT, "lbaudiodetective_amd", "csrc")
    obj_dir = os.path.join(fp.ROOT, "lbaudiodetective_amd", "lib", "obj")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    names = [os.path.splitext(f)[0] for f in os.listdir(csrc) if f.endswith((".hip", ".cpp"))]
    if not all(os.path.exists(os.path.join(obj_dir, n + ".o")) for n in names):
        # the library came without its objects: make them once, beside the variant (the Makefile's rules, another OUT)
        regular = tmp_path / "regular"
        subprocess.run(["make", "-C", csrc, "--no-print-directory", "-j16", f"OUT={regular}"], check=True, capture_output=True, timeout=900)
        obj_dir = str(regular / "obj")
    out = tmp_path / "variant"
    subprocess.run(["make", "-C", csrc, "--no-print-directory", f"OUT={out}", f"FLAGS_k_resample=-D{switch}", f"{out}/obj/k_resample.o"],
                   check=True, capture_output=True, timeout=600)
    objs = [os.path.join(obj_dir, n + ".o") for n in sorted(names) if n != "k_resample"] + [str(out / "obj" / "k_resample.o")]
    variant = str(tmp_path / "liblbaudiodetective_variant.so")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", variant, *objs, "-ldl"], check=True,
                   capture_output=True, timeout=600)
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path)], capture_output=True, text=True, timeout=300,
                         cwd=fp.ROOT, env={**os.environ, "LBAD_LIB": variant, "PYTHONPATH": fp.ROOT})
    lines = [l for l in run.stdout.splitlines() if " -> " in l]
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert len(lines) == len(_double_position_cases()) == 26 and all(l.endswith(": equal") for l in lines), run.stdout[-2000:]


if __name__ == "__main__":
    sys.exit(run_double_position_rows(sys.argv[1]))
