"""Shared by tools/fuzz_files.py and, through tests/frontend_paths.py, by tests/test_frontend.py and
tests/test_gpu_frontend.py: which code path of the device converter (k_resample.hip) a conversion takes, the grid of
rate pairs that reaches every one of them, the bit-pattern comparison of sample arrays, and writers for the CAF / WAV
test files.  It lives beside the tool so that the tool needs nothing from tests/.

The branch model restates the kernel's predicates in numpy; the constants are read out of the sources, so that the
grid keeps meaning what it says when one of them changes (the tests assert the model's answer for every grid case
before the device runs).  It is a model of WHICH loop runs, never of a sample value: expected samples come from the
oracle alone."""
import collections
import math
import os
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lbaudiodetective_amd", "csrc")

PATHS = ("rational-staged", "rational-unstaged", "rational-q1", "tiled-staged", "tiled-unstaged-input",
         "tiled-ragged-taps", "plain", "copy", "linear")


def _constants():
    k = open(os.path.join(CSRC, "k_resample.hip")).read()
    a = open(os.path.join(CSRC, "audiofile.cpp")).read()

    def one(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]

    c = {name: int(one(k, r"constexpr int %s = (\d+);" % name)) for name in ("kThreads", "kRowLen", "kTapGroup", "kInMax", "kInMaxR")}
    c["kPeriods"] = int(one(k, r"#define LBAD_RS_PERIODS (\d+)"))
    c["grid_max"] = int(one(k, r"if \(bx > (\d+)\) bx = \1;"))
    c["q_max"] = int(one(a, r"if \(q > (\d+) \|\|"))
    c["p_max"] = 1 << int(one(a, r"\|\| p > \(1ull << (\d+)\)\) return nullptr;"))
    mib = one(a, r"\* \(double\)q \* 8\.0 > (\d+)\.0 \* 1024\.0 \* 1024\.0\) return nullptr;")
    c["table_bytes_max"] = int(mib) * 1024 * 1024
    c["res"] = int(one(a, r"const int res = (\d+);"))
    z = one(a, r"const int zero_crossings = mode == 0 \? (\d+) : (\d+);")
    c["zero_crossings"] = (int(z[0]), int(z[1]))
    return c


K = _constants()


def output_count(n_in, rate_in, rate_out):
    """resample_plan(): samples at the processing rate of a file of n_in frames."""
    if n_in == 0:
        return 0
    if rate_in == rate_out:
        return n_in
    return int(float(n_in) / (rate_in / rate_out))


def _geometry(rate_in, rate_out, mode):
    ratio = rate_in / rate_out
    scale = ratio if ratio > 1.0 else 1.0
    zc = K["zero_crossings"][mode]
    return ratio, scale, zc * scale, K["res"] / scale, zc * K["res"] + 2


def phase_table(rate_in, rate_out, mode):
    """audiofile.cpp: phase_table() without the weights -- (p, q, m_min, m_span), or None when the pair is not rational
    in audiofile.hpp's sense (then the position is the double product n * ratio)."""
    if rate_in != math.floor(rate_in) or rate_out != math.floor(rate_out) or rate_in > 4294967295.0 or rate_out > 4294967295.0:
        return None
    g = math.gcd(int(rate_in), int(rate_out))
    p, q = int(rate_in) // g, int(rate_out) // g
    _, _, half, coord, table_n = _geometry(rate_in, rate_out, mode)
    if q > K["q_max"] or p > K["p_max"] or (2.0 * half + 2.0) * q * 8.0 > K["table_bytes_max"]:
        return None
    frac = np.arange(q, dtype=np.float64) / float(q)
    c0, c1 = np.ceil(frac - half), np.floor(frac + half)
    m = c0[:, None] + np.arange(int((c1 - c0).max()) + 1, dtype=np.float64)[None, :]
    x = np.abs(m - frac[:, None]) * coord
    covered = (m <= c1[:, None]) & (x.astype(np.int64) + 1 < table_n)
    lo, hi = [], []
    for r in range(q):                                       # (covered taps are contiguous)
        idx = np.flatnonzero(covered[r])
        if idx.size:
            stop = idx[0] + int(np.argmin(np.append(covered[r, idx[0]:], False)))
            lo.append(int(m[r, idx[0]]))
            hi.append(int(m[r, stop - 1]))
    if not lo:
        return p, q, 0, 0
    return p, q, min(lo), max(hi) - min(lo) + 1


def converter_paths(rate_in, rate_out, mode, n_in):
    """Counter: path name -> blocks (double position, copy, linear) or slots (rational) of resample_batch_kernel that
    take it for one file; plus an "info" dict on the counter object (grid size, slots, periods of the last group)."""
    T = K["kThreads"]
    out = collections.Counter()
    out.info = {}
    n_out = output_count(n_in, rate_in, rate_out)
    out.info["n_out"] = n_out
    if n_out == 0:
        return out
    blocks = min(-(-n_out // T), K["grid_max"])
    out.info["blocks"] = blocks
    if rate_in == rate_out:
        out["copy"] = -(-n_out // T)
        return out
    if mode == 2:
        out["linear"] = -(-n_out // T)
        return out
    ratio, scale, half, coord, _ = _geometry(rate_in, rate_out, mode)
    ph = phase_table(rate_in, rate_out, mode)
    if ph is not None:
        P, Q, m_min, m_span = ph
        kp = K["kPeriods"]
        chunks, periods = -(-Q // T), -(-n_out // Q)
        groups = -(-periods // kp)
        out.info.update(q=Q, p=P, chunks=chunks, slots=chunks * groups, last_group_periods=periods - (groups - 1) * kp)
        c, g = np.meshgrid(np.arange(chunks, dtype=np.int64), np.arange(groups, dtype=np.int64))
        t0 = c * T
        lanes = np.minimum(Q - t0, T)
        all_staged = np.ones(c.shape, bool)
        for k in range(kp):
            nf = (g * kp + k) * Q + t0
            active = nf < n_out
            nl = np.minimum(nf + lanes - 1, n_out - 1)
            kbase = nf * P // Q + m_min
            kend = nl * P // Q + m_min + m_span - 1
            all_staged &= (kend - kbase + 1 <= K["kInMaxR"]) | ~active
        for name, slots in (("rational-staged", int(all_staged.sum())), ("rational-unstaged", int((~all_staged).sum())),
                            ("rational-q1", chunks * groups if Q == 1 else 0)):
            if slots:
                out[name] = slots
        return out
    n = np.arange(n_out, dtype=np.float64)
    pos = n * ratio
    k0, k1 = np.ceil(pos - half), np.floor(pos + half)
    fr = np.clip(k0 - (pos - half), 0.0, 1.0)
    fq = (fr * 1073741824.0).astype(np.uint64)
    taps = k1 - k0 + 1
    for b in range(0, n_out, T):
        s = slice(b, min(b + T, n_out))
        fmin, fmax = float(fq[s].min()) / 1073741824.0, float(fq[s].max() + 1) / 1073741824.0
        if (fmax - fmin) * coord + 6.0 <= float(K["kRowLen"]):
            staged = k1[s].max() - k0[s].min() + 1 <= K["kInMax"]
            out["tiled-staged" if staged else "tiled-unstaged-input"] += 1
            if taps[s].min() != taps[s].max():
                out["tiled-ragged-taps"] += 1
        else:
            out["plain"] += 1
    return out


def is_double_position(rate_in, rate_out, mode):
    return rate_in != rate_out and mode != 2 and phase_table(rate_in, rate_out, mode) is None


# ---- the converter grid: (file rate, processing rate, {mode: paths the case is there for}) -------------------------------
# The third element names what the branch model must find for that mode (a subset of what it does find; "only" rows
# list everything).  Mode 2 (linear) is run for the three rows marked with it.
_TS, _TU, _TR, _PL = "tiled-staged", "tiled-unstaged-input", "tiled-ragged-taps", "plain"
_RS, _RU, _RQ = "rational-staged", "rational-unstaged", "rational-q1"
GRID = [
    # double position, every block tiled and staged, tap counts equal across a block
    (44100.0, 5512.5, {0: {_TS}, 1: {_TS}, 2: {"linear"}}, "only"),
    (11025.0, 5512.5, {0: {_TS}, 1: {_TS}}, "only"),
    # tiled and staged, tap counts differ inside a block (general_tap on the last rows); interpolating
    (44100.0, 44100.5, {0: {_TS, _TR}, 1: {_TS, _TR}}, "only"),
    (5512.0, 5512.5, {0: {_TS, _TR}, 1: {_TS, _TR}}, "only"),
    # tiled blocks whose input span exceeds the staged range, next to plain ones
    (96000.0, 8000.5, {0: {_TU, _PL}, 1: {_TU, _PL}}, "subset"),
    # tiled and plain blocks in one file
    (44100.0, 5512.25, {0: {_TS, _PL}, 1: {_TS, _PL}}, "subset"),
    (44100.0, 22051.0, {0: {_TS, _PL}, 1: {_TS, _PL}}, "subset"),
    (44100.0, 11025.5, {0: {_TS, _PL}, 1: {_TS, _PL}}, "subset"),
    # plain sinc_sample in every block
    (44100.0, 5000.5, {0: {_PL}, 1: {_PL}}, "only"),
    (22254.54545, 5512.0, {0: {_PL}, 1: {_PL}}, "only"),
    (8000.0, 16000.5, {0: {_PL}, 1: {_PL}}, "only"),
    (96000.0, 5512.5, {0: {_PL}, 1: {_PL}}, "only"),
    (192000.0, 5512.5, {0: {_PL}, 1: {_PL}}, "only"),
    # rational, several chunks per period, every range staged
    (44100.0, 5512.0, {0: {_RS}, 1: {_RS}, 2: {"linear"}}, "only"),
    (22050.0, 5512.0, {0: {_RS}, 1: {_RS}}, "only"),
    (32000.0, 5512.0, {0: {_RS}, 1: {_RS}}, "only"),
    # rational, interpolating, fewer lanes than a block
    (44100.0, 48000.0, {0: {_RS}, 1: {_RS}, 2: {"linear"}}, "only"),
    (8000.0, 44100.0, {0: {_RS}, 1: {_RS}}, "only"),
    (4000.0, 44100.0, {0: {_RS}, 1: {_RS}}, "only"),
    # rational with q = 1: one lane per slot, more slots than blocks
    (48000.0, 8000.0, {0: {_RS, _RQ}, 1: {_RS, _RQ}}, "only"),
    (44100.0, 11025.0, {0: {_RS, _RQ}, 1: {_RS, _RQ}}, "only"),
    # rational with ranges too long to stage (the per-tap global loop)
    (96000.0, 5512.0, {0: {_RU}, 1: {_RU}}, "subset"),
    (88200.0, 5512.0, {0: {_RU}, 1: {_RU}}, "subset"),
    (192000.0, 5512.0, {0: {_RU}, 1: {_RU}}, "subset"),
    (64000.0, 5512.0, {0: {_RU, _RS}, 1: {_RU, _RS}}, "subset"),
    # still rational although q is large (q = 3277)
    (48000.0, 16385.0, {0: {_RS}, 1: {_RS}}, "only"),
    # equal rates
    (44100.0, 44100.0, {0: {"copy"}, 1: {"copy"}, 2: {"copy"}}, "only"),
]


def grid_frames(rate_in, rate_out, want_out=5000):
    """Input frames that give `several thousand` outputs with n_out % 256 neither 0 nor 1."""
    n_in = int(math.ceil(want_out * rate_in / rate_out)) + 3
    while output_count(n_in, rate_in, rate_out) % K["kThreads"] in (0, 1):
        n_in += 1
    return n_in


def frames_for_outputs(n_out, rate_in, rate_out):
    """The smallest input length whose conversion has n_out samples (when interpolating not every count exists: then
    the next one above)."""
    n_in = max(int(n_out * rate_in / rate_out) - 2, 1)
    while output_count(n_in, rate_in, rate_out) < n_out:
        n_in += 1
    return n_in


def edge_frames(rate_in, rate_out, mode):
    """The edge lengths of one rate pair: 0, 1, 2 frames, just under / over one kernel half-width, exactly 1 / 256 / 257
    outputs and, on the rational path, lengths whose last period group has one and two of its periods active."""
    ratio, scale, half, _, _ = _geometry(rate_in, rate_out, mode)
    out = [0, 1, 2, max(int(half) - 1, 1), int(half) + 2]
    out += [frames_for_outputs(k, rate_in, rate_out) for k in (1, K["kThreads"], K["kThreads"] + 1)]
    ph = phase_table(rate_in, rate_out, mode)
    if ph is not None:
        q, kp = ph[1], K["kPeriods"]
        for active in range(1, kp):                          # (groups of kPeriods periods of q outputs)
            out.append(frames_for_outputs((kp + active - 1) * q + max(q // 3, 1), rate_in, rate_out))
    return sorted(set(out))


EDGE_PAIRS = [(44100.0, 5512.5), (44100.0, 44100.5), (96000.0, 8000.5), (44100.0, 5000.5), (8000.0, 16000.5),
              (44100.0, 5512.0), (44100.0, 48000.0), (48000.0, 8000.0), (64000.0, 5512.0), (44100.0, 44100.0)]


# ---- comparison ----------------------------------------------------------------------------------------------
def bit_mismatch(got, want):
    """None when the two float32 arrays hold the same bit patterns (a NaN of the expectation matches any NaN), else a
    message with the first differing index, the count and both values in hex."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return f"length {got.shape} != expected {want.shape}"
    g, w = got.view(np.uint32), want.view(np.uint32)
    nan_w = np.isnan(want)
    diff = np.where(nan_w, ~np.isnan(got), g != w)
    if not diff.any():
        return None
    i = int(np.flatnonzero(diff)[0])
    return (f"{int(diff.sum())} of {got.size} samples differ, first at {i}: got 0x{int(g[i]):08x} ({got[i]!r}), "
            f"expected 0x{int(w[i]):08x} ({want[i]!r})")


def assert_same_bits(got, want, what=""):
    msg = bit_mismatch(got, want)
    assert msg is None, f"{what}: {msg}"


def signal(n, seed, channels=1):
    """Noise of about +-0.3 with a sine on top (neighbouring taps do not cancel to zero): float64 [n, channels]."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.3, 0.3, (n, channels)) + 0.25 * np.sin(np.arange(n)[:, None] * 0.013 + np.arange(channels)[None, :])
    return x


# ---- file writers --------------------------------------------------------------------------------------------
def caf_bytes(rate, fourcc, flags, bytes_per_packet, frames_per_packet, channels, bits, payload, pakt=None, pad=None):
    """pakt: (packets, valid frames, priming frames); pad: length of a `free` chunk in front of the data chunk."""
    desc = struct.pack(">d4sIIIII", float(rate), fourcc, flags, bytes_per_packet, frames_per_packet, channels, bits)
    out = b"caff" + struct.pack(">HH", 1, 0) + b"desc" + struct.pack(">q", len(desc)) + desc
    if pakt is not None:
        body = struct.pack(">qqii", pakt[0], pakt[1], pakt[2], 0)
        out += b"pakt" + struct.pack(">q", len(body)) + body
    if pad is not None:
        out += b"free" + struct.pack(">q", pad) + bytes(pad)
    return out + b"data" + struct.pack(">q", 4 + len(payload)) + bytes(4) + payload


def caf_lpcm(path, rate, raw, kind, little):
    """raw: [frames, channels] array already of the sample type (integers: int64 values of the stated width; floats:
    float32 / float64); kind: i8 / i16 / i24 / i32 / f32 / f64."""
    open(path, "wb").write(caf_lpcm_bytes(rate, raw, kind, little))


def caf_lpcm_bytes(rate, raw, kind, little, pad=None):
    raw = np.asarray(raw)
    if raw.ndim == 1:
        raw = raw[:, None]
    frames, channels = raw.shape
    bits = int(kind[1:])
    e = "<" if little else ">"
    if kind[0] == "f":
        data = np.ascontiguousarray(raw.astype(f"{e}f{bits // 8}", copy=False)).tobytes()
    else:
        b = np.ascontiguousarray(raw.astype("<i8")).view(np.uint8).reshape(frames, channels, 8)[:, :, : bits // 8]
        data = (b if little else b[:, :, ::-1]).tobytes()
    return caf_bytes(rate, b"lpcm", (1 if kind[0] == "f" else 0) | (2 if little else 0), channels * bits // 8, 1, channels, bits,
                     data, pad=pad)


def wav_bytes(rate, raw, kind):
    """kind: u8 / i16 / i24 / i32 / f32; raw as for caf_lpcm (u8: values 0..255)."""
    raw = np.asarray(raw)
    if raw.ndim == 1:
        raw = raw[:, None]
    frames, channels = raw.shape
    bits = int(kind[1:])
    if kind == "f32":
        data, tag = np.ascontiguousarray(raw.astype("<f4", copy=False)).tobytes(), 3
    else:
        data, tag = np.ascontiguousarray(raw.astype("<i8")).view(np.uint8).reshape(frames, channels, 8)[:, :, : bits // 8].tobytes(), 1
    block = channels * bits // 8
    hdr = b"WAVEfmt " + struct.pack("<IHHIIHH", 16, tag, channels, int(rate), int(rate) * block, block, bits)
    return b"RIFF" + struct.pack("<I", 4 + len(hdr) + 8 + len(data)) + hdr + b"data" + struct.pack("<I", len(data)) + data


def write_f32_caf(path, rate, x):
    open(path, "wb").write(caf_lpcm_bytes(rate, np.asarray(x, np.float32), "f32", False))
