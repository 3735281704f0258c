#!/usr/bin/env python3
"""One push of a resampler bank against the things it stands beside, alternating in one process after warm-up:
    python3 tools/prof_resampler_bank.py [reps] [--out DIR] [--channels N] [--rate-in HZ] [--rate-out HZ] [--no-host]
1 024 channels at 44.1 kHz -> 5512 Hz (mode 0: 386 taps), every channel 3 140 samples into its signal, receive one second of new
samples each: 5 512 or 5 513 outputs per channel, four periods of the 1 378 phases.  --rate-in / --rate-out: another pair (the
stream bank then runs at that output rate; the result goes to resampler_bank_IN_OUT.json) -- 48000 -> 8000 has q = 1, where a
workgroup takes consecutive outputs and not positions inside a period.  LBAD_LIB=<a library built with
EXTRA_CXXFLAGS=-DLBAD_RSBANK_CONSECUTIVE> measures that first form of the kernel on every pair.  Legs:
    rs_f32     ResamplerBank.push_device on float32 samples (convert, commit)
    rs_i16     the same on int16 samples
    chain_f32  ResamplerBank.push_device followed by StreamBank.push_device on what it emitted (5512 Hz / 2048 / 64, every channel
    chain_i16  carrying 6 000 samples: one frame a channel), on one stream -- the whole live path
    sb         StreamBank.push_device alone on the same converted samples already in HBM: chain minus sb is what conversion adds
    host       what a user has today: the library's host converter through read_audio_url on temporary float32 WAVs of the same
               samples, 32 channels (one file after the other; the converter itself runs on up to 16 threads); host_scaled_ms is
               that time x channels / 32 -- SCALED, not measured
Every round restores the state first, outside the clock: all banks are reset and primed.  Times: a host clock around the calls and
the synchronise that ends them (all legs), and device events (all but host).  Medians and quartiles of `reps` rounds (default 7, at
least 5) in ms.  After the clock stops the float32 leg's output must equal the host converter's samples of channels 0 and 31 bit
for bit, the int16 leg's the float32 leg's (the signals are multiples of 1 / 32768), and both chains' sub-fingerprints sb's.  One
JSON object, printed and written to DIR/resampler_bank.json (default DIR: profiles).  No bar: nothing here decides acceptance.
    timeout -k 10 600 python3 tools/prof_resampler_bank.py 7
The kernel times of DESIGN.md 4.4p come from a run of its own under the tracer:
    rocprofv3 --kernel-trace --stats -d DIR -o rsb --output-format csv -- python3 tools/prof_resampler_bank.py 5 --no-host --out DIR"""
import json
import os
import statistics
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lbaudiodetective_amd as lb  # noqa: E402

SEED = 0x4C424152
WINDOW, STRIDE = 2048, 64
PRIME, SB_PRIME, HOST_CHANNELS = 3140, 6000, 32


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
CHANNELS = int(_option("--channels", 1024))
RATE_IN, RATE = int(_option("--rate-in", 44100)), int(_option("--rate-out", 5512))
NEW = RATE_IN                                                                         # one second
HOST = "--no-host" not in sys.argv
_values = {sys.argv.index(o) + 1 for o in ("--out", "--channels", "--rate-in", "--rate-out") if o in sys.argv}          # (positions of the options' values)
args = [a for i, a in enumerate(sys.argv) if i and not a.startswith("--") and i not in _values]
REPS = max(5, int(args[0]) if args else 7)


def _stats(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    return {"median": round(q[1], 4), "p25": round(q[0], 4), "p75": round(q[2], 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn, device=True):
    """(host ms up to the end of the device's work, device ms between events around the calls)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b) if device else 0.0


def write_float_wav(path, x, rate):
    x = np.ascontiguousarray(x, "<f4")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + x.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, rate, rate * 4, 4, 32))
        f.write(b"data" + struct.pack("<I", x.nbytes) + x.tobytes())


torch.cuda.set_device(0)
det = lb.Detective().configure(sample_rate=RATE, window=WINDOW, stride=STRIDE)
signal = lb.synth_clips_device(SEED, 0, CHANNELS, RATE_IN, PRIME + NEW)                # [channels, prime + new], multiples of 1 / 32768
assert -32768.0 <= float(signal.min()) * 32768.0 and float(signal.max()) * 32768.0 <= 32767.0      # every sample is an int16
prime = signal[:, :PRIME].contiguous().reshape(-1)
fresh = {"f32": signal[:, PRIME:].contiguous().reshape(-1)}
fresh["i16"] = (fresh["f32"] * 32768.0).to(torch.int16)
sb_prime = lb.synth_clips_device(SEED + 1, 0, CHANNELS, RATE, SB_PRIME).reshape(-1)
prime_counts, fresh_counts, sb_prime_counts, everyone = [PRIME] * CHANNELS, [NEW] * CHANNELS, [SB_PRIME] * CHANNELS, list(range(CHANNELS))
emitted_prime = int(lb.debug_resampler_bank_plan(RATE_IN, RATE, 0, [0], [0], [PRIME])[0][0])
new_each, _, m_lo, m_hi = lb.debug_resampler_bank_plan(RATE_IN, RATE, 0, [PRIME], [emitted_prime], [NEW])
per = int(new_each[0])                                                                # outputs of one channel
outputs = per * CHANNELS
rs = {k: lb.ResamplerBank(RATE_IN, RATE, CHANNELS) for k in ("rs_f32", "rs_i16", "chain_f32", "chain_i16")}
sb = {k: lb.StreamBank(det, CHANNELS, 4) for k in ("chain_f32", "chain_i16", "sb")}
rs_out = {k: torch.zeros(outputs, dtype=torch.float32, device="cuda") for k in rs}
sb_frames = CHANNELS * (((SB_PRIME + per - WINDOW) // STRIDE) // 128)                   # what a stream-bank push completes
sb_out = {k: torch.zeros((max(sb_frames, 1), 32), dtype=torch.uint8, device="cuda") for k in sb}
scratch = torch.zeros(outputs, dtype=torch.float32, device="cuda")
converted_counts = None
tmp = tempfile.TemporaryDirectory()
paths = []
if HOST:
    host_signal = signal[:HOST_CHANNELS].cpu().numpy()
    for c in range(HOST_CHANNELS):
        paths.append(os.path.join(tmp.name, f"channel{c}.wav"))
        write_float_wav(paths[-1], host_signal[c], RATE_IN)
host_result = {}


def restore():
    for bank in rs.values():
        bank.reset(everyone)
        bank.push_device(prime, prime_counts, out=scratch)
    for bank in sb.values():
        bank.reset(everyone)
        bank.push_device(sb_prime, sb_prime_counts)
    torch.cuda.synchronize()


def leg_rs(which):
    global converted_counts
    counts, _ = rs[which].push_device(fresh[which[-3:]], fresh_counts, out=rs_out[which])
    assert int(counts.sum()) == outputs
    converted_counts = counts


def leg_chain(which):
    counts, converted = rs[which].push_device(fresh[which[-3:]], fresh_counts, out=rs_out[which])
    rows, _ = sb[which].push_device(converted, counts, new_out=sb_out[which])
    assert int(rows.sum()) == sb_frames


def leg_sb():
    rows, _ = sb["sb"].push_device(rs_out["rs_f32"], converted_counts, new_out=sb_out["sb"])
    assert int(rows.sum()) == sb_frames


def leg_host():
    for c, path in enumerate(paths):
        host_result[c] = lb.read_audio_url(path, float(RATE), 0)[0]


legs = {"rs_f32": lambda: leg_rs("rs_f32"), "rs_i16": lambda: leg_rs("rs_i16"), "chain_f32": lambda: leg_chain("chain_f32"),
        "chain_i16": lambda: leg_chain("chain_i16"), "sb": leg_sb}
if HOST:
    legs["host"] = leg_host
host = {k: [] for k in legs}
device = {k: [] for k in legs}
for rep in range(REPS + 1):                                                           # (the first round warms every leg up)
    restore()
    for k, f in legs.items():
        h, d = timed(f, k != "host")
        if rep:
            host[k].append(h)
            device[k].append(d)
# after the clock: the same bits
torch.cuda.synchronize()
for k in ("rs_i16", "chain_f32", "chain_i16"):
    assert torch.equal(rs_out[k].view(torch.int32), rs_out["rs_f32"].view(torch.int32)), f"{k}: the converted samples differ from rs_f32's"
for k in ("chain_f32", "chain_i16"):
    assert torch.equal(sb_out[k], sb_out["sb"]), f"{k}: the chain's sub-fingerprints differ from the stream bank's alone"
if HOST:
    got = rs_out["rs_f32"].cpu().numpy()
    for c in (0, HOST_CHANNELS - 1):
        assert np.array_equal(got[c * per:(c + 1) * per].view(np.uint32), host_result[c][emitted_prime:emitted_prime + per].view(np.uint32)), \
            f"channel {c} differs from the host converter"
taps = m_hi - m_lo + 1
res = {"channels": CHANNELS, "primed": PRIME, "new_samples": NEW, "outputs": outputs, "taps": taps, "reps": REPS, "rate_in": RATE_IN,
       "rate_out": RATE, "tap_products": outputs * taps, "weight_bytes_without_reuse": outputs * taps * 8,
       "host_ms": {k: _stats(v) for k, v in host.items()}, "device_ms": {k: _stats(device[k]) for k in legs if k != "host"}}
for fmt in ("f32", "i16"):
    res[f"chain_{fmt}_minus_sb_device_ms"] = round(res["device_ms"][f"chain_{fmt}"]["median"] - res["device_ms"]["sb"]["median"], 4)
    res[f"rs_{fmt}_gtaps_per_s"] = round(outputs * taps / res["device_ms"][f"rs_{fmt}"]["median"] / 1e6, 2)
if HOST:
    res["host_channels"] = HOST_CHANNELS
    res["host_scaled_ms"] = round(res["host_ms"]["host"]["median"] * CHANNELS / HOST_CHANNELS, 2)
    res["host_scaled_over_chain_f32_host"] = round(res["host_scaled_ms"] / res["host_ms"]["chain_f32"]["median"], 1)
print(json.dumps(res), flush=True)
os.makedirs(OUT, exist_ok=True)
name = "resampler_bank.json" if (RATE_IN, RATE) == (44100, 5512) else f"resampler_bank_{RATE_IN}_{RATE}.json"
with open(os.path.join(OUT, name), "w") as f:
    f.write(json.dumps(res, indent=1) + "\n")
