#!/usr/bin/env python3
"""Frame phases against what they replace, alternating in one process after warm-up:
    python3 tools/prof_phases.py [reps] [--out DIR] [--clips N] [--channels N] [--commit ID]
Headline settings (44.1 kHz, window 1024, stride 64).  Two parts, device events around every leg, medians and quartiles of `reps`
rounds (default 7, at least 5) in ms:
  (a) batch: N (100 000) clips of one second in a padded block (pitch 44 100 + 128 x 64 samples), for P = 1, 2, 4, 8
        phases   Detective.fingerprint_clips_device_phases(clips, P): stage 1 once (plus one frame per clip), stage 2 per phase
        loop     P x LBAudioDetectiveFingerprintClipsDevice on the clip pointer advanced by p x (128 / P) x 64 samples, the surplus
                 last frame ignored: P stage-1 passes -- the calls the parent commit has
      after the clock, every frame both legs hold is compared bit for bit.
  (b) live: one push of 44 100 samples into each of C (1 024) channels that carry 3 140
        phased   a phased bank at P = 1, 4, 8
        plain    an unphased bank of C channels (one phase: what the parent commit gives)
        shifted  the work-around the parent commit allows: an unphased bank of C x P channels fed copies shifted by the phase offsets
One JSON object, printed and written to DIR/phases.json (default DIR: profiles) with the commit it ran on (--commit, else git).
    timeout -k 10 900 python3 tools/prof_phases.py 7"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import lbaudiodetective_amd as lb  # noqa: E402

SEED = 0x4C424150
RATE, WINDOW, STRIDE = 44100, 1024, 64
HOP = 128 * STRIDE
SECOND, CARRIED = 44100, 3140
PITCH = SECOND + HOP


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _commit():
    given = _option("--commit")
    if given:
        return given
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=30).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "-uno"], capture_output=True, text=True, timeout=30).stdout.strip()
        return (head + ("+changes" if dirty else "")) if head else "unknown"
    except (OSError, subprocess.SubprocessError):
        return "unknown"


OUT = _option("--out", os.path.join(ROOT, "profiles"))
CLIPS = int(_option("--clips", 100000))
CHANNELS = int(_option("--channels", 1024))
_values = {OUT, str(CLIPS), str(CHANNELS), _option("--commit")}
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in _values]
REPS = max(5, int(args[0]) if args else 7)


def _stats(v):
    q = statistics.quantiles(v, n=4)
    return {"median": round(q[1], 4), "p25": round(q[0], 4), "p75": round(q[2], 4), "iqr": round(q[2] - q[0], 4), "min": round(min(v), 4),
            "max": round(max(v), 4)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def beats(fast, slow):
    """the faster leg's median is below the slower one's by more than both interquartile ranges"""
    return bool(slow["median"] - fast["median"] > fast["iqr"] + slow["iqr"])


torch.cuda.set_device(0)
L = lb.lib()
det = lb.Detective().configure(sample_rate=RATE, window=WINDOW, stride=STRIDE)
res = {"commit": _commit(), "sample_rate": RATE, "window": WINDOW, "stride": STRIDE, "reps": REPS, "clips": CLIPS, "channels": CHANNELS,
       "clip_pitch_samples": PITCH, "batch": {}, "live": {}}

# ---- (a) the batch call against its loop ------------------------------------------------------------------------------------
block = lb.synth_clips_device(SEED, 0, CLIPS + 1, RATE, PITCH).reshape(-1)             # (one clip more: room behind the last for the loop)
clips = block[:CLIPS * PITCH].view(CLIPS, PITCH)
count0 = det.subfingerprint_count(PITCH)
for phases in (1, 2, 4, 8):
    h = 128 // phases
    out_phases = torch.zeros((CLIPS, phases, count0, 8), dtype=torch.int32, device="cuda").view(torch.uint32)
    out_loop = torch.zeros((phases, CLIPS, count0, 32), dtype=torch.uint8, device="cuda")

    def leg_phases():
        det.fingerprint_clips_device_phases(clips, phases, out=out_phases)

    def leg_loop():
        for p in range(phases):
            st = L.LBAudioDetectiveFingerprintClipsDevice(det._ref, C.c_void_p(block.data_ptr() + 4 * p * h * STRIDE), CLIPS, PITCH,
                                                          C.c_void_p(out_loop[p].data_ptr()), None)
            assert st == 0, st

    legs = {"phases": leg_phases, "loop": leg_loop}
    ms = {k: [] for k in legs}
    for rep in range(REPS + 1):                                                       # (the first round warms both legs up)
        for k, f in legs.items():
            t = timed(f)
            if rep:
                ms[k].append(t)
    torch.cuda.synchronize()
    got = out_phases.view(torch.uint8).view(CLIPS, phases, count0, 32)
    for p in range(phases):
        n = det.subfingerprint_count_at_phase(PITCH, phases, p)
        assert torch.equal(got[:, p, :n], out_loop[p][:, :n]), f"P {phases}, phase {p}: the call and the loop differ"
    st = {k: _stats(v) for k, v in ms.items()}
    res["batch"][str(phases)] = {"device_ms": st, "loop_over_phases": round(st["loop"]["median"] / st["phases"]["median"], 3),
                                 "phases_beats_loop": beats(st["phases"], st["loop"])}
    del out_phases, out_loop
one = res["batch"]["1"]["device_ms"]["phases"]["median"]
for phases in (2, 4, 8):
    res["batch"][str(phases)]["phases_over_one_pass"] = round(res["batch"][str(phases)]["device_ms"]["phases"]["median"] / one, 3)
del clips, block
torch.cuda.empty_cache()

# ---- (b) one push of a phased bank against the unphased bank and against C x P shifted channels --------------------------------
signal = lb.synth_clips_device(SEED + 1, 0, CHANNELS, RATE, CARRIED + SECOND + HOP)
plain = lb.StreamBank(det, CHANNELS, 21)
prime_plain = signal[:, :CARRIED].contiguous().reshape(-1)
fresh_plain = signal[:, CARRIED:CARRIED + SECOND].contiguous().reshape(-1)


def push_leg(bank, prime, fresh, n_channels):
    everyone = list(range(n_channels))
    room = torch.zeros((bank.virtual_channels * 6, 32), dtype=torch.uint8, device="cuda")

    def restore():
        bank.reset(everyone)
        bank.push_device(prime, [CARRIED] * n_channels)

    def leg():
        bank.push_device(fresh, [SECOND] * n_channels, new_out=room)
    return restore, leg


live = {"plain": push_leg(plain, prime_plain, fresh_plain, CHANNELS)}
keep = [plain]
for phases in (1, 4, 8):
    h = 128 // phases
    phased = lb.StreamBank(det, CHANNELS, 21, phases=phases)
    live[f"phased{phases}"] = push_leg(phased, prime_plain, fresh_plain, CHANNELS)
    keep.append(phased)
    if phases > 1:
        offs = [p * h * STRIDE for p in range(phases)]
        prime = torch.stack([signal[:, o:o + CARRIED] for o in offs], dim=1).contiguous().reshape(-1)
        fresh = torch.stack([signal[:, o + CARRIED:o + CARRIED + SECOND] for o in offs], dim=1).contiguous().reshape(-1)
        shifted = lb.StreamBank(det, CHANNELS * phases, 21)
        live[f"shifted{phases}"] = push_leg(shifted, prime, fresh, CHANNELS * phases)
        keep.append(shifted)
ms = {k: [] for k in live}
for rep in range(REPS + 1):
    for k, (restore, leg) in live.items():
        restore()
        t = timed(leg)
        if rep:
            ms[k].append(t)
st = {k: _stats(v) for k, v in ms.items()}
res["live"]["device_ms"] = st
for phases in (1, 4, 8):
    row = {"phased_over_plain": round(st[f"phased{phases}"]["median"] / st["plain"]["median"], 3)}
    if phases > 1:
        row["shifted_over_phased"] = round(st[f"shifted{phases}"]["median"] / st[f"phased{phases}"]["median"], 3)
        row["phased_beats_shifted"] = beats(st[f"phased{phases}"], st[f"shifted{phases}"])
    res["live"][str(phases)] = row
print(json.dumps(res), flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "phases.json"), "w") as f:
    f.write(json.dumps(res, indent=1) + "\n")
