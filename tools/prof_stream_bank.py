#!/usr/bin/env python3
"""One push of a stream bank against the two things it stands beside, alternating in one process after warm-up:
    python3 tools/prof_stream_bank.py [reps] [--out DIR] [--channels N]
1 024 channels at 44.1 kHz / 1024 (hop 8 192), every channel carrying 3 140 samples, receive 44 100 new samples each (one second):
five complete frames per channel, 5 120 in all, each across the seam of carried and new samples.  Legs:
    bank     StreamBank.push_device with outNewPacked (staging, fingerprint_clips_device, commit) of a bank with the default pass
             size, one frame per channel: five passes of 1 024 frames
    bank1    the same of a bank made with frames_per_pass = 5 120: the whole push in one pass (five times the staging memory)
    a        Detective.fingerprint_clips_device on the same 5 120 frames already laid out as one-frame clips of 9 216 samples: what
             the bank calls, without the bank -- bank1 minus a is the bank's overhead, bank minus bank1 what the passes cost
    b        the loop a user has today: 1 024 x Stream.push of the channel's 44 100 host samples (synchronous, one channel a call)
Every round restores the state first, outside the clock: the banks' channels are reset and primed with the 3 140 samples, fresh
Stream handles are primed likewise.  Times: a host clock around the calls and the synchronise that ends them (all legs), and
device events (bank, bank1 and a).  Medians and quartiles of `reps` rounds (default 7, at least 5) in ms.  After the clock stops the
banks' new sub-fingerprints must equal leg a's bit for bit, and channel 0's those of its Stream.  One JSON object, printed and
written to DIR/stream_bank.json (default DIR: profiles).  No bar: nothing here decides acceptance.
    timeout -k 10 600 python3 tools/prof_stream_bank.py 7"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lbaudiodetective_amd as lb  # noqa: E402

SEED = 0x4C424147
RATE, WINDOW, HOP = 44100, 1024, 8192
CARRIED, NEW = 3140, 44100


def _option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = _option("--out", os.path.join(ROOT, "profiles"))
CHANNELS = int(_option("--channels", 1024))
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in {OUT, str(CHANNELS)}]
REPS = max(5, int(args[0]) if args else 7)


def _stats(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    return {"median": round(q[1], 4), "p25": round(q[0], 4), "p75": round(q[2], 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn):
    """(host ms up to the end of the device's work, device ms between events around the calls)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


torch.cuda.set_device(0)
det = lb.Detective().configure(sample_rate=RATE, window=WINDOW)
signal = lb.synth_clips_device(SEED, 0, CHANNELS, RATE, CARRIED + NEW)                 # [channels, carried + new]
prime = signal[:, :CARRIED].contiguous().reshape(-1)
fresh = signal[:, CARRIED:].contiguous().reshape(-1)
clips = signal.unfold(1, WINDOW + HOP, HOP).contiguous()                              # [channels, frames, 9216]
per = clips.shape[1]
frames = CHANNELS * per
clips = clips.reshape(frames, WINDOW + HOP)
host_prime, host_fresh = signal[:, :CARRIED].cpu().numpy(), signal[:, CARRIED:].cpu().numpy()
prime_counts, fresh_counts, everyone = [CARRIED] * CHANNELS, [NEW] * CHANNELS, list(range(CHANNELS))
banks = {"bank": lb.StreamBank(det, CHANNELS, 21), "bank1": lb.StreamBank(det, CHANNELS, 21, frames_per_pass=frames)}
bank_out = {k: torch.zeros((frames, 32), dtype=torch.uint8, device="cuda") for k in banks}
a_out = torch.zeros((frames, 1, 32), dtype=torch.uint8, device="cuda")
streams = []


def restore():
    for bank in banks.values():
        bank.reset(everyone)
        bank.push_device(prime, prime_counts)
    streams[:] = [lb.Stream(det) for _ in range(CHANNELS)]
    for c, s in enumerate(streams):
        s.push(host_prime[c])
    torch.cuda.synchronize()


def leg_bank(which):
    counts, _ = banks[which].push_device(fresh, fresh_counts, new_out=bank_out[which])
    assert int(counts.sum()) == frames


def leg_b():
    for c, s in enumerate(streams):
        s.push(host_fresh[c])


legs = {"bank": lambda: leg_bank("bank"), "bank1": lambda: leg_bank("bank1"), "a": lambda: det.fingerprint_clips_device(clips, out=a_out), "b": leg_b}
host = {k: [] for k in legs}
device = {k: [] for k in legs}
for rep in range(REPS + 1):                                                           # (the first round warms every leg up)
    restore()
    for k, f in legs.items():
        h, d = timed(f)
        if rep:
            host[k].append(h)
            device[k].append(d)
# after the clock: the same bits
torch.cuda.synchronize()
for k in banks:
    assert torch.equal(bank_out[k], a_out.reshape(frames, 32)), f"{k}: the bank's sub-fingerprints differ from the batch call's"
got = lb.unpack_packed(bank_out["bank"][:per].cpu().numpy(), 200)
assert np.array_equal(got, streams[0].fingerprint().to_bools()), "channel 0 differs from its Stream"
res = {"channels": CHANNELS, "carried": CARRIED, "new_samples": NEW, "frames": frames, "reps": REPS, "sample_rate": RATE, "window": WINDOW,
       "staged_bytes": frames * (WINDOW + HOP) * 4, "host_ms": {k: _stats(v) for k, v in host.items()},
       "device_ms": {k: _stats(device[k]) for k in ("bank", "bank1", "a")}}
for k in banks:
    res[k + "_minus_a_device_ms"] = round(res["device_ms"][k]["median"] - res["device_ms"]["a"]["median"], 4)
    res[k + "_over_a_device"] = round(res["device_ms"][k]["median"] / res["device_ms"]["a"]["median"], 4)
res["b_over_bank_host"] = round(res["host_ms"]["b"]["median"] / res["host_ms"]["bank"]["median"], 2)
print(json.dumps(res), flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "stream_bank.json"), "w") as f:
    f.write(json.dumps(res, indent=1) + "\n")
