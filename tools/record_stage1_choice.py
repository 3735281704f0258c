#!/usr/bin/env python3
"""Records tests/golden/stage1_choice.json: the answer of LBAudioDetectiveDebugStage1Choice (which stage-1 kernel instance, which
rows between the stages and which stage 2 one batch call takes) over a grid that holds every boundary the decision tests.
Needs no GPU.  tests/test_stage1_choice_cpu.py replays the file's rows against the library and wants every word equal, so
the file is recorded ONCE from a build whose routing is trusted (LBAD_LIB=<that build> python tools/record_stage1_choice.py)
and is not re-recorded to make a change pass.

    python tools/record_stage1_choice.py [--out tests/golden/stage1_choice.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INPUTS = ["rate", "window", "stride", "bands", "subfp_len", "variant", "waves", "cache", "fmt", "n_clips", "frames", "extra",
          "address_mod8", "tap", "tail"]
WINDOWS = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]
STRIDES = [1, 2, 6, 8, 63, 64, 65, 100, 200, 254, 1024, 1026]
BANDS = [1, 16, 32, 33, 64]
RATES = [4000, 5512, 8000, 11025, 16000, 22050, 44100, 48000, 96000]
# one configuration (rate, window, stride, bands, subfp_len) per kernel family, loader and q range, and the generic kernel's
# neighbours of each: the axes of the CALL (format, clip count and parity, alignment, variant, tap, tail) are crossed on these
CALL_CONFIGS = [
    (44100, 1024, 64, 32, 200),     # pruned, compact rows
    (48000, 1024, 64, 32, 200),     # pruned, a zero divisor: no sparse form
    (5512, 2048, 64, 32, 200),      # stream2, q 2..23 (the default)
    (11025, 2048, 64, 32, 200),     # stream2, q 0..31
    (5512, 2048, 8, 32, 200),       # full <4>, the file hop: the general span loader
    (48000, 4096, 64, 32, 200),     # stream
    (22050, 1024, 64, 32, 200),     # full <3>
    (11025, 512, 64, 2, 20),        # full <2>
    (8000, 256, 64, 32, 200),       # full <1>
    (8000, 64, 16, 7, 33),          # generic
]
# (clips, extra samples, address): one aligned clip, one clip a sample into a pair, several clips of even and of odd length
CALL_SHAPES = [(1, 0, 0), (1, 0, 4), (1, 1, 0), (3, 0, 0), (3, 1, 0)]
TUNING_WAVES = [0, 1, 2, 3, 4, 6, 7, 8, 12, 16]


def subfp_for(bands):
    return min(200, 128 * bands)


def grid():
    """rows of INPUTS; a clip is window + stride * 128 * frames + extra samples long.  Every boundary of the decision, each axis
    where it can change the answer -- not the full cross product (the file stays reviewable)"""
    rows = []
    # 1. the settings: which family a configuration has.  Stride 64 with every band count and rate at the windows that have
    # specialised kernels; the other strides, and the other windows, at fewer tables
    for w in WINDOWS:
        special = 256 <= w <= 4096
        for s in STRIDES:
            if s == 64 and special:
                tables = [(r, 32) for r in RATES] + [(r, b) for b in BANDS if b != 32 for r in (5512, 44100, 48000)]
            elif s == 64:
                tables = [(11025, 32), (44100, 32)]
            elif special:
                tables = [(5512, 32), (96000, 64)]
            else:
                tables = [(44100, 32)] if s in (1, 65) else []
            for r, b in tables:
                rows.append((r, w, s, b, subfp_for(b), 0, 0, 1, 0, 3, 1, 0, 0, 0, 0))
    # 2. the call: format, one clip / several, even / odd length, alignment, under the variants that look at them (1 takes the
    # generic kernel whatever the call; 3 and 4 are 2 but for one kernel and for compact rows); the tap and variant 4 where rows can be compact
    for n, cfg in enumerate(CALL_CONFIGS):
        for variant in (0, 2):
            for fmt in range(3):
                for n_clips, extra, addr in CALL_SHAPES:
                    rows.append(cfg + (variant, 0, 1, fmt, n_clips, 1, extra, addr, 0, 0))
        for fmt in range(3):                                            # 3: never the streaming kernel of 2048 samples
            rows.append(cfg + (3, 0, 1, fmt, 3, 1, 0, 0, 0, 0))
        rows.append(cfg + (1, 0, 1, 0, 3, 1, 0, 0, 0, 0))
        for variant in ((0, 1, 2, 3, 4) if n < 2 else (0,)):
            for tap in ((0, 1) if variant == 4 else (1,)):
                rows.append(cfg + (variant, 0, 1, 0, 3, 1, 0, 0, tap, 0))
        rows.append(cfg + (0, 0, 1, 1, 1, 1, 0, 2, 0, 0))               # int16 one sample into a pair
        for variant in (0, 2):                                          # a file tail: one float32 clip, full rows
            rows.append(cfg + (variant, 0, 1, 0, 1, 1, 0, 0, 0, 1))
        rows.append(cfg + (0, 0, 1, 0, 3, 1, 0, 0, 0, 1))               # ... refused with several clips or integer PCM
        rows.append(cfg + (0, 0, 1, 1, 1, 1, 0, 0, 0, 1))
    # 3. the tuning of the generic kernel (variant 1 takes it at every window): workgroup sizes that are listed, that are not and
    # that do not fit, cache on and off; from 2048 samples on at tables that read a wide span of bins and at one that reads a
    # narrow one (3300 Hz: the only kind beside which two waves of 8192 samples AND the cache fit)
    for w in WINDOWS:
        for r, b in (((44100, 32), (4000, 64), (3300, 32)) if w >= 2048 else ((44100, 32),)):
            for waves in (TUNING_WAVES if w >= 2048 else [0, 3, 4]):
                for cache in (1, 0):
                    rows.append((r, w, 64, b, subfp_for(b), 1, waves, cache, 0, 3, 1, 0, 0, 0, 0))
    for r in (11025, 16000):                                            # 8192 samples, a wide table: no cache at automatic tuning
        rows.append((r, 8192, 64, 32, 200, 0, 0, 1, 0, 3, 1, 0, 0, 0, 0))
    # 4. the other statuses: no whole frame, no clip, a format, and settings outside their ranges
    base = (44100, 1024, 64, 32, 200)
    rows.append(base + (0, 0, 1, 0, 3, 0, 0, 0, 0, 0))
    rows.append(base + (0, 0, 1, 0, 3, 0, 64 * 128 - 1, 0, 0, 0))
    rows.append(base + (0, 0, 1, 0, 0, 1, 0, 0, 0, 0))
    rows.append(base + (0, 0, 1, 3, 3, 1, 0, 0, 0, 0))
    for cfg in ((0, 1024, 64, 32, 200), (44100, 8, 64, 32, 200), (44100, 1000, 64, 32, 200), (44100, 16384, 64, 32, 200),
                (44100, 1024, 0, 32, 200), (44100, 1024, 64, 0, 200), (44100, 1024, 64, 65, 200), (44100, 1024, 64, 32, 0),
                (44100, 1024, 64, 32, 257), (44100, 1024, 64, 1, 129), (44100, 1024, 64, 64, 256), (44100, 1024, 64, 32, 256),
                (44100, 1024, 64, 32, 1), (44100, 1024, 64, 16, 200)):
        rows.append(cfg + (0, 0, 1, 0, 3, 1, 0, 0, 0, 0))
    return rows


def choice_words(lb, row):
    rate, window, stride, bands, subfp_len, variant, waves, cache, fmt, n_clips, frames, extra, addr, tap, tail = row
    spc = window + stride * 128 * frames + extra
    return lb.debug_stage1_choice(rate, window, stride, bands, subfp_len, variant, waves, bool(cache), fmt, n_clips, spc, addr,
                                  bool(tap), bool(tail)).words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "stage1_choice.json"))
    args = ap.parse_args()
    import lbaudiodetective_amd as lb
    out_rows = [list(r) + choice_words(lb, r) for r in grid()]
    with open(args.out, "w") as f:
        f.write('{"inputs": %s,\n' % json.dumps(INPUTS))
        f.write(' "samples_per_clip": "window + stride * 128 * frames + extra",\n')
        f.write(' "rows": [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in out_rows) + "]}\n")
    print("%d rows -> %s" % (len(out_rows), args.out))


if __name__ == "__main__":
    main()
