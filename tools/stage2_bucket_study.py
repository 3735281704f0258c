#!/usr/bin/env python3
"""CPU study for the bucket ranking of stage 2 (k_haar_select32.hip): how the candidates of a frame spread over the
histogram's buckets (the 11 leading bits of |v|: an eighth of a binade each).
    python3 tools/stage2_bucket_study.py [n_synth_clips] [--out profiles/stage2_bucket_study.json]
With the ORACLE's Haar coefficients of the bench's synthetic clips (44.1 kHz / 1024 / 64) and of the bird fixtures (at
44.1 kHz / 1024 and at the default 5512 Hz / 2048) it follows the kernel's threshold search (histogram from the top, then
bisection inside the threshold bucket when that leaves more than 128 keys) and reports per frame
  * the candidates and the buckets they occupy, the distribution of candidates per occupied bucket (segment length),
  * the in-segment compares (sum of length^2 over the segments) against the all-pairs count the kernel spent so far
    (three parts x two candidates x the part's blocks of eight keys),
  * the longest segment, and the trips of the in-segment loop per wave (threads 64 w .. 64 w + 63 rank list slots of the
    same numbers; a wave runs as long as its longest segment).
No GPU is needed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from oracle import oracle as O  # noqa: E402

KEEP, KCAND, SEED = 100, 128, 0x4C424144


def frame_stats(haar: np.ndarray, keep: int = KEEP):
    bits = np.ascontiguousarray(haar, np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF)
    hist = np.bincount(bits >> 20, minlength=2048)
    above = np.cumsum(hist[::-1])[::-1]                     # keys in buckets >= b
    above0 = above.copy()
    ok = np.nonzero(above[1:] >= keep)[0]
    path = "histogram"
    if ok.size == 0:                                        # fewer than keep keys outside bucket 0
        lo, hi, cnt = 0, 1 << 20, bits.size
    else:
        b = int(ok[-1]) + 1
        lo, hi, cnt = b << 20, (b + 1) << 20, int(above0[b])
    while cnt > KCAND and hi - lo > 1:
        path = "bisection"
        mid = lo + ((hi - lo) >> 1)
        c = int((bits >= mid).sum())
        if c >= keep:
            lo, cnt = mid, c
        else:
            hi = mid
    if cnt > KCAND:
        return {"path": "plateau", "nc": keep, "segments": None}
    cand = bits[bits >= lo]
    seg = np.bincount(cand >> 20, minlength=2048)
    seg = seg[seg > 0][::-1]                                # highest bucket first: the list's order
    nc = int(cand.size)
    owner = np.repeat(seg, seg)                             # slot -> length of its segment
    waves = [int(owner[w:w + 64].max()) if w < nc else 0 for w in (0, 64)]
    nblk = (nc + 7) // 8
    pblk = (nblk + 2) // 3
    all_pairs = sum(min(pblk, max(0, nblk - p * pblk)) for p in range(3)) * 8 * 128   # 64 threads x 2 candidates per part
    return {"path": path, "nc": nc, "segments": seg, "in_segment": int((seg.astype(np.int64) ** 2).sum()), "all_pairs": all_pairs,
            "longest": int(seg.max()), "wave_trips": waves}


def summarize(name, frames_stats):
    done = [s for s in frames_stats if s["segments"] is not None]
    lens = np.concatenate([s["segments"] for s in done]) if done else np.zeros(0, np.int64)
    longest = np.array([s["longest"] for s in done])
    ins = np.array([s["in_segment"] for s in done])
    trips = np.array([s["wave_trips"] for s in done])
    pct = lambda a, q: float(np.percentile(a, q)) if a.size else None      # noqa: E731
    out = {
        "set": name, "frames": len(frames_stats),
        "paths": {p: sum(1 for s in frames_stats if s["path"] == p) for p in ("histogram", "bisection", "plateau")},
        "candidates_per_frame": {"mean": float(np.mean([s["nc"] for s in done])), "min": min(s["nc"] for s in done), "max": max(s["nc"] for s in done)},
        "occupied_buckets_per_frame": {"mean": float(np.mean([s["segments"].size for s in done]))},
        "candidates_per_occupied_bucket": {"mean": float(lens.mean()), "p50": pct(lens, 50), "p90": pct(lens, 90), "p99": pct(lens, 99), "max": int(lens.max()),
                                           "histogram_1_to_32": np.bincount(np.minimum(lens, 33), minlength=34)[1:].tolist()},
        "in_segment_compares_per_frame": {"mean": float(ins.mean()), "p50": pct(ins, 50), "p99": pct(ins, 99), "max": int(ins.max())},
        "all_pairs_compares_per_frame": {"mean": float(np.mean([s["all_pairs"] for s in done]))},
        "longest_segment_per_frame": {"mean": float(longest.mean()), "p50": pct(longest, 50), "p90": pct(longest, 90), "p99": pct(longest, 99), "p999": pct(longest, 99.9),
                                      "max": int(longest.max()), "frames_over": {str(L): int((longest > L).sum()) for L in (8, 12, 16, 24, 32, 48, 64)}},
        "loop_trips_per_wave": {"wave0_mean": float(trips[:, 0].mean()), "wave1_mean": float(trips[:, 1].mean())},
    }
    print(json.dumps(out), flush=True)
    return out


def haar_of_pcm(pcm, cfg):
    _, _, haar = O.fingerprint_pcm(pcm, cfg, taps=True)
    return haar


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "stage2_bucket_study.json")
    args = [a for a in args if a != out_path]
    n_clips = int(args[0]) if args else 400
    O.build()
    results = []
    cfg = O.Config(44100, 1024)
    stats = []
    for c in range(n_clips):
        for h in haar_of_pcm(O.synth_clip(SEED, c, 44100, 44100), cfg):
            stats.append(frame_stats(h))
    results.append(summarize(f"bench synthetic clips 0..{n_clips - 1}, 44.1 kHz / 1024 / 64", stats))
    birds = sorted(os.listdir(os.path.join(ROOT, "tests", "golden", "birds")))
    for rate, window in ((44100, 1024), (5512, 2048)):
        cfg = O.Config(rate, window)
        stats = []
        for name in birds:
            pcm, file_rate = O.decode_audio_file(os.path.join(ROOT, "tests", "golden", "birds", name))
            if file_rate != rate:
                pcm = O.resample(pcm, file_rate, rate)
            for h in haar_of_pcm(pcm, cfg):
                stats.append(frame_stats(h))
        results.append(summarize(f"bird fixtures ({len(birds)} files), {rate} Hz / {window} / 64", stats))
    with open(out_path, "w") as f:
        json.dump({"what": "tools/stage2_bucket_study.py: candidates of stage 2 by histogram bucket, oracle coefficients, keep = 100, at most 128 candidates",
                   "sets": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
