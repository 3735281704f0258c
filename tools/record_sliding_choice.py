#!/usr/bin/env python3
"""Records tests/golden/sliding_choice.json: the answer of LBAudioDetectiveDebugSlidingChoice (which kernel one launch of a
ragged-corpus scan takes, and what it needs in front of it) over a grid that holds every boundary of the decision.  Needs no
GPU.  tests/test_sliding_choice_cpu.py replays the file's rows against the library and wants every word equal, so the file is
recorded ONCE from a build whose routing is trusted (LBAD_LIB=<that build> python tools/record_sliding_choice.py) and is not
re-recorded to make a change pass.

    python tools/record_sliding_choice.py [--out tests/golden/sliding_choice.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUBFP_LEN = 200
CUS = 256
QUERY_LENGTHS = [1, 7, 8, 12, 13, 15, 16, 21, 47, 48, 480, 481, 8192, 8193]
QUERIES_LEFT = [1, 2, 3, 4, 5, 8, 9]
LONGEST = [1, 7, 8, 12, 13, 15, 16, 70]
PARTIAL_RANGE = 7


def histograms():
    """(name, pairs, the ne_max it goes with): one length only (per longest entry), 1..70 uniform, and many entries of 8..15 with
    few long ones (the split of the scan triggers from a query of about 40 on)"""
    hs = [("single_%d" % n, [[n, 100000]], n) for n in LONGEST]
    hs.append(("uniform_1_70", [[n, 1000] for n in range(1, 71)], 70))
    hs.append(("short_8_15_few_long", [[n, 500000] for n in range(8, 16)] + [[n, 100] for n in range(20, 71, 10)], 70))
    return hs


def grid(hs):
    """rows of (histogram, ne_max, variant, query length, queries left, range, scores, host blocks): every boundary of the
    decision, each option where it can change the answer -- not the full cross product (the file stays reviewable)"""
    rows = []
    for h, (_, _, ne_max) in enumerate(hs):
        mixed = h >= len(LONGEST)                               # the two histograms of many lengths
        for nq in QUERY_LENGTHS:
            for left in QUERIES_LEFT:                           # the routing itself: device blocks, keys only, full range
                rows.append((h, ne_max, 0, nq, left, 0, 0, 0))
            rows.append((h, ne_max, 0, nq, 1, 0, 0, 1))         # host blocks: a single query may travel in the arguments
            if ne_max >= 15:
                for left in (1, 5):                             # per-entry scores: one query per launch
                    rows.append((h, ne_max, 0, nq, left, 0, 1, 1))
            if ne_max >= 16:
                for left in (1, 2, 4):                          # partial range: the other instances of the task kernel
                    rows.append((h, ne_max, 0, nq, left, PARTIAL_RANGE, 0, 1))
            if mixed or ne_max == 70:
                for variant in (3, 4):                          # the split forced / forbidden
                    for left in (1, 4):
                        rows.append((h, ne_max, variant, nq, left, 0, 0, 1))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sliding_choice.json"))
    args = ap.parse_args()
    import lbaudiodetective_amd as lb
    hs = histograms()
    out_rows = []
    for (h, ne_max, variant, nq, left, rng, scores, host) in grid(hs):
        pairs = hs[h][1]
        n_pos = sum(n * k for n, k in pairs)
        words = lb.debug_sliding_choice(pairs, n_pos, ne_max, variant, SUBFP_LEN, nq, left, rng, bool(scores), bool(host), CUS)
        out_rows.append([h, ne_max, variant, nq, left, rng, scores, host] + [int(w) for w in words])
    with open(args.out, "w") as f:
        f.write('{"subfp_len": %d, "cus": %d,\n' % (SUBFP_LEN, CUS))
        f.write(' "inputs": ["histogram", "ne_max", "variant", "n_query", "n_left", "range", "scores", "host_blocks"],\n')
        f.write(' "histograms": [\n' + ",\n".join("  " + json.dumps({"name": n, "pairs": p}) for n, p, _ in hs) + "],\n")
        f.write(' "rows": [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in out_rows) + "]}\n")
    print("%d rows -> %s" % (len(out_rows), args.out))


if __name__ == "__main__":
    main()
