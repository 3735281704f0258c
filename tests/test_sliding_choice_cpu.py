"""CPU check of the ONE decision behind every ragged-corpus launch (sliding.cpp: sliding_choose): which kernel and instance a
launch takes, how many queries, the split, the task counts and the grid, whether the plan is read, whether the query travels in
the kernel's arguments, whether the keys are maxed in place, and the systolic launch that may follow.  Every kernel returns the
same bits, so no parity test notices a query routed to a slower kernel; tests/golden/sliding_choice.json pins the routing as
it was recorded from the commit before the decision moved into one function (tools/record_sliding_choice.py; HISTORY.md, "After
round 6").  The library must reproduce the file exactly.  Needs no GPU."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sliding_choice.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_grid_holds_every_boundary(golden):
    rows = golden["rows"]
    col = {name: i for i, name in enumerate(golden["inputs"])}
    assert {r[col["n_query"]] for r in rows} == {1, 7, 8, 12, 13, 15, 16, 21, 47, 48, 480, 481, 8192, 8193}
    assert {r[col["n_left"]] for r in rows} >= {1, 2, 3, 4, 5, 8, 9}
    assert {r[col["ne_max"]] for r in rows} == {1, 7, 8, 12, 13, 15, 16, 70}
    assert {r[col["variant"]] for r in rows} == {0, 3, 4}
    assert {r[col["scores"]] for r in rows} == {0, 1} and {r[col["host_blocks"]] for r in rows} == {0, 1}
    assert {r[col["range"]] for r in rows} == {0, 7} and golden["cus"] == 256
    assert len(golden["histograms"]) >= 3 and len(rows) < 10000
    words = [r[len(col):] for r in rows]
    assert all(len(w) == 21 for w in words)
    # the split triggers by its rule (variant 0) and every family is there, the 8 + 8 + 36 instances included
    assert any(w[6] for r, w in zip(rows, words) if r[col["variant"]] == 0) and any(w[15] for w in words) and any(w[0] == 0 for w in words)
    instances = {(w[1],) + tuple(w[2:6]) for w in words if w[0]} | {(1, 1 if w[18] <= 6 else 4, w[0], 0, 0) for w in words if w[17]}
    assert len({i for i in instances if i[0] == 0}) == 8 and len({i for i in instances if i[0] == 1}) == 8
    assert {i[2] for i in instances if i[0] == 2} == {1, 7, 8, 12} and {i[1] for i in instances if i[0] == 2} == {2, 4, 8}


def test_library_reproduces_the_recorded_choice(lb, golden):
    n_in = len(golden["inputs"])
    hists = [[tuple(p) for p in h["pairs"]] for h in golden["histograms"]]
    n_pos = [sum(n * k for n, k in h) for h in hists]
    bad = []
    for r in golden["rows"]:
        h, ne_max, variant, nq, left, rg, scores, host = r[:n_in]
        got = lb.debug_sliding_choice(hists[h], n_pos[h], ne_max, variant, golden["subfp_len"], nq, left, rg, bool(scores), bool(host),
                                      golden["cus"])
        if got != r[n_in:]:
            bad.append((r[:n_in], got, r[n_in:]))
    assert not bad, (len(bad), bad[:3])


def test_argument_checks(lb):
    import ctypes as C
    from lbaudiodetective_amd import _native as N
    L = N.lib()
    out = (N.UInt32 * 21)()
    lens, counts = (N.UInt32 * 1)(20), (N.UInt64 * 1)(10)
    ok = L.LBAudioDetectiveDebugSlidingChoice(lens, counts, 1, 200, 20, 0, 200, 5, 1, 0, 0, 1, 256, out, 21)
    assert ok == 0 and out[0] == 1
    for args in ((lens, counts, 1, 200, 20, 0, 200, 0, 1, 0, 0, 1, 256, out, 21),      # no query
                 (lens, counts, 1, 200, 20, 0, 200, 5, 0, 0, 0, 1, 256, out, 21),      # none left
                 (lens, counts, 1, 200, 20, 0, 200, 5, 1, 0, 0, 1, 0, out, 21),        # no compute unit
                 (lens, counts, 1, 200, 20, 0, 201, 5, 1, 0, 0, 1, 256, out, 21),      # length the scan does not take
                 (lens, counts, 1, 200, 20, 0, 200, 5, 1, 0, 0, 1, 256, out, 20),      # capacity
                 (lens, counts, 1, 200, 20, 0, 200, 5, 1, 0, 0, 1, 256, None, 21)):
        assert L.LBAudioDetectiveDebugSlidingChoice(*args) != 0, args[7:]
