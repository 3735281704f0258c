"""CPU check of the ONE decision behind every batch call (api_detective.cpp: stage1_choose, and the instance functions the
launchers of k_fft_bands.hip, k_rows_full.hip and k_rows_stream2.hip dispatch on): whether the call launches, which stage-1
kernel and template instance, full or compact rows between the stages, which stage 2.  Every kernel returns the same bits, so
no parity test notices a configuration routed to another kernel; tests/golden/stage1_choice.json pins the routing as it was
recorded when the decision moved into one function, from the routing that shipped (tools/record_stage1_choice.py).  The library
must reproduce the file exactly.  The grid also decides which instances of tests/test_gpu_stage1_instances.py's inventory the
public settings can reach, and every case of that file has its routing checked here as well.  Needs no GPU."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage1_choice.json")
sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_stage1_choice as recorder                    # noqa: E402  (the grid itself: the file must be the grid's)
import test_gpu_stage1_instances as instances              # noqa: E402  (the inventory and the cases; importing needs no GPU)

N_WORDS = 12
ARGS = {0: 3, 1: 1, 2: 3, 3: 4, 4: 1}                       # template arguments per family
FAMILIES = ("generic", "pruned", "stream2", "full", "stream")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _instance(words):
    return (FAMILIES[words[2]],) + tuple(words[3:3 + ARGS[words[2]]])


def test_grid_holds_every_boundary(golden):
    rows = golden["rows"]
    assert golden["inputs"] == recorder.INPUTS and len(rows) < 1000 and os.path.getsize(GOLDEN) < (1 << 20)
    assert [tuple(r[:len(recorder.INPUTS)]) for r in rows] == recorder.grid()
    col = {name: i for i, name in enumerate(golden["inputs"])}
    values = lambda name: {r[col[name]] for r in rows}
    assert values("window") >= {16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192}
    assert values("stride") >= {1, 2, 6, 8, 63, 64, 65, 100, 200, 254, 1024, 1026}
    assert values("bands") >= {1, 16, 32, 33, 64}
    assert values("rate") >= {4000, 5512, 8000, 11025, 16000, 22050, 44100, 48000, 96000}
    assert values("fmt") >= {0, 1, 2} and values("variant") == {0, 1, 2, 3, 4} and values("n_clips") >= {1, 3}
    assert values("extra") >= {0, 1} and values("address_mod8") >= {0, 4} and values("tap") == {0, 1} and values("tail") == {0, 1}
    assert values("waves") == set(recorder.TUNING_WAVES) and values("cache") == {0, 1}
    words = [r[len(col):] for r in rows]
    assert all(len(w) == N_WORDS for w in words)
    live = [(r, w) for r, w in zip(rows, words) if w[1]]
    # both statuses, calls without a frame, compact rows, every stage 2, tunings that fell back by either word, and per window
    # size of the generic kernel a tuning that was taken and one that was not
    assert {w[0] for w in words} == {0, 1} and any(w[0] == 0 and not w[1] for w in words)
    assert {w[7] for _, w in live} == {0, 1} and {w[8] for _, w in live} == {0, 1, 2}
    assert any(w[9] for _, w in live) and any(w[10] and not w[9] for _, w in live)
    for log2w in range(4, 14):
        tuned = [w for r, w in live if w[2] == 0 and w[3] == log2w and r[col["waves"]]]
        assert any(not w[9] and not w[10] for w in tuned), log2w
        assert any(w[9] for w in tuned), log2w
    # the uncached instance taken AUTOMATICALLY exists (window 8192): tests/test_gpu_stage1_instances.py has a case for it
    assert any(w[10] and r[col["waves"]] == 0 and r[col["cache"]] == 1 for r, w in live)


def test_grid_reaches_exactly_the_inventory(golden):
    """What "unreachable" means: an instance of the inventory that no row of the grid takes."""
    n_in = len(golden["inputs"])
    reached = {_instance(r[n_in:]) for r in golden["rows"] if r[n_in + 1]}
    assert reached == instances.INVENTORY - set(instances.UNREACHABLE), (sorted(reached - instances.INVENTORY),
                                                                         sorted(instances.INVENTORY - reached))


def test_library_reproduces_the_recorded_choice(lb, golden):
    n_in = len(golden["inputs"])
    bad = []
    for r in golden["rows"]:
        got = recorder.choice_words(lb, r[:n_in])
        if got != r[n_in:]:
            bad.append((r[:n_in], got, r[n_in:]))
    assert not bad, (len(bad), bad[:3])


def test_every_instance_has_a_gpu_case():
    instances.test_every_instance_has_a_case()


def test_gpu_cases_route_as_they_name(lb):
    """Assertion 1 of every GPU case, here with the address the case's shape gives a tensor (allocations are 256-byte aligned)."""
    for case in instances.CASES:
        rate, window, stride, bands, subfp_len = case.cfg
        det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=subfp_len)
        instances.check_routing(lb, det, case, instances.case_shape(case)[2])


def test_wrapper_names_the_words(lb):
    ch = lb.debug_stage1_choice(44100, 1024, 64, 32, 200, fmt=1, n_clips=3, samples_per_clip=1024 + 64 * 128 * 2)
    assert (ch.status, ch.launches, ch.family, ch.args, ch.compact, ch.stage2, ch.fell_back, ch.per) == \
        (0, True, "pruned", (1,), True, "select32_sparse", False, 2)
    ch = lb.debug_stage1_choice(44100, 1024, 64, 32, 200, fmt=1, n_clips=3, samples_per_clip=1024 + 64 * 128 * 2, taps=True)
    assert (ch.compact, ch.stage2) == (False, "select32")
    ch = lb.debug_stage1_choice(8000, 64, 16, 7, 33, variant=2, n_clips=1, samples_per_clip=64 + 16 * 128)
    assert (ch.status, ch.launches, ch.family) == (1, False, None)          # no specialised kernel: ArgumentInvalid
    ch = lb.debug_stage1_choice(8000, 64, 16, 7, 33, n_clips=1, samples_per_clip=64 + 16 * 128)
    assert (ch.family, ch.args, ch.stage2) == ("generic", (6, 4, 1), "generic")


def test_argument_checks(lb):
    from lbaudiodetective_amd import _native as N
    L = N.lib()
    out = (N.UInt32 * N_WORDS)()
    good = [44100.0, 1024, 64, 32, 200, 0, 0, 1, 0, 3, 1024 + 64 * 128, 0, 0, 0, out, N_WORDS]
    assert L.LBAudioDetectiveDebugStage1Choice(*good) == 0 and list(out)[:3] == [0, 1, 1]

    def with_(i, v):
        a = list(good)
        a[i] = v
        return a
    for args in (with_(14, None), with_(15, N_WORDS - 1), with_(5, 5), with_(6, 17), with_(11, 8)):
        assert L.LBAudioDetectiveDebugStage1Choice(*args) != 0, args[:14]
    # what the CALL would refuse is a word, not the report's own status
    for args in (with_(8, 3), with_(1, 1000), with_(2, 0), with_(4, 257), with_(0, 0.0)):
        assert L.LBAudioDetectiveDebugStage1Choice(*args) == 0 and list(out)[:2] == [1, 0], args[:14]
