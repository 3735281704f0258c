"""CPU checks of the tail peaks: the symbols and their declared signatures, the Python names, the kernel file in the build, the
refusals that need neither a device nor a handle, the no-device status, the plan symbol against the tail plan at max_new + 2, and
the tests' reference (occurrences_tail_peaks_ref) against recording_ref's peaks-on list: a window's row is that list filtered to the
judged cells, and a channel's life cut into pushes plus one final call gives every peak of the whole recording exactly once -- on
inputs that are asserted HERE to hold plateaus, also across a push boundary, so that a GPU pass cannot be vacuous."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import occurrences_tail_peaks_ref as ref
import recording_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lbaudiodetective.h")
CSRC = os.path.join(ROOT, "lbaudiodetective_amd", "csrc")

PEAKS = "LBAudioDetectiveCorpusQueryPackedOccurrencesTailPeaksBatchKeysDevice"
PLAN = "LBAudioDetectiveDebugOccurrencesTailPeaksPlan"
MAX_NEW = 62
ONE_BITS = 0x3F800000


def _prototype(name):
    """the parameter types of `name` as include/lbaudiodetective.h declares it, comments removed"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return m.group(1), [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(2).split(",")]


def test_symbols_exist_with_the_declared_signatures(lb):
    N = lb._native
    raw = C.CDLL(lb.LIB_PATH)
    types = {"LBAudioDetectiveCorpusRef": N.Ref, "void*": C.c_void_p, "const void*": C.c_void_p, "UInt32": N.UInt32, "UInt64": N.UInt64,
             "Float32": N.Float32, "UInt32*": C.POINTER(N.UInt32), "UInt64*": C.POINTER(N.UInt64)}
    dev = "void*"
    want = {
        PEAKS: ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "const void*", "UInt32", "UInt32", "UInt32", "Float32",
                "UInt64", "UInt64", dev, dev, dev, dev],
        PLAN: _prototype("LBAudioDetectiveDebugOccurrencesTailPlan")[1],
    }
    assert len(want[PLAN]) == 14
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [types[p] for p in params], (name, args)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(PEAKS + r"\s*\([^)]*inNewCounts,\s*UInt32\s+inMaxNew,\s*UInt32\s+inFinal,\s*UInt32\s+inRange,\s*Float32\s+inThreshold,"
                     r"\s*UInt64\s+inCapacity,\s*UInt64\s+inIndexBase,\s*void\*\s*outKeys,\s*void\*\s*outLags,\s*void\*\s*outCounts,"
                     r"\s*void\*\s*inStream\)", text)
    assert re.search(r"#define\s+LBAD_OCCURRENCES_TAIL_PEAKS_MAX_NEW\s+62\b", text)
    # the header states once-in-a-life and the two more sub-fingerprints of the window
    doc = " ".join(open(HEADER).read().split())
    assert "ONCE IN A CHANNEL'S LIFE" in doc and "longest entry + d_k + 1" in doc and "TWO sub-fingerprints more" in doc
    assert len(lb._native.declared_symbols()[1]) == 10               # no status constant was added


def test_python_names(lb):
    assert callable(lb.Corpus.query_packed_occurrences_tail_peaks_batch_keys_device) and callable(lb.StreamBank.new_peaks)
    assert callable(lb.debug_occurrences_tail_peaks_plan) and "debug_occurrences_tail_peaks_plan" in lb.__all__


def test_the_kernel_file_is_built():
    """the peaks kernels are instances of k_occurrences_tail.hip's kernel pair: that file is built, the peaks' own file is gone
    from the build and from the tree, and the surviving file instantiates the PEAKS form"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_occurrences_tail\.hip\b", text, re.M)
    assert not re.search(r"^SRCS\s*:=.*\bk_occurrences_tail_peaks\.hip\b", text, re.M)
    assert not os.path.exists(os.path.join(CSRC, "k_occurrences_tail_peaks.hip"))
    src = open(os.path.join(CSRC, "k_occurrences_tail.hip")).read()
    for kernel in ("occurrences_tail_count_kernel", "occurrences_tail_scatter_kernel"):
        assert re.search(r"template\s*<bool PEAKS>\s*__global__[^{;]*\b" + kernel + r"\b", src), kernel
        assert kernel + "<PEAKS>" in src, kernel
    assert re.search(r"\blaunch_ot<true>\(", src) and re.search(r"\blaunch_ot<false>\(", src)


def _fakes():
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    return buf, p, C.c_void_p(p)          # ... and for a corpus handle


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """decided before anything touches a device or a handle, also on a machine without a GPU"""
    peaks = getattr(lb.lib(), PEAKS)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, p, fake = _fakes()

    def call(c, rows, R, per, new, max_new, final, t, cap, base, keys, lags, counts):
        return peaks(c, rows, R, per, new, max_new, final, 0, t, cap, base, keys, lags, counts, None)

    for final in (0, 1, 7):
        for lags in (p, None):                                       # outLags may be NULL: it changes no refusal
            assert call(None, p, 2, 3, p, 4, final, 0.5, 4, 0, p, lags, p) == bad
            assert call(fake, None, 2, 3, p, 4, final, 0.5, 4, 0, p, lags, p) == bad
            assert call(fake, p, 2, 3, None, 4, final, 0.5, 4, 0, p, lags, p) == bad            # a NULL inNewCounts
            assert call(fake, p, 2, 3, p, 4, final, 0.5, 4, 0, None, lags, p) == bad
            assert call(fake, p, 2, 3, p, 4, final, 0.5, 4, 0, p, lags, None) == bad            # a NULL outCounts
            for off in (1, 2, 3, 5, 7):
                assert call(fake, p, 2, 3, p + off, 4, final, 0.5, 4, 0, p, lags, p) == bad, off
            for max_new in (0, MAX_NEW + 1, 64, 1 << 20, 0xFFFFFFFF):
                assert call(fake, p, 2, 3, p, max_new, final, 0.5, 4, 0, p, lags, p) == bad, max_new
            assert call(fake, p, 0, 3, p, 4, final, 0.5, 4, 0, p, lags, p) == bad
            assert call(fake, p, 2, 0, p, 4, final, 0.5, 4, 0, p, lags, p) == bad
            for t in (0.0, -0.5, float("nan"), float("inf")):
                assert call(fake, p, 2, 3, p, 4, final, t, 4, 0, p, lags, p) == bad, t
            for cap in (0, (1 << 31) + 1):
                assert call(fake, p, 1, 3, p, 4, final, 0.5, cap, 0, p, lags, p) == bad, cap
            assert call(fake, p, 2, 3, p, 4, final, 0.5, 4, (1 << 32) + 1, p, lags, p) == bad


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-device status needs a machine without a GPU")
def test_entry_point_fails_without_gpu(lb):
    """no CPU fallback: arguments that pass the checks report kLBAudioDetectiveDeviceUnavailable, at both ends of inMaxNew"""
    peaks = getattr(lb.lib(), PEAKS)
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, p, fake = _fakes()
    for lags in (p, None):
        for final in (0, 1):
            for max_new in (1, 5, MAX_NEW):
                for new in (p, p + 4):
                    assert peaks(fake, p, 3, 50, new, max_new, final, 0, 0.5, 10, 7, p, lags, p, None) == nogp, (max_new, final)


def test_the_plan_is_the_tail_plan_at_two_more(lb):
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    shapes = ((1024, 256, 20, 70, 2000, 0), (9, 48, 1, 300, 150, 0), (5, 80, 1, 300, 150, 24 + 128 * 24 + 8), (5, 320, 1, 300, 150, 0),
              (7, 100, 0, 0, 0, 0))
    lanes = {}
    for max_new in (1, 2, 6, 7, 30, 31, 62):
        for shape in shapes:
            args = shape[:5] + (max_new,) + shape[5:]
            tail = shape[:5] + (max_new + 2,) + shape[5:]
            got = lb.debug_occurrences_tail_peaks_plan(*args)
            assert got == lb.debug_occurrences_tail_plan(*tail), (args, got)
            lanes[max_new] = got["lanes"]
    assert lanes == {1: 4, 2: 4, 6: 8, 7: 16, 30: 32, 31: 64, 62: 64}        # D doubles where max_new + 2 crosses a power of two
    for max_new in (0, 63, 64):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            lb.debug_occurrences_tail_peaks_plan(9, 48, 1, 300, 150, max_new)
        assert err.value.status == refused, max_new
    # the monitor's shape keeps eight lanes a recording at five new sub-fingerprints: two more records of window
    p = lb.debug_occurrences_tail_peaks_plan(1024, 256, 20, 70, 2000, 5)
    assert (p["lanes"], p["recordings_per_workgroup"], p["window_records"]) == (8, 32, 77)


# ---- the reference against recording_ref -----------------------------------------------------------------------------------------------
def _low_entropy(rng, n, pool):
    """n sub-fingerprints drawn from a small pool, in runs: profiles with plateaus"""
    out = np.zeros((n, pool.shape[1]), np.uint8)
    at = 0
    while at < n:
        run = int(rng.integers(1, 6))
        out[at:at + run] = pool[rng.integers(0, len(pool))]
        at += run
    return out


def test_the_judged_rule():
    assert list(ref.judged_range(48, 17, 5, False)) == [26, 27, 28, 29, 30] and list(ref.judged_range(48, 17, 5, True)) == [26, 27, 28, 29, 30, 31]
    assert list(ref.judged_range(48, 44, 8, False)) == [0, 1, 2, 3] and list(ref.judged_range(48, 44, 8, True)) == [0, 1, 2, 3, 4]
    assert list(ref.judged_range(48, 48, 3, False)) == [] and list(ref.judged_range(48, 48, 3, True)) == [0]     # last == 0
    assert list(ref.judged_range(48, 17, 0, False)) == [] and list(ref.judged_range(48, 17, 0, True)) == [31]    # d == 0
    assert list(ref.judged_range(48, 49, 3, True)) == [] and list(ref.judged_range(48, 0, 3, True)) == []
    q = np.array([.5, .5, .7, .7, .7, .2, .9], np.float32)
    assert [ref.is_peak(q, o) for o in range(7)] == [True, False, True, False, False, False, True]               # a plateau: its first cell


def test_a_window_row_is_the_filtered_peaks_list():
    """a few hundred random shapes: the reference's row equals recording_ref's peaks-on list with only the judged cells kept"""
    rng = np.random.default_rng(41)
    pool = rng.integers(0, 2, (4, 32)).astype(np.uint8)
    plateaus = matches = clipped = finals = 0
    for case in range(300):
        n_q = int(rng.integers(1, 41))
        lengths = [int(x) for x in rng.integers(1, n_q + 3, 3)]
        entries = [_low_entropy(rng, n, pool) for n in lengths]
        rec = _low_entropy(rng, n_q, pool)
        d, final, range_ = int(rng.integers(0, 11)), bool(rng.integers(0, 2)), (0, 4, 2)[case % 3]
        profs = ref.profiles(rec, entries, range_)
        cells = ref.judged_cells(profs, n_q, min(d, n_q), final)
        values = np.array([q for (_j, _o, q, _p) in cells] + [1.0], np.float32)
        t = np.float32(max(np.quantile(values, 0.5), 1e-6))
        keys, lags, count = ref.peaks_row(cells, t, 64)
        assert count <= 64
        cs = recording_ref.cells(rec, entries, range_)
        all_k, all_l = recording_ref.occurrences_all(cs, t, True)
        keep = [i for i, (k, lag) in enumerate(zip(all_k, all_l))
                if lengths[0xFFFFFFFF - (int(k) & 0xFFFFFFFF)] <= n_q and lag <= 0 and
                -int(lag) in ref.judged_range(n_q, lengths[0xFFFFFFFF - (int(k) & 0xFFFFFFFF)], min(d, n_q), final)]
        assert np.array_equal(keys[:count], all_k[keep]) and np.array_equal(lags[:count], all_l[keep]), case
        assert not keys[count:].any() and not lags[count:].any()
        got = ref.filter_batch_row(all_k, all_l, len(all_k), lengths, n_q, min(d, n_q), final, 64)
        assert np.array_equal(got[0], keys) and np.array_equal(got[1], lags) and got[2] == count
        matches += count
        finals += final and count > 0
        clipped += any(n <= n_q and n_q - n - d < 0 for n in lengths)
        plateaus += sum(1 for (j, o, q, _p) in cells for (j2, o2, q2, _p2) in cells if j2 == j and o2 == o + 1 and q2 == q >= t)
    assert matches > 300 and plateaus > 100 and clipped > 50 and finals > 50


LIFE_LENGTHS = (1, 2, 7, 10, 17, 22, 39, 40, 90)


@pytest.mark.parametrize("range_", [0, 4, 2])
def test_a_life_gives_every_peak_exactly_once(range_):
    """a recording of 200 sub-fingerprints in random pushes of 0 .. 8 into windows of min(total, 49 + slack), then the final call:
    the union of the calls' matches at absolute positions is the peaks-on list of the whole recording for the entries of at most
    40, each cell once, with equal bits -- with runs of equal cells at or above the threshold, one of them across a push boundary"""
    rng = np.random.default_rng(12 + range_)
    pool = rng.integers(0, 2, (5, 32)).astype(np.uint8)
    entries = [rng.integers(0, 2, (n, 32)).astype(np.uint8) for n in LIFE_LENGTHS]
    for block in [pool] + entries:                                   # a non-zero pair inside every range: a verbatim copy scores 1.0
        block[:, 0] = block[:, 2] = 1
    entries[3][:] = pool[0]                                          # ten times one sub-fingerprint
    total, longest = 200, 40
    rec = _low_entropy(rng, total, pool)
    rec[100:130] = pool[0]                                           # ... against thirty of it: q = 1.0 at 100 .. 120
    rec[50:72] = entries[5]
    rec[total - 40:] = entries[7]                                    # ends at the last record: the final call's
    pushes = []
    while sum(pushes) < total:
        pushes.append(int(min(rng.integers(0, 9), total - sum(pushes))))
    assert 0 in pushes and 8 in pushes
    slack = int(rng.integers(0, 12))
    cells = ref.life_cells(rec, entries, pushes, lambda fed, d: longest + 8 + 1 + slack, range_)
    for (fed, n, d, _final) in ref.life_calls(pushes, lambda fed, d: longest + 8 + 1 + slack):
        assert n == fed or n >= longest + d + 1                      # the header's window condition
    short = [e if len(e) <= longest else np.zeros((total + 1, 32), np.uint8) for e in entries]     # (longer than the recording: no lag <= 0)
    cs = recording_ref.cells(rec, short, range_)
    values = np.sort(np.concatenate([q for (q, entry_long) in cs if not entry_long]))
    t = np.float32(values[int(len(values) * 0.6)])
    assert 0 < t <= 1
    keys, lags = recording_ref.occurrences_all(cs, t, True)
    want = sorted((0xFFFFFFFF - (int(k) & 0xFFFFFFFF), -int(lag), int(k) >> 32) for k, lag in zip(keys, lags) if lag <= 0)
    assert all(len(entries[j]) <= longest for (j, _o, _b) in want) and len(want) > 50
    seen = ref.life(cells, t)
    assert len(seen) == len(set(seen)), "a peak is reported twice"
    assert sorted(seen) == want
    assert not any(j == 8 for (j, _o, _b) in seen)

    def run_start(j, at):
        """the first cell of the run of 1.0 that holds cell `at` of entry j (a masked range may let it begin earlier)"""
        q = cs[j][0]
        assert q[at] == 1 and t <= 1
        while at > 0 and q[at - 1] == 1:
            at -= 1
        return at

    assert (5, run_start(5, 50), ONE_BITS) in seen and (7, run_start(7, total - 40), ONE_BITS) in seen
    # the run of 1.0 reports its first cell only, though calls judge its cells one push after another
    assert (cs[3][0][100:121] == 1).all()
    assert [o for (j, o, b) in seen if j == 3 and run_start(3, 100) <= o <= 120] == [run_start(3, 100)]
    judged = {(j, at): (k, q) for (k, j, at, q, _peak) in cells}
    assert len(judged) == len(cells)                                 # every cell is judged by exactly one call
    flat = [(j, at) for (j, at), (k, q) in judged.items() if (j, at + 1) in judged and judged[(j, at + 1)][1] == q >= t]
    across = [(j, at) for (j, at) in flat if judged[(j, at + 1)][0] != judged[(j, at)][0]]
    assert len(flat) >= 20 and any(j == 3 for (j, _at) in across), "the inputs hold no plateau across a push boundary"
