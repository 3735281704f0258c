"""CPU checks of the timeline tail (every channel's timeline kept current from each push): the two symbols and their declared
signatures, the Python names, the two files in the build, every refusal that needs neither a device nor a handle (the overlap of
inPrevKeys and outKeys among them, and that they come before the no-device status), the no-device status, the host plan
(LBAudioDetectiveDebugTimelineTailPlan) against a restatement of it over a grid and at the named shapes, the compiled kernels of
k_timeline_tail.hip (no private segment, no register spilled), and the tests' reference against timeline_ref: rolling from a seed
along random push schedules equals the timeline of every window, and counts above max_new differ exactly as the header states."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import occurrences_tail_ref as tail
import timeline_ref
import timeline_tail_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "lbaudiodetective.h")
CSRC = os.path.join(ROOT, "lbaudiodetective_amd", "csrc")

CALL = "LBAudioDetectiveCorpusRecordingPackedTimelineTailBatchKeysDevice"
PLAN = "LBAudioDetectiveDebugTimelineTailPlan"

# what the header states
WALK, THREADS, REC_BYTES, SLOT_BYTES, TRI_BYTES, MAX_NEW = 64, 256, 36, 8, 5151 * 4, 64
LDS_BUDGET = 160 * 1024 - 64
MAX_ITEMS = 0xFFFFFFFF - 4096
DEFAULT_LIMIT = 256 << 20
MAX_RECS = 65535
FIELDS = ("lanes", "recordings_per_workgroup", "window_records", "strip_width", "lds_bytes", "recordings_per_pass", "scratch_bytes")


def _has_gpu():
    return torch.cuda.is_available()


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
    want = {
        CALL: ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "const void*", "UInt32", "UInt32", "Float32", "UInt64",
               "const void*", "void*", "void*", "void*"],
        PLAN: ["UInt32", "UInt32", "UInt32", "UInt32", "UInt64", "UInt32", "UInt64", "UInt32*", "UInt32*", "UInt32*", "UInt32*", "UInt64*",
               "UInt32*", "UInt64*"],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [types[p] for p in params], (name, args)
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    assert re.search(CALL + r"\s*\([^)]*Float32\s+inThreshold,\s*UInt64\s+inIndexBase,\s*const void\*\s*inPrevKeys\s*,\s*void\*\s*outKeys,"
                     r"\s*void\*\s*outLengths\s*,\s*void\*\s*inStream\)", text)
    # the header states the invariant, what a count above the bound does, and how shards merge
    doc = " ".join(open(HEADER).read().split())
    for phrase in ("INVARIANT: seed inPrevKeys with LBAudioDetectiveCorpusRecordingPackedTimelineBatchKeysDevice", "bit for bit",
                   "A count ABOVE inMaxNew still shifts by the true count but adds only the newest",
                   "shards merge by element-wise unsigned maximum", "overlapping [outKeys"):
        assert phrase in doc, phrase
    # no status constant was added
    assert len(lb._native.declared_symbols()[1]) == 10


def test_python_names(lb):
    assert callable(lb.Corpus.recording_timeline_tail_batch_keys_device)
    for name in ("debug_timeline_tail_plan", "LiveTimeline"):
        assert callable(getattr(lb, name)) and name in lb.__all__, name
    for name in ("update", "segments", "reseed"):
        assert callable(getattr(lb.LiveTimeline, name)), name
    doc = " ".join(lb.LiveTimeline.__doc__.split())
    assert "reseed() after entries were removed from the corpus" in doc and "channel was reset" in doc
    with pytest.raises(ValueError):
        lb.LiveTimeline(None, None, [0], 10, 0.5, max_new=65)


def test_the_files_are_built():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_timeline_tail\.hip\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bapi_timeline_tail\.cpp\b", text, re.M)
    src = open(os.path.join(CSRC, "k_timeline_tail.hip")).read()
    assert '#include "occurrences_tail_common.hpp"' in src           # the tail mapping and ot_cell as they are
    for used in ("ot_lane(", "ot_stage(", "ot_cell<", "atomicMax("):
        assert used in src, used


# ---- the refusals ----------------------------------------------------------------------------------------------------------------
def _fakes():
    buf = (C.c_uint64 * 64)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    return buf, p, C.c_void_p(p)          # ... and for a corpus handle


TOO_MANY = ((1, 1 << 31), (2, 1 << 30), (1 << 16, 1 << 15), (0xFFFFFFFF, 0xFFFFFFFF), (3, 715827883))
NAN, INF = float("nan"), float("inf")
FAR = 1 << 40                             # an address far from every other: no block of the shapes below reaches it


def _call(lb):
    L_ = lb.lib()

    def call(c, rows, R, per, new, max_new, prev, keys, lengths, t=0.5, base=0):
        return getattr(L_, CALL)(c, rows, R, per, new, max_new, 0, t, base, prev, keys, lengths, None)
    return call


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle -- also on a machine without a GPU, where a
    call that passes them reports the missing device: they come first -- with a handle that is never read."""
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, p, fake = _fakes()
    call = _call(lb)
    keys = p + FAR
    for lengths in (p, None):                                        # outLengths may be NULL: it changes no refusal
        for prev in (p, None):                                       # ... and so may inPrevKeys
            assert call(None, p, 2, 3, p, 4, prev, keys, lengths) == bad
            assert call(fake, None, 2, 3, p, 4, prev, keys, lengths) == bad
            assert call(fake, p, 2, 3, None, 4, prev, keys, lengths) == bad                  # a NULL inNewCounts
            assert call(fake, p, 2, 3, p, 4, prev, None, lengths) == bad                     # a NULL outKeys
            for off in (1, 2, 3, 5, 7):
                assert call(fake, p, 2, 3, p + off, 4, prev, keys, lengths) == bad, off      # inNewCounts not 4-byte aligned
            for max_new in (0, MAX_NEW + 1, 1 << 20, 0xFFFFFFFF):
                assert call(fake, p, 2, 3, p, max_new, prev, keys, lengths) == bad, max_new
            for t in (0.0, -0.5, NAN, INF, -INF):
                assert call(fake, p, 2, 3, p, 4, prev, keys, lengths, t=t) == bad, t
            assert call(fake, p, 2, 3, p, 4, prev, keys, lengths, base=(1 << 32) + 1) == bad  # an index base no corpus fits behind
            assert call(fake, p, 0, 3, p, 4, prev, keys, lengths) == bad                     # no recordings
            assert call(fake, p, 2, 0, p, 4, prev, keys, lengths) == bad                     # no sub-fingerprints
            for R, per in TOO_MANY:
                assert R * per > (1 << 31) - 1
                assert call(fake, p, R, per, p, 4, prev, keys, lengths) == bad, (R, per)
        # [inPrevKeys, + R x n x 8) meets [outKeys, + R x n x 8): the same block, either one a word into the other, the last byte
        R, per = 2, 3
        size = R * per * 8
        for delta in (0, 8, -8, size - 8, -(size - 8), size - 1, -(size - 1), 1):
            assert call(fake, p, R, per, p, 4, keys + delta, keys, lengths) == bad, delta


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_the_entry_point_fails_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks the call reports kLBAudioDetectiveDeviceUnavailable (and still reads no
    handle), with and without inPrevKeys and outLengths, with inNewCounts 4-byte but not 8-byte aligned, at both ends of inMaxNew
    and the index base, and with the two blocks touching but not meeting."""
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, p, fake = _fakes()
    call = _call(lb)
    keys = p + FAR
    for lengths in (p, None):
        for (R, per) in ((1, 1), (1, (1 << 31) - 1), (1 << 15, (1 << 16) - 1), (3, 715827882), (1 << 21, 1)):
            size = R * per * 8
            for prev in (None, keys + size, keys - size, p):
                for max_new in (1, 5, MAX_NEW):
                    for new in (p, p + 4):
                        for t, base in ((0.5, 0), (1e-30, 1 << 32), (1.5, 7)):
                            assert call(fake, p, R, per, new, max_new, prev, keys, lengths, t=t, base=base) == nogp, (R, per, max_new, t)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def _restated(R, per, ne_min, ne_max, entries, max_new, limit):
    """the plan as the header states it; None where the limit holds no strip"""
    lim = limit or DEFAULT_LIMIT
    lanes = 1
    while lanes < max_new:
        lanes *= 2
    ne_b = min(ne_max, per)
    win = min(per, ne_b + lanes - 1)
    width = ne_b - ne_min + lanes if entries and 1 <= ne_min <= ne_b else 0
    one = win * REC_BYTES + width * SLOT_BYTES
    rpw = min(THREADS // lanes, (LDS_BUDGET - TRI_BYTES - 4) // one) if one else THREADS // lanes
    lds = -(-(rpw * win * REC_BYTES + TRI_BYTES) // 8) * 8 + rpw * width * SLOT_BYTES
    rpp, scratch = R, 0
    if width:
        if lim < width * SLOT_BYTES:
            return None
        rpp = min(R, MAX_RECS, MAX_ITEMS // -(-entries // WALK), lim // (width * SLOT_BYTES))
        scratch = rpp * width * SLOT_BYTES
    return dict(zip(FIELDS, (lanes, rpw, win, width, lds, rpp, scratch)))


def _plan_or_none(lb, *args):
    try:
        return lb.debug_timeline_tail_plan(*args)
    except lb.LBAudioDetectiveError as e:
        assert e.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
        return None


GRID = [(R, per, ne_min, ne_max, entries, max_new)
        for R in (1, 9, 1024, 70000)
        for per in (1, 48, 77, 256, 1030, 2400)
        for (ne_min, ne_max) in ((1, 1), (1, 40), (20, 70), (49, 300), (1, 1024), (1000, 1024), (1024, 1024))
        for entries in (0, 1, 150, 2000, 5000000)
        for max_new in (1, 5, 8, 33, 64)]


def test_plan_over_a_grid(lb):
    """the plan equals its restatement under limits that give one, a few and all recordings a pass and under one too small; lanes
    and windows are the tail occurrences plan's; the LDS holds windows, table and strips within the budget with at least one
    recording a workgroup, and one more would not fit wherever fewer than 256 / lanes are taken"""
    one, few, every, refused, lowered, below_tail, no_strip = 0, 0, 0, 0, 0, 0, 0
    for (R, per, ne_min, ne_max, entries, max_new) in GRID:
        if R * per > (1 << 31) - 1:
            continue
        shape = lb.debug_occurrences_tail_plan(R, per, ne_min, ne_max, entries, max_new)
        width = _restated(R, per, ne_min, ne_max, entries, max_new, 0)["strip_width"]
        for limit in sorted({0, 1, max(1, width * 8 - 1), max(1, width * 8), 3 * width * 8 + 7, max(1, R * width * 8), 1 << 20}):
            case = (R, per, ne_min, ne_max, entries, max_new, limit)
            want = _restated(*case)
            p = _plan_or_none(lb, *case)
            assert p == want, (case, p, want)
            if p is None:
                refused += 1
                continue
            assert p["lanes"] == shape["lanes"] and p["window_records"] == shape["window_records"], case
            rpw, rpp, w = p["recordings_per_workgroup"], p["recordings_per_pass"], p["strip_width"]
            assert 1 <= rpw <= shape["recordings_per_workgroup"] and p["lds_bytes"] <= LDS_BUDGET, case
            assert p["lds_bytes"] >= rpw * (p["window_records"] * REC_BYTES + w * SLOT_BYTES) + TRI_BYTES, case
            assert rpw == THREADS // p["lanes"] or \
                (rpw + 1) * (p["window_records"] * REC_BYTES + w * SLOT_BYTES) + TRI_BYTES + 4 > LDS_BUDGET, case
            assert 1 <= rpp <= R and p["scratch_bytes"] == rpp * w * 8 <= (limit or DEFAULT_LIMIT), case
            if w:
                assert w == min(ne_max, per) - ne_min + p["lanes"] and -(-entries // WALK) * -(-rpp // rpw) <= MAX_ITEMS, case
                assert rpp <= MAX_RECS, case
                if R >= 9:
                    one += rpp == 1
                    few += rpp == 3
                    every += rpp == R
            else:
                assert (entries == 0 or ne_min > per) and rpp == R, case     # nothing but the finish to launch
                no_strip += 1
            lowered += rpw < THREADS // p["lanes"]
            below_tail += rpw < shape["recordings_per_workgroup"]
    assert min(one, few, every, refused, lowered, below_tail, no_strip) > 50, (one, few, every, refused, lowered, below_tail, no_strip)


def test_plan_of_the_named_shapes(lb):
    plan = lb.debug_timeline_tail_plan
    tail_plan = lb.debug_occurrences_tail_plan
    # the monitor's shape: eight lanes a recording, windows of 70 + 8 - 1 records, strips of 70 - 20 + 8 slots, all windows in one pass
    p = plan(1024, 256, 20, 70, 2000, 5)
    assert p == dict(zip(FIELDS, (8, 32, 77, 58, 32 * 77 * 36 + TRI_BYTES + 4 + 32 * 58 * 8, 1024, 1024 * 58 * 8)))
    assert plan(1024, 256, 20, 70, 100000, 5) == p                  # the strips do not grow with the entries
    # D = 1, 8 and 64 lanes
    for max_new, lanes in ((1, 1), (8, 8), (64, 64), (33, 64)):
        p = plan(9, 256, 1, 40, 150, max_new)
        assert (p["lanes"], p["strip_width"], p["window_records"]) == (lanes, 40 - 1 + lanes, 40 + lanes - 1)
    # the longest entry a corpus may hold against the shortest: the strips take a sub-window's place
    p, q = plan(4, 2000, 1, 1024, 10, 64), tail_plan(4, 2000, 1, 1024, 10, 64)
    assert (p["recordings_per_workgroup"], q["recordings_per_workgroup"], p["strip_width"], p["window_records"]) == (2, 3, 1087, 1087)
    assert p["lds_bytes"] == 2 * 1087 * 36 + TRI_BYTES + 4 + 2 * 1087 * 8 <= LDS_BUDGET < p["lds_bytes"] + 1087 * 44
    p, q = plan(4, 2000, 1, 512, 10, 1), tail_plan(4, 2000, 1, 512, 10, 1)
    assert (p["recordings_per_workgroup"], q["recordings_per_workgroup"], p["strip_width"]) == (6, 7, 512)
    # the GPU tests' shapes, and limits that force passes of four, two and one recording
    p = plan(9, 48, 1, 300, 150, 8)
    assert (p["lanes"], p["recordings_per_workgroup"], p["window_records"], p["strip_width"], p["recordings_per_pass"]) == (8, 32, 48, 55, 9)
    assert plan(5, 80, 1, 300, 150, 64)["strip_width"] == 80 - 1 + 64 and plan(5, 80, 1, 300, 150, 64)["recordings_per_workgroup"] == 4
    for limit, rpp in ((4 * 55 * 8 + 9, 4), (2 * 55 * 8, 2), (55 * 8, 1)):
        p = plan(9, 48, 1, 300, 150, 8, limit)
        assert p["recordings_per_pass"] == rpp and p["scratch_bytes"] == rpp * 55 * 8 <= limit
    # a limit that is too small
    with pytest.raises(lb.LBAudioDetectiveError) as err:
        plan(9, 48, 1, 300, 150, 8, 55 * 8 - 1)
    assert err.value.status == lb.constant("kLBAudioDetectiveArgumentInvalid")
    # more recordings than a pass may hold
    assert plan(70000, 1, 1, 1, 10, 1)["recordings_per_pass"] == MAX_RECS
    # an empty corpus, or no entry that takes part: no strip, nothing to launch but the finish, whatever the limit
    for args in ((7, 100, 0, 0, 0, 8, 1), (7, 48, 49, 300, 2, 8, 1)):
        p = plan(*args)
        assert (p["strip_width"], p["scratch_bytes"], p["recordings_per_pass"]) == (0, 0, 7)


def test_plan_refusals(lb):
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    for args in ((0, 100, 1, 40, 133, 8), (5, 0, 1, 40, 133, 8), (1 << 16, 1 << 15, 1, 40, 133, 8), (5, 100, 1, 1025, 133, 8),
                 (5, 100, 0, 40, 133, 8), (5, 100, 41, 40, 133, 8), (5, 100, 1, 40, (1 << 32) + 1, 8), (5, 100, 1, 40, 133, 0),
                 (5, 100, 1, 40, 133, MAX_NEW + 1)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            lb.debug_timeline_tail_plan(*args)
        assert err.value.status == refused, args
    N = lb._native
    out = [N.UInt32(0), N.UInt32(0), N.UInt32(0), N.UInt32(0), N.UInt64(0), N.UInt32(0), N.UInt64(0)]
    for missing in range(len(out)):
        ptrs = [None if i == missing else C.byref(o) for i, o in enumerate(out)]
        assert getattr(lb.lib(), PLAN)(5, 100, 1, 40, 133, 8, 0, *ptrs) == refused


# ---- the compiled kernels ----------------------------------------------------------------------------------------------------
def _makefile_flags(stem):
    """CXXFLAGS and FLAGS_<stem> as lbaudiodetective_amd/csrc/Makefile sets them: the build that is shipped"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")

    def var(name):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % re.escape(name), text, re.M)
        return m.group(1).split() if m else []

    arch = (var("ARCH") or ["gfx950"])[0]
    return [f.replace("$(ARCH)", arch) for f in var("CXXFLAGS") + var("FLAGS_" + stem)]


def test_the_kernels_use_no_scratch(tmp_path):
    """k_timeline_tail.hip compiles for gfx950 with the flags read from the Makefile; its two kernels report 0 bytes of private
    segment, no spilled register, scalar or vector, and no static LDS (windows, table and strips are the launch's); the compute
    kernel keeps within 64 vector registers, as recording_tail_kernel does: eight waves a SIMD fit 512 / 8 = 64"""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_timeline_tail.s"
    src = os.path.join(CSRC, "k_timeline_tail.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_timeline_tail") + \
          ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.agpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                         r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(3)] = tuple(int(m.group(i)) for i in (1, 2, 4, 5, 6, 7))
    assert len(meta) == 2, sorted(meta)
    for name, (agpr, static_lds, private, sgpr_spill, vgpr, vgpr_spill) in meta.items():
        assert (agpr, static_lds, private, sgpr_spill, vgpr_spill) == (0, 0, 0, 0, 0), name
        assert 0 < vgpr <= 64, (name, vgpr)
    assert any("timeline_tail_cells_kernel" in n for n in meta) and any("timeline_tail_finish_kernel" in n for n in meta)


# ---- the reference against the timeline's ----------------------------------------------------------------------------------------
def _bools(rng, n, length=32):
    return rng.integers(0, 2, (n, length)).astype(np.uint8)


N_WIN, MAXN = 24, 4
ENTRY_LENGTHS = (1, 2, 3, 7, 7, 12, 23, 24, 25, 60)                  # 24 is the window; 25 and 60 never take part


def _recording(rng):
    ent = [_bools(rng, n) for n in ENTRY_LENGTHS]
    ent[4] = ent[3].copy()                                           # the same entry twice: ties go to the lower index
    total = 160
    rec = _bools(rng, total)
    for at, j in ((5, 3), (30, 5), (31, 2), (60, 6), (61, 3), (100, 7), (130, 5), (150, 3), (total - 2, 1)):
        rec[at:at + len(ent[j])] = ent[j]
    return ent, rec


def _profiles_of_the_whole(rec, ent):
    """per entry the profile over the WHOLE recording: a window's cells are a slice of it, which is the fold's premise"""
    return timeline_ref.profiles(rec, ent)


def _timeline_of(whole, ent, end, n, t, base=0):
    """timeline_ref.fold of the window rec[end - n:end], its profiles cut out of the whole recording's"""
    profs = []
    for e, p in zip(ent, whole):
        if p is None or len(e) > n:
            profs.append(None)
        else:
            profs.append((p[0], p[1][end - n:end - len(e) + 1]))
    return timeline_ref.fold(n, profs, t, base)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rolling_from_a_seed_is_the_timeline_of_every_window(seed):
    """a recording of 160 sub-fingerprints with planted entries, a window of 24 and random push schedules with the counts 0, 1,
    max_new and more than the window among them: rolled from a seed the state is timeline_ref's keys and lengths of every window,
    at a threshold most cells miss and at one most cells reach, with an index base; a count above max_new differs exactly by the
    cells between the newest max_new and the true count, and the state is whole again once they have slid out"""
    rng = np.random.default_rng(seed)
    ent, rec = _recording(rng)
    lengths = [len(e) for e in ent]
    whole = _profiles_of_the_whole(rec, ent)
    cells = np.sort(np.concatenate([p[1] for p in whole if p is not None]))
    # (a window's profile is a slice of the whole recording's: a cell depends on the sub-fingerprints under it alone)
    ne, cut = whole[5]
    assert np.array_equal(timeline_ref.profiles(rec[40:40 + N_WIN], [ent[5]])[0][1], cut[40:40 + N_WIN - ne + 1])
    for t, base in ((cells[int(len(cells) * 0.97)], 0), (cells[len(cells) // 2], 1000), (np.float32(1.0), 0)):
        assert t > 0
        end = N_WIN
        keys, lens = timeline_ref.timeline(rec[:N_WIN], ent, t, 0, base)
        assert np.array_equal(keys, _timeline_of(whole, ent, end, N_WIN, t, base)[0])
        schedule = [0, 1, MAXN, 2, 3, 0, MAXN, 1] + rng.integers(0, MAXN + 1, 40).tolist()
        survived = shifted = 0
        for step, new in enumerate(schedule):
            if end + new > len(rec):
                break
            end += new
            window = rec[end - N_WIN:end]
            before = keys
            keys, lens = ref.update(keys, window, ent, new, MAXN, t, 0, base)
            want = _timeline_of(whole, ent, end, N_WIN, t, base)
            assert np.array_equal(keys, want[0]) and np.array_equal(lens, want[1]), (seed, step, new)
            if step == 2:                                            # (three windows restated in full by timeline_ref itself)
                full = timeline_ref.timeline(window, ent, t, 0, base)
                assert np.array_equal(full[0], want[0]) and np.array_equal(full[1], want[1])
            if new == 0:
                assert np.array_equal(keys, before)
            survived += int(new > 0 and ((keys[:N_WIN - new] == before[new:]) & (before[new:] != 0)).any())
            shifted += new
        assert shifted > N_WIN and survived > 5
        # a count of the whole window and more: nothing of the previous state survives, the newest max_new cells alone are added
        for new in (N_WIN, N_WIN + 9):
            end2 = end - 40
            state = _timeline_of(whole, ent, end2, N_WIN, t, base)[0]
            got, got_len = ref.update(state, rec[end2 + new - N_WIN:end2 + new], ent, new, MAXN, t, 0, base)
            only = ref.strip(rec[end2 + new - N_WIN:end2 + new], ent, MAXN, t, 0, base)
            assert np.array_equal(got, only) and np.array_equal(got_len, ref.lengths_of(only, lengths, base))
            whole_again = ref.update(None, rec[end2 + new - N_WIN:end2 + new], ent, N_WIN, 64, t, 0, base)[0]
            assert np.array_equal(whole_again, _timeline_of(whole, ent, end2 + new, N_WIN, t, base)[0])


def test_a_count_above_max_new_lacks_exactly_the_cells_in_between():
    rng = np.random.default_rng(7)
    ent, rec = _recording(rng)
    whole = _profiles_of_the_whole(rec, ent)
    t = np.sort(np.concatenate([p[1] for p in whole if p is not None]))[-400]
    end, new = 70, 9
    state = _timeline_of(whole, ent, end, N_WIN, t)[0]
    end += new
    window = rec[end - N_WIN:end]
    want = _timeline_of(whole, ent, end, N_WIN, t)[0]
    got, _ = ref.update(state, window, ent, new, MAXN, t)
    # shifted by the true count, the newest max_new cells added: what is missing are the cells of the 5 pushes' worth in between
    between = [(j, o, q) for (j, o, q) in tail.tail_cells(window, ent, new) if o not in tail.tail_range(N_WIN, len(ent[j]), MAXN)]
    missing = ref.strip_of_cells(N_WIN, between, t)
    assert missing.any() and not np.array_equal(got, want)
    assert np.array_equal(np.maximum(got, missing), want)
    differ = np.flatnonzero(got != want)
    assert np.all(got[differ] < want[differ]) and np.all(missing[differ] == want[differ])
    # once `window` more sub-fingerprints have come in pushes within the bound, the row is whole again
    keys = got
    for new in (4, 4, 4, 4, 4, 4):
        end += new
        keys, _ = ref.update(keys, rec[end - N_WIN:end], ent, new, MAXN, t)
    assert np.array_equal(keys, _timeline_of(whole, ent, end, N_WIN, t)[0])


def test_the_length_lookup_and_the_roll():
    one = 0x3F800000
    keys = np.array([0, (one << 32) | (0xFFFFFFFF - 1002), (one << 32) | (0xFFFFFFFF - 1005), (one << 32) | (0xFFFFFFFF - 999),
                     (one << 32) | 0xFFFFFFFF], np.uint64)
    # a zero key, entry 2, an index behind the corpus, one in front of the index base (wraps), index -1000 (wraps)
    assert ref.lengths_of(keys, [5, 6, 7, 8], 1000).tolist() == [0, 7, 0, 0, 0]
    assert ref.lengths_of(keys[-1:], [5, 6, 7, 8], 0).tolist() == [5]
    prev = np.arange(1, 7, dtype=np.uint64)
    strip = np.array([0, 0, 9, 0, 0, 2], np.uint64)
    assert ref.roll(prev, 0, strip).tolist() == [1, 2, 9, 4, 5, 6]
    assert ref.roll(prev, 2, strip).tolist() == [3, 4, 9, 6, 0, 2]
    assert ref.roll(prev, 6, strip).tolist() == strip.tolist() == ref.roll(None, 3, strip).tolist()
