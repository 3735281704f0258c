"""CPU checks of the recording tail (the tail occurrences' cells folded per (recording, entry)): the four symbols and their declared
signatures, the Python names, the two files in the build, the refusals that need neither a device nor a handle (and that they come
before the no-device status), the no-device status, the host plan (LBAudioDetectiveDebugRecordingTailPlan) over a grid of shapes and
limits against a restatement of it, the compiled kernel of k_recording_tail.hip (registers, no scratch memory, no register spilled
to it), and the tests' reference against itself on a recording cut into pushes."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import occurrences_tail_ref as tail
import recording_tail_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "lbaudiodetective.h")
CSRC = os.path.join(ROOT, "lbaudiodetective_amd", "csrc")

SCORES = "LBAudioDetectiveCorpusRecordingPackedScoresTailBatchDevice"
TOPK = "LBAudioDetectiveCorpusQueryPackedRecordingTopKTailBatchKeysDevice"
THRESHOLD = "LBAudioDetectiveCorpusQueryPackedRecordingThresholdTailBatchKeysDevice"
PLAN = "LBAudioDetectiveDebugRecordingTailPlan"

# what the header states
WALK, THREADS, REC_BYTES, TRI_BYTES, MAX_NEW, TOPK_MAX = 64, 256, 36, 5151 * 4, 64, 1024
LDS_BUDGET = 160 * 1024 - 64
MAX_ITEMS = 0xFFFFFFFF - 4096
DEFAULT_LIMIT = 256 << 20
MAX_RECS = 65535
FIELDS = ("lanes", "recordings_per_workgroup", "window_records", "lds_bytes", "recordings_per_pass", "scratch_bytes")


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
             "Float32": N.Float32, "UInt32*": C.POINTER(N.UInt32), "UInt64*": C.POINTER(N.UInt64), "Float32*": C.c_void_p,
             "SInt32*": C.c_void_p}
    dev = "void*"
    head = ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "const void*", "UInt32", "UInt32"]
    want = {
        SCORES: head + ["Float32*", "SInt32*", dev],
        TOPK: head + ["UInt32", "UInt64", dev, dev, dev],
        THRESHOLD: head + ["Float32", "UInt64", "UInt64", dev, dev, dev, dev],
        PLAN: ["UInt32", "UInt32", "UInt32", "UInt64", "UInt32", "UInt64", "UInt32", "UInt32*", "UInt32*", "UInt32*", "UInt64*", "UInt32*",
               "UInt64*"],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [types[p] for p in params], (name, args)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    # the order of the threshold call's outputs is the batch recording threshold's: keys, counts, lags
    assert re.search(THRESHOLD + r"\s*\([^)]*void\*\s*outKeys,\s*void\*\s*outCounts,\s*void\*\s*outLags,\s*void\*\s*inStream\)", text)
    assert re.search(TOPK + r"\s*\([^)]*UInt32\s+inK,\s*UInt64\s+inIndexBase,\s*void\*\s*outKeys,\s*void\*\s*outLags,\s*void\*\s*inStream\)", text)
    # the header states the three consequences of the contract
    doc = " ".join(open(HEADER).read().split())
    for phrase in ("EQUIVALENCE with the tail occurrences call", "ONCE PER PUSH", "INDEPENDENCE", "-(the LOWEST tail offset whose q_o equals the score)"):
        assert phrase in doc, phrase
    # no status constant was added
    assert len(lb._native.declared_symbols()[1]) == 10


def test_python_names(lb):
    for name in ("recording_scores_tail_batch_device", "query_packed_recording_topk_tail_batch_keys_device",
                 "query_packed_recording_threshold_tail_batch_keys_device"):
        assert callable(getattr(lb.Corpus, name)), name
    assert callable(lb.StreamBank.new_best) and callable(lb.StreamBank.new_matches_above)
    for name in ("debug_recording_tail_plan", "decode_tail_matches", "decode_tail_occurrences"):
        assert callable(getattr(lb, name)) and name in lb.__all__, name


def test_the_files_are_built():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_recording_tail\.hip\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bapi_recording_tail\.cpp\b", text, re.M)
    # the helpers both tail files share live in ONE header
    for src in ("k_occurrences_tail.hip", "k_recording_tail.hip"):
        assert '#include "occurrences_tail_common.hpp"' in open(os.path.join(CSRC, src)).read(), src


def test_decode_tail_matches(lb):
    one, half = 0x3F800000, 0x3F000000
    keys = np.array([[(one << 32) | (0xFFFFFFFF - 1007), (half << 32) | (0xFFFFFFFF - 1002), 0],
                     [0, 0, 0]], np.uint64).view(np.int64)
    lags = np.array([[-13, 0, 0], [0, 0, 0]], np.int32)
    for counts in (None, [2, 0]):
        rows = lb.decode_tail_matches(keys, lags, [100, 90], 48, counts=counts, index_base=1000)
        assert rows[0][0].tolist() == [7, 2] and rows[0][1].tolist() == [1.0, 0.5] and rows[0][2].tolist() == [100 - 48 + 13, 100 - 48]
        assert all(len(a) == 0 for a in rows[1])
    with pytest.raises(ValueError):
        lb.decode_tail_matches(keys, lags, [100, 90], 48, counts=[1])


# ---- the refusals ----------------------------------------------------------------------------------------------------------------
def _fakes():
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    return buf, p, C.c_void_p(p)          # ... and for a corpus handle


TOO_MANY = ((1, 1 << 31), (2, 1 << 30), (1 << 16, 1 << 15), (0xFFFFFFFF, 0xFFFFFFFF), (3, 715827883))
NAN, INF = float("nan"), float("inf")


def _calls(lb):
    """the three calls behind one shape: f(c, rows, R, per, new, max_new, lags) with every other argument valid, and the name of
    each call's required output pointers"""
    L_ = lb.lib()
    _buf, p, _fake = _fakes()
    return {
        "scores": lambda c, rows, R, per, new, max_new, lags, out=p: getattr(L_, SCORES)(c, rows, R, per, new, max_new, 0, out, lags, None),
        "topk": lambda c, rows, R, per, new, max_new, lags, out=p, k=3, base=0:
            getattr(L_, TOPK)(c, rows, R, per, new, max_new, 0, k, base, out, lags, None),
        "threshold": lambda c, rows, R, per, new, max_new, lags, out=p, t=0.5, cap=4, base=0, counts=p:
            getattr(L_, THRESHOLD)(c, rows, R, per, new, max_new, 0, t, cap, base, out, counts, lags, None),
    }


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle -- also on a machine without a GPU, where a
    call that passes them reports the missing device: they come first -- with a handle that is never read."""
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, p, fake = _fakes()
    calls = _calls(lb)
    for lags in (p, None):                                           # outLags may be NULL: it changes no refusal
        for name, call in calls.items():
            assert call(None, p, 2, 3, p, 4, lags) == bad, name
            assert call(fake, None, 2, 3, p, 4, lags) == bad, name
            assert call(fake, p, 2, 3, None, 4, lags) == bad, name                       # a NULL inNewCounts
            assert call(fake, p, 2, 3, p, 4, lags, out=None) == bad, name                # a NULL outScores / outKeys
            for off in (1, 2, 3, 5, 7):
                assert call(fake, p, 2, 3, p + off, 4, lags) == bad, (name, off)         # inNewCounts not 4-byte aligned
            for max_new in (0, MAX_NEW + 1, 1 << 20, 0xFFFFFFFF):
                assert call(fake, p, 2, 3, p, max_new, lags) == bad, (name, max_new)
            assert call(fake, p, 0, 3, p, 4, lags) == bad, name                          # no recordings
            assert call(fake, p, 2, 0, p, 4, lags) == bad, name                          # no sub-fingerprints
            for R, per in TOO_MANY:
                assert R * per > (1 << 31) - 1
                assert call(fake, p, R, per, p, 4, lags) == bad, (name, R, per)
        topk, threshold = calls["topk"], calls["threshold"]
        for k in (0, TOPK_MAX + 1, 0xFFFFFFFF):
            assert topk(fake, p, 2, 3, p, 4, lags, k=k) == bad, k
        assert topk(fake, p, (1 << 21) + 1, 1, p, 4, lags, k=TOPK_MAX) == bad            # more than 2^31 slots
        assert topk(fake, p, 2, 3, p, 4, lags, base=(1 << 32) + 1) == bad                # an index base no corpus fits behind
        assert threshold(fake, p, 2, 3, p, 4, lags, counts=None) == bad                  # a NULL outCounts
        for t in (0.0, -0.5, NAN, INF, -INF):
            assert threshold(fake, p, 2, 3, p, 4, lags, t=t) == bad, t
        for cap in (0, (1 << 31) + 1, 1 << 40):
            assert threshold(fake, p, 1, 3, p, 4, lags, cap=cap) == bad, cap
        assert threshold(fake, p, 2, 3, p, 4, lags, base=(1 << 32) + 1) == bad
        for R, cap in ((2, (1 << 30) + 1), ((1 << 21) + 1, 1 << 10), (3, 1 << 30), (1 << 16, (1 << 15) + 1)):
            assert R * cap > 1 << 31
            assert threshold(fake, p, R, 1, p, 4, lags, cap=cap) == bad, (R, cap)        # more than 2^31 slots
    assert re.search(r"#define\s+LBAD_TOPK_MAX\s+%d\b" % TOPK_MAX, open(HEADER).read())


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks every call reports kLBAudioDetectiveDeviceUnavailable (and still reads
    no handle), with and without outLags, with inNewCounts 4-byte but not 8-byte aligned, at both ends of inMaxNew, K and the
    capacity."""
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, p, fake = _fakes()
    calls = _calls(lb)
    for lags in (p, None):
        for (R, per) in ((1, 1), (1, (1 << 31) - 1), (1 << 15, (1 << 16) - 1), (3, 715827882), (1 << 21, 1)):
            for max_new in (1, 5, MAX_NEW):
                for new in (p, p + 4):
                    assert calls["scores"](fake, p, R, per, new, max_new, lags) == nogp, (R, per, max_new)
                    for k in (1, TOPK_MAX):
                        assert calls["topk"](fake, p, R, per, new, max_new, lags, k=k, base=1 << 32) == nogp, (R, per, max_new, k)
                    for t, cap in ((0.5, 1), (1e-30, (1 << 31) // R), (1.5, 10)):
                        assert calls["threshold"](fake, p, R, per, new, max_new, lags, t=t, cap=cap) == nogp, (R, per, max_new, t, cap)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def _restated(R, per, ne_max, entries, max_new, limit, key_form):
    """the plan as the header states it"""
    lim = limit or DEFAULT_LIMIT
    lanes = 1
    while lanes < max_new:
        lanes *= 2
    win = min(per, min(ne_max, per) + lanes - 1)
    rpw = min(THREADS // lanes, (LDS_BUDGET - TRI_BYTES) // (win * REC_BYTES)) if win else THREADS // lanes
    rpp, scratch = R, 0
    if entries:
        blocks = -(-entries // WALK)
        rpp = min(R, MAX_RECS, MAX_ITEMS // blocks)
        if key_form:
            rpp = min(rpp, max(1, lim // (entries * 8)))
            scratch = rpp * entries * 8
    return dict(zip(FIELDS, (lanes, rpw, win, rpw * win * REC_BYTES + TRI_BYTES, rpp, scratch)))


GRID = [(R, per, ne_max, entries, max_new)
        for R in (1, 2, 9, 1024, 70000)
        for per in (1, 48, 70, 77, 256, 1030, 2400)
        for ne_max in (1, 2, 40, 70, 1023, 1024)
        for entries in (1, 64, 65, 150, 2000, 100000, 5000000)
        for max_new in (1, 2, 3, 5, 8, 17, 33, 63, 64)]


def test_plan_over_a_grid(lb):
    """the plan equals its restatement, in the scores form and the key forms, under limits that give one, two and all recordings a
    pass; the shape is the tail occurrences plan's; the LDS within the budget with at least one recording a workgroup; the key
    forms' rows within the limit wherever more than one recording is taken"""
    one, two, every, lowered, widths = 0, 0, 0, 0, set()
    for (R, per, ne_max, entries, max_new) in GRID:
        if R * per > (1 << 31) - 1:
            continue
        shape = lb.debug_occurrences_tail_plan(R, per, 1, ne_max, entries, max_new)
        for key_form in (False, True):
            if not key_form and R * entries > (1 << 31) - 1:
                continue
            for limit in (0, 1, entries * 8, entries * 16 + 7, R * entries * 8, 1 << 20):
                case = (R, per, ne_max, entries, max_new, limit, key_form)
                p = lb.debug_recording_tail_plan(R, per, ne_max, entries, max_new, limit, key_form)
                want = _restated(R, per, ne_max, entries, max_new, limit, key_form)
                assert p == want, (case, p, want)
                assert all(p[f] == shape[f] for f in FIELDS[:4]), case
                rpp, rpw = p["recordings_per_pass"], p["recordings_per_workgroup"]
                assert max_new <= p["lanes"] < 2 * max_new and p["lanes"] & (p["lanes"] - 1) == 0, case
                assert 1 <= rpw <= THREADS // p["lanes"] and p["lds_bytes"] <= LDS_BUDGET, case
                assert rpw == THREADS // p["lanes"] or (rpw + 1) * p["window_records"] * REC_BYTES + TRI_BYTES > LDS_BUDGET, case
                assert 1 <= p["window_records"] <= per, case
                assert 1 <= rpp <= min(R, MAX_RECS), case
                assert -(-entries // WALK) * -(-rpp // rpw) <= MAX_ITEMS, case               # the units fit 32 bits
                if key_form:
                    assert p["scratch_bytes"] == rpp * entries * 8 and (rpp == 1 or p["scratch_bytes"] <= (limit or DEFAULT_LIMIT)), case
                    if R >= 9:
                        one += rpp == 1
                        two += rpp == 2
                        every += rpp == R
                else:
                    assert p["scratch_bytes"] == 0 and rpp == min(R, MAX_RECS), case         # the scores form ignores the limit
                lowered += rpw < THREADS // p["lanes"]
                widths.add(p["lanes"])
    assert one > 100 and two > 100 and every > 100 and lowered > 100 and widths == {1, 2, 4, 8, 32, 64}


def test_plan_of_the_named_shapes(lb):
    plan = lb.debug_recording_tail_plan
    # the monitor's shape: eight lanes a recording, 32 recordings a workgroup, windows of 70 + 8 - 1 records, all windows in one pass
    p = plan(1024, 256, 70, 2000, 5, key_form=True)
    assert p == dict(zip(FIELDS, (8, 32, 77, 32 * 77 * 36 + TRI_BYTES, 1024, 1024 * 2000 * 8)))
    assert plan(1024, 256, 70, 2000, 5) == dict(p, scratch_bytes=0)
    assert plan(1024, 256, 70, 100000, 5, key_form=True)["recordings_per_pass"] == DEFAULT_LIMIT // (100000 * 8) == 335
    assert plan(1024, 256, 70, 100000, 5)["recordings_per_pass"] == 1024
    # the GPU tests' shapes: passes of two recordings and of one
    assert plan(9, 48, 300, 150, 8, 2 * 150 * 8 + 5, True)["recordings_per_pass"] == 2
    assert plan(9, 48, 300, 150, 8, 150 * 8, True)["recordings_per_pass"] == 1 == plan(9, 48, 300, 150, 8, 1, True)["recordings_per_pass"]
    assert plan(5, 80, 300, 150, 64)["recordings_per_workgroup"] == 4 and plan(5, 80, 300, 150, 33)["lanes"] == 64
    p = plan(4, 1030, 1024, 6, 8)
    assert (p["lanes"], p["recordings_per_workgroup"], p["window_records"]) == (8, 3, 1030)
    # more recordings than a pass may hold
    assert plan(70000, 1, 1, 10, 1)["recordings_per_pass"] == MAX_RECS
    # an empty corpus: nothing to launch
    p = plan(7, 100, 0, 0, 8, key_form=True)
    assert p["scratch_bytes"] == 0 and p["recordings_per_pass"] == 7


def test_plan_refusals(lb):
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    for args in ((0, 100, 40, 133, 8, 0, False), (5, 0, 40, 133, 8, 0, False), (1 << 16, 1 << 15, 40, 133, 8, 0, False),
                 (5, 100, 1025, 133, 8, 0, False), (5, 100, 0, 133, 8, 0, False), (5, 100, 40, (1 << 32) + 1, 8, 0, True),
                 (5, 100, 40, 133, 0, 0, False), (5, 100, 40, 133, MAX_NEW + 1, 0, True), (1 << 16, 100, 40, 1 << 15, 8, 0, False)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            lb.debug_recording_tail_plan(*args)
        assert err.value.status == refused, args
    assert lb.debug_recording_tail_plan(1 << 16, 100, 40, 1 << 15, 8, 0, True)["recordings_per_pass"] == 1024       # (the key forms: no such product)
    N = lb._native
    out = [N.UInt32(0), N.UInt32(0), N.UInt32(0), N.UInt64(0), N.UInt32(0), N.UInt64(0)]
    for missing in range(len(out)):
        ptrs = [None if i == missing else C.byref(o) for i, o in enumerate(out)]
        assert getattr(lb.lib(), PLAN)(5, 100, 40, 133, 8, 0, 0, *ptrs) == refused


# ---- the compiled kernel -----------------------------------------------------------------------------------------------------
def _makefile_flags(stem):
    """CXXFLAGS and FLAGS_<stem> as lbaudiodetective_amd/csrc/Makefile sets them: the build that is shipped"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")

    def var(name):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % re.escape(name), text, re.M)
        return m.group(1).split() if m else []

    arch = (var("ARCH") or ["gfx950"])[0]
    return [f.replace("$(ARCH)", arch) for f in var("CXXFLAGS") + var("FLAGS_" + stem)]


def test_the_kernel_uses_no_scratch_and_few_registers(tmp_path):
    """k_recording_tail.hip compiles for gfx950 with the flags read from the Makefile; its one kernel reports 0 bytes of private
    segment, no spilled register, scalar or vector, no static LDS (the windows are the launch's), and at most 64 vector registers:
    eight waves a SIMD fit 512 / 8 = 64, so the registers never lower the occupancy the LDS windows leave."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_recording_tail.s"
    src = os.path.join(CSRC, "k_recording_tail.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_recording_tail") + \
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
    assert len(meta) == 1 and "recording_tail_kernel" in next(iter(meta)), sorted(meta)
    agpr, static_lds, private, sgpr_spill, vgpr, vgpr_spill = next(iter(meta.values()))
    assert (agpr, static_lds, private, sgpr_spill, vgpr_spill) == (0, 0, 0, 0, 0)
    assert 0 < vgpr <= 64, vgpr


# ---- the reference against itself ------------------------------------------------------------------------------------------------
def _bools(rng, n, length=32):
    return rng.integers(0, 2, (n, length)).astype(np.uint8)


def test_the_fold_rule():
    rng = np.random.default_rng(3)
    ent = [_bools(rng, n) for n in (1, 5, 17, 30, 31, 60, 0)]
    rec = _bools(rng, 30)
    rec[30 - 17:] = ent[2]
    cells = tail.tail_cells(rec, ent, 4)
    sc, lags = ref.fold_cells(cells, len(ent))
    assert sc.dtype == np.float32 and lags.dtype == np.int32
    assert sc[2] == 1.0 and lags[2] == -13                                   # the planted copy ends at the newest record
    assert not sc[4:].any() and not lags[4:].any()                           # longer than the recording, or empty: +0 and 0
    for j in range(4):
        mine = [(o, q) for (jj, o, q) in cells if jj == j]
        best = max(q for (_o, q) in mine)
        assert sc[j] == best and lags[j] == -min(o for (o, q) in mine if q == best)
    s0, l0 = ref.scores(rec, ent, 0)
    assert not s0.any() and not l0.any()                                     # d = 0: no cell
    # a tie inside the tail: the lower offset
    tied = [(0, 10, np.float32(0.5)), (0, 11, np.float32(0.75)), (0, 12, np.float32(0.75)), (0, 13, np.float32(0.25))]
    assert ref.fold_cells(tied, 1)[1].tolist() == [-11]
    # the selections: score descending and the lower index first; ascending index and the true count
    sc = np.array([0.5, 0.0, 0.75, 0.5, 0.25], np.float32)
    lg = np.array([-1, 0, -3, -4, -5], np.int32)
    keys, klags = ref.topk_row(sc, lg, 6, 10)
    assert (0xFFFFFFFF - (keys[:4] & np.uint64(0xFFFFFFFF)) - 10).tolist() == [2, 0, 3, 4] and not keys[4:].any()
    assert klags.tolist() == [-3, -1, -4, -5, 0, 0]
    keys, klags, count = ref.threshold_row(sc, lg, 0.5, 2)
    assert count == 3 and (0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF))).tolist() == [0, 2] and klags.tolist() == [-1, -3]


def test_pushes_report_each_entry_once_per_push_inside_the_whole_recording():
    """a random recording of 200 sub-fingerprints cut into pushes -- the first its whole window, then 1 .. 8 new ones into windows
    that grow to 60 and slide --: per push and entry the threshold rows are the folded tail-occurrences rows, and every reported
    (entry, absolute start) is a cell of the whole recording's occurrences with equal bits -- the push's best cell for that entry"""
    rng = np.random.default_rng(12)
    ent = [_bools(rng, n) for n in (1, 2, 7, 17, 22, 39, 40, 41, 90)]
    total, longest, limit = 200, 40, 60
    rec = _bools(rng, total)
    rec[50:72] = ent[4]
    rec[total - 40:] = ent[6]
    whole = {(j, o): int(np.float32(q).view(np.uint32)) for (j, o, q) in tail.full_cells(rec, ent, longest)}
    qs = np.sort(np.array([np.uint32(b).view(np.float32) for b in whole.values()], np.float32))
    seen, fed, first, pushes = [], 0, True, 0
    while fed < total:
        d = 47 if first else int(min(rng.integers(1, 9), total - fed))
        fed += d
        n = fed if first else min(fed, limit)
        assert n >= min(fed, longest + d - 1)
        short = [e if len(e) <= longest else np.zeros((n + 1, 32), np.uint8) for e in ent]        # (longer than the window: skipped)
        cells = tail.tail_cells(rec[fed - n:fed], short, d)
        sc, lags = ref.fold_cells(cells, len(ent))
        for t in (qs[len(qs) // 2], qs[int(len(qs) * 0.9)], np.float32(1.0)):
            cap = 16
            assert t > 0
            got = ref.threshold_row(sc, lags, t, cap)
            occ = tail.tail_row(cells, t, d * len(ent))
            assert occ[2] <= d * len(ent)
            want = ref.fold_occurrence_row(*occ, cap)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        keys, klags = ref.topk_row(sc, lags, len(ent))
        idx = 0xFFFFFFFF - (keys[keys != 0] & np.uint64(0xFFFFFFFF))
        assert len(set(idx.tolist())) == len(idx)                    # an entry at most once per push
        for key, lag, j in zip(keys[keys != 0].tolist(), klags[keys != 0].tolist(), idx.tolist()):
            start = fed - n - lag
            assert whole[(j, start)] == key >> 32                    # a cell of the whole recording, bit for bit ...
            mine = [int(q.view(np.uint32)) for (jj, _o, q) in cells if jj == j]
            assert key >> 32 == max(mine)                            # ... and the push's best for that entry
            seen.append((j, start))
        first = False
        pushes += 1
    assert pushes > 20 and (4, 50) in seen and (6, total - 40) in seen and not any(j in (7, 8) for (j, _s) in seen)
    assert seen.count((4, 50)) == 1 and seen.count((6, total - 40)) == 1
