"""CPU checks of the tail occurrences: the symbols and their declared signatures, the Python names, the two files in the build,
the refusals that need neither a device nor a handle (and that they come before the no-device status), the no-device status, the
host plan (LBAudioDetectiveDebugOccurrencesTailPlan) over a grid of shapes and scratch limits against a restatement of it, the
compiled kernels of k_occurrences_tail.hip (no scratch memory, no register spilled to it), and the tests' reference against
itself: the cells of a recording cut into pushes are the cells of the whole recording, each exactly once."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import occurrences_tail_ref as ref
from align_ref import profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "lbaudiodetective.h")
CSRC = os.path.join(ROOT, "lbaudiodetective_amd", "csrc")

TAIL = "LBAudioDetectiveCorpusQueryPackedOccurrencesTailBatchKeysDevice"
PLAN = "LBAudioDetectiveDebugOccurrencesTailPlan"

# what the header states
WALK, THREADS, REC_BYTES, TRI_BYTES, MAX_NEW = 64, 256, 36, 5151 * 4, 64
LDS_BUDGET = 160 * 1024 - 64
MAX_ITEMS = 0xFFFFFFFF - 4096
DEFAULT_LIMIT = 256 << 20
MAX_RECS = 65535
FIELDS = ("lanes", "recordings_per_workgroup", "window_records", "lds_bytes", "recordings_per_pass", "entries_per_chunk", "scratch_bytes")


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
    dev = "void*"
    want = {
        TAIL: ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "const void*", "UInt32", "UInt32", "Float32", "UInt64", "UInt64",
               dev, dev, dev, dev],
        PLAN: ["UInt32", "UInt32", "UInt32", "UInt32", "UInt64", "UInt32", "UInt64", "UInt32*", "UInt32*", "UInt32*", "UInt64*", "UInt32*",
               "UInt64*", "UInt64*"],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [types[p] for p in params], (name, args)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(TAIL + r"\s*\([^)]*inNewCounts,\s*UInt32\s+inMaxNew,\s*UInt32\s+inRange,\s*Float32\s+inThreshold,\s*UInt64\s+inCapacity,"
                     r"\s*UInt64\s+inIndexBase,\s*void\*\s*outKeys,\s*void\*\s*outLags,\s*void\*\s*outCounts,\s*void\*\s*inStream\)", text)
    assert re.search(r"#define\s+LBAD_OCCURRENCES_TAIL_MAX_NEW\s+64\b", text)
    # the header says what a device count above the bound means, and that there is no peak rule
    doc = " ".join(open(HEADER).read().split())
    assert "a device value above it counts as inMaxNew" in doc and "There is NO peak rule" in doc and "EXACTLY ONCE" in doc
    # no status constant was added
    assert len(lb._native.declared_symbols()[1]) == 10


def test_python_names(lb):
    assert callable(lb.Corpus.query_packed_occurrences_tail_batch_keys_device) and callable(lb.StreamBank.new_occurrences)
    for name in ("debug_occurrences_tail_plan", "decode_tail_occurrences"):
        assert callable(getattr(lb, name)) and name in lb.__all__, name


def test_the_files_are_built():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_occurrences_tail\.hip\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bapi_occurrences_tail\.cpp\b", text, re.M)


def _fakes():
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    return buf, p, C.c_void_p(p)          # ... and for a corpus handle


TOO_MANY = ((1, 1 << 31), (2, 1 << 30), (1 << 16, 1 << 15), (0xFFFFFFFF, 0xFFFFFFFF), (3, 715827883))
NAN, INF = float("nan"), float("inf")


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle -- also on a machine without a GPU, where a
    call that passes them reports the missing device: they come first -- with a handle that is never read."""
    tail = getattr(lb.lib(), TAIL)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, p, fake = _fakes()

    def call(c, rows, R, per, new, max_new, t, cap, base, keys, lags, counts):
        return tail(c, rows, R, per, new, max_new, 0, t, cap, base, keys, lags, counts, None)

    for lags in (p, None):                                           # outLags may be NULL: it changes no refusal
        assert call(None, p, 2, 3, p, 4, 0.5, 4, 0, p, lags, p) == bad
        assert call(fake, None, 2, 3, p, 4, 0.5, 4, 0, p, lags, p) == bad
        assert call(fake, p, 2, 3, None, 4, 0.5, 4, 0, p, lags, p) == bad                # a NULL inNewCounts
        assert call(fake, p, 2, 3, p, 4, 0.5, 4, 0, None, lags, p) == bad
        assert call(fake, p, 2, 3, p, 4, 0.5, 4, 0, p, lags, None) == bad                # a NULL outCounts
        for off in (1, 2, 3, 5, 7):
            assert call(fake, p, 2, 3, p + off, 4, 0.5, 4, 0, p, lags, p) == bad, off    # inNewCounts not 4-byte aligned
        for max_new in (0, MAX_NEW + 1, 1 << 20, 0xFFFFFFFF):
            assert call(fake, p, 2, 3, p, max_new, 0.5, 4, 0, p, lags, p) == bad, max_new
        assert call(fake, p, 0, 3, p, 4, 0.5, 4, 0, p, lags, p) == bad                   # no recordings
        assert call(fake, p, 2, 0, p, 4, 0.5, 4, 0, p, lags, p) == bad                   # no sub-fingerprints
        for R, per in TOO_MANY:
            assert R * per > (1 << 31) - 1
            assert call(fake, p, R, per, p, 4, 0.5, 1, 0, p, lags, p) == bad, (R, per)
        for t in (0.0, -0.5, NAN, INF, -INF):
            assert call(fake, p, 2, 3, p, 4, t, 4, 0, p, lags, p) == bad, t
        for cap in (0, (1 << 31) + 1, 1 << 40):
            assert call(fake, p, 1, 3, p, 4, 0.5, cap, 0, p, lags, p) == bad, cap
        assert call(fake, p, 2, 3, p, 4, 0.5, 4, (1 << 32) + 1, p, lags, p) == bad       # an index base no corpus fits behind
        for R, cap in ((2, (1 << 30) + 1), ((1 << 21) + 1, 1 << 10), (3, 1 << 30), (1 << 16, (1 << 15) + 1)):
            assert R * cap > 1 << 31
            assert call(fake, p, R, 1, p, 4, 0.5, cap, 0, p, lags, p) == bad, (R, cap)   # more than 2^31 slots


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_point_fails_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks the call reports kLBAudioDetectiveDeviceUnavailable (and still reads
    no handle), with and without outLags, with inNewCounts 4-byte but not 8-byte aligned, at both ends of inMaxNew."""
    tail = getattr(lb.lib(), TAIL)
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, p, fake = _fakes()
    for lags in (p, None):
        for (R, per, rng, t, cap, base) in ((1, 1, 0, 0.5, 1, 0), (1, (1 << 31) - 1, 64, 1.5, 1 << 31, 1 << 32),
                                            (1 << 15, (1 << 16) - 1, 0, 1e-30, 1 << 16, 0), (3, 715827882, 0, 1.0, 10, 7),
                                            (1 << 21, 1, 0, 0.25, 1 << 10, 0)):
            for max_new in (1, 5, MAX_NEW):
                for new in (p, p + 4):
                    assert tail(fake, p, R, per, new, max_new, rng, t, cap, base, p, lags, p, None) == nogp, (R, per, max_new)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def _single_scratch(entries):
    """occurrences_scratch_bytes with one tile: the carried total, a first slot and an offset per entry, a count and a position per
    entry, a flag per block of 64 entries"""
    return 24 + entries * 24 + -(-entries // WALK) * 4


def _single_chunk(lim):
    """occurrences_chunk_entries with one tile: the chunk under the limit"""
    per_block = WALK * 24 + 4
    if lim < 24 + per_block:
        return 0
    return min((lim - 24) // per_block, MAX_ITEMS // WALK) * WALK


def _restated(R, per, ne_min, ne_max, entries, max_new, limit):
    """the plan as the header states it; None: refused"""
    lim = limit or DEFAULT_LIMIT
    lanes = 1
    while lanes < max_new:
        lanes *= 2
    win = min(per, min(ne_max, per) + lanes - 1)
    rpw = min(THREADS // lanes, (LDS_BUDGET - TRI_BYTES) // (win * REC_BYTES))
    fit = _single_chunk(lim)
    if fit == 0:
        return None
    rounded = -(-entries // WALK) * WALK
    chunk = fit if fit < entries else rounded
    one = _single_scratch(chunk)
    rpp = 1
    if chunk >= entries:
        rpp = min(R, lim // one, MAX_ITEMS // entries, MAX_RECS)
    return dict(zip(FIELDS, (lanes, rpw, win, rpw * win * REC_BYTES + TRI_BYTES, rpp, chunk, rpp * one)))


GRID = [(R, per, ne_min, ne_max, entries, max_new)
        for R in (1, 2, 9, 1024, 70000)
        for per in (1, 48, 70, 77, 256, 1030, 2400)
        for ne_min, ne_max in ((1, 1), (20, 70), (1, 1024))
        for entries in (1, 64, 65, 150, 2000, 100000, 5000000)
        for max_new in (1, 2, 5, 8, 33, 64)]


def test_plan_over_a_grid(lb):
    """the plan equals its restatement; the LDS within the budget with at least one recording a workgroup, scratch within the
    limit, chunks of whole blocks, at least one recording a pass, the item cap; passes of several recordings and one recording per
    pass in chunks both occur"""
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    many, chunked, refusals, lowered, widths = 0, 0, 0, 0, set()
    block = _single_scratch(WALK)
    for (R, per, ne_min, ne_max, entries, max_new) in GRID:
        if R * per > (1 << 31) - 1:
            continue
        rounded = -(-entries // WALK) * WALK
        whole = _single_scratch(rounded)
        for limit in (0, block - 1, block, 3 * block + 5, whole, 2 * whole + 1, 1 << 20):
            lim = limit or DEFAULT_LIMIT
            want = _restated(R, per, ne_min, ne_max, entries, max_new, limit)
            case = (R, per, ne_min, ne_max, entries, max_new, limit)
            assert (want is None) == (lim < block), case
            if want is None:
                with pytest.raises(lb.LBAudioDetectiveError) as err:
                    lb.debug_occurrences_tail_plan(R, per, ne_min, ne_max, entries, max_new, limit)
                assert err.value.status == refused
                refusals += 1
                continue
            p = lb.debug_occurrences_tail_plan(R, per, ne_min, ne_max, entries, max_new, limit)
            assert p == want, (case, p, want)
            chunk, rpp, rpw = p["entries_per_chunk"], p["recordings_per_pass"], p["recordings_per_workgroup"]
            assert max_new <= p["lanes"] < 2 * max_new and p["lanes"] & (p["lanes"] - 1) == 0, case
            assert 1 <= rpw <= THREADS // p["lanes"] and p["lds_bytes"] <= LDS_BUDGET, case
            assert rpw == THREADS // p["lanes"] or (rpw + 1) * p["window_records"] * REC_BYTES + TRI_BYTES > LDS_BUDGET, case
            assert 1 <= p["window_records"] <= per, case
            assert p["scratch_bytes"] <= lim, case
            assert chunk % WALK == 0 and 0 < chunk <= rounded, case
            assert 1 <= rpp <= min(R, MAX_RECS), case
            assert rpp * min(chunk, entries) <= MAX_ITEMS, case
            if rpp > 1:                                              # several recordings a pass only with the whole corpus in one chunk
                assert chunk == rounded, case
                many += 1
            if chunk < entries:
                assert rpp == 1, case
                chunked += 1
            lowered += rpw < THREADS // p["lanes"]
            widths.add(p["lanes"])
    assert many > 100 and chunked > 100 and refusals > 100 and lowered > 100 and widths == {1, 2, 8, 64}


def test_plan_of_the_named_shapes(lb):
    plan = lb.debug_occurrences_tail_plan
    # the monitor's shape: eight lanes a recording, 32 recordings a workgroup, windows of 70 + 8 - 1 records, one pass, one chunk
    p = plan(1024, 256, 20, 70, 2000, 5)
    assert p == dict(zip(FIELDS, (8, 32, 77, 32 * 77 * 36 + TRI_BYTES, 1024, 2048, 1024 * _single_scratch(2048))))
    assert plan(1024, 256, 20, 70, 100000, 5)["recordings_per_pass"] == DEFAULT_LIMIT // _single_scratch(100032) == 111
    # the GPU tests' shapes: passes of two recordings; one recording a pass in chunks of 128 and of 64 entries
    assert plan(9, 48, 1, 300, 150, 8)["window_records"] == 48 and plan(9, 48, 1, 300, 150, 8)["recordings_per_pass"] == 9
    for limit, rpp, chunk in ((2 * _single_scratch(192) + 9, 2, 192), (_single_scratch(128), 1, 128), (_single_scratch(64), 1, 64)):
        p = plan(9, 48, 1, 300, 150, 8, limit)
        assert (p["recordings_per_pass"], p["entries_per_chunk"]) == (rpp, chunk), (limit, p)
    assert plan(5, 80, 1, 300, 150, 64)["recordings_per_workgroup"] == 4 and plan(5, 80, 1, 300, 150, 33)["lanes"] == 64
    # long entries lower the recordings per workgroup: 3 windows of 1 030 fit, 4 do not; the longest window of all fits once
    p = plan(4, 1030, 5, 1024, 6, 8)
    assert (p["lanes"], p["recordings_per_workgroup"], p["window_records"]) == (8, 3, 1030)
    assert 3 * 1030 * 36 + TRI_BYTES <= LDS_BUDGET < 4 * 1030 * 36 + TRI_BYTES
    p = plan(4, 5000, 1, 1024, 6, 64)
    assert (p["lanes"], p["recordings_per_workgroup"], p["window_records"]) == (64, 3, 1024 + 63) and p["lds_bytes"] <= LDS_BUDGET
    # an empty corpus: nothing to launch
    p = plan(7, 100, 0, 0, 0, 8)
    assert p["entries_per_chunk"] == 0 and p["scratch_bytes"] == 0 and p["recordings_per_pass"] == 7


def test_plan_refusals(lb):
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    block = _single_scratch(WALK)
    for args in ((0, 100, 1, 40, 133, 8, 0), (5, 0, 1, 40, 133, 8, 0), (1 << 16, 1 << 15, 1, 40, 133, 8, 0), (5, 100, 41, 40, 133, 8, 0),
                 (5, 100, 1, 1025, 133, 8, 0), (5, 100, 0, 40, 133, 8, 0), (5, 300, 1, 40, 133, 8, block - 1), (5, 300, 1, 40, 133, 8, 1),
                 (5, 100, 1, 40, (1 << 32) + 1, 8, 0), (5, 100, 1, 40, 133, 0, 0), (5, 100, 1, 40, 133, MAX_NEW + 1, 0)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            lb.debug_occurrences_tail_plan(*args)
        assert err.value.status == refused, args
    assert lb.debug_occurrences_tail_plan(5, 300, 1, 40, 133, 8, block)["recordings_per_pass"] == 1
    N = lb._native
    out = [N.UInt32(0), N.UInt32(0), N.UInt32(0), N.UInt64(0), N.UInt32(0), N.UInt64(0), N.UInt64(0)]
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


def test_tail_kernels_use_no_scratch(tmp_path):
    """k_occurrences_tail.hip compiles for gfx950 with the flags read from the Makefile; its four kernels -- the plain and the
    peaks instance of the count and of the scatter kernel -- report 0 bytes of private segment and no spilled register, scalar or
    vector (the metadata only)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_occurrences_tail.s"
    src = os.path.join(CSRC, "k_occurrences_tail.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_occurrences_tail") + \
          ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    for kernel in ("occurrences_tail_count_kernel", "occurrences_tail_scatter_kernel"):
        hits = {k: v for k, v in meta.items() if kernel in k}
        # the two instances of the template: PEAKS false and true in the mangled name
        assert len(hits) == 2 and sorted("ILb1E" in k for k in hits) == [False, True], (kernel, sorted(meta))
        assert all(("ILb0E" in k) != ("ILb1E" in k) for k in hits), sorted(hits)
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 4, sorted(meta)


# ---- the reference against itself ------------------------------------------------------------------------------------------------
def _bools(rng, n, length=32):
    return rng.integers(0, 2, (n, length)).astype(np.uint8)


def test_the_cell_rule():
    assert list(ref.tail_range(48, 17, 5)) == [27, 28, 29, 30, 31]   # the entry ends inside the newest five
    assert list(ref.tail_range(48, 44, 8)) == [0, 1, 2, 3, 4]        # clipped at offset 0
    assert list(ref.tail_range(48, 48, 3)) == [0] and list(ref.tail_range(48, 49, 3)) == []
    assert list(ref.tail_range(48, 1, 1)) == [47] and list(ref.tail_range(48, 17, 0)) == []
    assert list(ref.tail_range(48, 17, 48)) == list(range(32))       # every new: the whole profile
    assert ref.clamp_new(20, 8, 48) == 8 and ref.clamp_new(3, 8, 48) == 3 and ref.clamp_new(100, 64, 48) == 48
    assert ref.key_of(np.float32(1.0), 7, 1000) == (0x3F800000 << 32) | (0xFFFFFFFF - 1007)


def test_a_tail_cell_is_the_profiles():
    rng = np.random.default_rng(3)
    ent = [_bools(rng, n) for n in (1, 5, 17, 30, 31, 60)]
    rec = _bools(rng, 30)
    rec[30 - 17:] = ent[2]
    cells = ref.tail_cells(rec, ent, 4)
    assert [j for (j, _o, _q) in cells] == [0] * 4 + [1] * 4 + [2] * 4 + [3]          # 31 and 60 are longer: skipped
    for j, o, q in cells:
        assert q == profile(rec, ent[j], 0)[0][o] and isinstance(q, np.float32)
    keys, lags, count = ref.tail_row(cells, 1.0, 4)
    assert count == 1 and keys[0] == ref.key_of(np.float32(1.0), 2) and lags[0] == -13 and not keys[1:].any() and not lags[1:].any()
    keys, lags, count = ref.tail_row(cells, 1e-30, 4)                 # a cut row: the first four in (entry, offset) order, the true count
    assert count == sum(q > 0 for (_j, _o, q) in cells) > 4 and np.count_nonzero(keys) == 4 and (np.diff(lags) <= 0).all()
    # the filter of a batch row is the same row
    every = ref.tail_cells(rec, ent[:4], 30)
    bk, bl, bc = ref.tail_row(every, 0.4, 512)
    assert bc <= 512
    want = ref.tail_row(ref.tail_cells(rec, ent[:4], 4), 0.4, 8)
    got = ref.filter_batch_row(bk, bl, bc, [len(e) for e in ent], 30, 4, 8)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_pushes_cover_every_cell_exactly_once():
    """a random recording of 200 sub-fingerprints cut into pushes -- the first its whole window, then 1 .. 8 new ones into windows
    that grow to 60 and slide -- : the union of the tail cells at absolute positions is the filtered full profile, each cell once,
    with equal bits"""
    rng = np.random.default_rng(12)
    ent = [_bools(rng, n) for n in (1, 2, 7, 17, 22, 39, 40, 41, 90)]
    total, longest, limit = 200, 40, 60
    rec = _bools(rng, total)
    rec[50:72] = ent[4]
    rec[total - 40:] = ent[6]
    seen, fed, first = [], 0, True
    while fed < total:
        d = 47 if first else int(min(rng.integers(1, 9), total - fed))
        fed += d
        n = fed if first else min(fed, limit)
        assert n >= min(fed, longest + d - 1)
        short = [e if len(e) <= longest else np.zeros((n + 1, 32), np.uint8) for e in ent]        # (longer than the window: skipped)
        for j, o, q in ref.tail_cells(rec[fed - n:fed], short, d):
            seen.append((j, fed - n + o, int(q.view(np.uint32))))
        first = False
    want = [(j, o, int(np.float32(q).view(np.uint32))) for (j, o, q) in ref.full_cells(rec, ent, longest)]
    assert len(seen) == len(set(seen)) == len(want) and sorted(seen) == sorted(want)
    assert (4, 50, 0x3F800000) in seen and (6, total - 40, 0x3F800000) in seen and not any(j in (7, 8) for (j, _o, _b) in seen)
