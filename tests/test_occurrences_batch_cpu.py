"""CPU checks of the batch occurrences and the batch recording threshold: the symbols and their declared signatures, the Python
names, the refusals that need neither a device nor a handle (and that they come before the no-device status), the no-device
status, the host plan (LBAudioDetectiveDebugOccurrencesBatchPlan) over a grid of shapes and scratch limits against a restatement
of it, and the compiled kernels of k_occurrences_batch.hip (no scratch memory, no register spilled to it)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "lbaudiodetective.h")
CSRC = os.path.join(ROOT, "lbaudiodetective_amd", "csrc")

OCC = "LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice"
THR = "LBAudioDetectiveCorpusQueryPackedRecordingThresholdBatchKeysDevice"
PLAN = "LBAudioDetectiveDebugOccurrencesBatchPlan"
FORCE = "LBAudioDetectiveDebugSetOccurrencesBatchForm"

# what the header and occurrences_common.hpp state
TILE, WALK, WAVES, REC_BYTES, TRI_BYTES = 126, 64, 4, 36, 5151 * 4
LDS_BUDGET = 160 * 1024 - 64
MAX_ITEMS = 0xFFFFFFFF - 4096
DEFAULT_LIMIT = 256 << 20
MAX_RECS = 65535
FORM_S, FORM_W = 0, 1


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
        OCC: ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "UInt32", "Float32", "UInt32", "UInt64", "UInt64", dev, dev,
              dev, dev],
        THR: ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "UInt32", "Float32", "UInt64", "UInt64", dev, dev, dev, dev],
        PLAN: ["UInt32", "UInt32", "UInt32", "UInt32", "UInt64", "UInt64", "UInt32*", "UInt64*", "UInt32*", "UInt64*", "UInt64*", "UInt64*"],
        FORCE: ["UInt32"],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [types[p] for p in params], (name, args)
    # the outputs' order: keys, lags, counts for the occurrences; keys, counts, lags for the threshold (the single calls')
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(OCC + r"\s*\([^)]*outKeys,\s*void\*\s*outLags,\s*void\*\s*outCounts,\s*void\*\s*inStream\)", text)
    assert re.search(THR + r"\s*\([^)]*outKeys,\s*void\*\s*outCounts,\s*void\*\s*outLags,\s*void\*\s*inStream\)", text)
    # no status constant was added
    assert len(lb._native.declared_symbols()[1]) == 10


def test_python_names(lb):
    for method in ("query_packed_occurrences_batch_keys_device", "query_packed_recording_threshold_batch_keys_device"):
        assert callable(getattr(lb.Corpus, method)), method
    assert callable(lb.StreamBank.occurrences) and callable(lb.StreamBank.matches_above)
    for name in ("debug_occurrences_batch_plan", "debug_set_occurrences_batch_form"):
        assert callable(getattr(lb, name)) and name in lb.__all__, name


def test_the_files_are_built():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_occurrences_batch\.hip\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bapi_occurrences_batch\.cpp\b", text, re.M)


def _fakes():
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    return buf, p, C.c_void_p(p)          # ... and for a corpus handle


TOO_MANY = ((1, 1 << 31), (2, 1 << 30), (1 << 16, 1 << 15), (0xFFFFFFFF, 0xFFFFFFFF), (3, 715827883))
NAN, INF = float("nan"), float("inf")


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle -- also on a machine without a GPU, where
    a call that passes them reports the missing device: they come first -- with a handle that is never read."""
    occ, thr = getattr(lb.lib(), OCC), getattr(lb.lib(), THR)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, p, fake = _fakes()

    def both(c, rows, R, per, t, cap, base, keys, lags, counts):
        """the two calls with the same arguments (the occurrences with and without peaks)"""
        got = {occ(c, rows, R, per, 0, t, peaks, cap, base, keys, lags, counts, None) for peaks in (0, 1)}
        got.add(thr(c, rows, R, per, 0, t, cap, base, keys, counts, lags, None))
        return got

    for lags in (p, None):                                           # outLags may be NULL: it changes no refusal
        assert both(None, p, 2, 3, 0.5, 4, 0, p, lags, p) == {bad}
        assert both(fake, None, 2, 3, 0.5, 4, 0, p, lags, p) == {bad}
        assert both(fake, p, 2, 3, 0.5, 4, 0, None, lags, p) == {bad}
        assert both(fake, p, 2, 3, 0.5, 4, 0, p, lags, None) == {bad}                   # a NULL outCounts
        assert both(fake, p, 0, 3, 0.5, 4, 0, p, lags, p) == {bad}                      # no recordings
        assert both(fake, p, 2, 0, 0.5, 4, 0, p, lags, p) == {bad}                      # no sub-fingerprints
        for R, per in TOO_MANY:
            assert R * per > (1 << 31) - 1
            assert both(fake, p, R, per, 0.5, 1, 0, p, lags, p) == {bad}, (R, per)
        for t in (0.0, -0.5, NAN, INF, -INF):
            assert both(fake, p, 2, 3, t, 4, 0, p, lags, p) == {bad}, t
        for cap in (0, (1 << 31) + 1, 1 << 40):
            assert both(fake, p, 1, 3, 0.5, cap, 0, p, lags, p) == {bad}, cap
        assert both(fake, p, 2, 3, 0.5, 4, (1 << 32) + 1, p, lags, p) == {bad}          # an index base no corpus fits behind
        for R, cap in ((2, (1 << 30) + 1), ((1 << 21) + 1, 1 << 10), (3, 1 << 30), (1 << 16, (1 << 15) + 1)):
            assert R * cap > 1 << 31
            assert both(fake, p, R, 1, 0.5, cap, 0, p, lags, p) == {bad}, (R, cap)      # more than 2^31 slots


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks the calls report kLBAudioDetectiveDeviceUnavailable (and still read
    no handle), with and without outLags."""
    occ, thr = getattr(lb.lib(), OCC), getattr(lb.lib(), THR)
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, p, fake = _fakes()
    for lags in (p, None):
        for (R, per, rng, t, cap, base) in ((1, 1, 0, 0.5, 1, 0), (1, (1 << 31) - 1, 64, 1.5, 1 << 31, 1 << 32),
                                            (1 << 15, (1 << 16) - 1, 0, 1e-30, 1 << 16, 0), (3, 715827882, 0, 1.0, 10, 7),
                                            (1 << 21, 1, 0, 0.25, 1 << 10, 0)):
            for peaks in (0, 1):
                assert occ(fake, p, R, per, rng, t, peaks, cap, base, p, lags, p, None) == nogp, (R, per)
            assert thr(fake, p, R, per, rng, t, cap, base, p, p, lags, None) == nogp, (R, per)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def _tiles(per, ne_min, ne_max):
    """occurrences_tiles: a bound over every pair of the call, cases A and B"""
    most = 1
    if ne_max > per:
        most = ne_max - per + 1
    if ne_min <= per:
        most = max(most, per - ne_min + 1)
    return -(-most // TILE)


def _groups(tiles):
    return -(-tiles // WAVES)


def _single_scratch(entries, tiles):
    """occurrences_scratch_bytes, the single call's formula: the carried total, a first slot and an offset per entry, a count and
    a position per entry and tile, a flag per block of 64 entries and group of 4 tiles"""
    return 24 + entries * (16 + 8 * tiles) + -(-entries // WALK) * _groups(tiles) * 4


def _single_chunk(tiles, lim):
    """occurrences_chunk_entries: the single call's chunk under the limit"""
    per_block = WALK * (16 + 8 * tiles) + _groups(tiles) * 4
    if lim < 24 + per_block:
        return 0
    return min((lim - 24) // per_block, (MAX_ITEMS // tiles) // WALK) * WALK


def _wave_lds(ne_max):
    """four windows of 126 + 2 + longest entry records of 36 bytes, and the table"""
    return WAVES * (TILE + 2 + ne_max) * REC_BYTES + TRI_BYTES


def _shared_lds(per, ne_max):
    return (WAVES * TILE + 2 + min(ne_max, per)) * REC_BYTES + TRI_BYTES


def _restated(R, per, ne_min, ne_max, entries, limit, force_shared=False):
    """the plan as the header states it; None: refused"""
    lim = limit or DEFAULT_LIMIT
    tiles = _tiles(per, ne_min, ne_max)
    fit = _single_chunk(tiles, lim)
    if fit == 0:
        return None
    rounded = -(-entries // WALK) * WALK
    chunk = fit if fit < entries else rounded
    one = _single_scratch(chunk, tiles)
    rpp = 1
    if chunk >= entries:
        rpp = min(R, lim // one, MAX_ITEMS // (entries * tiles), MAX_RECS)
    wave = tiles < WAVES and _wave_lds(ne_max) <= LDS_BUDGET and not force_shared
    return {"form": FORM_W if wave else FORM_S, "tiles": tiles, "recordings_per_pass": rpp, "entries_per_chunk": chunk,
            "scratch_bytes": rpp * one, "lds_bytes": _wave_lds(ne_max) if wave else _shared_lds(per, ne_max)}


GRID = [(R, per, ne_min, ne_max, entries)
        for R in (1, 2, 5, 1024, 70000)
        for per in (1, 17, 100, 128, 129, 256, 300, 378, 379, 525, 600, 2400)
        for ne_min, ne_max in ((1, 40), (20, 70), (300, 866), (300, 867), (600, 1024), (1, 1024))
        for entries in (1, 63, 64, 65, 133, 2000, 100000, 5000000)]


def test_plan_over_a_grid(lb):
    """the plan equals its restatement; scratch within the limit, chunks of whole blocks, at least one recording a pass, the item
    cap, the single call's plan at one recording, and the form by its stated rule"""
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    seen = {FORM_S: 0, FORM_W: 0}
    many, chunked, refusals = 0, 0, 0
    for (R, per, ne_min, ne_max, entries) in GRID:
        if R * per > (1 << 31) - 1:
            continue
        tiles = _tiles(per, ne_min, ne_max)
        block = _single_scratch(WALK, tiles)
        rounded = -(-entries // WALK) * WALK
        whole = _single_scratch(rounded, tiles)
        for limit in (0, block - 1, block, block + 1, 3 * block + 5, whole, 2 * whole + 1, 1 << 20):
            lim = limit or DEFAULT_LIMIT
            want = _restated(R, per, ne_min, ne_max, entries, limit)
            case = (R, per, ne_min, ne_max, entries, limit)
            assert (want is None) == (lim < block), case
            if want is None:
                with pytest.raises(lb.LBAudioDetectiveError) as err:
                    lb.debug_occurrences_batch_plan(R, per, ne_min, ne_max, entries, limit)
                assert err.value.status == refused
                refusals += 1
                continue
            p = lb.debug_occurrences_batch_plan(R, per, ne_min, ne_max, entries, limit)
            assert p == want, (case, p, want)
            chunk, rpp = p["entries_per_chunk"], p["recordings_per_pass"]
            assert p["scratch_bytes"] <= lim, case
            assert chunk % WALK == 0 and 0 < chunk <= rounded, case
            assert 1 <= rpp <= min(R, MAX_RECS), case
            assert rpp * min(chunk, entries) * tiles <= MAX_ITEMS, case
            # several recordings a pass only with the whole corpus in one chunk
            if rpp > 1:
                assert chunk == rounded, case
                many += 1
            if chunk < entries:
                assert rpp == 1, case
                chunked += 1
            # one recording: the single call's tiles, chunk and scratch
            if R == 1:
                single = _single_chunk(tiles, lim)
                assert chunk == (single if single < entries else rounded), case
                assert p["scratch_bytes"] == _single_scratch(chunk, tiles), case
            assert p["lds_bytes"] <= LDS_BUDGET, case
            seen[p["form"]] += 1
    assert seen[FORM_S] > 100 and seen[FORM_W] > 100 and many > 100 and chunked > 100 and refusals > 100


def test_plan_of_the_named_shapes(lb):
    plan = lb.debug_occurrences_batch_plan
    # the four blocks of the GPU tests against their corpus (133 entries of 1 .. 400, and its first 131 of 1 .. 40)
    for per, form, tiles in ((100, FORM_W, 3), (129, FORM_W, 3), (300, FORM_W, 3), (525, FORM_S, 5)):
        p = plan(5 if form == FORM_W else 3, per, 1, 400, 133)
        assert (p["form"], p["tiles"]) == (form, tiles), (per, p)
    for per, tiles in ((100, 1), (129, 2), (300, 3)):
        assert plan(5, per, 1, 40, 131)["tiles"] == tiles and plan(5, per, 1, 40, 131)["form"] == FORM_W
    assert plan(3, 525, 1, 40, 131)["tiles"] == 5 and plan(3, 525, 1, 40, 131)["form"] == FORM_S
    # the monitor's shape runs in one pass, one chunk
    p = plan(1024, 256, 20, 70, 2000)
    one = _single_scratch(2048, 2)
    assert (p["form"], p["tiles"], p["recordings_per_pass"], p["entries_per_chunk"], p["scratch_bytes"]) == (FORM_W, 2, 1024, 2048, 1024 * one)
    # 100 000 entries: the recordings that fit the default limit
    assert plan(1024, 256, 20, 70, 100000)["recordings_per_pass"] == DEFAULT_LIMIT // _single_scratch(100032, 2) == 83
    # a limit that forces one recording per pass with several chunks ...
    t3 = _tiles(300, 1, 400)
    p = plan(5, 300, 1, 400, 133, _single_scratch(WALK, t3))
    assert (p["recordings_per_pass"], p["entries_per_chunk"]) == (1, 64)                     # three chunks of 133
    # ... and one that forces several passes of more than one recording
    p = plan(5, 300, 1, 400, 133, 2 * _single_scratch(192, t3) + 9)
    assert (p["recordings_per_pass"], p["entries_per_chunk"]) == (2, 192)                    # passes of 2, 2, 1
    # the last shapes of form W: three tiles, and the longest entry whose four windows fit
    assert plan(5, 378, 1, 40, 133)["form"] == FORM_W and plan(5, 379, 1, 40, 133)["form"] == FORM_S
    assert plan(5, 100, 1, 477, 133)["form"] == FORM_W and plan(5, 100, 1, 478, 133)["form"] == FORM_S
    assert _wave_lds(866) <= LDS_BUDGET < _wave_lds(867)
    assert plan(5, 600, 300, 866, 133)["form"] == FORM_W and plan(5, 600, 300, 867, 133)["form"] == FORM_S
    # an empty corpus: nothing to launch
    p = plan(7, 100, 0, 0, 0)
    assert p["entries_per_chunk"] == 0 and p["scratch_bytes"] == 0


def test_forcing_form_s(lb):
    try:
        lb.debug_set_occurrences_batch_form(True)
        p = lb.debug_occurrences_batch_plan(1024, 256, 20, 70, 2000)
        assert p == _restated(1024, 256, 20, 70, 2000, 0, force_shared=True) and p["form"] == FORM_S
        # another switch than the siblings'
        assert lb.debug_recording_batch_plan(1024, 256, 20, 70, 2000)["form"] == FORM_W
        assert lb.debug_timeline_batch_plan(1024, 256, 20, 70, 2000)["form"] == FORM_W
    finally:
        lb.debug_set_occurrences_batch_form(False)
    assert lb.debug_occurrences_batch_plan(1024, 256, 20, 70, 2000)["form"] == FORM_W
    try:
        lb.debug_set_recording_batch_form(True)
        assert lb.debug_occurrences_batch_plan(1024, 256, 20, 70, 2000)["form"] == FORM_W
    finally:
        lb.debug_set_recording_batch_form(False)


def test_plan_refusals(lb):
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    block = _single_scratch(WALK, _tiles(300, 1, 40))
    for args in ((0, 100, 1, 40, 133, 0), (5, 0, 1, 40, 133, 0), (1 << 16, 1 << 15, 1, 40, 133, 0), (5, 100, 41, 40, 133, 0),
                 (5, 100, 1, 1025, 133, 0), (5, 100, 0, 40, 133, 0), (5, 300, 1, 40, 133, block - 1), (5, 300, 1, 40, 133, 1),
                 (5, 100, 1, 40, (1 << 32) + 1, 0)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            lb.debug_occurrences_batch_plan(*args)
        assert err.value.status == refused, args
    assert lb.debug_occurrences_batch_plan(5, 300, 1, 40, 133, block)["recordings_per_pass"] == 1
    N = lb._native
    out = [N.UInt32(0), N.UInt64(0), N.UInt32(0), N.UInt64(0), N.UInt64(0), N.UInt64(0)]
    for missing in range(6):
        ptrs = [None if i == missing else C.byref(o) for i, o in enumerate(out)]
        assert getattr(lb.lib(), PLAN)(5, 100, 1, 40, 133, 0, *ptrs) == refused


# ---- the compiled kernels ----------------------------------------------------------------------------------------------------
def _makefile_flags(stem):
    """CXXFLAGS and FLAGS_<stem> as lbaudiodetective_amd/csrc/Makefile sets them: the build that is shipped"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")

    def var(name):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % re.escape(name), text, re.M)
        return m.group(1).split() if m else []

    arch = (var("ARCH") or ["gfx950"])[0]
    return [f.replace("$(ARCH)", arch) for f in var("CXXFLAGS") + var("FLAGS_" + stem)]


def test_batch_kernels_use_no_scratch(tmp_path):
    """k_occurrences_batch.hip compiles for gfx950 with the flags read from the Makefile; every kernel in it -- the count and the
    scatter kernel in both forms, each for a range that covers the length and for one that does not, the totals kernel and the
    threshold compaction's two -- reports 0 bytes of private segment and no spilled register, scalar or vector (the metadata
    only)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_occurrences_batch.s"
    src = os.path.join(CSRC, "k_occurrences_batch.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_occurrences_batch") + \
          ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    for kernel, instances in (("occurrences_batch_count_kernel", 4), ("occurrences_batch_scatter_kernel", 4),
                              ("occurrences_batch_totals_kernel", 1), ("threshold_batch_count_kernel", 1),
                              ("threshold_batch_scatter_kernel", 1)):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == instances, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 11, sorted(meta)
