"""CPU checks of the batch recording timeline: the symbols and their declared signatures, the Python names, the refusals that need
neither a device nor a handle, the no-device status, the host plan (LBAudioDetectiveDebugTimelineBatchPlan) over a grid of shapes
and scratch limits, and the compiled kernels of k_timeline_batch.hip (no scratch memory, no register spilled to it)."""
import ctypes as C
import itertools
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

BATCH = "LBAudioDetectiveCorpusRecordingPackedTimelineBatchKeysDevice"
PLAN = "LBAudioDetectiveDebugTimelineBatchPlan"
FORCE = "LBAudioDetectiveDebugSetTimelineBatchForm"

# what the header and occurrences_common.hpp state
TILE, WALK, WAVES, REC_BYTES, TRI_BYTES = 126, 128, 4, 36, 5151 * 4
LDS_BUDGET = 160 * 1024 - 64
MAX_ITEMS = 0xFFFFFFFF - 4096
DEFAULT_LIMIT = 256 << 20
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
        BATCH: ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "UInt32", "Float32", "UInt64", dev, dev, dev],
        PLAN: ["UInt32", "UInt32", "UInt32", "UInt32", "UInt64", "UInt64", "UInt32*", "UInt64*", "UInt32*", "UInt64*", "UInt64*", "UInt64*"],
        FORCE: ["UInt32"],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [types[p] for p in params], (name, args)
    # no status constant was added
    assert len(lb._native.declared_symbols()[1]) == 10


def test_python_names(lb):
    assert callable(lb.Corpus.recording_timeline_batch_keys_device) and callable(lb.StreamBank.timeline)
    for name in ("debug_timeline_batch_plan", "debug_set_timeline_batch_form", "decode_timeline_batch_keys", "decode_timeline_keys"):
        assert callable(getattr(lb, name)) and name in lb.__all__, name


def test_the_files_are_built():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_timeline_batch\.hip\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bapi_timeline_batch\.cpp\b", text, re.M)


def test_the_constants_are_the_single_calls():
    """the batch file walks the single call's entry blocks and folds by the single call's rule"""
    def constant(name, file):
        return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, file)).read()).group(1))

    assert constant("kTbEntries", "k_timeline_batch.hip") == constant("kTlEntries", "k_timeline.hip") == WALK
    assert constant("kTbFoldRows", "k_timeline_batch.hip") == constant("kTlFoldRows", "k_timeline.hip")
    assert constant("kTbFoldSlices", "k_timeline_batch.hip") == constant("kTlFoldSlices", "k_timeline.hip")
    assert constant("kOcTile", "occurrences_common.hpp") == TILE and constant("kOcRecBytes", "occurrences_common.hpp") == REC_BYTES


def _fakes():
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    return buf, p, C.c_void_p(p)          # ... and for a corpus handle


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle: the call returns on a machine without a GPU,
    with a handle that is never read."""
    call = getattr(lb.lib(), BATCH)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, p, fake = _fakes()
    for outlen in (p, None):                                         # outLengths may be NULL: it changes no refusal
        assert call(None, p, 2, 3, 0, 0.7, 0, p, outlen, None) == bad
        assert call(fake, None, 2, 3, 0, 0.7, 0, p, outlen, None) == bad
        assert call(fake, p, 2, 3, 0, 0.7, 0, None, outlen, None) == bad
        assert call(fake, p, 0, 3, 0, 0.7, 0, p, outlen, None) == bad                   # no recordings
        assert call(fake, p, 2, 0, 0, 0.7, 0, p, outlen, None) == bad                   # no sub-fingerprints
        for R, per in ((1, 1 << 31), (2, 1 << 30), (1 << 16, 1 << 15), (0xFFFFFFFF, 0xFFFFFFFF), (3, 715827883)):
            assert R * per > (1 << 31) - 1
            assert call(fake, p, R, per, 0, 0.7, 0, p, outlen, None) == bad, (R, per)
        for t in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert call(fake, p, 2, 3, 0, t, 0, p, outlen, None) == bad, t
        assert call(fake, p, 2, 3, 0, 0.7, (1 << 32) + 1, p, outlen, None) == bad       # an index base no corpus fits behind


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_point_fails_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks the call reports kLBAudioDetectiveDeviceUnavailable (and still reads
    no handle), with and without outLengths."""
    call = getattr(lb.lib(), BATCH)
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, p, fake = _fakes()
    for outlen in (p, None):
        assert call(fake, p, 1, 1, 0, 0.7, 0, p, outlen, None) == nogp
        assert call(fake, p, 1, (1 << 31) - 1, 64, 1.5, 1 << 32, p, outlen, None) == nogp     # (t > 1 is legal)
        assert call(fake, p, 1 << 15, (1 << 16) - 1, 0, 0.7, 0, p, outlen, None) == nogp
        assert call(fake, p, 3, 715827882, 0, 0.7, 0, p, outlen, None) == nogp                # 3 x that = 2^31 - 2


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def _tiles(per, ne_min):
    return -(-(per - min(per, ne_min) + 1) // TILE)


def _single_scratch(entries, tiles):
    """the header's single-call formula"""
    return -(-entries // WALK) * tiles * TILE * 8


def _wave_lds(ne_max):
    """four windows of 126 + 2 + longest entry records of 36 bytes, and the table"""
    return WAVES * (TILE + 2 + ne_max) * REC_BYTES + TRI_BYTES


def _shared_lds(per, ne_max):
    return (WAVES * TILE + 2 + min(ne_max, per)) * REC_BYTES + TRI_BYTES


GRID = [(R, per, ne_min, ne_max, entries)
        for R in (1, 2, 5, 1024, 70000)
        for per in (1, 17, 100, 128, 129, 256, 300, 378, 379, 525, 2400)
        for ne_min, ne_max in ((1, 40), (20, 70), (1, 866), (1, 867), (600, 1024), (1, 1024))
        for entries in (1, 127, 128, 129, 261, 2000, 100000, 5000000)]


def test_plan_over_a_grid(lb):
    """scratch within the limit, chunks of whole blocks, at least one recording a pass, the item cap, the single call's plan at one
    recording, and the form by its stated rule"""
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    seen = {FORM_S: 0, FORM_W: 0}
    many, chunked = 0, 0
    for (R, per, ne_min, ne_max, entries) in GRID:
        if R * per > (1 << 31) - 1:
            continue
        tiles = _tiles(per, ne_min)
        block = _single_scratch(WALK, tiles)
        whole = _single_scratch(entries, tiles)
        for limit in (0, block, block + 1, 3 * block + 5, whole, 2 * whole + 1, 1 << 20):
            lim = limit or DEFAULT_LIMIT
            if lim < block:
                with pytest.raises(lb.LBAudioDetectiveError) as err:
                    lb.debug_timeline_batch_plan(R, per, ne_min, ne_max, entries, limit)
                assert err.value.status == refused
                continue
            p = lb.debug_timeline_batch_plan(R, per, ne_min, ne_max, entries, limit)
            case = (R, per, ne_min, ne_max, entries, limit, p)
            assert p["tiles"] == tiles, case
            assert p["scratch_bytes"] <= lim, case
            chunk, rpp = p["entries_per_chunk"], p["recordings_per_pass"]
            rounded = -(-entries // WALK) * WALK
            assert chunk % WALK == 0 and 0 < chunk <= rounded, case
            assert 1 <= rpp <= R, case
            assert p["scratch_bytes"] == rpp * _single_scratch(chunk, tiles), case
            assert rpp * min(chunk, entries) * tiles <= MAX_ITEMS, case
            # passes and chunks: several recordings a pass only with the whole corpus in one chunk, and then as many as fit
            single_chunk = min(lim // block, (MAX_ITEMS // tiles) // WALK) * WALK          # the single call's chunk under the limit
            if single_chunk >= entries:
                assert chunk == rounded, case
                assert rpp == min(R, lim // whole, MAX_ITEMS // (entries * tiles), 65535), case
                many += rpp > 1
            else:
                assert rpp == 1 and chunk == single_chunk, case
                chunked += 1
            # one recording: the single call's tiles, chunk and scratch
            if R == 1:
                assert chunk == (single_chunk if single_chunk < entries else rounded), case
                assert p["scratch_bytes"] == _single_scratch(chunk, tiles), case
            # the form
            wave = tiles < WAVES and _wave_lds(ne_max) <= LDS_BUDGET
            assert p["form"] == (FORM_W if wave else FORM_S), case
            assert p["lds_bytes"] == (_wave_lds(ne_max) if wave else _shared_lds(per, ne_max)), case
            assert p["lds_bytes"] <= LDS_BUDGET, case
            seen[p["form"]] += 1
    assert seen[FORM_S] > 100 and seen[FORM_W] > 100 and many > 100 and chunked > 100


def test_plan_forms_of_the_named_shapes(lb):
    plan = lb.debug_timeline_batch_plan
    assert plan(1024, 128, 20, 70, 2000)["form"] == FORM_W
    assert plan(1024, 256, 20, 70, 2000)["form"] == FORM_W and plan(1024, 256, 20, 70, 2000)["tiles"] == 2
    assert plan(1024, 128, 20, 1024, 2000)["form"] == FORM_S
    for ne_min, ne_max in ((1, 40), (20, 70), (1, 1024), (100, 100)):
        assert plan(3, 525, ne_min, ne_max, 2000)["form"] == FORM_S
    assert plan(8, 2400, 20, 70, 100000)["form"] == FORM_S
    # the last shapes of form W: three tiles, and the longest entry whose four windows fit
    assert plan(5, 378, 1, 40, 261)["form"] == FORM_W and plan(5, 379, 1, 40, 261)["form"] == FORM_S
    assert plan(5, 100, 1, 866, 261)["form"] == FORM_W and plan(5, 100, 1, 867, 261)["form"] == FORM_S
    # the flagship shape runs in one pass, one chunk
    p = plan(1024, 256, 20, 70, 2000)
    assert (p["recordings_per_pass"], p["entries_per_chunk"], p["scratch_bytes"]) == (1024, 2048, 1024 * 16 * 2 * 126 * 8)
    # an empty corpus: nothing to launch
    p = plan(7, 100, 0, 0, 0)
    assert p["entries_per_chunk"] == 0 and p["scratch_bytes"] == 0


def test_forcing_form_s(lb):
    try:
        lb.debug_set_timeline_batch_form(True)
        p = lb.debug_timeline_batch_plan(1024, 256, 20, 70, 2000)
        assert p["form"] == FORM_S and p["lds_bytes"] == _shared_lds(256, 70)
    finally:
        lb.debug_set_timeline_batch_form(False)
    assert lb.debug_timeline_batch_plan(1024, 256, 20, 70, 2000)["form"] == FORM_W


def test_plan_refusals(lb):
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    block = _single_scratch(WALK, _tiles(300, 1))
    for args in ((0, 100, 1, 40, 261, 0), (5, 0, 1, 40, 261, 0), (1 << 16, 1 << 15, 1, 40, 261, 0), (5, 100, 41, 40, 261, 0),
                 (5, 100, 1, 1025, 261, 0), (5, 100, 0, 40, 261, 0), (5, 300, 1, 40, 261, block - 1), (5, 300, 1, 40, 261, 1)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            lb.debug_timeline_batch_plan(*args)
        assert err.value.status == refused, args
    assert lb.debug_timeline_batch_plan(5, 300, 1, 40, 261, block)["recordings_per_pass"] == 1
    N = lb._native
    out = [N.UInt32(0), N.UInt64(0), N.UInt32(0), N.UInt64(0), N.UInt64(0), N.UInt64(0)]
    for missing in range(6):
        ptrs = [None if i == missing else C.byref(o) for i, o in enumerate(out)]
        assert getattr(lb.lib(), PLAN)(5, 100, 1, 40, 261, 0, *ptrs) == refused


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
    """k_timeline_batch.hip compiles for gfx950 with the flags read from the Makefile; every kernel in it -- both forms of the
    maxima kernel, each for a range that covers the length and for one that does not, and the fold -- reports 0 bytes of private
    segment and no spilled register, scalar or vector (the metadata only).  No kernel's name contains one of k_timeline.hip's."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_timeline_batch.s"
    src = os.path.join(CSRC, "k_timeline_batch.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_timeline_batch") + \
          ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    for kernel, instances in (("timeline_batch_shared_kernel", 2), ("timeline_batch_wave_kernel", 2), ("timeline_batch_fold_kernel", 1)):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == instances, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 5, sorted(meta)
    assert not any(old in k for k in meta for old in ("timeline_maxima_kernel", "timeline_fold_kernel", "timeline_lengths_kernel"))
