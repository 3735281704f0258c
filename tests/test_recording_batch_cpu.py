"""CPU checks of the batch recording scores and the batch recording top-K: the symbols and their declared signatures, the Python
names, the refusals that need neither a device nor a handle (and that they come before the no-device status), the no-device
status, the host plan (LBAudioDetectiveDebugRecordingBatchPlan) over a grid of shapes, scratch limits and both call forms, and the
compiled kernels of k_recording_batch.hip (no scratch memory, no register spilled to it)."""
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

SCORES = "LBAudioDetectiveCorpusRecordingPackedScoresBatchDevice"
TOPK = "LBAudioDetectiveCorpusQueryPackedRecordingTopKBatchKeysDevice"
PLAN = "LBAudioDetectiveDebugRecordingBatchPlan"
FORCE = "LBAudioDetectiveDebugSetRecordingBatchForm"

# what the header and occurrences_common.hpp state
TILE, WALK, WAVES, REC_BYTES, TRI_BYTES = 126, 64, 4, 36, 5151 * 4
LDS_BUDGET = 160 * 1024 - 64
MAX_ITEMS = 0xFFFFFFFF - 4096
DEFAULT_LIMIT = 256 << 20
MAX_RECS = 65535
TOPK_MAX = 1024
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
             "Float32*": C.c_void_p, "SInt32*": C.c_void_p, "UInt32*": C.POINTER(N.UInt32), "UInt64*": C.POINTER(N.UInt64)}
    dev = "void*"
    want = {
        SCORES: ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "UInt32", "Float32*", "SInt32*", dev],
        TOPK: ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "UInt32", "UInt32", "UInt64", dev, dev, dev],
        PLAN: ["UInt32", "UInt32", "UInt32", "UInt32", "UInt64", "UInt64", "UInt32", "UInt32*", "UInt64*", "UInt32*", "UInt64*", "UInt64*",
               "UInt64*"],
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
    for method in ("recording_scores_batch_device", "query_packed_recording_topk_batch_keys_device"):
        assert callable(getattr(lb.Corpus, method)), method
    assert callable(lb.StreamBank.identify_recordings) and callable(lb.StreamBank.identify)
    for name in ("debug_recording_batch_plan", "debug_set_recording_batch_form"):
        assert callable(getattr(lb, name)) and name in lb.__all__, name


def test_the_files_are_built():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_recording_batch\.hip\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bapi_recording_batch\.cpp\b", text, re.M)


def test_the_constants_are_the_single_calls():
    def constant(name, file):
        return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, file)).read()).group(1))

    assert constant("kOcEntries", "occurrences_common.hpp") == constant("kOcBlock", "k_occurrences.hip") == WALK
    assert constant("kOcTile", "occurrences_common.hpp") == constant("kOcKeep", "k_occurrences.hip") == TILE
    assert constant("kOcRecBytes", "occurrences_common.hpp") == REC_BYTES
    assert constant("kRbMaxRecs", "k_recording_batch.hip") == MAX_RECS
    assert constant("kRbFoldThreads", "k_recording_batch.hip") == constant("kFoldThreads", "k_recording.hip")


def _fakes():
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    return buf, p, C.c_void_p(p)          # ... and for a corpus handle


TOO_MANY = ((1, 1 << 31), (2, 1 << 30), (1 << 16, 1 << 15), (0xFFFFFFFF, 0xFFFFFFFF), (3, 715827883))


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle -- also on a machine without a GPU, where
    a call that passes them reports the missing device: they come first -- with a handle that is never read."""
    scores, topk = getattr(lb.lib(), SCORES), getattr(lb.lib(), TOPK)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, p, fake = _fakes()
    for lags in (p, None):                                           # outLags may be NULL: it changes no refusal
        assert scores(None, p, 2, 3, 0, p, lags, None) == bad
        assert scores(fake, None, 2, 3, 0, p, lags, None) == bad
        assert scores(fake, p, 2, 3, 0, None, lags, None) == bad
        assert scores(fake, p, 0, 3, 0, p, lags, None) == bad                           # no recordings
        assert scores(fake, p, 2, 0, 0, p, lags, None) == bad                           # no sub-fingerprints
        assert topk(None, p, 2, 3, 0, 1, 0, p, lags, None) == bad
        assert topk(fake, None, 2, 3, 0, 1, 0, p, lags, None) == bad
        assert topk(fake, p, 2, 3, 0, 1, 0, None, lags, None) == bad
        assert topk(fake, p, 0, 3, 0, 1, 0, p, lags, None) == bad
        assert topk(fake, p, 2, 0, 0, 1, 0, p, lags, None) == bad
        for R, per in TOO_MANY:
            assert R * per > (1 << 31) - 1
            assert scores(fake, p, R, per, 0, p, lags, None) == bad, (R, per)
            assert topk(fake, p, R, per, 0, 1, 0, p, lags, None) == bad, (R, per)
        for k in (0, TOPK_MAX + 1, 0xFFFFFFFF):
            assert topk(fake, p, 2, 3, 0, k, 0, p, lags, None) == bad, k
        assert topk(fake, p, 2, 3, 0, 1, (1 << 32) + 1, p, lags, None) == bad           # an index base no corpus fits behind
        assert topk(fake, p, (1 << 21) + 1, 1, 0, TOPK_MAX, 0, p, lags, None) == bad    # more than 2^31 slots


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks the calls report kLBAudioDetectiveDeviceUnavailable (and still read
    no handle), with and without outLags."""
    scores, topk = getattr(lb.lib(), SCORES), getattr(lb.lib(), TOPK)
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, p, fake = _fakes()
    for lags in (p, None):
        assert scores(fake, p, 1, 1, 0, p, lags, None) == nogp
        assert scores(fake, p, 1, (1 << 31) - 1, 64, p, lags, None) == nogp
        assert scores(fake, p, 1 << 15, (1 << 16) - 1, 0, p, lags, None) == nogp
        assert scores(fake, p, 3, 715827882, 0, p, lags, None) == nogp                        # 3 x that = 2^31 - 2
        assert topk(fake, p, 1, 1, 0, 1, 0, p, lags, None) == nogp
        assert topk(fake, p, 1, (1 << 31) - 1, 64, TOPK_MAX, 1 << 32, p, lags, None) == nogp
        assert topk(fake, p, 1 << 21, 1, 0, TOPK_MAX, 0, p, lags, None) == nogp               # exactly 2^31 slots
        assert topk(fake, p, 3, 715827882, 0, 10, 0, p, lags, None) == nogp


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def _tiles(per, ne_min, ne_max):
    """occurrences_tiles: a bound over every pair of the call, cases A and B"""
    most = 1
    if ne_max > per:
        most = ne_max - per + 1
    if ne_min <= per:
        most = max(most, per - ne_min + 1)
    return -(-most // TILE)


def _single_scratch(entries, tiles):
    """the single call's formula: one 64-bit partial per entry and tile"""
    return entries * tiles * 8


def _single_chunk(tiles, lim):
    """recording_chunk_entries: the single call's chunk under the limit"""
    return min(lim // (WALK * 8 * tiles), (MAX_ITEMS // tiles) // WALK) * WALK


def _wave_lds(ne_max):
    """four windows of 126 + 2 + longest entry records of 36 bytes, and the table"""
    return WAVES * (TILE + 2 + ne_max) * REC_BYTES + TRI_BYTES


def _shared_lds(per, ne_max):
    return (WAVES * TILE + 2 + min(ne_max, per)) * REC_BYTES + TRI_BYTES


GRID = [(R, per, ne_min, ne_max, entries)
        for R in (1, 2, 5, 1024, 70000)
        for per in (1, 17, 100, 128, 129, 256, 300, 378, 379, 525, 600, 2400)
        for ne_min, ne_max in ((1, 40), (20, 70), (300, 866), (300, 867), (600, 1024), (1, 1024))
        for entries in (1, 63, 64, 65, 133, 2000, 100000, 5000000)]


def test_plan_over_a_grid(lb):
    """scratch within the limit, chunks of whole blocks, at least one recording a pass, the item cap, the score-row bound of the
    key form, the single call's plan at one recording, and the form by its stated rule"""
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    seen = {FORM_S: 0, FORM_W: 0}
    many, chunked = 0, 0
    for (R, per, ne_min, ne_max, entries) in GRID:
        if R * per > (1 << 31) - 1:
            continue
        tiles = _tiles(per, ne_min, ne_max)
        block = _single_scratch(WALK, tiles)
        rounded = -(-entries // WALK) * WALK
        whole = _single_scratch(rounded, tiles)
        for limit in (0, block, block + 1, 3 * block + 5, whole, 2 * whole + 1, 1 << 20):
            lim = limit or DEFAULT_LIMIT
            for key_form in (False, True):
                if not key_form and R * entries > (1 << 31) - 1:
                    continue                                   # (the scores form refuses the shape itself)
                if lim < block:
                    with pytest.raises(lb.LBAudioDetectiveError) as err:
                        lb.debug_recording_batch_plan(R, per, ne_min, ne_max, entries, limit, key_form)
                    assert err.value.status == refused
                    continue
                p = lb.debug_recording_batch_plan(R, per, ne_min, ne_max, entries, limit, key_form)
                case = (R, per, ne_min, ne_max, entries, limit, key_form, p)
                assert p["tiles"] == tiles, case
                assert p["scratch_bytes"] <= lim, case
                chunk, rpp = p["entries_per_chunk"], p["recordings_per_pass"]
                assert chunk % WALK == 0 and 0 < chunk <= rounded, case
                assert 1 <= rpp <= min(R, MAX_RECS), case
                assert p["scratch_bytes"] == rpp * _single_scratch(chunk, tiles), case
                assert rpp * min(chunk, entries) * tiles <= MAX_ITEMS, case
                # passes and chunks: several recordings a pass only with the whole corpus in one chunk, and then as many as fit
                single_chunk = _single_chunk(tiles, lim)
                if single_chunk >= entries:
                    assert chunk == rounded, case
                    most = min(R, lim // whole, MAX_ITEMS // (entries * tiles), MAX_RECS)
                    if key_form:                               # the rows of a score and a lag per entry under the same limit
                        rows = max(1, lim // (entries * 8))
                        most = min(most, rows)
                        assert rpp == 1 or rpp * entries * 8 <= lim, case
                    assert rpp == most, case
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
    plan = lb.debug_recording_batch_plan
    assert plan(1024, 128, 20, 70, 2000)["form"] == FORM_W
    assert plan(1024, 256, 20, 70, 2000)["form"] == FORM_W and plan(1024, 256, 20, 70, 2000)["tiles"] == 2
    assert plan(1024, 128, 20, 1024, 2000)["form"] == FORM_S                   # 897 offsets of the longest entry: 8 tiles
    for ne_min, ne_max in ((1, 40), (20, 70), (1, 1024), (100, 100)):
        assert plan(3, 525, ne_min, ne_max, 2000)["form"] == FORM_S
    assert plan(8, 2400, 20, 70, 100000)["form"] == FORM_S
    # the last shapes of form W: three tiles ...
    assert plan(5, 378, 1, 40, 133)["form"] == FORM_W and plan(5, 378, 1, 40, 133)["tiles"] == 3
    assert plan(5, 379, 1, 40, 133)["form"] == FORM_S and plan(5, 379, 1, 40, 133)["tiles"] == 4
    # ... also where the entries LONGER than the recordings decide the tiles (case A): 378 | 379 offsets of the longest
    assert plan(5, 100, 1, 477, 133)["form"] == FORM_W and plan(5, 100, 1, 478, 133)["form"] == FORM_S
    # ... and the longest entry whose four windows fit (three tiles on both sides)
    assert _wave_lds(866) <= LDS_BUDGET < _wave_lds(867)
    assert plan(5, 600, 300, 866, 133)["form"] == FORM_W and plan(5, 600, 300, 866, 133)["tiles"] == 3
    assert plan(5, 600, 300, 867, 133)["form"] == FORM_S and plan(5, 600, 300, 867, 133)["tiles"] == 3
    # the monitor's shape runs in one pass, one chunk, in both call forms
    for key_form in (False, True):
        p = plan(1024, 256, 20, 70, 2000, 0, key_form)
        assert (p["recordings_per_pass"], p["entries_per_chunk"], p["scratch_bytes"]) == (1024, 2048, 1024 * 2048 * 2 * 8)
    # 100 000 entries: 167 recordings a pass under the default limit, 670 under 1 GiB
    assert plan(1024, 256, 20, 70, 100000)["recordings_per_pass"] == min(1024, DEFAULT_LIMIT // (100032 * 2 * 8)) == 167
    assert plan(1024, 256, 20, 70, 100000, 1 << 30)["recordings_per_pass"] == 670
    assert plan(1024, 256, 20, 70, 100000, 1 << 30, True)["recordings_per_pass"] == 670
    # an empty corpus: nothing to launch
    p = plan(7, 100, 0, 0, 0)
    assert p["entries_per_chunk"] == 0 and p["scratch_bytes"] == 0


def test_the_score_row_bound(lb):
    """the key form never takes more recordings a pass than rows of (score, lag) x entries fit the limit -- but at least one.  (A
    recording's partials take 8 bytes per entry and tile, rounded up to whole blocks, so this bound never lies below the partials'
    own: both forms plan the same passes, and the rows always fit.)"""
    plan = lb.debug_recording_batch_plan
    entries, per, tiles = 100000, 100, 1
    partial = 100032 * tiles * 8
    for limit in (partial, 2 * partial, 10 * partial + 7, 1 << 30):
        free = plan(1024, per, 20, 70, entries, limit)["recordings_per_pass"]
        keyed = plan(1024, per, 20, 70, entries, limit, True)["recordings_per_pass"]
        assert free == min(1024, limit // partial)
        assert keyed == min(free, max(1, limit // (entries * 8))) == free, limit
        assert keyed * entries * 8 <= limit or keyed == 1
    # the rows alone would not fit, one recording a pass still runs: at least 1
    small = 64 * 3 * 8                                                       # one block of 64 entries at 3 tiles
    p = plan(5, 300, 1, 40, 64, small, True)
    assert p["recordings_per_pass"] == 1 and p["entries_per_chunk"] == 64
    assert plan(5, 300, 1, 40, 64, 5 * small, True)["recordings_per_pass"] == 5 and 5 * 64 * 8 <= 5 * small


def test_forcing_form_s(lb):
    try:
        lb.debug_set_recording_batch_form(True)
        p = lb.debug_recording_batch_plan(1024, 256, 20, 70, 2000)
        assert p["form"] == FORM_S and p["lds_bytes"] == _shared_lds(256, 70)
        # another switch than the batch timeline's
        assert lb.debug_timeline_batch_plan(1024, 256, 20, 70, 2000)["form"] == FORM_W
    finally:
        lb.debug_set_recording_batch_form(False)
    assert lb.debug_recording_batch_plan(1024, 256, 20, 70, 2000)["form"] == FORM_W
    try:
        lb.debug_set_timeline_batch_form(True)
        assert lb.debug_recording_batch_plan(1024, 256, 20, 70, 2000)["form"] == FORM_W
    finally:
        lb.debug_set_timeline_batch_form(False)


def test_plan_refusals(lb):
    refused = lb.constant("kLBAudioDetectiveArgumentInvalid")
    block = _single_scratch(WALK, _tiles(300, 1, 40))
    for args in ((0, 100, 1, 40, 133, 0), (5, 0, 1, 40, 133, 0), (1 << 16, 1 << 15, 1, 40, 133, 0), (5, 100, 41, 40, 133, 0),
                 (5, 100, 1, 1025, 133, 0), (5, 100, 0, 40, 133, 0), (5, 300, 1, 40, 133, block - 1), (5, 300, 1, 40, 133, 1),
                 (5, 100, 1, 40, (1 << 32) + 1, 0, True), (1 << 16, 100, 1, 40, 1 << 15, 0, False)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            lb.debug_recording_batch_plan(*args)
        assert err.value.status == refused, args
    assert lb.debug_recording_batch_plan(1 << 16, 100, 1, 40, 1 << 15, 0, True)["tiles"] == 1     # (the scores form's product only)
    assert lb.debug_recording_batch_plan(5, 300, 1, 40, 133, block)["recordings_per_pass"] == 1
    N = lb._native
    out = [N.UInt32(0), N.UInt64(0), N.UInt32(0), N.UInt64(0), N.UInt64(0), N.UInt64(0)]
    for missing in range(6):
        ptrs = [None if i == missing else C.byref(o) for i, o in enumerate(out)]
        assert getattr(lb.lib(), PLAN)(5, 100, 1, 40, 133, 0, 0, *ptrs) == refused


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
    """k_recording_batch.hip compiles for gfx950 with the flags read from the Makefile; every kernel in it -- both forms of the
    maxima kernel, each for a range that covers the length and for one that does not, the fold and the lag gather -- reports 0
    bytes of private segment and no spilled register, scalar or vector (the metadata only).  No kernel's name contains one of
    k_recording.hip's."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_recording_batch.s"
    src = os.path.join(CSRC, "k_recording_batch.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_recording_batch") + \
          ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    for kernel, instances in (("recording_batch_shared_kernel", 2), ("recording_batch_wave_kernel", 2), ("recording_batch_fold_kernel", 1),
                              ("recording_batch_lag_gather_kernel", 1)):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == instances, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 6, sorted(meta)
    assert not any(old in k for k in meta for old in ("recording_maxima_kernel", "recording_fold_kernel", "recording_lag_gather_kernel"))
