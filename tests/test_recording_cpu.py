"""CPU checks of the recording-scores calls: the five symbols and their declared signatures, the Python names, the argument
checks that need neither a device nor a handle, the no-device status, the compiled kernels of k_recording.hip (no scratch memory,
no register spilled to it), and a numpy statement of the fold the kernels perform."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from align_ref import align, profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "lbaudiodetective.h")

SYMBOLS = ("LBAudioDetectiveCorpusRecordingScoresDevice", "LBAudioDetectiveCorpusRecordingPackedScoresDevice",
           "LBAudioDetectiveCorpusQueryRecordingTopK", "LBAudioDetectiveCorpusQueryPackedRecordingTopKKeysDevice",
           "LBAudioDetectiveCorpusQueryPackedRecordingThresholdKeysDevice")


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
    # (Float32* / SInt32* of the Device forms are device pointers: the table passes them as addresses)
    host = {"LBAudioDetectiveCorpusRef": N.Ref, "LBAudioDetectiveFingerprintRef": N.Ref, "void*": C.c_void_p, "const void*": C.c_void_p,
            "UInt32": N.UInt32, "UInt64": N.UInt64, "Float32": N.Float32, "SInt64*": C.POINTER(N.SInt64),
            "Float32*": C.POINTER(N.Float32), "UInt32*": C.POINTER(N.UInt32), "SInt32*": C.POINTER(N.SInt32)}
    device = dict(host, **{"Float32*": C.c_void_p, "SInt32*": C.c_void_p})
    ref, fp, dev = "LBAudioDetectiveCorpusRef", "LBAudioDetectiveFingerprintRef", "void*"
    want = {
        SYMBOLS[0]: ([ref, fp, "UInt32", "Float32*", "SInt32*", dev], device),
        SYMBOLS[1]: ([ref, "const void*", "UInt32", "UInt32", "Float32*", "SInt32*", dev], device),
        SYMBOLS[2]: ([ref, fp, "UInt32", "UInt32", "SInt64*", "Float32*", "SInt32*", "UInt32*"], host),
        SYMBOLS[3]: ([ref, "const void*", "UInt32", "UInt32", "UInt32", "UInt64", dev, dev, dev], device),
        SYMBOLS[4]: ([ref, "const void*", "UInt32", "UInt32", "Float32", "UInt64", "UInt64", dev, dev, dev, dev], device),
    }
    for name, (params, ctype) in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [ctype[p] for p in params], (name, args)
    # no status constant was added
    assert len(lb._native.declared_symbols()[1]) == 10


def test_python_names(lb):
    for attr in ("recording_scores_device", "query_recording_topk", "query_packed_recording_topk_keys_device",
                 "query_packed_recording_threshold_keys_device"):
        assert callable(getattr(lb.Corpus, attr))


def _fakes(lb):
    N = lb._native
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    fake = C.c_void_p(p)                  # ... and for a corpus or fingerprint handle
    host = ((N.SInt64 * 4)(), (N.Float32 * 4)(), (N.SInt32 * 4)(), N.UInt32(0))
    return buf, p, fake, host


def _topk_max():
    return int(re.search(r"^#define\s+LBAD_TOPK_MAX\s+(\d+)", open(HEADER).read(), re.M).group(1))


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle: the calls return on a machine without a
    GPU, with handles that are never read."""
    Lib = lb.lib()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, p, fake, (idx, sc, lags, count) = _fakes(lb)
    scores, packed_scores, host_topk, topk, threshold = (getattr(Lib, s) for s in SYMBOLS)
    kmax = _topk_max()
    for outlags, hostlags in ((p, lags), (None, None)):              # outLags may be NULL: it changes no refusal
        # NULL handles and pointers
        assert scores(None, fake, 0, p, outlags, None) == bad
        assert scores(fake, None, 0, p, outlags, None) == bad
        assert scores(fake, fake, 0, None, outlags, None) == bad
        assert packed_scores(None, p, 3, 0, p, outlags, None) == bad
        assert packed_scores(fake, None, 3, 0, p, outlags, None) == bad
        assert packed_scores(fake, p, 3, 0, None, outlags, None) == bad
        assert host_topk(None, fake, 0, 4, idx, sc, hostlags, C.byref(count)) == bad
        assert host_topk(fake, None, 0, 4, idx, sc, hostlags, C.byref(count)) == bad
        assert host_topk(fake, fake, 0, 4, None, sc, hostlags, C.byref(count)) == bad
        assert host_topk(fake, fake, 0, 4, idx, None, hostlags, C.byref(count)) == bad
        assert host_topk(fake, fake, 0, 4, idx, sc, hostlags, None) == bad
        assert topk(None, p, 3, 0, 4, 0, p, outlags, None) == bad
        assert topk(fake, None, 3, 0, 4, 0, p, outlags, None) == bad
        assert topk(fake, p, 3, 0, 4, 0, None, outlags, None) == bad
        assert threshold(None, p, 3, 0, 0.7, 4, 0, p, p, outlags, None) == bad
        assert threshold(fake, None, 3, 0, 0.7, 4, 0, p, p, outlags, None) == bad
        assert threshold(fake, p, 3, 0, 0.7, 4, 0, None, p, outlags, None) == bad
        assert threshold(fake, p, 3, 0, 0.7, 4, 0, p, None, outlags, None) == bad
        # inK
        for k in (0, kmax + 1):
            assert host_topk(fake, fake, 0, k, idx, sc, hostlags, C.byref(count)) == bad, k
            assert topk(fake, p, 3, 0, k, 0, p, outlags, None) == bad, k
        # the threshold and the capacity
        for t in (0.0, -0.0, -1.0, float("nan"), float("inf")):
            assert threshold(fake, p, 3, 0, t, 4, 0, p, p, outlags, None) == bad, t
        for capacity in (0, (1 << 31) + 1):
            assert threshold(fake, p, 3, 0, 0.7, capacity, 0, p, p, outlags, None) == bad, capacity
        # no sub-fingerprints, or more than a lag can count
        for per in (0, 1 << 31, 0xFFFFFFFF):
            assert packed_scores(fake, p, per, 0, p, outlags, None) == bad, per
            assert topk(fake, p, per, 0, 4, 0, p, outlags, None) == bad, per
            assert threshold(fake, p, per, 0, 0.7, 4, 0, p, p, outlags, None) == bad, per
        # an index base no corpus fits behind
        assert topk(fake, p, 3, 0, 4, (1 << 32) + 1, p, outlags, None) == bad
        assert threshold(fake, p, 3, 0, 0.7, 4, (1 << 32) + 1, p, p, outlags, None) == bad


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks the five calls report kLBAudioDetectiveDeviceUnavailable (and still
    read no handle), with and without outLags."""
    Lib = lb.lib()
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, p, fake, (idx, sc, lags, count) = _fakes(lb)
    scores, packed_scores, host_topk, topk, threshold = (getattr(Lib, s) for s in SYMBOLS)
    for outlags, hostlags in ((p, lags), (None, None)):
        assert scores(fake, fake, 0, p, outlags, None) == nogp
        assert packed_scores(fake, p, 1, 0, p, outlags, None) == nogp
        assert packed_scores(fake, p, (1 << 31) - 1, 64, p, outlags, None) == nogp
        assert host_topk(fake, fake, 0, 1, idx, sc, hostlags, C.byref(count)) == nogp
        assert host_topk(fake, fake, 0, _topk_max(), idx, sc, hostlags, C.byref(count)) == nogp
        assert topk(fake, p, 3, 0, _topk_max(), 1 << 32, p, outlags, None) == nogp
        assert threshold(fake, p, 3, 0, 1.5, 1 << 31, 1 << 32, p, p, outlags, None) == nogp       # (t > 1 is legal)


def _makefile_flags(stem):
    """CXXFLAGS and FLAGS_<stem> as lbaudiodetective_amd/csrc/Makefile sets them: the build that is shipped"""
    text = open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "Makefile")).read().replace("\\\n", " ")

    def var(name):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % re.escape(name), text, re.M)
        return m.group(1).split() if m else []

    arch = (var("ARCH") or ["gfx950"])[0]
    return [f.replace("$(ARCH)", arch) for f in var("CXXFLAGS") + var("FLAGS_" + stem)]


def test_the_files_are_built():
    text = open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_recording\.hip\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bapi_recording\.cpp\b", text, re.M)


def test_recording_kernels_use_no_scratch(tmp_path):
    """k_recording.hip compiles for gfx950 with the flags read from the Makefile (CXXFLAGS and any FLAGS_k_recording); every kernel
    in it -- the maxima kernel for a range that covers the length and for one that does not, the fold and the lag gather --
    reports 0 bytes of private segment and no spilled register, scalar or vector (the metadata only).  No new kernel's name
    contains an occurrences kernel's."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_recording.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_recording.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_recording") + \
          ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    for kernel, instances in (("recording_maxima_kernel", 2), ("recording_fold_kernel", 1), ("recording_lag_gather_kernel", 1)):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == instances, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 4, sorted(meta)
    assert not any(old in k for k in meta for old in ("occurrences_count_kernel", "occurrences_scatter_kernel"))


def test_the_fold_is_the_alignment():
    """What the kernels do, in numpy: every cell of a pair's profile as the 64-bit value  bits << 32 | ~o;  the maximum of the
    values is align_ref.align's score (its bits) and offset, ties at the lowest offset, on 200 random pairs.  Sub-fingerprints
    of 6 Booleans make ties frequent; all-zero sides make profiles that are 0 everywhere."""
    rng = np.random.default_rng(2024)
    tied = zero = 0
    for pair in range(200):
        L = 6 if pair % 2 else 200
        nq, ne = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        q = rng.integers(0, 2, (nq, L)).astype(np.uint8)
        e = rng.integers(0, 2, (ne, L)).astype(np.uint8)
        if pair % 10 == 0:
            e[:] = 0
        if pair % 10 == 5 and nq > ne:                                  # the entry twice inside the query: two cells of 1.0
            q = np.concatenate([e, q[:nq - ne], e])
        range_ = (0, 3, L)[pair % 3]
        cells, entry_long = profile(q, e, range_)
        assert np.all(np.isfinite(cells)) and not np.signbit(cells).any()          # finite and >= +0: the bits order like the values
        o = np.arange(len(cells), dtype=np.uint64)
        values = (cells.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - o)
        best = values.max()
        score = np.array([best >> np.uint64(32)], np.uint64).astype(np.uint32).view(np.float32)[0]
        offset = int(np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF)))
        want_score, want_lag = align(q, e, range_)
        assert score.view(np.uint32) == np.float32(want_score).view(np.uint32)
        assert (offset if entry_long else -offset) == want_lag
        tied += int(np.count_nonzero(cells == score) > 1)
        zero += int(score == 0)
    assert tied >= 20 and zero >= 10
