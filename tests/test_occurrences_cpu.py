"""CPU checks of the occurrences calls: the three symbols and their declared signatures, the cap's macro, the Python names, the
argument checks that need neither a device nor a handle, the no-device status, and the compiled kernels of k_occurrences.hip
(no scratch memory, no register spilled to it)."""
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

SYMBOLS = ("LBAudioDetectiveCorpusQueryOccurrencesKeysDevice", "LBAudioDetectiveCorpusQueryPackedOccurrencesKeysDevice",
           "LBAudioDetectiveCorpusQueryOccurrences")


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
    ctype = {"LBAudioDetectiveCorpusRef": N.Ref, "LBAudioDetectiveFingerprintRef": N.Ref, "void*": C.c_void_p, "const void*": C.c_void_p,
             "UInt32": N.UInt32, "UInt64": N.UInt64, "Float32": N.Float32, "SInt64*": C.POINTER(N.SInt64),
             "Float32*": C.POINTER(N.Float32), "UInt64*": C.POINTER(N.UInt64), "SInt32*": C.POINTER(N.SInt32)}
    ref, fp, dev = "LBAudioDetectiveCorpusRef", "LBAudioDetectiveFingerprintRef", "void*"
    want = {
        SYMBOLS[0]: [ref, fp, "UInt32", "Float32", "UInt32", "UInt64", "UInt64", dev, dev, dev, dev],
        SYMBOLS[1]: [ref, "const void*", "UInt32", "UInt32", "Float32", "UInt32", "UInt64", "UInt64", dev, dev, dev, dev],
        SYMBOLS[2]: [ref, fp, "UInt32", "Float32", "UInt32", "UInt64", "SInt64*", "Float32*", "SInt32*", "UInt64*"],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [ctype[p] for p in params], (name, args)
    # no status constant was added
    assert len(lb._native.declared_symbols()[1]) == 10


def test_the_cap_is_at_least_1024():
    m = re.search(r"^#define\s+LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS\s+(\d+)\b", open(HEADER).read(), re.M)
    assert m and int(m.group(1)) >= 1024


def test_python_names(lb):
    for attr in ("query_occurrences", "query_occurrences_keys_device", "query_packed_occurrences_keys_device"):
        assert callable(getattr(lb.Corpus, attr))
    assert callable(lb.decode_occurrence_keys)


def _fakes(lb):
    N = lb._native
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    fake = C.c_void_p(p)                  # ... and for a corpus or fingerprint handle
    host = ((N.SInt64 * 4)(), (N.Float32 * 4)(), (N.SInt32 * 4)(), N.UInt64(0))
    return buf, p, fake, host


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle: the calls return on a machine without a
    GPU, with handles that are never read."""
    Lib = lb.lib()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, p, fake, (idx, sc, lags, total) = _fakes(lb)
    dev, packed, host = (getattr(Lib, s) for s in SYMBOLS)
    for peaks in (0, 1):
        for outlags, hostlags in ((p, lags), (None, None)):          # outLags may be NULL: it changes no refusal
            for t in (0.0, -0.0, -1.0, float("nan"), float("inf")):
                assert dev(fake, fake, 0, t, peaks, 4, 0, p, outlags, p, None) == bad, t
                assert packed(fake, p, 3, 0, t, peaks, 4, 0, p, outlags, p, None) == bad, t
                assert host(fake, fake, 0, t, peaks, 4, idx, sc, hostlags, C.byref(total)) == bad, t
            for capacity in (0, (1 << 31) + 1):
                assert dev(fake, fake, 0, 0.7, peaks, capacity, 0, p, outlags, p, None) == bad
                assert packed(fake, p, 3, 0, 0.7, peaks, capacity, 0, p, outlags, p, None) == bad
                assert host(fake, fake, 0, 0.7, peaks, capacity, idx, sc, hostlags, C.byref(total)) == bad
            # no sub-fingerprints, or more than a lag can count
            for per in (0, 1 << 31, 0xFFFFFFFF):
                assert packed(fake, p, per, 0, 0.7, peaks, 4, 0, p, outlags, p, None) == bad, per
            # NULL handles and pointers
            assert dev(None, fake, 0, 0.7, peaks, 4, 0, p, outlags, p, None) == bad
            assert dev(fake, None, 0, 0.7, peaks, 4, 0, p, outlags, p, None) == bad
            assert dev(fake, fake, 0, 0.7, peaks, 4, 0, None, outlags, p, None) == bad
            assert dev(fake, fake, 0, 0.7, peaks, 4, 0, p, outlags, None, None) == bad
            assert packed(None, p, 3, 0, 0.7, peaks, 4, 0, p, outlags, p, None) == bad
            assert packed(fake, None, 3, 0, 0.7, peaks, 4, 0, p, outlags, p, None) == bad
            assert packed(fake, p, 3, 0, 0.7, peaks, 4, 0, None, outlags, p, None) == bad
            assert packed(fake, p, 3, 0, 0.7, peaks, 4, 0, p, outlags, None, None) == bad
            assert host(None, fake, 0, 0.7, peaks, 4, idx, sc, hostlags, C.byref(total)) == bad
            assert host(fake, None, 0, 0.7, peaks, 4, idx, sc, hostlags, C.byref(total)) == bad
            assert host(fake, fake, 0, 0.7, peaks, 4, None, sc, hostlags, C.byref(total)) == bad
            assert host(fake, fake, 0, 0.7, peaks, 4, idx, None, hostlags, C.byref(total)) == bad
            assert host(fake, fake, 0, 0.7, peaks, 4, idx, sc, hostlags, None) == bad
            # an index base no corpus fits behind
            assert dev(fake, fake, 0, 0.7, peaks, 4, (1 << 32) + 1, p, outlags, p, None) == bad
            assert packed(fake, p, 3, 0, 0.7, peaks, 4, (1 << 32) + 1, p, outlags, p, None) == bad


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks the three calls report kLBAudioDetectiveDeviceUnavailable (and
    still read no handle), with and without outLags."""
    Lib = lb.lib()
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, p, fake, (idx, sc, lags, total) = _fakes(lb)
    dev, packed, host = (getattr(Lib, s) for s in SYMBOLS)
    for peaks in (0, 1):
        assert dev(fake, fake, 0, 0.7, peaks, 4, 0, p, p, p, None) == nogp
        assert dev(fake, fake, 0, 0.7, peaks, 4, 0, p, None, p, None) == nogp
        assert dev(fake, fake, 64, 1.5, peaks, 1 << 31, 1 << 32, p, p, p, None) == nogp        # (t > 1 is legal)
        assert packed(fake, p, 1, 0, 0.7, peaks, 4, 0, p, p, p, None) == nogp
        assert packed(fake, p, (1 << 31) - 1, 0, 0.7, peaks, 4, 0, p, None, p, None) == nogp
        assert host(fake, fake, 0, 0.7, peaks, 4, idx, sc, lags, C.byref(total)) == nogp
        assert host(fake, fake, 0, 0.7, peaks, 4, idx, sc, None, C.byref(total)) == nogp


def _makefile_flags(stem):
    """CXXFLAGS and FLAGS_<stem> as lbaudiodetective_amd/csrc/Makefile sets them: the build that is shipped"""
    text = open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "Makefile")).read().replace("\\\n", " ")

    def var(name):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % re.escape(name), text, re.M)
        return m.group(1).split() if m else []

    arch = (var("ARCH") or ["gfx950"])[0]
    return [f.replace("$(ARCH)", arch) for f in var("CXXFLAGS") + var("FLAGS_" + stem)]


def test_the_file_is_built():
    text = open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bk_occurrences\.hip\b", text.replace("\\\n", " "), re.M)


def test_occurrences_kernels_use_no_scratch(tmp_path):
    """k_occurrences.hip compiles for gfx950 with the flags read from the Makefile (CXXFLAGS and any FLAGS_k_occurrences); every
    kernel in it -- the count and the scatter kernel, each for a range that covers the length and for one that does not --
    reports 0 bytes of private segment and no spilled register, scalar or vector (the metadata only)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_occurrences.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_occurrences.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_occurrences") + \
          ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    for kernel, instances in (("occurrences_count_kernel", 2), ("occurrences_scatter_kernel", 2)):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == instances, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 4, sorted(meta)
