"""CPU checks of the recording segments call (LBAudioDetectiveTimelineSegmentsFromKeysDevice): the symbol and its declared
signature, the Python names, the build list, every refusal that needs no device -- with fake pointers that are never read --, the
no-device status, and the compiled kernel of k_segments.hip (no scratch memory, no register spilled to it)."""
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

SEGMENTS = "LBAudioDetectiveTimelineSegmentsFromKeysDevice"
CAP = 8192                      # LBAD_SEGMENTS_MAX_SUBFINGERPRINTS


def _has_gpu():
    return torch.cuda.is_available()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototype(name):
    """the parameter types of `name` as include/lbaudiodetective.h declares it, comments removed"""
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in the header"
    return m.group(1), [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(2).split(",")]


def test_symbol_exists_with_the_declared_signature(lb):
    N = lb._native
    raw = C.CDLL(lb.LIB_PATH)
    types = {"void*": C.c_void_p, "const void*": C.c_void_p, "UInt32": N.UInt32}
    params = ["const void*", "const void*", "UInt32", "UInt32", "UInt32", "void*", "void*", "void*", "void*", "void*"]
    assert hasattr(raw, SEGMENTS), f"{SEGMENTS} is not exported"
    ret, got = _prototype(SEGMENTS)
    assert (ret, got) == ("OSStatus", params), got
    res, args = N._SIGNATURES[SEGMENTS]
    assert res is N.OSStatus and args == [types[p] for p in params], args
    # the cap is the header's, and no status constant was added
    assert re.search(r"#define\s+LBAD_SEGMENTS_MAX_SUBFINGERPRINTS\s+8192\b", _header())
    assert N.SEGMENTS_MAX_SUBFINGERPRINTS == CAP
    assert len(N.declared_symbols()[1]) == 10


def test_python_names(lb):
    assert callable(lb.Corpus.recording_segments_batch_keys_device) and callable(lb.StreamBank.segments)
    for name in ("timeline_segments_device", "decode_segments"):
        assert callable(getattr(lb, name)) and name in lb.__all__, name
    # what was there stays
    assert callable(lb.Corpus.recording_segments) and callable(lb.timeline_segments) and "timeline_segments" in lb.__all__


def test_the_files_are_built():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_segments\.hip\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bapi_segments\.cpp\b", text, re.M)


def _fakes():
    """four distinct 8-byte aligned addresses that stand for device blocks: never dereferenced"""
    buf = (C.c_uint64 * 64)()
    base = C.addressof(buf)
    assert base % 8 == 0
    return buf, [base + 64 * i for i in range(6)]


def _args(a, R=2, per=3, cap=4, **change):
    """(inKeys, inLengths, R, per, cap, outStarts, outKeys, outLengths, outCounts, stream) with valid fakes, then `change`"""
    v = dict(inKeys=a[0], inLengths=a[1], R=R, per=per, cap=cap, outStarts=a[2], outKeys=a[3], outLengths=a[4], outCounts=a[5], stream=None)
    v.update(change)
    return tuple(v[k] for k in ("inKeys", "inLengths", "R", "per", "cap", "outStarts", "outKeys", "outLengths", "outCounts", "stream"))


# shapes that pass every check: the cap itself, the largest products
LEGAL = [(1, 1, 1), (2, 3, 4), (1, CAP, 1), (5, CAP, CAP + 3), ((1 << 30) - 1, 2, 2), (((1 << 31) - 2) // CAP, CAP, CAP),
         (1, 1, (1 << 31) - 1), ((1 << 31) - 1, 1, 1)]


def test_bad_arguments_are_refused_before_any_device(lb):
    """Every refusal is decided before anything touches a device: the call returns on a machine without a GPU, and the fake
    pointers are never read."""
    call = getattr(lb.lib(), SEGMENTS)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, a = _fakes()
    for outlen in (a[4], None):                                       # outLengths may be NULL: it changes no refusal
        for name in ("inKeys", "inLengths", "outStarts", "outKeys", "outCounts"):
            assert call(*_args(a, outLengths=outlen, **{name: None})) == bad, name
        for name in ("R", "per", "cap"):
            assert call(*_args(a, outLengths=outlen, **{name: 0})) == bad, name
        for per in (CAP + 1, 1 << 14, 0xFFFFFFFF):
            assert call(*_args(a, R=1, per=per, cap=1, outLengths=outlen)) == bad, per
        for R, per, cap in (((1 << 31) // CAP, CAP, 1), (1 << 30, 2, 1), (1 << 31, 1, 1), (0xFFFFFFFF, CAP, 1),       # R x per
                            (2, 3, 1 << 30), (1, 1, 1 << 31), (1 << 16, 1, 1 << 15), (3, 1, 715827883), (0xFFFFFFFF, 1, 0xFFFFFFFF)):
            assert R * per > (1 << 31) - 1 or R * cap > (1 << 31) - 1
            assert call(*_args(a, R=R, per=per, cap=cap, outLengths=outlen)) == bad, (R, per, cap)
        # alignment: 8 bytes for the key blocks, 4 for the others
        for name in ("inKeys", "outKeys"):
            for off in (1, 2, 4):
                assert call(*_args(a, outLengths=outlen, **{name: a[0 if name == "inKeys" else 3] + off})) == bad, (name, off)
        for name, at in (("inLengths", 1), ("outStarts", 2), ("outCounts", 5)):
            for off in (1, 2, 3):
                assert call(*_args(a, outLengths=outlen, **{name: a[at] + off})) == bad, (name, off)
        # in place
        assert call(*_args(a, outLengths=outlen, outKeys=a[0])) == bad
    for off in (1, 2, 3):
        assert call(*_args(a, outLengths=a[4] + off)) == bad, off
    assert call(*_args(a, outLengths=a[1])) == bad


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_point_fails_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks the call reports kLBAudioDetectiveDeviceUnavailable (and still reads no
    pointer), with and without outLengths -- the cap itself and the largest products included."""
    call = getattr(lb.lib(), SEGMENTS)
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, a = _fakes()
    assert any(per == CAP for _R, per, _c in LEGAL) and any(R * per == (1 << 31) - 2 and per <= CAP for R, per, _c in LEGAL)
    for outlen in (a[4], None):
        for R, per, cap in LEGAL:
            assert R * per <= (1 << 31) - 1 and R * cap <= (1 << 31) - 1 and per <= CAP
            assert call(*_args(a, R=R, per=per, cap=cap, outLengths=outlen)) == nogp, (R, per, cap)
        assert call(*_args(a, outLengths=outlen, inKeys=a[0] + 8, outStarts=a[2] + 4, outCounts=a[5] + 4)) == nogp


# ---- the compiled kernel -----------------------------------------------------------------------------------------------------
def _makefile_flags(stem):
    """CXXFLAGS and FLAGS_<stem> as lbaudiodetective_amd/csrc/Makefile sets them: the build that is shipped"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")

    def var(name):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % re.escape(name), text, re.M)
        return m.group(1).split() if m else []

    arch = (var("ARCH") or ["gfx950"])[0]
    return [f.replace("$(ARCH)", arch) for f in var("CXXFLAGS") + var("FLAGS_" + stem)]


def test_segments_kernel_uses_no_scratch(tmp_path):
    """k_segments.hip compiles for gfx950 with the flags read from the Makefile; every kernel in it reports 0 bytes of private
    segment and no spilled register, scalar or vector (the metadata only), and no static LDS beside the dynamic block."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_segments.s"
    src = os.path.join(CSRC, "k_segments.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_segments") + \
          ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    assert len(meta) >= 1 and all("timeline_segments_kernel" in k for k in meta), sorted(meta)
    assert all(v == (0, 0, 0) for v in meta.values()), meta
    fixed = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", isa)]      # (one per kernel of the file)
    assert len(fixed) == len(meta) and all(x == 0 for x in fixed), fixed
