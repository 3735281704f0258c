"""CPU checks of the gather of corpus entries: the three symbols and their declared signatures, the Python names, the argument
checks that need neither a device nor a handle, the no-device status, and the compiled kernels of k_gather.hip (no scratch
memory, no register spilled to it)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

SYMBOLS = ("LBAudioDetectiveCorpusGatherKeysDevice", "LBAudioDetectiveCorpusGatherIndices", "LBAudioDetectiveCorpusCopyFingerprint")


def _has_gpu():
    return torch.cuda.is_available()


def _prototype(name):
    """the return type and parameter types of `name` as include/lbaudiodetective.h declares it, comments removed"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lbaudiodetective.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return m.group(1), [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(2).split(",")]


def test_symbols_exist_with_the_declared_signatures(lb):
    N = lb._native
    raw = C.CDLL(lb.LIB_PATH)
    ctype = {"LBAudioDetectiveCorpusRef": N.Ref, "LBAudioDetectiveFingerprintRef": N.Ref, "OSStatus": N.OSStatus, "void*": C.c_void_p,
             "const void*": C.c_void_p, "UInt64": N.UInt64, "const UInt64*": C.POINTER(N.UInt64), "UInt64*": C.POINTER(N.UInt64)}
    ref = "LBAudioDetectiveCorpusRef"
    want = {
        SYMBOLS[0]: ("OSStatus", [ref, "const void*", "UInt64", "UInt64", "void*", "UInt64", "void*", "void*"]),
        SYMBOLS[1]: ("OSStatus", [ref, "const UInt64*", "UInt64", "void*", "UInt64", "UInt64*"]),
        SYMBOLS[2]: ("LBAudioDetectiveFingerprintRef", [ref, "UInt64"]),
    }
    for name, (ret, params) in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert _prototype(name) == (ret, params), (name, _prototype(name))
        res, args = N._SIGNATURES[name]
        assert res is ctype[ret] and args == [ctype[p] for p in params], (name, res, args)
    # no status constant was added
    assert len(lb._native.declared_symbols()[1]) == 10


def test_python_names(lb):
    for attr in ("gather_keys_device", "gather", "fingerprint"):
        assert callable(getattr(lb.Corpus, attr))
    assert not hasattr(lb.ShardedCorpus, "gather")        # (no sharded wrapper: a rank serves the keys of its own range)


def _fakes(lb):
    N = lb._native
    buf = (C.c_uint64 * 16)()
    p = (C.addressof(buf) + 15) & ~15      # 16-byte aligned; stands for a device pointer and for a corpus handle: never dereferenced
    return buf, p, C.c_void_p(p), (N.UInt64 * 4)(0, 1, 2, 3), (N.UInt64 * 5)(*([0xDEAD] * 5))


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle: the calls return on a machine without a
    GPU, with corpus handles that are never read."""
    Lib = lb.lib()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    buf, p, fake, idx, off = _fakes(lb)
    dev, host, copy = (getattr(Lib, s) for s in SYMBOLS)
    # a NULL corpus
    assert dev(None, p, 4, 0, p, 4, p, None) == bad
    assert dev(None, None, 0, 0, None, 0, p, None) == bad
    assert host(None, idx, 4, p, 4, off) == bad
    assert host(None, None, 0, None, 0, off) == bad
    assert copy(None, 0) is None
    # a NULL outOffsets
    assert dev(fake, p, 4, 0, p, 4, None, None) == bad
    assert dev(fake, None, 0, 0, None, 0, None, None) == bad
    assert host(fake, idx, 4, p, 4, None) == bad
    # a NULL list with a non-zero count
    assert dev(fake, None, 4, 0, p, 4, p, None) == bad
    assert host(fake, None, 4, p, 4, off) == bad
    # a NULL outPacked with a non-zero capacity
    assert dev(fake, p, 4, 0, None, 4, p, None) == bad
    assert host(fake, idx, 4, None, 4, off) == bad
    # more than 2^31 elements
    assert dev(fake, p, (1 << 31) + 1, 0, p, 4, p, None) == bad
    assert dev(fake, p, (1 << 31) + 1, 0, None, 0, p, None) == bad
    assert host(fake, idx, (1 << 31) + 1, p, 4, off) == bad
    # an index base no corpus fits behind
    assert dev(fake, p, 4, (1 << 32) + 1, p, 4, p, None) == bad
    assert dev(fake, None, 0, (1 << 32) + 1, None, 0, p, None) == bad
    # device pointers the kernels' vector accesses cannot take: packed rows off 16 bytes, keys or offsets off 8
    assert dev(fake, p, 4, 0, p + 8, 4, p, None) == bad
    assert dev(fake, p + 4, 4, 0, p, 4, p, None) == bad
    assert dev(fake, p, 4, 0, p, 4, p + 4, None) == bad
    assert list(off) == [0xDEAD] * 5 and not any(buf)


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks both calls report kLBAudioDetectiveDeviceUnavailable, the copy
    returns NULL (and none of them reads a handle)."""
    Lib = lb.lib()
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    buf, p, fake, idx, off = _fakes(lb)
    dev, host, copy = (getattr(Lib, s) for s in SYMBOLS)
    assert dev(fake, p, 4, 0, p, 4, p, None) == nogp
    assert dev(fake, p, 4, 1 << 32, None, 0, p, None) == nogp          # the sizing call
    assert dev(fake, None, 0, 12345, None, 0, p, None) == nogp
    assert dev(fake, p, 1 << 31, 0, p, 1 << 40, p, None) == nogp
    assert host(fake, idx, 4, p, 4, off) == nogp
    assert host(fake, idx, 4, None, 0, off) == nogp
    assert host(fake, None, 0, None, 0, off) == nogp
    assert copy(fake, 0) is None
    assert list(off) == [0xDEAD] * 5 and not any(buf)


def test_gather_kernels_use_no_scratch(tmp_path):
    """k_gather.hip compiles for gfx950 with the Makefile's flags; every kernel in it -- lengths, tiles, offsets and the two
    copies -- reports 0 bytes of private segment and no spilled register, scalar or vector (the metadata only)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_gather.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_gather.hip")
    assert os.path.exists(src), "k_gather.hip is missing"
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-x", "hip", "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"),
           src, "-o", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    for kernel in ("gather_lengths_kernel", "gather_tiles_kernel", "gather_offsets_kernel", "gather_copy_planes_kernel",
                   "gather_copy_records_kernel"):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == 1, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 5, sorted(meta)
    # the tile constant is declared where the GPU tests read it
    assert re.search(r"constexpr\s+uint32_t\s+kGatherTileKeys\s*=\s*\d+\s*;", open(src).read())
