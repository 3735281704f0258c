"""CPU checks of the removal of corpus entries: the three symbols and their declared signatures, the Python names, the argument
checks that need neither a device nor a handle, the no-device status, and the compiled kernels of k_remove.hip (no scratch
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

SYMBOLS = ("LBAudioDetectiveCorpusRemoveIndices", "LBAudioDetectiveCorpusRemoveKeysDevice",
           "LBAudioDetectiveCorpusSetRemoveScratchLimit")


def _has_gpu():
    return torch.cuda.is_available()


def _prototype(name):
    """the parameter types of `name` as include/lbaudiodetective.h declares it, comments removed"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lbaudiodetective.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return m.group(1), [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(2).split(",")]


def test_symbols_exist_with_the_declared_signatures(lb):
    N = lb._native
    raw = C.CDLL(lb.LIB_PATH)
    ctype = {"LBAudioDetectiveCorpusRef": N.Ref, "void*": C.c_void_p, "const void*": C.c_void_p, "UInt64": N.UInt64,
             "const UInt64*": C.POINTER(N.UInt64), "UInt32*": C.POINTER(N.UInt32), "UInt64*": C.POINTER(N.UInt64)}
    ref = "LBAudioDetectiveCorpusRef"
    want = {
        SYMBOLS[0]: [ref, "const UInt64*", "UInt64", "UInt32*", "UInt64*"],
        SYMBOLS[1]: [ref, "const void*", "UInt64", "UInt64", "void*", "UInt64*", "void*"],
        SYMBOLS[2]: [ref, "UInt64"],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [ctype[p] for p in params], (name, args)
    # no status constant was added
    assert len(lb._native.declared_symbols()[1]) == 10


def test_python_names(lb):
    for attr in ("remove", "remove_keys_device", "set_remove_scratch_limit"):
        assert callable(getattr(lb.Corpus, attr))
    assert not hasattr(lb.ShardedCorpus, "remove")       # (removing from one shard would shift the bases of all later ones)


def _fakes(lb):
    N = lb._native
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer and for a corpus handle: never dereferenced
    return buf, p, C.c_void_p(p), (N.UInt64 * 4)(0, 1, 2, 3), (N.UInt32 * 4)(), N.UInt64(0)


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle: the calls return on a machine without a
    GPU, with corpus handles that are never read."""
    Lib = lb.lib()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    buf, p, fake, idx, new, removed = _fakes(lb)
    host, dev = Lib.LBAudioDetectiveCorpusRemoveIndices, Lib.LBAudioDetectiveCorpusRemoveKeysDevice
    # NULL handle, NULL outRemoved, NULL list with a non-zero count
    assert host(None, idx, 4, new, C.byref(removed)) == bad
    assert host(fake, idx, 4, new, None) == bad
    assert host(fake, None, 4, new, C.byref(removed)) == bad
    assert host(None, None, 0, None, C.byref(removed)) == bad
    assert dev(None, p, 4, 0, p, C.byref(removed), None) == bad
    assert dev(fake, p, 4, 0, p, None, None) == bad
    assert dev(fake, None, 4, 0, p, C.byref(removed), None) == bad
    assert dev(None, None, 0, 0, None, C.byref(removed), None) == bad
    # an index base no corpus fits behind
    assert dev(fake, p, 4, (1 << 32) + 1, p, C.byref(removed), None) == bad
    assert dev(fake, None, 0, (1 << 32) + 1, None, C.byref(removed), None) == bad
    assert Lib.LBAudioDetectiveCorpusSetRemoveScratchLimit(None, 1 << 20) == bad
    assert removed.value == 0


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks both calls report kLBAudioDetectiveDeviceUnavailable (and still
    read no handle)."""
    Lib = lb.lib()
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    buf, p, fake, idx, new, removed = _fakes(lb)
    host, dev = Lib.LBAudioDetectiveCorpusRemoveIndices, Lib.LBAudioDetectiveCorpusRemoveKeysDevice
    assert host(fake, idx, 4, new, C.byref(removed)) == nogp
    assert host(fake, idx, 4, None, C.byref(removed)) == nogp
    assert host(fake, None, 0, None, C.byref(removed)) == nogp
    assert dev(fake, p, 4, 0, p, C.byref(removed), None) == nogp
    assert dev(fake, p, 4, 1 << 32, None, C.byref(removed), None) == nogp
    assert dev(fake, None, 0, 12345, None, C.byref(removed), None) == nogp


def test_remove_kernels_use_no_scratch(tmp_path):
    """k_remove.hip compiles for gfx950 with the Makefile's flags; every kernel in it -- the two mark kernels, count, offsets,
    map, the two gathers and the scatter -- reports 0 bytes of private segment and no spilled register, scalar or vector (the
    metadata only)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_remove.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_remove.hip")
    assert os.path.exists(src), "k_remove.hip is missing"
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
    for kernel, instances in (("remove_mark_kernel", 2), ("remove_count_kernel", 1), ("remove_offsets_kernel", 1),
                              ("remove_map_kernel", 1), ("remove_gather_planes_kernel", 1), ("remove_gather_records_kernel", 1),
                              ("remove_scatter_kernel", 1)):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == instances, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 8, sorted(meta)
