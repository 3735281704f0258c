"""CPU checks of the corpus join: the three symbols and their declared signatures, the Python names, the argument checks that
need neither a device nor a handle, the no-device status, decode_join_keys on hand-made CSR, and the compiled kernels of
k_join.hip (no scratch memory, no register spilled to it)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

SYMBOLS = ("LBAudioDetectiveCorpusJoinThresholdKeysDevice", "LBAudioDetectiveCorpusJoinThreshold",
           "LBAudioDetectiveCorpusSetJoinScratchLimit")


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
    ctype = {"LBAudioDetectiveCorpusRef": N.Ref, "void*": C.c_void_p, "UInt32": N.UInt32, "UInt64": N.UInt64, "Float32": N.Float32,
             "SInt64*": C.POINTER(N.SInt64), "Float32*": C.POINTER(N.Float32), "UInt64*": C.POINTER(N.UInt64)}
    ref, dev = "LBAudioDetectiveCorpusRef", "void*"
    want = {
        SYMBOLS[0]: [ref, ref, "UInt64", "UInt64", "UInt32", "Float32", "UInt32", "UInt64", "UInt64", dev, dev, dev],
        SYMBOLS[1]: [ref, ref, "UInt64", "UInt64", "UInt32", "Float32", "UInt32", "UInt64", "SInt64*", "SInt64*", "Float32*", "UInt64*"],
        SYMBOLS[2]: [ref, "UInt64"],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [ctype[p] for p in params], (name, args)
    # no status constant was added: a cut list is no error
    assert len(lb._native.declared_symbols()[1]) == 10


def test_python_names(lb):
    for attr in ("join_threshold_keys_device", "join_threshold", "set_join_scratch_limit"):
        assert callable(getattr(lb.Corpus, attr))
    assert callable(lb.decode_join_keys) and "decode_join_keys" in lb.__all__


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle: the calls return on a machine without a
    GPU, with corpus handles that are never read."""
    Lib = lb.lib()
    N = lb._native
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    fake = C.c_void_p(p)                  # ... and for a corpus handle
    rows, idx, sc, total = (N.SInt64 * 4)(), (N.SInt64 * 4)(), (N.Float32 * 4)(), N.UInt64(0)
    dev, host = Lib.LBAudioDetectiveCorpusJoinThresholdKeysDevice, Lib.LBAudioDetectiveCorpusJoinThreshold
    for t in (0.0, -1.0, float("nan"), float("inf"), -0.0):
        assert dev(fake, fake, 0, 1, 0, t, 0, 4, 0, p, p, None) == bad, t
        assert host(fake, fake, 0, 1, 0, t, 0, 4, rows, idx, sc, C.byref(total)) == bad, t
    for capacity in (0, (1 << 31) + 1):
        assert dev(fake, fake, 0, 1, 0, 0.7, 0, capacity, 0, p, p, None) == bad
        assert host(fake, fake, 0, 1, 0, 0.7, 0, capacity, rows, idx, sc, C.byref(total)) == bad
    # no rows
    assert dev(fake, fake, 0, 0, 0, 0.7, 0, 4, 0, p, p, None) == bad
    assert host(fake, fake, 0, 0, 0, 0.7, 0, 4, rows, idx, sc, C.byref(total)) == bad
    # rows that no corpus can hold (its entries are counted in 32 bits)
    assert dev(fake, fake, 1 << 32, 1, 0, 0.7, 0, 4, 0, p, p, None) == bad
    assert dev(fake, fake, 0, (1 << 32) + 1, 0, 0.7, 0, 4, 0, p, p, None) == bad
    # NULL handles and pointers
    assert dev(None, fake, 0, 1, 0, 0.7, 0, 4, 0, p, p, None) == bad
    assert dev(fake, None, 0, 1, 0, 0.7, 0, 4, 0, p, p, None) == bad
    assert dev(fake, fake, 0, 1, 0, 0.7, 0, 4, 0, None, p, None) == bad
    assert dev(fake, fake, 0, 1, 0, 0.7, 0, 4, 0, p, None, None) == bad
    assert host(None, fake, 0, 1, 0, 0.7, 0, 4, rows, idx, sc, C.byref(total)) == bad
    assert host(fake, None, 0, 1, 0, 0.7, 0, 4, rows, idx, sc, C.byref(total)) == bad
    assert host(fake, fake, 0, 1, 0, 0.7, 0, 4, None, idx, sc, C.byref(total)) == bad
    assert host(fake, fake, 0, 1, 0, 0.7, 0, 4, rows, None, sc, C.byref(total)) == bad
    assert host(fake, fake, 0, 1, 0, 0.7, 0, 4, rows, idx, None, C.byref(total)) == bad
    assert host(fake, fake, 0, 1, 0, 0.7, 0, 4, rows, idx, sc, None) == bad
    assert Lib.LBAudioDetectiveCorpusSetJoinScratchLimit(None, 1 << 20) == bad
    # an index base no corpus fits behind
    assert dev(fake, fake, 0, 1, 0, 0.7, 0, 4, (1 << 32) + 1, p, p, None) == bad


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks both calls report kLBAudioDetectiveDeviceUnavailable (and still
    read no handle)."""
    Lib = lb.lib()
    N = lb._native
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    fake = C.c_void_p(p)
    rows, idx, sc, total = (N.SInt64 * 4)(), (N.SInt64 * 4)(), (N.Float32 * 4)(), N.UInt64(0)
    assert Lib.LBAudioDetectiveCorpusJoinThresholdKeysDevice(fake, fake, 0, 1, 0, 0.7, 1, 4, 0, p, p, None) == nogp
    assert Lib.LBAudioDetectiveCorpusJoinThresholdKeysDevice(fake, fake, 5, 100, 64, 1.5, 0, 1 << 31, 1 << 32, p, p, None) == nogp   # (t > 1 is legal)
    assert Lib.LBAudioDetectiveCorpusJoinThreshold(fake, fake, 0, 1, 0, 0.7, 1, 4, rows, idx, sc, C.byref(total)) == nogp


def _key(score, index):
    return (int(np.float32(score).view(np.uint32)) << 32) | (0xFFFFFFFF - index)


def test_decode_join_keys(lb):
    # five rows: empty rows first, in the middle and last
    keys = np.array([_key(0.9, 4), _key(0.75, 9), _key(1.0, 0), 0, 0], np.uint64).view(np.int64)
    offsets = np.array([0, 0, 2, 2, 3, 3], np.int64)
    rows, idx, sc, total = lb.decode_join_keys(keys, offsets)
    assert total == 3 and rows.tolist() == [1, 1, 3] and idx.tolist() == [4, 9, 0]
    assert sc.dtype == np.float32 and sc.tolist() == [np.float32(0.9), np.float32(0.75), 1.0]
    rows, _, _, _ = lb.decode_join_keys(keys, offsets, first=100)           # the call's first row
    assert rows.tolist() == [101, 101, 103]
    # a cut list: seven matches, room for four; the total is the true one
    keys = np.array([_key(0.8, 1), _key(0.8, 2), _key(0.7, 0), _key(0.7, 5)], np.uint64).view(np.int64)
    offsets = np.array([0, 2, 2, 5, 7], np.int64)
    rows, idx, sc, total = lb.decode_join_keys(keys, offsets)
    assert total == 7 and rows.tolist() == [0, 0, 2, 2] and idx.tolist() == [1, 2, 0, 5]
    # nothing matched; torch tensors decode as well
    rows, idx, sc, total = lb.decode_join_keys(torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    assert total == 0 and len(rows) == len(idx) == len(sc) == 0
    # an index above 2^31 and a key whose score bits set the sign of the int64 view
    keys = np.array([_key(1.0, 0xFFFFFFF0)], np.uint64).view(np.int64)
    rows, idx, sc, total = lb.decode_join_keys(keys, np.array([0, 1], np.int64))
    assert rows.tolist() == [0] and idx.tolist() == [0xFFFFFFF0] and sc.tolist() == [1.0]


def test_join_kernels_use_no_scratch(tmp_path):
    """k_join.hip compiles for gfx950 with the Makefile's flags; every kernel in it -- the builder, the two scans and the count
    and scatter kernels of 1 .. 8 sub-fingerprints -- reports 0 bytes of private segment and no spilled register, scalar or
    vector (the metadata only)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_join.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_join.hip")
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
    for kernel, instances in (("join_build_rows_kernel", 1), ("join_row_scan_kernel", 1), ("join_offsets_kernel", 1),
                              ("join_count_kernel", 8), ("join_scatter_kernel", 8)):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == instances, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 19, sorted(meta)
