"""CPU checks of the duplicate groups: the two symbols and their declared signatures, the Python names, every argument check
(all of them are decided before anything touches a device: the pointers below are never read), the no-device status, and the
compiled kernels of k_groups.hip (no scratch memory, no register spilled to it)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

LABELS = "LBAudioDetectiveGroupLabelsFromKeysDevice"
EXTRA = "LBAudioDetectiveGroupExtraKeysFromLabelsDevice"


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
    ctype = {"const void*": C.c_void_p, "void*": C.c_void_p, "UInt32": N.UInt32, "UInt64": N.UInt64, "UInt64*": C.POINTER(N.UInt64)}
    cdev, dev, u64 = "const void*", "void*", "UInt64"
    want = {
        LABELS: [cdev, u64, cdev, u64, u64, u64, cdev, u64, u64, "UInt32", dev, dev, dev],
        EXTRA: [cdev, u64, u64, u64, dev, "UInt64*", dev],
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
    for name in ("group_labels_from_keys_device", "group_extra_keys_from_labels_device"):
        assert callable(getattr(lb, name)) and name in lb.__all__
    for attr in ("duplicate_groups", "deduplicate"):
        assert callable(getattr(lb.Corpus, attr))


def _labels_args(p, **kw):
    """arguments of the labels call that pass every check (CSR form, 4 rows, 8 slots, 16 entries), then changed by name"""
    a = dict(keys=p, slots=8, offsets=p, pitch=0, rows=4, first=0, row_keys=None, base=0, n=16, reset=1, labels=p, count=p, stream=None)
    a.update(kw)
    return [a[k] for k in ("keys", "slots", "offsets", "pitch", "rows", "first", "row_keys", "base", "n", "reset", "labels", "count", "stream")]


def _extra_args(p, total, **kw):
    a = dict(labels=p, n=16, base=0, capacity=8, keys=p, count=C.byref(total), stream=None)
    a.update(kw)
    return [a[k] for k in ("labels", "n", "base", "capacity", "keys", "count", "stream")]


def test_bad_arguments_are_refused_before_anything_is_read(lb):
    Lib = lb.lib()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    assert p % 8 == 0
    labels, extra = getattr(Lib, LABELS), getattr(Lib, EXTRA)
    refused = [
        dict(labels=None),
        dict(keys=None),                                      # ... with slots to read
        dict(base=(1 << 32) + 1, n=0),
        dict(base=(1 << 32) - 15),                            # base + entries = 2^32 + 1
        dict(n=(1 << 32) + 1),
        dict(slots=(1 << 31) + 1),
        dict(rows=(1 << 32) + 1, n=1 << 32, row_keys=p),
        dict(first=13),                                       # 13 + 4 rows > 16 entries
        dict(first=0, rows=17),
        dict(first=1 << 63, rows=1 << 63),                    # (a sum that wraps)
        dict(offsets=None, pitch=0),                          # the pitch rules
        dict(offsets=None, pitch=3),                          # 4 x 3 != 8
        dict(offsets=None, pitch=2, slots=7),
        dict(offsets=None, pitch=1 << 62, rows=4, slots=0),   # (a product that wraps to 0)
        dict(offsets=None, pitch=0, rows=0, slots=0),
        dict(offsets=None, pitch=2, rows=0, slots=8),
        dict(keys=p + 4), dict(offsets=p + 4), dict(row_keys=p + 4), dict(labels=p + 2), dict(labels=p + 1),
    ]
    for kw in refused:
        assert labels(*_labels_args(p, **kw)) == bad, kw
    total = lb._native.UInt64(7)
    refused = [
        dict(labels=None), dict(keys=None), dict(count=None),
        dict(capacity=0), dict(capacity=(1 << 31) + 1),
        dict(base=(1 << 32) + 1, n=0), dict(base=(1 << 32) - 15), dict(n=(1 << 32) + 1),
        dict(labels=p + 2), dict(keys=p + 4),
    ]
    for kw in refused:
        assert extra(*_extra_args(p, total, **kw)) == bad, kw


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks both calls report kLBAudioDetectiveDeviceUnavailable (and still
    read nothing)."""
    Lib = lb.lib()
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    labels, extra = getattr(Lib, LABELS), getattr(Lib, EXTRA)
    passing = [
        dict(),
        dict(count=None, reset=0),
        dict(keys=None, slots=0),                              # no slot: no keys needed
        dict(offsets=None, pitch=2),                           # pitched rows, 4 x 2 = 8
        dict(offsets=None, pitch=5, rows=0, slots=0),
        dict(row_keys=p, first=1 << 40),                       # (the first row is not used with row keys)
        dict(first=12),
        dict(base=(1 << 32) - 16), dict(base=1 << 32, n=0, rows=0, slots=0),
        dict(slots=1 << 31), dict(rows=1 << 32, n=1 << 32, labels=p + 4),
    ]
    for kw in passing:
        assert labels(*_labels_args(p, **kw)) == nogp, kw
    total = lb._native.UInt64(7)
    for kw in (dict(), dict(capacity=1), dict(capacity=1 << 31), dict(n=0), dict(base=(1 << 32) - 16), dict(labels=p + 4)):
        assert extra(*_extra_args(p, total, **kw)) == nogp, kw
    assert total.value == 0


def test_groups_kernels_use_no_scratch(tmp_path):
    """k_groups.hip compiles for gfx950 with the Makefile's flags; every kernel in it -- init, hook and flatten, and the count,
    tile scan and scatter of the extra keys -- reports 0 bytes of private segment and no spilled register, scalar or vector
    (the metadata only)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_groups.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_groups.hip")
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
    for kernel in ("groups_init_kernel", "groups_hook_kernel", "groups_flatten_kernel", "groups_extra_count_kernel",
                   "groups_extra_tiles_kernel", "groups_extra_scatter_kernel"):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == 1, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 6, sorted(meta)
