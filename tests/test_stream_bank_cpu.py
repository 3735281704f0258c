"""CPU checks of the stream bank: the nine symbols and their declared signatures (header, _native._SIGNATURES and the library
agree), the Python names, the argument checks that need neither a device nor a handle, the no-device status, the host plan of a
push against three lines of numpy, and the compiled kernels of k_stream_bank.hip (no scratch memory, no spilled register)."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

BANK = "LBAudioDetectiveStreamBank"
SYMBOLS = (BANK + "New", BANK + "Dispose", BANK + "PushDevice", BANK + "Push", BANK + "GetCounts", BANK + "WindowDevice",
           BANK + "CopyFingerprint", BANK + "ResetChannels", "LBAudioDetectiveDebugStreamBankPlan")


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
    u32p, u64p = C.POINTER(N.UInt32), C.POINTER(N.UInt64)
    ctype = {"LBAudioDetectiveStreamBankRef": N.Ref, "LBAudioDetectiveRef": N.Ref, "LBAudioDetectiveFingerprintRef": N.Ref,
             "OSStatus": N.OSStatus, "void": None, "void*": C.c_void_p, "const Float32*": C.c_void_p, "UInt32": N.UInt32, "UInt64": N.UInt64,
             "const UInt32*": u32p, "UInt32*": u32p, "UInt64*": u64p}
    bank, push = "LBAudioDetectiveStreamBankRef", ["LBAudioDetectiveStreamBankRef", "const Float32*", "const UInt32*", "UInt32*", "void*", "UInt64", "UInt64*", "void*"]
    want = {
        SYMBOLS[0]: (bank, ["LBAudioDetectiveRef", "UInt32", "UInt32", "UInt32"]),
        SYMBOLS[1]: ("void", [bank]),
        SYMBOLS[2]: ("OSStatus", push),
        SYMBOLS[3]: ("OSStatus", push),
        SYMBOLS[4]: ("OSStatus", [bank, "UInt64*", "UInt32*"]),
        SYMBOLS[5]: ("OSStatus", [bank, "const UInt32*", "UInt32", "UInt32", "void*", "void*"]),
        SYMBOLS[6]: ("LBAudioDetectiveFingerprintRef", [bank, "UInt32"]),
        SYMBOLS[7]: ("OSStatus", [bank, "const UInt32*", "UInt32"]),
        SYMBOLS[8]: ("OSStatus", ["UInt32", "UInt32", "UInt32", "UInt32", "const UInt32*", "const UInt32*", "UInt32*", "UInt32*", "UInt32*"]),
    }
    assert len(want) == 9
    for name, (ret, params) in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert _prototype(name) == (ret, params), (name, _prototype(name))
        res, args = N._SIGNATURES[name]
        assert res is ctype[ret] and args == [ctype[p] for p in params], (name, res, args)
    # every declared function has a signature and the other way round; no status constant was added
    funcs, consts = N.declared_symbols()
    assert set(SYMBOLS) <= set(funcs) and set(funcs) == set(N._SIGNATURES)
    assert len(consts) == 10 and len(N.CONSTANTS) == 10


def test_python_names(lb):
    for attr in ("push_device", "push", "totals", "pending", "window_device", "fingerprint", "reset", "dispose", "identify"):
        assert callable(getattr(lb.StreamBank, attr)), attr
    assert "StreamBank" in lb.__all__ and callable(lb.debug_stream_bank_plan)
    assert lb.Stream is not lb.StreamBank and callable(lb.Stream.push)


def _fakes(lb):
    N = lb._native
    buf = (C.c_uint64 * 16)()
    p = (C.addressof(buf) + 15) & ~15      # 16-byte aligned; stands for a device pointer and for a handle: never dereferenced
    counts = (N.UInt32 * 4)(5, 0, 7, 1)
    new = (N.UInt32 * 4)(*([0xDEAD] * 4))
    total = N.UInt64(0xDEAD)
    return buf, p, C.c_void_p(p), counts, new, total


def _untouched(buf, new, total):
    return list(new) == [0xDEAD] * 4 and total.value == 0xDEAD and not any(buf)


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle: the calls return on a machine without a
    GPU, with handles that are never read, and nothing is written."""
    Lib = lb.lib()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    buf, p, fake, counts, new, total = _fakes(lb)
    make, dispose, push_dev, push_host, get, window, copy, reset, plan = (getattr(Lib, s) for s in SYMBOLS)
    # creation: a NULL detective, zero channels, zero history
    assert make(None, 4, 3, 0) is None
    assert make(fake, 0, 3, 0) is None
    assert make(fake, 4, 0, 0) is None
    dispose(None)
    for push in (push_dev, push_host):
        assert push(None, p, counts, new, p, 100, C.byref(total), None) == bad               # a NULL bank
        assert push(fake, p, None, new, p, 100, C.byref(total), None) == bad                 # NULL counts
        assert push(fake, p + 2, counts, new, p, 100, C.byref(total), None) == bad           # samples off 4 bytes
        assert push(fake, p, counts, new, p + 8, 100, C.byref(total), None) == bad           # packed rows off 16 bytes
        assert push(fake, p, counts, new, p + 4, 100, C.byref(total), None) == bad
    assert get(None, (lb._native.UInt64 * 4)(), None) == bad
    assert get(fake, None, None) == bad
    assert window(None, counts, 4, 1, p, None) == bad
    assert window(fake, None, 4, 1, p, None) == bad                                          # a NULL list with a count
    assert window(fake, counts, 4, 1, None, None) == bad                                     # a NULL outPacked
    assert window(fake, counts, 4, 1, p + 8, None) == bad                                    # ... off 16 bytes
    assert window(fake, counts, 4, 0, p, None) == bad                                        # an empty window
    assert copy(None, 0) is None
    assert reset(None, counts, 4) == bad
    assert reset(fake, None, 4) == bad
    assert _untouched(buf, new, total)
    # the plan: NULL pointers, no channel, no history, a window that is none, a stride of 0, more carried than a channel can carry
    out = [(lb._native.UInt32 * 4)(*([0xDEAD] * 4)) for _ in range(3)]
    pend = (lb._native.UInt32 * 4)(0, 1, 2, 3)
    assert plan(1024, 64, 3, 4, pend, counts, *out) == 0
    assert [list(o) for o in out] == [[0] * 4, [5, 1, 9, 4], [0] * 4]
    out = [(lb._native.UInt32 * 4)(*([0xDEAD] * 4)) for _ in range(3)]
    for args in ((1024, 64, 3, 4, None, counts), (1024, 64, 3, 4, pend, None), (1024, 64, 3, 0, pend, counts), (1024, 64, 0, 4, pend, counts),
                 (1000, 64, 3, 4, pend, counts), (1024, 0, 3, 4, pend, counts), (1024, 64, 3, 4, (lb._native.UInt32 * 4)(0, 0, 1024 + 8192, 0), counts)):
        assert plan(*args, *out) == bad, args
    assert plan(1024, 64, 3, 4, pend, counts, out[0], None, out[2]) == bad
    assert [list(o) for o in out] == [[0xDEAD] * 4] * 3


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the first checks every call reports kLBAudioDetectiveDeviceUnavailable (the
    handle-returning ones NULL), and none of them reads a handle or writes anything."""
    Lib = lb.lib()
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    buf, p, fake, counts, new, total = _fakes(lb)
    make, dispose, push_dev, push_host, get, window, copy, reset, plan = (getattr(Lib, s) for s in SYMBOLS)
    assert make(fake, 4, 3, 0) is None
    for push in (push_dev, push_host):
        assert push(fake, p, counts, new, p, 100, C.byref(total), None) == nogp
        assert push(fake, p + 4, counts, None, None, 0, None, None) == nogp
        assert push(fake, None, counts, new, None, 0, C.byref(total), None) == nogp
    totals = (lb._native.UInt64 * 4)(*([0xDEAD] * 4))
    assert get(fake, totals, None) == nogp and list(totals) == [0xDEAD] * 4
    assert window(fake, counts, 4, 1, p, None) == nogp
    assert window(fake, None, 0, 1, p, None) == nogp
    assert copy(fake, 0) is None
    assert reset(fake, counts, 4) == nogp
    assert _untouched(buf, new, total)
    with pytest.raises(lb.LBAudioDetectiveError):
        lb.StreamBank(lb.Detective(), 4, 3)


@pytest.mark.parametrize("window,stride", [(1024, 64), (2048, 64), (64, 8)])
@pytest.mark.parametrize("history", [1, 3])
def test_plan_matches_numpy(lb, window, stride, history):
    """carried and new counts from: 0, 1, hop - 1, hop, what brings the sum to W + hop - 1, W + hop and W + 3 hop + 5, and carried
    above hop with at least two frames -- every pair of them a channel can meet (carried < W + hop)"""
    hop = 128 * stride
    carried = [p for p in (0, 1, hop - 1, hop, hop + 1, window + hop - 1) if p < window + hop]
    pairs = []
    for p in carried:
        fresh = [0, 1, hop - 1, hop] + [s - p for s in (window + hop - 1, window + hop, window + 3 * hop + 5) if s >= p]
        if p > hop:
            fresh += [window + 2 * hop - p, window + 2 * hop - p + 17]                       # two frames
        pairs += list(itertools.product([p], fresh))
    p, n = (np.array(x, dtype=np.int64) for x in zip(*pairs))
    assert ((p > hop) & (((p + n - window) // stride) // 128 >= 2) & (p + n >= window)).any()
    ready, after, kept = lb.debug_stream_bank_plan(window, stride, history, p, n)
    # three lines of numpy
    want_ready = np.where(p + n < window, 0, ((p + n - window) // stride) // 128)
    want_after = p + n - want_ready * hop
    want_kept = np.minimum(want_ready, history)
    assert np.array_equal(ready, want_ready) and np.array_equal(after, want_after) and np.array_equal(kept, want_kept)
    assert (after < window + hop).all() and want_ready.max() == 3
    det = lb.Detective().configure(window=window, stride=stride)
    for q in np.unique(p + n):                                                               # the count StreamPush uses
        assert want_ready[p + n == q][0] == det.subfingerprint_count(int(q))


def test_stream_bank_kernels_use_no_scratch(tmp_path):
    """k_stream_bank.hip compiles for gfx950 with the Makefile's flags; every kernel in it -- stage, the two commits and the
    window -- reports 0 bytes of private segment and no spilled register, scalar or vector (the metadata only)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_stream_bank.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_stream_bank.hip")
    assert os.path.exists(src), "k_stream_bank.hip is missing"
    assert re.search(r"SRCS\s*:=[^\n]*\bk_stream_bank\.hip\b(?:.*\\\n)*.*\bapi_stream_bank\.cpp\b",
                     open(os.path.join(os.path.dirname(src), "Makefile")).read())
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
    for kernel in ("bank_stage_kernel", "bank_commit_rows_kernel", "bank_commit_carry_kernel", "bank_window_kernel"):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == 1, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 4, sorted(meta)
