"""CPU checks of the resampler bank: the eight symbols and their declared signatures (header, _native._SIGNATURES and the library
agree), the Python names, the argument checks that need neither a device nor a handle, the pairs New refuses, the no-device status,
the host plan of a call against the definition -- brute force and the independent oracle converter --, and the compiled kernels of
k_resample_bank.hip (no scratch memory, no spilled register)."""
import ctypes as C
import os
import re
import shutil
import subprocess
from math import gcd

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

BANK = "LBAudioDetectiveResamplerBank"
SYMBOLS = (BANK + "New", BANK + "Dispose", BANK + "PushDevice", BANK + "Push", BANK + "FinishChannels", BANK + "GetCounts",
           BANK + "ResetChannels", "LBAudioDetectiveDebugResamplerBankPlan")
# (rate in, rate out, mode): the pairs the definition was checked on
PAIRS = [(44100, 5512, 0), (48000, 5512, 0), (8000, 44100, 0), (44100, 48000, 0), (44100, 5512, 1), (48000, 8000, 1)]
SEED = 0x52534231


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
    u32p, u64p, s32p = C.POINTER(N.UInt32), C.POINTER(N.UInt64), C.POINTER(N.SInt32)
    ctype = {"LBAudioDetectiveResamplerBankRef": N.Ref, "OSStatus": N.OSStatus, "void": None, "void*": C.c_void_p, "const void*": C.c_void_p,
             "Float32*": C.c_void_p, "Float64": N.Float64, "UInt32": N.UInt32, "UInt64": N.UInt64, "const UInt32*": u32p, "UInt32*": u32p,
             "UInt64*": u64p, "const UInt64*": u64p, "SInt32*": s32p}
    bank = "LBAudioDetectiveResamplerBankRef"
    push = [bank, "const void*", "UInt32", "const UInt32*", "UInt32*", "Float32*", "UInt64", "UInt64*", "void*"]
    want = {
        SYMBOLS[0]: (bank, ["Float64", "Float64", "UInt32", "UInt32"]),
        SYMBOLS[1]: ("void", [bank]),
        SYMBOLS[2]: ("OSStatus", push),
        SYMBOLS[3]: ("OSStatus", push),
        SYMBOLS[4]: ("OSStatus", [bank, "const UInt32*", "UInt32", "UInt32*", "Float32*", "UInt64", "UInt64*", "void*"]),
        SYMBOLS[5]: ("OSStatus", [bank, "UInt64*", "UInt64*"]),
        SYMBOLS[6]: ("OSStatus", [bank, "const UInt32*", "UInt32"]),
        SYMBOLS[7]: ("OSStatus", ["Float64", "Float64", "UInt32", "UInt32", "const UInt64*", "const UInt64*", "const UInt32*", "UInt32",
                                  "UInt32*", "UInt32*", "SInt32*", "SInt32*"]),
    }
    assert len(want) == 8
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
    for attr in ("push_device", "push", "finish", "totals", "reset", "dispose", "feed"):
        assert callable(getattr(lb.ResamplerBank, attr)), attr
    assert "ResamplerBank" in lb.__all__ and "debug_resampler_bank_plan" in lb.__all__ and callable(lb.debug_resampler_bank_plan)
    assert lb.ResamplerBank is not lb.StreamBank


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
    make, dispose, push_dev, push_host, finish, get, reset, plan = (getattr(Lib, s) for s in SYMBOLS)
    dispose(None)
    for push in (push_dev, push_host):
        assert push(None, p, 0, counts, new, p, 100, C.byref(total), None) == bad            # a NULL bank
        assert push(fake, p, 0, None, new, p, 100, C.byref(total), None) == bad              # NULL counts
        assert push(fake, p + 2, 0, counts, new, p, 100, C.byref(total), None) == bad        # float32 samples off 4 bytes
        assert push(fake, p + 1, 0, counts, new, p, 100, C.byref(total), None) == bad
        assert push(fake, p + 1, 1, counts, new, p, 100, C.byref(total), None) == bad        # int16 samples off 2 bytes
        assert push(fake, p + 3, 1, counts, new, p, 100, C.byref(total), None) == bad
        assert push(fake, p, 2, counts, new, p, 100, C.byref(total), None) == bad            # a format that is none
        assert push(fake, p, 0xFFFFFFFF, counts, new, p, 100, C.byref(total), None) == bad
        assert push(fake, p, 0, counts, new, p + 2, 100, C.byref(total), None) == bad        # outSamples off 4 bytes
        assert push(fake, p, 1, counts, new, p + 1, 100, C.byref(total), None) == bad
    assert finish(None, counts, 4, new, p, 100, C.byref(total), None) == bad
    assert finish(fake, None, 4, new, p, 100, C.byref(total), None) == bad                   # a NULL list with a count
    assert finish(fake, counts, 4, new, p + 2, 100, C.byref(total), None) == bad             # outSamples off 4 bytes
    u64 = (lb._native.UInt64 * 4)(*([0xDEAD] * 4))
    assert get(None, u64, u64) == bad
    assert get(fake, None, None) == bad
    assert reset(None, counts, 4) == bad
    assert reset(fake, None, 4) == bad
    assert _untouched(buf, new, total) and list(u64) == [0xDEAD] * 4
    # the plan: NULL pointers, no channel, a pair the bank does not take, an output total that is not the input total's
    zeros = (lb._native.UInt64 * 4)()
    out = [(lb._native.UInt32 * 4)(*([0xDEAD] * 4)) for _ in range(2)]
    lo, hi = lb._native.SInt32(7), lb._native.SInt32(7)
    assert plan(44100.0, 5512.0, 0, 4, zeros, zeros, counts, 0, *out, C.byref(lo), C.byref(hi)) == 0
    assert [list(o) for o in out] == [[0] * 4, [5, 0, 7, 1]] and (lo.value, hi.value) == (-192, 193)
    out = [(lb._native.UInt32 * 4)(*([0xDEAD] * 4)) for _ in range(2)]
    lo, hi = lb._native.SInt32(7), lb._native.SInt32(7)
    ones = (lb._native.UInt64 * 4)(1, 1, 1, 1)
    for args in ((44100.0, 5512.0, 0, 4, None, zeros, counts, 0), (44100.0, 5512.0, 0, 4, zeros, None, counts, 0),
                 (44100.0, 5512.0, 0, 4, zeros, zeros, None, 0), (44100.0, 5512.0, 0, 0, zeros, zeros, counts, 0),
                 (44100.0, 44100.0, 0, 4, zeros, zeros, counts, 0), (44100.0, 5512.0, 2, 4, zeros, zeros, counts, 0),
                 (44100.5, 5512.0, 0, 4, zeros, zeros, counts, 0), (44100.0, 5512.0, 0, 4, zeros, ones, counts, 0)):
        assert plan(*args, *out, C.byref(lo), C.byref(hi)) == bad, args
    assert plan(44100.0, 5512.0, 0, 4, zeros, zeros, counts, 0, out[0], None, C.byref(lo), C.byref(hi)) == bad
    assert [list(o) for o in out] == [[0xDEAD] * 4] * 2 and (lo.value, hi.value) == (7, 7)


def test_new_refuses_what_the_bank_cannot_convert(lb):
    """equal rates, a mode that is none, no channel (too many), a rate that is no whole number of Hz, q > 16384, a tap span beyond
    what a workgroup stages -- with or without a device"""
    make = getattr(lb.lib(), SYMBOLS[0])
    for args in ((44100.0, 44100.0, 0, 4), (44100.0, 5512.0, 2, 4), (44100.0, 5512.0, 3, 4), (44100.0, 5512.0, 0, 0),
                 (44100.0, 5512.0, 0, (1 << 24) + 1), (44100.5, 5512.0, 0, 4), (44100.0, 44101.0, 0, 4), (0.0, 5512.0, 0, 4),
                 (44100.0, -1.0, 0, 4), (float("nan"), 5512.0, 0, 4), (44100.0 * 60, 44100.0, 0, 4), (8000.0 * 400, 8000.0, 1, 4)):
        assert make(*args) is None, args
    with pytest.raises(lb.LBAudioDetectiveError):
        lb.ResamplerBank(44100, 44100, 4)
    # the header states the cap the last two pairs exceed (spans 2 x 24 x 60 + 1 and 2 x 4 x 400 + 1)
    header = open(os.path.join(ROOT, "include", "lbaudiodetective.h")).read()
    cap = int(re.search(r"#define LBAD_RESAMPLER_BANK_MAX_TAP_SPAN (\d+)", header).group(1))
    assert cap < 2 * 24 * 60 + 1 and cap < 2 * 4 * 400 + 1
    assert lb.debug_resampler_bank_plan(44100 * 50, 44100, 0, [0], [0], [0])[3] * 2 + 1 <= cap         # 50: within it


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the first checks every call reports kLBAudioDetectiveDeviceUnavailable (New:
    NULL), and none of them reads a handle or writes anything."""
    Lib = lb.lib()
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    buf, p, fake, counts, new, total = _fakes(lb)
    make, dispose, push_dev, push_host, finish, get, reset, plan = (getattr(Lib, s) for s in SYMBOLS)
    assert make(44100.0, 5512.0, 0, 4) is None
    for push in (push_dev, push_host):
        assert push(fake, p, 0, counts, new, p, 100, C.byref(total), None) == nogp
        assert push(fake, p + 2, 1, counts, new, p + 4, 100, C.byref(total), None) == nogp
        assert push(fake, None, 0, counts, None, None, 0, None, None) == nogp
    assert finish(fake, counts, 4, new, p, 100, C.byref(total), None) == nogp
    assert finish(fake, None, 0, new, None, 0, C.byref(total), None) == nogp
    u64 = (lb._native.UInt64 * 4)(*([0xDEAD] * 4))
    assert get(fake, u64, None) == nogp and list(u64) == [0xDEAD] * 4
    assert reset(fake, counts, 4) == nogp
    assert _untouched(buf, new, total)
    with pytest.raises(lb.LBAudioDetectiveError):
        lb.ResamplerBank(44100, 5512, 4)


@pytest.mark.parametrize("rate_in,rate_out,mode", PAIRS)
def test_plan_matches_the_definition_and_the_oracle(lb, oracle, rate_in, rate_out, mode):
    """For L in 0..39, m_hi - 1 .. m_hi + 2 and a few random values: the plan of L samples from the start emits emitted(L), counted
    by brute force as the n with (n p) div q + m_hi < L; those outputs are final -- the oracle's conversion of the signal with
    everything from L on replaced by 1e6 has the untouched signal's bits there --; with inFinish the total is the oracle's count
    for L samples; and the same L reached in two calls emits the same, carrying x[max(0, ip(next) + m_lo), L)."""
    g = gcd(rate_in, rate_out)
    p, q = rate_in // g, rate_out // g
    _, _, m_lo, m_hi = lb.debug_resampler_bank_plan(rate_in, rate_out, mode, [0], [0], [0])
    span = m_hi - m_lo + 1
    assert m_lo < 0 < m_hi
    if (rate_in, rate_out, mode) == (44100, 5512, 0):
        assert (m_lo, m_hi) == (-192, 193)
    n_sig = int(3 * span + 40 * max(rate_in / rate_out, 1.0) + 3000)
    x = oracle.synth_clip(SEED, 3, rate_in, n_sig)
    whole = oracle.resample(x, rate_in, rate_out, mode)
    rng = np.random.default_rng(SEED + rate_in + mode)
    lengths = sorted(set(list(range(40)) + list(range(m_hi - 1, m_hi + 3)) + [int(v) for v in rng.integers(m_hi + 3, n_sig - span, 30)]))
    zero = np.zeros(len(lengths), np.uint64)
    new, carried, _, _ = lb.debug_resampler_bank_plan(rate_in, rate_out, mode, zero, zero, lengths)
    finished = lb.debug_resampler_bank_plan(rate_in, rate_out, mode, zero, zero, lengths, finish=True)
    assert not finished[1].any()
    some = 0
    for i, L in enumerate(lengths):
        emitted = 0
        while (emitted * p) // q + m_hi < L:
            emitted += 1
        assert new[i] == emitted, (L, new[i], emitted)
        assert emitted == (0 if L <= m_hi else -((L - m_hi) * q // -p))                       # the closed form
        assert carried[i] == L - max(0, (emitted * p) // q + m_lo) and carried[i] < span
        assert finished[0][i] == int(oracle.lib().lbo_resample_count(L, float(rate_in), float(rate_out))) >= emitted
        spoiled = x.copy()
        spoiled[L:] = 1e6
        got = oracle.resample(spoiled, rate_in, rate_out, mode)
        assert emitted <= whole.size and np.array_equal(got[:emitted].view(np.uint32), whole[:emitted].view(np.uint32)), L
        if emitted < whole.size and L > m_hi:
            some += got[emitted].view(np.uint32) != whole[emitted].view(np.uint32)          # the next output does read x[L ...)
        # in two calls: a first, then the rest from the state the first leaves
        a = L // 3
        first = lb.debug_resampler_bank_plan(rate_in, rate_out, mode, [0], [0], [a])[0]
        rest = lb.debug_resampler_bank_plan(rate_in, rate_out, mode, [a], first, [L - a])
        assert int(first[0]) + int(rest[0][0]) == emitted and rest[1][0] == carried[i]
    assert some >= 1, "the spoiled samples were never in reach: the check above shows nothing"
    assert new[-1] > 300


def test_resampler_bank_kernels_use_no_scratch(tmp_path):
    """k_resample_bank.hip compiles for gfx950 with the Makefile's flags; every kernel in it -- convert and commit, each for
    float32 and for int16 samples -- reports 0 bytes of private segment and no spilled register, scalar or vector (the metadata
    only)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_resample_bank.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_resample_bank.hip")
    assert os.path.exists(src), "k_resample_bank.hip is missing"
    assert re.search(r"SRCS\s*:=[^\n]*\bk_resample_bank\.hip\b(?:.*\\\n)*.*\bapi_resampler_bank\.cpp\b",
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
    for kernel in ("resampler_bank_convert_kernel", "resampler_bank_commit_kernel"):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == 2, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 4, sorted(meta)
