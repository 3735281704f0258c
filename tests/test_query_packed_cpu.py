"""CPU checks of the packed-query feature (LBAudioDetectiveCorpusQueryPackedKeysDevice, ...QueryPackedTopKKeysDevice and the debug
entry point LBAudioDetectiveDebugQueryBlocks): the symbols and their declared signatures, the argument checks that need no device,
the host side of the debug entry point (the builders behind the handle-taking calls, which the device builders must reproduce)
and the compiled builder kernels of k_query.hip (no scratch memory, nothing spilled)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

TOP1 = "LBAudioDetectiveCorpusQueryPackedKeysDevice"
TOPK = "LBAudioDetectiveCorpusQueryPackedTopKKeysDevice"
DEBUG = "LBAudioDetectiveDebugQueryBlocks"


def _prototype(name):
    """(return type, [parameter types]) of `name` as include/lbaudiodetective.h declares it, comments removed"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lbaudiodetective.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    params = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(2).split(",")]      # drop the parameter names
    return m.group(1), params


def test_symbols_exist_with_the_declared_signatures(lb):
    N = lb._native
    raw = C.CDLL(lb.LIB_PATH)
    ctype = {"LBAudioDetectiveCorpusRef": N.Ref, "const void*": C.c_void_p, "void*": C.c_void_p, "UInt32": N.UInt32, "UInt64": N.UInt64,
             "const Boolean*": C.c_void_p, "UInt32*": C.c_void_p, "UInt64*": C.POINTER(N.UInt64), "OSStatus": N.OSStatus}
    want = {
        TOP1: ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "UInt32", "UInt64", "void*", "void*"],
        TOPK: ["LBAudioDetectiveCorpusRef", "const void*", "UInt32", "UInt32", "UInt32", "UInt32", "UInt64", "void*", "void*", "void*"],
        DEBUG: ["UInt32", "const void*", "const Boolean*", "UInt32", "UInt32", "UInt32", "UInt32", "UInt32*", "UInt64", "UInt64*"],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [ctype[p] for p in params], (name, args)
    # the Python layer offers them
    for attr in ("query_packed_keys_device", "query_packed_topk_keys_device"):
        assert callable(getattr(lb.Corpus, attr))
    assert callable(lb.identify_clips_device) and callable(lb.debug_query_blocks)


def test_null_and_zero_arguments_are_refused_without_a_device(lb):
    """Every refusal below is decided before anything touches a device: the calls return on a machine without one."""
    L = lb.lib()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    fake = C.c_void_p(p)                  # ... and for a corpus handle where another argument is refused first
    top1 = L.LBAudioDetectiveCorpusQueryPackedKeysDevice
    topk = L.LBAudioDetectiveCorpusQueryPackedTopKKeysDevice
    assert top1(None, p, 1, 5, 0, 0, p, None) == bad              # NULL corpus
    assert topk(None, p, 1, 5, 0, 1, 0, p, p, None) == bad
    assert topk(None, p, 1, 5, 0, 1, 0, p, None, None) == bad
    # (with a handle that is never read: the other arguments are looked at first)
    assert top1(fake, None, 1, 5, 0, 0, p, None) == bad           # NULL queries
    assert top1(fake, p, 1, 5, 0, 0, None, None) == bad           # NULL keys
    assert top1(fake, p, 0, 5, 0, 0, p, None) == bad              # no queries
    assert top1(fake, p, 1, 0, 0, 0, p, None) == bad              # no sub-fingerprints
    assert topk(fake, None, 1, 5, 0, 1, 0, p, p, None) == bad
    assert topk(fake, p, 1, 5, 0, 1, 0, None, p, None) == bad
    assert topk(fake, p, 0, 5, 0, 1, 0, p, p, None) == bad
    assert topk(fake, p, 1, 0, 0, 1, 0, p, p, None) == bad
    assert topk(fake, p, 1, 5, 0, 0, 0, p, p, None) == bad        # K outside 1 .. LBAD_TOPK_MAX
    assert topk(fake, p, 1, 5, 0, 1025, 0, p, p, None) == bad
    # the debug entry point: a kind that does not exist, no source, two sources, no count, shapes a builder does not take
    dbg = L.LBAudioDetectiveDebugQueryBlocks
    n = C.c_uint64(0)
    bools = np.zeros((1, 5, 200), np.uint8)
    b = bools.ctypes.data
    assert dbg(4, None, b, 1, 5, 200, 0, None, 0, C.byref(n)) == bad
    assert dbg(0, None, None, 1, 5, 200, 0, None, 0, C.byref(n)) == bad
    assert dbg(0, p, b, 1, 5, 200, 0, None, 0, C.byref(n)) == bad
    assert dbg(0, None, b, 1, 5, 200, 0, None, 0, None) == bad
    assert dbg(0, None, b, 0, 5, 200, 0, None, 0, C.byref(n)) == bad
    assert dbg(0, None, b, 1, 0, 200, 0, None, 0, C.byref(n)) == bad
    assert dbg(0, None, b, 1, 5, 199, 0, None, 0, C.byref(n)) == bad       # the specialised scan: 200 Booleans ...
    assert dbg(0, None, b, 1, 9, 200, 0, None, 0, C.byref(n)) == bad       # ... and at most 8 sub-fingerprints
    assert dbg(1, None, b, 1, 5, 201, 0, None, 0, C.byref(n)) == bad       # a ragged corpus: at most 200 Booleans
    # a capacity that is too small reports the size
    assert dbg(1, None, b, 1, 5, 200, 0, None, 0, C.byref(n)) == bad and n.value == 6 * 16
    assert dbg(0, None, b, 1, 5, 200, 0, None, 0, C.byref(n)) == bad and n.value == 144


def _f32(words):
    return np.asarray(words, np.uint32).view(np.float32)


def test_host_blocks_are_what_the_scans_document(lb):
    """The host side of the debug entry point (no device): layout facts the device builders are compared against on the GPU --
    an all-zero sub-fingerprint has possible = 0 and rh = rl = 0, an all-ones one counts every pair inside the range, bits are
    where the packed layout has them."""
    rng = np.random.default_rng(7)
    for n_sub in range(1, 9):
        b = rng.integers(0, 2, (3, n_sub, 200)).astype(np.uint8)
        b[0, 0] = 0
        b[1, n_sub - 1] = 1
        for rg, pairs in ((0, 100), (1, 1), (2, 1), (119, 60), (120, 60), (200, 100), (1000, 100)):
            blk = lb.debug_query_blocks(0, 3, n_sub, 200, rg, bools=b)
            assert blk.shape == (3, 144)
            planes = (n_sub * 200 + 127) // 128
            off = planes * 4 + 7 * n_sub
            # the tight bitstream
            bits = ((blk[:, :planes * 4, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(3, -1)[:, :n_sub * 200]
            assert np.array_equal(bits.astype(np.uint8), b.reshape(3, -1))
            poss = _f32(blk[:, off:off + n_sub])
            want = (b[:, :, :2 * pairs].reshape(3, n_sub, -1, 2).max(-1)).sum(-1)
            assert np.array_equal(poss, want.astype(np.float32))
            rh, rl = _f32(blk[:, off + n_sub:off + 2 * n_sub]), _f32(blk[:, off + 2 * n_sub:off + 3 * n_sub])
            assert poss[0, 0] == 0 and rh[0, 0] == 0 and rl[0, 0] == 0 and blk[0, off + n_sub] == 0 and blk[0, off + 2 * n_sub] == 0
            assert poss[1, n_sub - 1] == pairs
            with np.errstate(divide="ignore"):
                assert np.array_equal(rh, np.where(poss > 0, np.float32(1) / poss, np.float32(0)).astype(np.float32))
            assert not blk[:, off + 3 * n_sub:].any()                      # zero padding up to plane_query_words()
    for per in (1, 5, 12):
        for length in (200, 199, 64, 33):
            b = rng.integers(0, 2, (2, per, length)).astype(np.uint8)
            b[0, 0] = 0
            blk = lb.debug_query_blocks(1, 2, per, length, 0, bools=b).reshape(2, per + 1, 16)
            assert not blk[:, per].any()                                   # the zero sub-fingerprint of slack
            pairs = (length + 1) // 2
            pad = np.zeros((2, per, 2 * pairs), np.uint8)
            pad[:, :, :length] = b
            live = pad.reshape(2, per, pairs, 2).max(-1).sum(-1)
            assert np.array_equal(blk[:, :per, 13], live) and np.array_equal(blk[:, :per, 12], live * (live + 1) // 2)
            al = lb.debug_query_blocks(2, 2, per, length, 0, bools=b).reshape(2, per, 8)
            assert np.array_equal(al, blk[:, :per, :8])                    # the alignment reads the unmasked P / N words
            rows = lb.debug_query_blocks(3, 2, per, length, 0, bools=b).reshape(2, per, 8)
            assert np.array_equal(lb.unpack_packed(rows.reshape(-1, 8), length).reshape(b.shape), b)


def test_builder_kernels_use_no_scratch(tmp_path):
    """k_query.hip compiles for gfx950 and every builder kernel reports 0 bytes of private segment and no spilled register."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_query.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_query.hip")
    # the flags of lbaudiodetective_amd/csrc/Makefile
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-x", "hip", "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"),
           src, "-o", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    found = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        found[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4))
    for kernel in ("build_plane_queries_kernel", "build_sliding_queries_kernel", "build_query_rows_kernelILb0E", "build_query_rows_kernelILb1E"):
        hits = {k: v for k, v in found.items() if kernel in k}
        assert len(hits) == 1, (kernel, sorted(found))
        assert list(hits.values())[0] == (0, 0, 0), hits
    assert len(found) == 4, sorted(found)
    assert "scratch_" not in isa                 # no instruction addresses a private segment
