"""CPU checks of the recording-timeline calls: the three symbols and their declared signatures, the Python names, the argument
checks that need neither a device nor a handle, the no-device status, the compiled kernels of k_timeline.hip (no scratch memory,
no register spilled to it), the numpy reference against a brute-force triple loop, and the greedy segments on hand-made winners."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import timeline_ref
from align_ref import profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "lbaudiodetective.h")

SYMBOLS = ("LBAudioDetectiveCorpusRecordingTimelineKeysDevice", "LBAudioDetectiveCorpusRecordingPackedTimelineKeysDevice",
           "LBAudioDetectiveCorpusQueryRecordingTimeline")


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
    types = {"LBAudioDetectiveCorpusRef": N.Ref, "LBAudioDetectiveFingerprintRef": N.Ref, "void*": C.c_void_p, "const void*": C.c_void_p,
             "UInt32": N.UInt32, "UInt64": N.UInt64, "Float32": N.Float32, "SInt64*": C.POINTER(N.SInt64),
             "Float32*": C.POINTER(N.Float32), "UInt32*": C.POINTER(N.UInt32), "UInt64*": C.POINTER(N.UInt64)}
    ref, fp, dev = "LBAudioDetectiveCorpusRef", "LBAudioDetectiveFingerprintRef", "void*"
    want = {
        SYMBOLS[0]: [ref, fp, "UInt32", "Float32", "UInt64", dev, dev, dev],
        SYMBOLS[1]: [ref, "const void*", "UInt32", "UInt32", "Float32", "UInt64", dev, dev, dev],
        SYMBOLS[2]: [ref, fp, "UInt32", "Float32", "SInt64*", "Float32*", "UInt32*", "UInt64*"],
    }
    for name, params in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), (name, got)
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [types[p] for p in params], (name, args)
    # no status constant was added
    assert len(lb._native.declared_symbols()[1]) == 10


def test_python_names(lb):
    for attr in ("recording_timeline_keys_device", "recording_timeline", "recording_segments"):
        assert callable(getattr(lb.Corpus, attr))
    assert callable(lb.decode_timeline_keys) and callable(lb.timeline_segments)


def _fakes(lb):
    N = lb._native
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)                  # stands for a device pointer: never dereferenced
    fake = C.c_void_p(p)                  # ... and for a corpus or fingerprint handle
    host = ((N.SInt64 * 4)(), (N.Float32 * 4)(), (N.UInt32 * 4)(), N.UInt64(0))
    return buf, p, fake, host


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle: the calls return on a machine without a
    GPU, with handles that are never read."""
    Lib = lb.lib()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, p, fake, (idx, sc, lens, count) = _fakes(lb)
    keys, packed_keys, host = (getattr(Lib, s) for s in SYMBOLS)
    for outlen, hostlen in ((p, lens), (None, None)):                # outLengths may be NULL: it changes no refusal
        # NULL handles and pointers
        assert keys(None, fake, 0, 0.7, 0, p, outlen, None) == bad
        assert keys(fake, None, 0, 0.7, 0, p, outlen, None) == bad
        assert keys(fake, fake, 0, 0.7, 0, None, outlen, None) == bad
        assert packed_keys(None, p, 3, 0, 0.7, 0, p, outlen, None) == bad
        assert packed_keys(fake, None, 3, 0, 0.7, 0, p, outlen, None) == bad
        assert packed_keys(fake, p, 3, 0, 0.7, 0, None, outlen, None) == bad
        assert host(None, fake, 0, 0.7, idx, sc, hostlen, C.byref(count)) == bad
        assert host(fake, None, 0, 0.7, idx, sc, hostlen, C.byref(count)) == bad
        assert host(fake, fake, 0, 0.7, None, sc, hostlen, C.byref(count)) == bad
        assert host(fake, fake, 0, 0.7, idx, None, hostlen, C.byref(count)) == bad
        assert host(fake, fake, 0, 0.7, idx, sc, hostlen, None) == bad
        # the threshold
        for t in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert keys(fake, fake, 0, t, 0, p, outlen, None) == bad, t
            assert packed_keys(fake, p, 3, 0, t, 0, p, outlen, None) == bad, t
            assert host(fake, fake, 0, t, idx, sc, hostlen, C.byref(count)) == bad, t
        # no sub-fingerprints, or more than an offset can count
        for per in (0, 1 << 31, 0xFFFFFFFF):
            assert packed_keys(fake, p, per, 0, 0.7, 0, p, outlen, None) == bad, per
        # an index base no corpus fits behind
        assert keys(fake, fake, 0, 0.7, (1 << 32) + 1, p, outlen, None) == bad
        assert packed_keys(fake, p, 3, 0, 0.7, (1 << 32) + 1, p, outlen, None) == bad


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks the three calls report kLBAudioDetectiveDeviceUnavailable (and still
    read no handle), with and without outLengths."""
    Lib = lb.lib()
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, p, fake, (idx, sc, lens, count) = _fakes(lb)
    keys, packed_keys, host = (getattr(Lib, s) for s in SYMBOLS)
    for outlen, hostlen in ((p, lens), (None, None)):
        assert keys(fake, fake, 0, 0.7, 0, p, outlen, None) == nogp
        assert keys(fake, fake, 64, 1.5, 1 << 32, p, outlen, None) == nogp                 # (t > 1 is legal)
        assert packed_keys(fake, p, 1, 0, 0.7, 0, p, outlen, None) == nogp
        assert packed_keys(fake, p, (1 << 31) - 1, 64, 0.7, 1 << 32, p, outlen, None) == nogp
        assert host(fake, fake, 0, 0.7, idx, sc, hostlen, C.byref(count)) == nogp


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
    assert re.search(r"^SRCS\s*:=.*\bk_timeline\.hip\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bapi_timeline\.cpp\b", text, re.M)


def test_the_walk_is_a_named_multiple_of_64():
    src = open(os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_timeline.hip")).read()
    walk = int(re.search(r"constexpr\s+uint32_t\s+kTlEntries\s*=\s*(\d+)\s*;", src).group(1))
    assert walk >= 64 and walk % 64 == 0
    # ... and the header states the chunk in the same number
    header = re.sub(r"\s*\n\s*\*\s*", " ", open(HEADER).read())
    assert f"ceil(entries / {walk}) x tiles x 126 x 8 bytes" in header


def test_timeline_kernels_use_no_scratch(tmp_path):
    """k_timeline.hip compiles for gfx950 with the flags read from the Makefile (CXXFLAGS and any FLAGS_k_timeline); every kernel
    in it -- the maxima kernel for a range that covers the length and for one that does not, the fold and the lengths kernel --
    reports 0 bytes of private segment and no spilled register, scalar or vector (the metadata only).  No new kernel's name
    contains an occurrences or recording kernel's."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_timeline.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_timeline.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_timeline") + \
          ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    for kernel, instances in (("timeline_maxima_kernel", 2), ("timeline_fold_kernel", 1), ("timeline_lengths_kernel", 1)):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == instances, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 4, sorted(meta)
    assert not any(old in k for k in meta for old in ("occurrences_count_kernel", "occurrences_scatter_kernel", "recording_maxima_kernel"))


def _brute(query, entries, threshold, index_base):
    """the contract as a triple loop over (offset, entry, step) on align_ref's cells"""
    nq = len(query)
    keys = [0] * nq
    lengths = [0] * nq
    for o in range(nq):
        for j, e in enumerate(entries):
            if len(e) > nq or o > nq - len(e):
                continue
            cell = profile(query, e, 0)[0][o]
            if not cell >= np.float32(threshold):
                continue
            key = (int(np.float32(cell).view(np.uint32)) << 32) | (0xFFFFFFFF - (index_base + j))
            if key > keys[o]:
                keys[o], lengths[o] = key, len(e)
    return np.array(keys, np.uint64), np.array(lengths, np.uint32)


def test_the_reference_is_the_brute_force_loop():
    """entries of 1, 3, 5 and 9 against a query of 7; two identical entries (the lower index wins every tie); an entry longer than
    the query (never named); a planted entry (a cell of 1.0)"""
    rng = np.random.default_rng(7)
    L = 12                                                       # short sub-fingerprints: ties between different entries too
    query = rng.integers(0, 2, (7, L)).astype(np.uint8)
    three = query[2:5].copy()                                    # 1.0 at offset 2
    entries = [rng.integers(0, 2, (1, L)).astype(np.uint8), three, rng.integers(0, 2, (5, L)).astype(np.uint8),
               rng.integers(0, 2, (9, L)).astype(np.uint8), three.copy(), query[6:7].copy()]
    for t in (0.3, 0.7, 1.0):
        for base in (0, 1000):
            keys, lengths = timeline_ref.timeline(query, entries, t, 0, base)
            want_keys, want_lengths = _brute(query, entries, t, base)
            assert np.array_equal(keys, want_keys) and np.array_equal(lengths, want_lengths)
            idx, sc = timeline_ref.decode(keys, base)
            assert 3 not in idx and 4 not in idx                 # the 9 is longer than the query; the second 3 loses every tie
            assert idx[2] == 1 and sc[2] == 1.0 and lengths[2] == 3
            assert idx[6] == 5 and sc[6] == 1.0 and lengths[6] == 1
            assert np.all((idx >= 0) == (lengths > 0)) and np.all(sc[idx >= 0] >= np.float32(t))
    assert np.count_nonzero(timeline_ref.timeline(query, entries, 0.3)[0]) > np.count_nonzero(timeline_ref.timeline(query, entries, 1.0)[0])


def test_greedy_segments(lb):
    """timeline_segments on hand-made winners, and the reference's greedy on the same"""
    def run(idx, sc, ln):
        idx, sc, ln = np.array(idx, np.int64), np.array(sc, np.float32), np.array(ln, np.uint32)
        got = lb.timeline_segments(idx, sc, ln)
        keys = np.where(idx >= 0, (sc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (0xFFFFFFFF - np.maximum(idx, 0)).astype(np.uint64),
                        0).astype(np.uint64)
        ref = timeline_ref.segments(keys, ln)
        assert [tuple(x) for x in zip(*(a.tolist() for a in got))] == [(o, j, float(s), n) for o, j, s, n in ref]
        return list(zip(got[0].tolist(), got[1].tolist(), got[3].tolist()))

    # overlap suppression: the 0.9 at 2 covers [2, 6); the 0.8s at 0 (span [0, 3)) and at 4 meet it, the 0.7 at 6 does not
    assert run([5, -1, 7, -1, 8, -1, 9, -1], [0.8, 0, 0.9, 0, 0.8, 0, 0.7, 0], [3, 0, 4, 0, 2, 0, 2, 0]) == [(2, 7, 4), (6, 9, 2)]
    # ties to the lower offset: the same key at 1 and at 3 with spans that meet
    assert run([-1, 4, -1, 4, -1, -1], [0, 1.0, 0, 1.0, 0, 0], [0, 3, 0, 3, 0, 0]) == [(1, 4, 3)]
    # ... and the same score: the lower INDEX is the higher key, wherever it lies
    assert run([6, 4, -1, -1], [1.0, 1.0, 0, 0], [2, 2, 0, 0]) == [(1, 4, 2)]
    # adjacent spans that do not overlap are both kept, and one that ends at the recording's last offset
    assert run([1, -1, 2, -1, 3, -1], [0.9, 0, 0.8, 0, 1.0, 0], [2, 0, 2, 0, 2, 0]) == [(0, 1, 2), (2, 2, 2), (4, 3, 2)]
    # nothing
    assert run([-1, -1], [0, 0], [0, 0]) == []
