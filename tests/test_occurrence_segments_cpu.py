"""CPU checks of the occurrence segments calls (LBAudioDetectiveOccurrenceSegmentsFromKeysDevice,
LBAudioDetectiveCorpusEntryLengthsFromKeysDevice): the symbols and their declared signatures, the Python names, the build list,
every refusal that needs no device -- with fake pointers that are never read --, the no-device status, the host statement
lbaudiodetective_amd.occurrence_segments against the brute-force reference of occurrence_segments_ref.py, the example that
separates it from timeline_segments, and the compiled kernels of k_occurrence_segments.hip (no scratch memory, no register spilled
to it, no static LDS)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import occurrence_segments_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "lbaudiodetective.h")
CSRC = os.path.join(ROOT, "lbaudiodetective_amd", "csrc")

SEGMENTS = "LBAudioDetectiveOccurrenceSegmentsFromKeysDevice"
LENGTHS = "LBAudioDetectiveCorpusEntryLengthsFromKeysDevice"
CAP = 8192                      # LBAD_SEGMENTS_MAX_SUBFINGERPRINTS and LBAD_OCCURRENCE_SEGMENTS_MAX_CANDIDATES
TOP = (1 << 31) - 1


def _has_gpu():
    return torch.cuda.is_available()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototype(name):
    """the parameter types of `name` as include/lbaudiodetective.h declares it, comments removed"""
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in the header"
    return m.group(1), [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(2).split(",")]


def test_symbols_exist_with_the_declared_signatures(lb):
    N = lb._native
    raw = C.CDLL(lb.LIB_PATH)
    types = {"void*": C.c_void_p, "const void*": C.c_void_p, "UInt32": N.UInt32, "UInt64": N.UInt64,
             "LBAudioDetectiveCorpusRef": N.Ref}
    declared = {SEGMENTS: ["const void*"] * 4 + ["UInt32"] * 4 + ["void*"] * 6,
                LENGTHS: ["LBAudioDetectiveCorpusRef", "const void*", "UInt64", "UInt64", "void*", "void*"]}
    for name, params in declared.items():
        assert hasattr(raw, name), f"{name} is not exported"
        ret, got = _prototype(name)
        assert (ret, got) == ("OSStatus", params), got
        res, args = N._SIGNATURES[name]
        assert res is N.OSStatus and args == [types[p] for p in params], args
    # the caps are the header's, and no status constant was added
    assert re.search(r"#define\s+LBAD_OCCURRENCE_SEGMENTS_MAX_CANDIDATES\s+8192\b", _header())
    assert re.search(r"#define\s+LBAD_SEGMENTS_MAX_SUBFINGERPRINTS\s+8192\b", _header())
    assert N.OCCURRENCE_SEGMENTS_MAX_CANDIDATES == CAP
    assert len(N.declared_symbols()[1]) == 10


def test_python_names(lb):
    for name in ("entry_lengths_from_keys_device", "recording_occurrence_segments_batch_keys_device", "recording_occurrence_segments"):
        assert callable(getattr(lb.Corpus, name)), name
    assert callable(lb.StreamBank.occurrence_segments)
    for name in ("occurrence_segments", "occurrence_segments_device", "decode_occurrence_segments"):
        assert callable(getattr(lb, name)) and name in lb.__all__, name
    # what was there stays
    assert callable(lb.Corpus.recording_segments) and callable(lb.StreamBank.segments) and callable(lb.timeline_segments)


def test_the_files_are_built():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_occurrence_segments\.hip\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bapi_occurrence_segments\.cpp\b", text, re.M)
    assert re.search(r"^SRCS\s*:=.*\bk_segments\.hip\b", text, re.M) and re.search(r"^SRCS\s*:=.*\bapi_segments\.cpp\b", text, re.M)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
NAMES = ("inKeys", "inLags", "inLengths", "inCounts", "R", "slots", "per", "cap", "outStarts", "outKeys", "outLags", "outLengths",
         "outCounts", "stream")
POINTERS = {"inKeys": (0, 8), "inLags": (1, 4), "inLengths": (2, 4), "inCounts": (3, 8), "outStarts": (4, 4), "outKeys": (5, 8),
            "outLags": (6, 4), "outLengths": (7, 4), "outCounts": (8, 4)}          # name -> (fake block, element bytes)
OPTIONAL = ("inCounts", "outLags", "outLengths")


def _fakes():
    """nine distinct 8-byte aligned addresses that stand for device blocks: never dereferenced"""
    buf = (C.c_uint64 * 96)()
    base = C.addressof(buf)
    assert base % 8 == 0
    return buf, [base + 64 * i for i in range(9)]


def _args(a, R=2, slots=5, per=3, cap=4, **change):
    v = dict(R=R, slots=slots, per=per, cap=cap, stream=None)
    v.update({name: a[at] for name, (at, _) in POINTERS.items()})
    v.update(change)
    return tuple(v[k] for k in NAMES)


def _optional_sets(a):
    """the optional pointers given and NULL, in every combination: none of them changes a refusal"""
    for bits in range(8):
        yield {name: (a[POINTERS[name][0]] if bits >> i & 1 else None) for i, name in enumerate(OPTIONAL)}


# shapes (R, slots, per, cap) that pass every check: both caps at once, the largest products
LEGAL = [(1, 1, 1, 1), (2, 5, 3, 4), (1, CAP, CAP, 1), (5, CAP, CAP, CAP + 3), (TOP // CAP, CAP, CAP, CAP), (TOP, 1, 1, 1),
         (1, 1, 1, TOP), ((1 << 30) - 1, 2, 1, 2), (TOP // CAP, 1, CAP, 1), (TOP // CAP, CAP, 1, 1)]


def test_bad_arguments_are_refused_before_any_device(lb):
    """Every refusal is decided before anything touches a device: the call returns on a machine without a GPU, and the fake
    pointers are never read."""
    call = getattr(lb.lib(), SEGMENTS)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, a = _fakes()
    for opt in _optional_sets(a):
        for name in POINTERS:
            if name not in OPTIONAL:
                assert call(*_args(a, **{**opt, name: None})) == bad, name
        for name in ("R", "slots", "per", "cap"):
            assert call(*_args(a, **opt, **{name: 0})) == bad, name
        for per in (CAP + 1, 1 << 14, 0xFFFFFFFF):
            assert call(*_args(a, R=1, slots=1, per=per, cap=1, **opt)) == bad, per
        for slots in (CAP + 1, 1 << 14, 0xFFFFFFFF):
            assert call(*_args(a, R=1, slots=slots, per=1, cap=1, **opt)) == bad, slots
        for R, slots, per, cap in (((1 << 31) // CAP, CAP, 1, 1), (1 << 31, 1, 1, 1), (0xFFFFFFFF, CAP, 1, 1),        # R x slots
                                   ((1 << 31) // CAP, 1, CAP, 1), (1 << 30, 1, 2, 1), (0xFFFFFFFF, 1, CAP, 1),        # R x per
                                   (2, 3, 3, 1 << 30), (1, 1, 1, 1 << 31), (1 << 16, 1, 1, 1 << 15), (3, 1, 1, 715827883),
                                   (0xFFFFFFFF, 1, 1, 0xFFFFFFFF)):                                                  # R x cap
            assert max(R * slots, R * per, R * cap) > TOP and slots <= CAP and per <= CAP
            assert call(*_args(a, R=R, slots=slots, per=per, cap=cap, **opt)) == bad, (R, slots, per, cap)
    # alignment: every pointer to its element, the optional ones when given
    for name, (at, size) in POINTERS.items():
        for off in range(1, size):
            assert call(*_args(a, **{name: a[at] + off})) == bad, (name, off)
    # in place: an output equal to the input of its kind
    for opt in _optional_sets(a):
        assert call(*_args(a, **{**opt, "outKeys": a[0]})) == bad
    assert call(*_args(a, outLags=a[1])) == bad
    assert call(*_args(a, outLengths=a[2])) == bad


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_point_fails_without_gpu(lb):
    """No CPU fallback: with arguments that pass the checks the call reports kLBAudioDetectiveDeviceUnavailable (and still reads no
    pointer), whichever optional pointers are given -- both caps at once and the largest products included."""
    call = getattr(lb.lib(), SEGMENTS)
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, a = _fakes()
    assert any(slots == CAP and per == CAP for _R, slots, per, _c in LEGAL)
    for opt in _optional_sets(a):
        for R, slots, per, cap in LEGAL:
            assert max(R * slots, R * per, R * cap) <= TOP and slots <= CAP and per <= CAP
            assert call(*_args(a, R=R, slots=slots, per=per, cap=cap, **opt)) == nogp, (R, slots, per, cap)
        assert call(*_args(a, **{**opt, "inKeys": a[0] + 8, "inLags": a[1] + 4, "outStarts": a[4] + 4, "outCounts": a[8] + 4})) == nogp


def test_lengths_call_refusals(lb):
    """What needs no handle is refused first: a NULL handle, NULL pointers, a count of 0 or of 2^31, an index base above 2^32, a
    misaligned pointer -- the handle is a fake that is never read."""
    call = getattr(lb.lib(), LENGTHS)
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    _buf, a = _fakes()
    fake = a[8]
    assert call(None, a[0], 4, 0, a[1], None) == bad
    assert call(fake, None, 4, 0, a[1], None) == bad
    assert call(fake, a[0], 4, 0, None, None) == bad
    for count in (0, 1 << 31, (1 << 31) + 1, 1 << 32, (1 << 64) - 1):
        assert call(fake, a[0], count, 0, a[1], None) == bad, count
    assert call(fake, a[0], 4, (1 << 32) + 1, a[1], None) == bad
    for off in (1, 2, 4):
        assert call(fake, a[0] + off, 4, 0, a[1], None) == bad, off
    for off in (1, 2, 3):
        assert call(fake, a[0], 4, 0, a[1] + off, None) == bad, off


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_lengths_call_fails_without_gpu(lb):
    """... then the device: legal arguments, the largest count among them, report kLBAudioDetectiveDeviceUnavailable before the
    (fake) handle is read."""
    call = getattr(lb.lib(), LENGTHS)
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    _buf, a = _fakes()
    for count, base in ((1, 0), (TOP, 0), (7, 1 << 32), (4, 12345)):
        assert call(a[8], a[0], count, base, a[1] + 4, None) == nogp, (count, base)


# ---- the host statement --------------------------------------------------------------------------------------------------------
def _key(score, index):
    return (int(np.float32(score).view(np.uint32)) << 32) | (0xFFFFFFFF - int(index))


def _random_row(rng):
    """a row of mixed shapes: few distinct keys (ties), starts that collide, spans clipped at both ends, recordings inside longer
    entries (lag > 0), empty spans, zero lengths and cells that are none (index -1)"""
    per = int(rng.integers(1, 200))
    n = int(rng.integers(0, 120))
    kinds = int(rng.integers(1, 8))
    pool_sc = rng.integers(0x3E000000, 0x3F800000, kinds).astype(np.uint32).view(np.float32)
    pool_ix = rng.integers(0, 50, kinds)
    pick = rng.integers(0, kinds, n)
    idx = np.where(rng.random(n) < 0.1, -1, pool_ix[pick]).astype(np.int64)
    sc = pool_sc[pick]
    lags = rng.integers(-per - 5, 12, n).astype(np.int32)
    lengths = np.where(rng.random(n) < 0.1, 0, rng.integers(1, 2 * per + 5, n)).astype(np.uint32)
    short = rng.random(n) < 0.7
    lengths = np.where(short & (lengths != 0), rng.integers(1, 12, n), lengths).astype(np.uint32)
    return idx, sc, lags, lengths, per


def test_host_statement_against_the_brute_force_reference(lb):
    rng = np.random.default_rng(20261021)
    seen = 0
    for _ in range(200):
        idx, sc, lags, lengths, per = _random_row(rng)
        keys = [0 if i < 0 else _key(s, i) for i, s in zip(idx, sc)]
        want = ref.segments(keys, lags, lengths, per)
        got = lb.occurrence_segments(idx, sc, lags, lengths, per)
        assert [g.dtype for g in got] == [np.int64, np.int64, np.float32, np.int32, np.uint32]
        assert got[0].tolist() == [w[0] for w in want]
        assert [_key(s, i) for i, s in zip(got[1], got[2])] == [w[1] for w in want]
        assert got[3].tolist() == [w[2] for w in want] and got[4].tolist() == [w[3] for w in want]
        # the spans do not overlap and lie inside the recording
        ends = [min(per, -w[2] + w[3]) for w in want]
        assert all(e <= s for e, s in zip(ends, got[0][1:])) and all(0 <= w[0] < e <= per for w, e in zip(want, ends))
        seen += len(want)
    assert seen > 400


def test_the_second_best_at_an_offset_is_reported(lb):
    """X covers [12, 22) and scores 1.0, W starts at 5 with length 10 and 0.95, S starts at 5 with length 5 and 0.90: the timeline
    keeps W at offset 5, the greedy over its winners accepts X and rejects W, and S is never a candidate -- X alone.  Over all
    cells the answer is S, then X."""
    per, X, W, S = 30, 3, 1, 2
    cells = [(X, 1.0, -12, 10), (W, 0.95, -5, 10), (S, 0.90, -5, 5)]
    idx, sc, lags, lengths = (np.array(c) for c in zip(*cells))
    got = lb.occurrence_segments(idx, sc.astype(np.float32), lags, lengths, per)
    assert got[0].tolist() == [5, 12] and got[1].tolist() == [S, X]
    assert got[2].tolist() == [np.float32(0.90), np.float32(1.0)] and got[3].tolist() == [-5, -12] and got[4].tolist() == [5, 10]
    want = ref.segments([_key(s, i) for i, s, _, _ in cells], lags, lengths, per)
    assert [(w[0], w[4]) for w in want] == [(5, 2), (12, 0)]
    # the timeline's per-offset winners of the same cells: W at 5 (0.95 beats 0.90), X at 12
    t_idx, t_sc, t_len = np.full(per, -1, np.int64), np.zeros(per, np.float32), np.zeros(per, np.uint32)
    t_idx[5], t_sc[5], t_len[5] = W, 0.95, 10
    t_idx[12], t_sc[12], t_len[12] = X, 1.0, 10
    old = lb.timeline_segments(t_idx, t_sc, t_len)
    assert old[0].tolist() == [12] and old[1].tolist() == [X]


def test_the_reference_on_cases_worked_by_hand():
    """the reference itself, on rows whose answer is plain: touching spans, the tie rules, a lag word of INT32_MIN, a recording
    inside a longer entry, the count"""
    k = _key(0.5, 7)
    assert [x[0] for x in ref.segments([k, k], [-3, -6], [3, 3], 10)] == [3, 6]                    # touch: both
    assert [x[4] for x in ref.segments([k, k], [-4, -3], [3, 3], 10)] == [1]                       # equal keys: the lower start
    assert [x[4] for x in ref.segments([k, k], [2, 5], [40, 40], 10)] == [0]                       # ... and start: the lower slot
    assert ref.segments([k, k, k], [ref.INT32_MIN, 3, -10], [5, 3, 1], 10) == []                   # no candidates
    assert [x[:1] + x[2:] for x in ref.segments([_key(0.9, 1), k], [4, -2], [100, 3], 10)] == [(0, 4, 100, 0)]
    assert [x[4] for x in ref.segments([k, _key(0.9, 1)], [0, 0], [2, 2], 10, count=1)] == [0]     # behind the count: ignored
    assert ref.segments([0, k], [0, 0], [2, 0], 10) == []                                          # zero key, zero length


# ---- the compiled kernels ------------------------------------------------------------------------------------------------------
def _makefile_flags(stem):
    """CXXFLAGS and FLAGS_<stem> as lbaudiodetective_amd/csrc/Makefile sets them: the build that is shipped"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")

    def var(name):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % re.escape(name), text, re.M)
        return m.group(1).split() if m else []

    arch = (var("ARCH") or ["gfx950"])[0]
    return [f.replace("$(ARCH)", arch) for f in var("CXXFLAGS") + var("FLAGS_" + stem)]


def test_occurrence_segments_kernels_use_no_scratch(tmp_path):
    """k_occurrence_segments.hip compiles for gfx950 with the flags read from the Makefile; every kernel in it reports 0 bytes of
    private segment and no spilled register, scalar or vector (the metadata only), and no static LDS beside the dynamic block."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_occurrence_segments.s"
    src = os.path.join(CSRC, "k_occurrence_segments.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + _makefile_flags("k_occurrence_segments") + \
          ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    assert len(meta) == 2 and any("occurrence_segments_kernel" in k for k in meta) and \
        any("entry_lengths_uniform_kernel" in k for k in meta), sorted(meta)
    assert all(v == (0, 0, 0) for v in meta.values()), meta
    fixed = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", isa)]      # (one per kernel of the file)
    assert len(fixed) == len(meta) and all(x == 0 for x in fixed), fixed
