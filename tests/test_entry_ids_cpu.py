"""CPU checks of the entry ids: the six symbols and their declared signatures (header, _native._SIGNATURES and the library agree),
the Python names, the refusal order -- what needs no handle first, then the missing device -- and the compiled kernels of
k_ids.hip (no scratch memory, no spilled register)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

CORPUS = "LBAudioDetectiveCorpus"
SYMBOLS = (CORPUS + "SetEntryIdsDevice", CORPUS + "SetEntryIds", CORPUS + "GetEntryIds", CORPUS + "HasEntryIds", CORPUS + "IdsFromKeysDevice",
           CORPUS + "KeysFromIdsDevice")


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
    u64p = C.POINTER(N.UInt64)
    ctype = {"LBAudioDetectiveCorpusRef": N.Ref, "OSStatus": N.OSStatus, "UInt32": N.UInt32, "UInt64": N.UInt64, "void*": C.c_void_p,
             "const void*": C.c_void_p, "const UInt64*": u64p, "UInt64*": u64p}
    ref = "LBAudioDetectiveCorpusRef"
    lists = ("OSStatus", [ref, "const void*", "UInt64", "UInt64", "void*", "void*"])
    want = {
        SYMBOLS[0]: ("OSStatus", [ref, "UInt64", "UInt64", "const void*", "void*"]),
        SYMBOLS[1]: ("OSStatus", [ref, "UInt64", "UInt64", "const UInt64*"]),
        SYMBOLS[2]: ("OSStatus", [ref, "UInt64", "UInt64", "UInt64*"]),
        SYMBOLS[3]: ("UInt32", [ref]),
        SYMBOLS[4]: lists,
        SYMBOLS[5]: lists,
    }
    assert len(want) == 6
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
    assert isinstance(lb.Corpus.has_entry_ids, property)
    for attr in ("set_entry_ids", "entry_ids", "ids_from_keys_device", "keys_from_ids_device", "remove_ids", "gather_ids"):
        assert callable(getattr(lb.Corpus, attr)), attr
        assert not hasattr(lb.ShardedCorpus, attr), attr          # (a rank takes down by id on its own)


def _fakes(lb):
    N = lb._native
    buf = (C.c_uint64 * 16)()
    p = (C.addressof(buf) + 15) & ~15      # 16-byte aligned; stands for a device pointer and for a corpus handle: never dereferenced
    return buf, p, C.c_void_p(p), (N.UInt64 * 4)(5, 6, 7, 8), (N.UInt64 * 4)(*([0xDEAD] * 4))


def test_bad_arguments_are_refused_before_any_handle_is_read(lb):
    """Every refusal below is decided before anything touches a device or a handle: the calls return on a machine without a
    GPU, with corpus handles that are never read, and nothing is written."""
    Lib = lb.lib()
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    buf, p, fake, ids, out = _fakes(lb)
    set_dev, set_host, get, has, from_keys, from_ids = (getattr(Lib, s) for s in SYMBOLS)
    # a NULL corpus
    assert set_dev(None, 0, 4, p, None) == bad and set_dev(None, 0, 0, None, None) == bad
    assert set_host(None, 0, 4, ids) == bad and set_host(None, 0, 0, None) == bad
    assert get(None, 0, 4, out) == bad and get(None, 0, 0, None) == bad
    assert has(None) == 0
    for lists in (from_keys, from_ids):
        assert lists(None, p, 4, 0, p, None) == bad and lists(None, None, 0, 0, None, None) == bad
    # a NULL pointer with a non-zero count
    assert set_dev(fake, 0, 4, None, None) == bad
    assert set_host(fake, 0, 4, None) == bad
    assert get(fake, 0, 4, None) == bad
    for lists in (from_keys, from_ids):
        assert lists(fake, None, 4, 0, p, None) == bad
        assert lists(fake, p, 4, 0, None, None) == bad
    # device pointers off 8 bytes
    assert set_dev(fake, 0, 4, p + 4, None) == bad
    for lists in (from_keys, from_ids):
        assert lists(fake, p + 4, 4, 0, p, None) == bad
        assert lists(fake, p, 4, 0, p + 4, None) == bad
        # an index base no corpus fits behind, also with an empty list; more than 2^31 elements
        assert lists(fake, p, 4, (1 << 32) + 1, p, None) == bad
        assert lists(fake, None, 0, (1 << 32) + 1, None, None) == bad
        assert lists(fake, p, (1 << 31) + 1, 0, p, None) == bad
    # ranges no corpus holds
    assert set_dev(fake, (1 << 32) + 1, 1, p, None) == bad and set_dev(fake, 0, (1 << 32) + 1, p, None) == bad
    assert set_host(fake, (1 << 32) + 1, 1, ids) == bad and set_host(fake, 0, (1 << 32) + 1, ids) == bad
    assert get(fake, (1 << 32) + 1, 1, out) == bad and get(fake, 0, (1 << 32) + 1, out) == bad
    assert list(out) == [0xDEAD] * 4 and list(ids) == [5, 6, 7, 8] and not any(buf)


@pytest.mark.skipif(_has_gpu(), reason="the no-device status needs a machine without a GPU")
def test_entry_points_fail_without_gpu(lb):
    """No CPU fallback: with arguments that pass the first checks every call reports kLBAudioDetectiveDeviceUnavailable -- also an
    empty range or list, and what only the corpus could refuse -- and none of them reads a handle or writes anything."""
    Lib = lb.lib()
    nogp = lb.constant("kLBAudioDetectiveDeviceUnavailable")
    buf, p, fake, ids, out = _fakes(lb)
    set_dev, set_host, get, has, from_keys, from_ids = (getattr(Lib, s) for s in SYMBOLS)
    assert set_dev(fake, 0, 4, p, None) == nogp and set_dev(fake, 0, 0, None, None) == nogp
    assert set_dev(fake, 1 << 32, 1 << 32, p, None) == nogp
    assert set_host(fake, 0, 4, ids) == nogp and set_host(fake, 7, 0, None) == nogp
    assert get(fake, 0, 4, out) == nogp and get(fake, 0, 0, None) == nogp
    for lists in (from_keys, from_ids):
        assert lists(fake, p, 4, 0, p, None) == nogp
        assert lists(fake, p, 1 << 31, 1 << 32, p, None) == nogp
        assert lists(fake, None, 0, 12345, None, None) == nogp
    assert list(out) == [0xDEAD] * 4 and list(ids) == [5, 6, 7, 8] and not any(buf)


def test_id_kernels_use_no_scratch(tmp_path):
    """k_ids.hip compiles for gfx950 with the Makefile's flags; every kernel in it -- ids from keys, the index's init and insert,
    keys from ids, the removal's gather and scatter -- reports 0 bytes of private segment and no spilled register, scalar or
    vector (the metadata only).  Both new files are among the Makefile's sources."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_ids.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_ids.hip")
    assert os.path.exists(src), "k_ids.hip is missing"
    makefile = open(os.path.join(os.path.dirname(src), "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bk_ids\.hip\b", makefile, re.M) and re.search(r"^SRCS\s*:=.*\bapi_ids\.cpp\b", makefile, re.M)
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
    for kernel in ("ids_from_keys_kernel", "ids_index_init_kernel", "ids_index_insert_kernel", "keys_from_ids_kernel",
                   "ids_compact_gather_kernel", "ids_compact_scatter_kernel"):
        hits = {k: v for k, v in meta.items() if kernel in k}
        assert len(hits) == 1, (kernel, sorted(meta))
        assert all(v == (0, 0, 0) for v in hits.values()), hits
    assert len(meta) == 6, sorted(meta)
    assert "asm" not in re.sub(r"//.*", "", open(src).read())      # no inline assembly
