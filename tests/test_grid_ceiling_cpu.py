"""CPU checks of the tests' grid ceiling (LBAudioDetectiveDebugSetGridCeiling, LBAudioDetectiveDebugGridCeiling): the default,
set and read back, 0 restores the default, the strided-launch counter never decreases, the NULL refusal, and the two symbols in
the header and in _native.py's table.  No device is touched: no launch happens here, so the counter stands still."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("LBAudioDetectiveDebugSetGridCeiling", "LBAudioDetectiveDebugGridCeiling")


def test_default_set_read_and_restore(lb):
    n, strided = lb.debug_grid_ceiling()
    assert n == 0 and strided >= 0
    try:
        lb.debug_set_grid_ceiling(3)
        assert lb.debug_grid_ceiling() == (3, strided)            # (no launch in between: the counter stands still)
        lb.debug_set_grid_ceiling(0xFFFFFFFF)
        assert lb.debug_grid_ceiling()[0] == 0xFFFFFFFF
    finally:
        lb.debug_set_grid_ceiling(0)
    assert lb.debug_grid_ceiling() == (0, strided)


def test_the_counter_never_decreases(lb):
    seen = [lb.debug_grid_ceiling()[1]]
    try:
        for n in (1, 4, 0, 7, 0):
            lb.debug_set_grid_ceiling(n)
            seen.append(lb.debug_grid_ceiling()[1])
    finally:
        lb.debug_set_grid_ceiling(0)
    assert all(b >= a for a, b in zip(seen, seen[1:]))


def test_null_pointers_are_refused(lb):
    bad = lb.constant("kLBAudioDetectiveArgumentInvalid")
    N = lb._native
    n, strided = N.UInt32(77), N.UInt64(77)
    call = lb.lib().LBAudioDetectiveDebugGridCeiling
    assert call(None, None) == bad
    assert call(C.byref(n), None) == bad and call(None, C.byref(strided)) == bad
    assert (n.value, strided.value) == (77, 77)                  # a refused call writes nothing
    assert call(C.byref(n), C.byref(strided)) == 0 and n.value == 0


def test_symbols_in_the_header_and_in_the_table(lb):
    header = open(os.path.join(ROOT, "include", "lbaudiodetective.h")).read()
    N = lb._native
    for name in SYMBOLS:
        assert re.search(r"^OSStatus\s+%s\(" % name, header, re.M), name
        assert name in N._SIGNATURES and hasattr(lb.lib(), name)
    assert N._SIGNATURES[SYMBOLS[0]] == (N.OSStatus, [N.UInt32])
    assert N._SIGNATURES[SYMBOLS[1]][1] == [C.POINTER(N.UInt32), C.POINTER(N.UInt64)]
    assert "tests" in header[header.index("TESTS ONLY"):header.index(SYMBOLS[0])].lower()
    assert "NEVER depend" in header[header.index("TESTS ONLY"):header.index(SYMBOLS[0])]
