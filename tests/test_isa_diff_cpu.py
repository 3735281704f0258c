"""CPU checks of tools/isa_diff.py's --pair (no compiler, no GPU): a kernel whose symbol changed is compared under ONE name with its
own symbol replaced by a placeholder in code and descriptor, every other kernel is left alone, and a side that matches no kernel or
more than one ends the run."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def isa_diff():
    spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _trees():
    old = {"_Z9old_countv": (["\ts_load_dword s0, _Z9old_countv@rel", "\ts_endpgm"], ["\t.amdhsa_kernarg_size 8 ; _Z9old_countv"], "a.hip"),
           "_Z4samev": (["\ts_endpgm"], ["\t.amdhsa_next_free_vgpr 4"], "a.hip")}
    new = {"_Z5countILb0EEvv": (["\ts_load_dword s0, _Z5countILb0EEvv@rel", "\ts_endpgm"], ["\t.amdhsa_kernarg_size 8 ; _Z5countILb0EEvv"], "b.hip"),
           "_Z5countILb1EEvv": (["\ts_nop 0", "\ts_endpgm"], ["\t.amdhsa_kernarg_size 8"], "b.hip"),
           "_Z4samev": (["\ts_endpgm"], ["\t.amdhsa_next_free_vgpr 4"], "b.hip")}
    return old, new


def test_a_pair_is_compared_under_one_name_with_a_placeholder(isa_diff):
    old, new = _trees()
    isa_diff.take_pairs(["old_count=countILb0E"], old, new)
    name = "_Z9old_countv -> _Z5countILb0EEvv"
    assert set(old) == {name, "_Z4samev"} and set(new) == {name, "_Z5countILb1EEvv", "_Z4samev"}
    assert old[name][:2] == new[name][:2] == (["\ts_load_dword s0, <kernel>@rel", "\ts_endpgm"], ["\t.amdhsa_kernarg_size 8 ; <kernel>"])
    assert (old[name][2], new[name][2]) == ("a.hip", "b.hip")
    assert old["_Z4samev"] == _trees()[0]["_Z4samev"] and new["_Z5countILb1EEvv"] == _trees()[1]["_Z5countILb1EEvv"]


def test_a_pair_that_differs_still_differs(isa_diff):
    old, new = _trees()
    isa_diff.take_pairs(["old_count=countILb1E"], old, new)
    name = "_Z9old_countv -> _Z5countILb1EEvv"
    assert old[name][0] != new[name][0] and old[name][1] != new[name][1]


@pytest.mark.parametrize("pair", ["old_count=countILb", "nothing=countILb0E", "old_count=nothing", "_Z=countILb0E", "old_count"])
def test_a_side_must_match_exactly_one_kernel(isa_diff, pair):
    old, new = _trees()
    with pytest.raises(SystemExit) as stop:
        isa_diff.take_pairs([pair], old, new)
    assert "isa_diff: --pair" in str(stop.value)
    assert (old, new) == _trees()                                     # nothing was taken
