"""CPU checks of the COMPILED headline stage-1 kernel, frame_rows_pruned_kernel<0> (hipcc cross-compiles gfx950 without a
GPU).  Its main loop -- one quarter frame per workgroup and iteration -- may hold the butterflies, the split pass, the band
sums and the short constant division of const_div.hpp, and nothing of what was taken out of it:

  * the IEEE division sequence (v_div_scale / v_rcp / v_div_fmas / v_div_fixup) only inside ONE basic block, the fallback
    a wave enters through a scalar branch when its guard trips;
  * no scalar spilled to a vector lane and fetched back (v_readlane_b32 / v_writelane_b32), no scratch, two waves per SIMD;
  * exactly the 498 v_pk_fma_f32 and 131 v_pk_add_f32 of the radix-2 network: the butterflies are what they were.
"""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNEL = "frame_rows_pruned_kernelILi0EE"
DIVISION = ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_rcp_f32")


@pytest.fixture(scope="module")
def pruned_isa(tmp_path_factory):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "k_rows_pruned.s"
    src = os.path.join(ROOT, "lbaudiodetective_amd", "csrc", "k_rows_pruned.hip")
    # the flags of lbaudiodetective_amd/csrc/Makefile, FLAGS_k_rows_pruned included
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None",
           "-x", "hip", "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"), src, "-o", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    return open(out).read()


def _opcode(line):
    """Mnemonic of an instruction line without its encoding suffix, None for labels, comments and directives."""
    t = line.strip()
    if not t or t[0] in ";." or t.endswith(":") or re.match(r"\.?\w+:", t):
        return None
    return re.sub(r"_(e32|e64|dpp|sdwa)$", "", t.split()[0])


def _function(isa):
    """(instruction lines of the kernel, its text up to the resource summary the compiler prints behind it)"""
    m = re.search(r"^(_ZN4lbad\S*%s\S*):.*?\n(.*?)^\.Lfunc_end\d+:(.*?); Occupancy: \d+\n" % KERNEL, isa, re.M | re.S)
    assert m, "kernel not found"
    return m.group(2).splitlines(), m.group(0)


def _main_loop(lines):
    """The longest depth-1 loop: from its header label to the last branch back to it.  Returns a list of basic blocks,
    each a list of opcodes (a block ends at a label)."""
    best = None
    for i, line in enumerate(lines):
        m = re.match(r"(\.LBB\d+_\d+):.*Loop Header: Depth=1", line)
        if not m:
            continue
        back = [j for j in range(i + 1, len(lines)) if re.search(r"s_c?branch\S*\s+%s\s*$" % re.escape(m.group(1)), lines[j])]
        if back and (best is None or back[-1] - i > best[1] - best[0]):
            best = (i, back[-1])
    assert best, "no loop found"
    blocks = [[]]
    for line in lines[best[0]:best[1] + 1]:
        if re.match(r"\.LBB\d+_\d+:", line):
            blocks.append([])
            continue
        op = _opcode(line)
        if op:
            blocks[-1].append(op)
    return [b for b in blocks if b]


def test_loop_has_the_butterflies_and_no_division_outside_the_fallback(pruned_isa):
    lines, _ = _function(pruned_isa)
    blocks = _main_loop(lines)
    total = collections.Counter(op for b in blocks for op in b)
    assert sum(total.values()) > 1000, "this is not the main loop"
    assert total["v_pk_fma_f32"] == 498 and total["v_pk_add_f32"] == 131, (total["v_pk_fma_f32"], total["v_pk_add_f32"])
    with_div = [b for b in blocks if any(op in DIVISION for op in b)]
    assert len(with_div) == 1, "division instructions in %d basic blocks of the loop" % len(with_div)
    fallback = collections.Counter(with_div[0])
    # four quotients redone: nothing else lives in the fallback block
    assert (fallback["v_div_scale_f32"], fallback["v_rcp_f32"], fallback["v_div_fmas_f32"], fallback["v_div_fixup_f32"]) == (8, 4, 4, 4)
    assert fallback["v_pk_fma_f32"] == 0 and fallback["v_pk_add_f32"] == 0 and len(with_div[0]) < 64, len(with_div[0])
    # a wave reaches it through a scalar branch on the ballot, never by masking lanes
    before = blocks[blocks.index(with_div[0]) - 1]
    assert any(op.startswith("s_cbranch_vcc") or op.startswith("s_cbranch_scc") for op in before[-4:]), before[-6:]


def test_loop_fetches_no_spilled_scalar(pruned_isa):
    lines, _ = _function(pruned_isa)
    total = collections.Counter(op for b in _main_loop(lines) for op in b)
    assert total["v_readlane_b32"] == 0 and total["v_writelane_b32"] == 0, (total["v_readlane_b32"], total["v_writelane_b32"])
    # the span loads share their addresses: three 64-bit adds for twelve loads (one per load before), five for the rows
    assert total["global_load_lds_dword"] == 12
    assert total["v_lshl_add_u64"] <= 8, total["v_lshl_add_u64"]


def test_two_waves_per_simd_without_scratch(pruned_isa):
    _, text = _function(pruned_isa)
    assert re.search(r"; ScratchSize: 0\b", text), "the kernel uses scratch memory"
    assert re.search(r"; Occupancy: 2\b", text), re.findall(r"; Occupancy: \d+", text)
    assert not re.search(r"\bscratch_(load|store)", text)
    vgprs = int(re.search(r"; TotalNumVgprs: (\d+)", text).group(1))
    assert vgprs <= 256, vgprs
