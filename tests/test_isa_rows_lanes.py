"""CPU checks of the COMPILED second headline stage-1 kernel, frame_rows_lanes_kernel<0> (hipcc cross-compiles gfx950 without a
GPU): the form of k_rows_pruned.hip in which every band's bins lie in one lane and the band sums are adds in registers.  Its
main loop -- one quarter frame per workgroup and iteration -- must hold

  * exactly the 498 v_pk_fma_f32 and 131 v_pk_add_f32 of the radix-2 network: the butterflies are those of
    frame_rows_pruned_kernel;
  * no ds_read_b32 and no ds_write_b32: the power terms never visit LDS;
  * the IEEE division sequence in ONE basic block, reached through a scalar branch, with the lane's three quotients in it;
  * the twelve global_load_lds_dword of the span prefetch, and no scalar fetched back from a vector lane;

and the kernel as a whole two waves per SIMD, no scratch and at most 256 VGPRs.
"""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNEL = "frame_rows_lanes_kernelILi%dEE"
DIVISION = ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_rcp_f32")


@pytest.fixture(scope="module")
def lanes_isa(tmp_path_factory):
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


def _function(isa, fmt=0):
    """(instruction lines of the kernel, its text up to the resource summary the compiler prints behind it)"""
    m = re.search(r"^(_ZN4lbad\S*%s\S*):.*?\n(.*?)^\.Lfunc_end\d+:(.*?); Occupancy: \d+\n" % (KERNEL % fmt), isa, re.M | re.S)
    assert m, "kernel not found"
    return m.group(2).splitlines(), m.group(0)


def _main_loop(lines):
    """The largest depth-1 loop as the compiler marks it: the block of its header label and every block annotated `in Loop:
    Header=<that label>` (block placement may rotate the loop or move a cold block behind the back edge, so the span from the
    header to the last branch back would miss blocks).  Returns a list of (label, opcodes) per basic block."""
    blocks, label, note = [], None, ""
    for line in lines:
        m = re.match(r"(\.LBB\d+_\d+):(.*)", line)
        if m:
            label, note = m.group(1), m.group(2)
            blocks.append((label, note, []))
            continue
        op = _opcode(line)
        if op and blocks:
            blocks[-1][2].append((op, line))
    best = []
    for label, note, _ in blocks:
        if "Loop Header: Depth=1" not in note:
            continue
        name = label[2:]                                        # .LBB2_16 -> BB2_16
        body = [(l, ops) for l, n, ops in blocks if l == label or re.search(r"in Loop: Header=%s Depth=1\b" % re.escape(name), n)]
        if sum(len(ops) for _, ops in body) > sum(len(ops) for _, ops in best):
            best = body
    assert best, "no loop found"
    return best


def _count(blocks):
    return collections.Counter(op for _, ops in blocks for op, _ in ops)


def test_loop_has_the_butterflies_and_no_band_sums_through_lds(lanes_isa):
    lines, _ = _function(lanes_isa)
    total = _count(_main_loop(lines))
    assert sum(total.values()) > 1000, "this is not the main loop"
    assert total["v_pk_fma_f32"] == 498 and total["v_pk_add_f32"] == 131, (total["v_pk_fma_f32"], total["v_pk_add_f32"])
    assert total["ds_read_b32"] == 0 and total["ds_write_b32"] == 0, (total["ds_read_b32"], total["ds_write_b32"])
    assert total["global_load_lds_dword"] == 12
    assert total["v_readlane_b32"] == 0 and total["v_writelane_b32"] == 0, (total["v_readlane_b32"], total["v_writelane_b32"])


def test_division_only_in_the_fallback_block_with_three_quotients(lanes_isa):
    lines, _ = _function(lanes_isa)
    blocks = _main_loop(lines)
    with_div = [(l, ops) for l, ops in blocks if any(op in DIVISION for op, _ in ops)]
    assert len(with_div) == 1, "division instructions in %d basic blocks of the loop" % len(with_div)
    label, ops = with_div[0]
    fallback = collections.Counter(op for op, _ in ops)
    # the lane's three quotients redone: nothing else lives in the fallback block
    assert (fallback["v_div_scale_f32"], fallback["v_rcp_f32"], fallback["v_div_fmas_f32"], fallback["v_div_fixup_f32"]) == (6, 3, 3, 3)
    assert fallback["v_pk_fma_f32"] == 0 and fallback["v_pk_add_f32"] == 0 and len(ops) < 64, len(ops)
    # a wave reaches it through a scalar branch on the ballot, never by masking lanes: every branch to the block tests vcc or
    # scc, and the block is no fall-through of the one in front of it
    into = [op for _, bops in blocks for op, line in bops if re.search(r"\s%s\s*$" % re.escape(label), line)]
    assert into and all(op.startswith("s_cbranch_vcc") or op.startswith("s_cbranch_scc") for op in into), into
    before = blocks[[l for l, _ in blocks].index(label) - 1][1]
    assert before[-1][0] == "s_branch", before[-1]


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_two_waves_per_simd_without_scratch(lanes_isa, fmt):
    _, text = _function(lanes_isa, fmt)
    assert re.search(r"; ScratchSize: 0\b", text), "the kernel uses scratch memory"
    assert re.search(r"; Occupancy: 2\b", text), re.findall(r"; Occupancy: \d+", text)
    assert not re.search(r"\bscratch_(load|store)", text)
    vgprs = int(re.search(r"; TotalNumVgprs: (\d+)", text).group(1))
    assert vgprs <= 256, vgprs
