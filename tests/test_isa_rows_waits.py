"""CPU checks of the waits in the COMPILED headline stage-1 kernels of k_rows_pruned.hip, frame_rows_lanes_kernel<0> and
frame_rows_pruned_kernel<0> (hipcc cross-compiles gfx950 without a GPU).  In the main loop -- one quarter frame per workgroup
and iteration, the band-sum loop nested in it included -- a wave waits for its span prefetch in ONE place, at the loop head in
front of the first barrier:

  * exactly one s_waitcnt carries a vmcnt field, and it precedes the first s_barrier: no LDS read that follows the
    prefetch inside an iteration (pass-1 and pass-2 tree rows, power terms, the claim slot) is ordered behind the
    global_load_lds that fill the span buffer;
  * the claim is a global_atomic_add and the loop holds no flat_ instruction: a flat access may touch LDS, and the compiler
    drains the prefetch in front of it;
  * the twelve global_load_lds_dword, the 498 v_pk_fma_f32 and the 131 v_pk_add_f32 are still there;

and the kernel as a whole uses no scratch and at most 248 VGPRs.
"""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("frame_rows_lanes_kernelILi0EE", "frame_rows_pruned_kernelILi0EE")


@pytest.fixture(scope="module")
def rows_isa(tmp_path_factory):
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


def _function(isa, kernel):
    """(instruction lines of the kernel, its text up to the resource summary the compiler prints behind it)"""
    m = re.search(r"^(_ZN4lbad\S*%s\S*):.*?\n(.*?)^\.Lfunc_end\d+:(.*?); Occupancy: \d+\n" % kernel, isa, re.M | re.S)
    assert m, "kernel not found"
    return m.group(2).splitlines(), m.group(0)


def _main_loop(lines):
    """The largest depth-1 loop with the loops nested in it, as the compiler marks them: the block of the header label, every
    block annotated `in Loop: Header=<that label> Depth=1`, every inner header annotated `Parent Loop <that label> Depth=1`
    and the blocks of those inner loops.  Returns the instructions as (opcode, line) in the order of the listing, which starts
    at the loop head."""
    blocks, label = [], None
    for line in lines:
        m = re.match(r"(\.LBB\d+_\d+):(.*)", line)
        if m:
            label = m.group(1)
            blocks.append((label, m.group(2), []))
            continue
        if re.match(r"; %bb\.\d+:", line.strip()):               # a fall-through block: no label, same annotation
            blocks.append((None, line, []))
            continue
        op = _opcode(line)
        if op and blocks:
            blocks[-1][2].append((op, line.strip()))
    best = []
    for label, note, _ in blocks:
        if not label or "Loop Header: Depth=1" not in note:
            continue
        name = re.escape(label[2:])                                 # .LBB2_16 -> BB2_16
        inner = [l[2:] for l, n, _ in blocks if l and re.search(r"Parent Loop %s Depth=1\b" % name, n)]
        heads = "|".join([name] + [re.escape(i) for i in inner])
        body = [ops for l, n, ops in blocks
                if l == label or (l and l[2:] in inner) or re.search(r"in Loop: Header=(%s) Depth=\d\b" % heads, n)]
        if sum(len(ops) for ops in body) > sum(len(ops) for ops in best):
            best = body
    assert best, "no loop found"
    return [x for ops in best for x in ops]


@pytest.mark.parametrize("kernel", KERNELS)
def test_one_wait_for_the_prefetch_at_the_loop_head(rows_isa, kernel):
    lines, _ = _function(rows_isa, kernel)
    loop = _main_loop(lines)
    assert len(loop) > 1000, "this is not the main loop"
    waits = [i for i, (op, line) in enumerate(loop) if op == "s_waitcnt" and "vmcnt" in line]
    barriers = [i for i, (op, _) in enumerate(loop) if op == "s_barrier"]
    assert barriers, "no barrier in the loop"
    assert len(waits) == 1, [loop[i][1] + "  before: " + loop[i + 1][1] for i in waits]
    assert waits[0] < barriers[0], (waits[0], barriers[0])


@pytest.mark.parametrize("kernel", KERNELS)
def test_claim_is_a_global_atomic_and_nothing_flat(rows_isa, kernel):
    lines, _ = _function(rows_isa, kernel)
    loop = _main_loop(lines)
    total = collections.Counter(op for op, _ in loop)
    assert total["global_atomic_add"] == 1, {op: n for op, n in total.items() if "atomic" in op}
    flat = [line for op, line in loop if op.startswith("flat_")]
    assert not flat, flat


@pytest.mark.parametrize("kernel", KERNELS)
def test_loop_keeps_its_loads_and_butterflies(rows_isa, kernel):
    lines, _ = _function(rows_isa, kernel)
    total = collections.Counter(op for op, _ in _main_loop(lines))
    assert total["global_load_lds_dword"] == 12, total["global_load_lds_dword"]
    assert total["v_pk_fma_f32"] == 498 and total["v_pk_add_f32"] == 131, (total["v_pk_fma_f32"], total["v_pk_add_f32"])


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_at_most_248_vgprs(rows_isa, kernel):
    _, text = _function(rows_isa, kernel)
    assert re.search(r"; ScratchSize: 0\b", text), "the kernel uses scratch memory"
    assert not re.search(r"\bscratch_(load|store)", text)
    vgprs = int(re.search(r"; NumVgprs: (\d+)", text).group(1))
    assert vgprs <= 248, vgprs
