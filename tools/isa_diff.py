#!/usr/bin/env python3
"""Are the kernels of two source trees the same code?  Compiles .hip files of both trees for the device only, with the flags of
lbaudiodetective_amd/csrc/Makefile (FLAGS_<file> included), splits the assembly per kernel symbol and compares, kernel by kernel,
the instruction text (comments dropped, the compiler's local labels renamed: they carry the function's number in its file) and
the .amdhsa_kernel descriptor block.  Exits non-zero when a kernel differs or is missing on either side.  Needs hipcc, no GPU.

    python tools/isa_diff.py OLD_TREE NEW_TREE --old k_sliding.hip --new k_sliding.hip k_sliding_short.hip k_records.hip

(a refactor that moves kernels between files: every kernel of the old files must be found, identical, in the new ones).

    --pair OLD_REGEX=NEW_REGEX   (repeatable) a kernel whose symbol changed, such as one that became a template instance: each side
                                 must match exactly one kernel symbol of its tree; the two are compared with their own symbol name
                                 replaced by a placeholder in the code and in the descriptor, and reported under "old -> new"."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("lbaudiodetective_amd", "csrc")


def makefile_flags(tree, stem):
    """CXXFLAGS and FLAGS_<stem> as the Makefile of `tree` sets them"""
    text = open(os.path.join(tree, CSRC, "Makefile")).read().replace("\\\n", " ")
    def var(name):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % re.escape(name), text, re.M)
        return m.group(1).split() if m else []
    arch = (var("ARCH") or ["gfx950"])[0]
    return [f.replace("$(ARCH)", arch) for f in var("CXXFLAGS") + var("FLAGS_" + stem)]


def compile_asm(tree, name, out_dir):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        sys.exit("isa_diff: no hipcc")
    stem = os.path.splitext(name)[0]
    out = os.path.join(out_dir, stem + ".s")
    cmd = [hipcc] + makefile_flags(tree, stem) + ["-x", "hip", "--cuda-device-only", "-S", os.path.join(tree, CSRC, name), "-o", out]
    run = subprocess.run(cmd, capture_output=True, text=True)
    if run.returncode != 0:
        sys.exit("isa_diff: %s\n%s" % (" ".join(cmd), run.stderr[-3000:]))
    return open(out).read()


def normalise(lines):
    """comments and blank lines dropped; .LBB<n>_<m>, .Ltmp<n>, .Lfunc_*<n> renamed in order of appearance"""
    names = {}
    def rename(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))
    out = []
    for line in lines:
        line = line.split(";")[0].rstrip()
        if line.strip():
            out.append(re.sub(r"\.(?:LBB\d+_\d+|Ltmp\d+|Lfunc_(?:begin|end)\d+)", rename, line))
    return out


def kernels(asm):
    """kernel symbol -> (instruction lines, descriptor lines)"""
    lines = asm.split("\n")
    found = {}
    for i, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        sym = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        start = next(j for j, l in enumerate(lines) if l.split(";")[0].strip() == sym + ":")
        stop = next(j for j in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[j]))
        found[sym] = (normalise(lines[start + 1:stop]), normalise(lines[i + 1:end]))
    return found


def collect(tree, files, jobs):
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(jobs) as pool:
        asms = list(pool.map(lambda f: compile_asm(tree, f, tmp), files))
    all_kernels = {}
    for name, asm in zip(files, asms):
        for sym, k in kernels(asm).items():
            if sym in all_kernels:
                sys.exit("isa_diff: %s is defined twice in %s" % (sym, tree))
            all_kernels[sym] = k + (name,)
    return all_kernels


def take_pairs(pairs, old, new):
    """--pair: the two kernels of each pair leave `old` and `new` and come back under one name, their own symbols a placeholder"""
    for pair in pairs:
        if "=" not in pair:
            sys.exit("isa_diff: --pair wants OLD_REGEX=NEW_REGEX, not %r" % pair)
        found = []
        for rx, side, what in zip(pair.split("=", 1), (old, new), ("old", "new")):
            hits = [sym for sym in side if re.search(rx, sym)]
            if len(hits) != 1:
                sys.exit("isa_diff: --pair %r matches %d kernels of the %s tree, not one: %s" % (rx, len(hits), what, sorted(hits)))
            found.append(hits[0])
        name = "%s -> %s" % tuple(found)
        for side, sym in zip((old, new), found):
            code, desc, file = side.pop(sym)
            side[name] = ([l.replace(sym, "<kernel>") for l in code], [l.replace(sym, "<kernel>") for l in desc], file)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--old", nargs="+", required=True, metavar="FILE", help=".hip files of the old tree (names inside " + CSRC + ")")
    ap.add_argument("--new", nargs="+", metavar="FILE", help=".hip files of the new tree (default: the same names)")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD_REGEX=NEW_REGEX",
                    help="a kernel whose symbol changed: one kernel each side, compared with its own name as a placeholder (repeatable)")
    ap.add_argument("--jobs", type=int, default=4)
    args = ap.parse_args()
    old = collect(args.old_tree, args.old, args.jobs)
    new = collect(args.new_tree, args.new or args.old, args.jobs)
    take_pairs(args.pair, old, new)
    bad = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in new or sym not in old:
            print("MISSING in the %s tree: %s" % ("new" if sym in old else "old", sym))
            bad += 1
            continue
        (code_a, desc_a, _), (code_b, desc_b, file_b) = old[sym], new[sym]
        if code_a != code_b or desc_a != desc_b:
            what = "descriptor" if code_a == code_b else "instructions, the descriptor " + ("too" if desc_a != desc_b else "is the same")
            first = next((n for n, (x, y) in enumerate(zip(code_a, code_b)) if x != y), min(len(code_a), len(code_b)))
            print("DIFFERENT %s (%s, now in %s; %d / %d lines, first difference at %d)" % (sym, what, file_b, len(code_a), len(code_b), first))
            bad += 1
    same = len(set(old) & set(new)) - sum(1 for s in set(old) & set(new) if old[s][:2] != new[s][:2])
    print("isa_diff: %d kernels old, %d new, %d identical, %d different or missing" % (len(old), len(new), same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
