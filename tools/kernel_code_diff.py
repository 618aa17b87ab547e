#!/usr/bin/env python3
"""Is the device code of this tree the device code of another tree, kernel by kernel?  For a change that must not touch a kernel
(a host-side refactor): no GPU needed.

    tools/kernel_code_diff.py PARENT_TREE [--jobs N] [--only kmg_lists.hip ...] > profiles/<name>_isa.txt

PARENT_TREE is a checkout of the commit to compare with (git worktree add, or git archive | tar -x).  For every translation
unit of the Makefile's SRC outside the pinned files (kmg_table.hip, kmg_cube.hip: profiles/traffic.json is pinned to their text)
both trees are compiled with the Makefile's own FLAGS plus `-S --cuda-device-only`, the assembly is split by kernel symbol, and
each kernel's text is compared after
  * dropping comments and assembler directives -- the .amdhsa_ resource lines of the kernel descriptor are KEPT (registers, LDS,
    scratch, occupancy inputs),
  * replacing the function number in local labels (.LBB<n>_<m>, .Lfunc_end<n>, ...): it follows the order in which the host
    code instantiates the kernels, which such a change may alter.
A plain text comparison: it knows no instruction.  Exit status 0 when every file has the same set of kernel symbols and every
kernel the same text; 1 otherwise (the differing kernels are named, with the first differing line)."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "kmeans-gpu_amd"
PINNED = {"kmg_table.hip", "kmg_cube.hip"}


def makefile_vars(tree):
    """HIPCC, ARCH, FLAGS and SRC as the tree's Makefile states them (continuation lines joined, $(ARCH) expanded)"""
    text = open(os.path.join(tree, PKG, "Makefile")).read().replace("\\\n", " ")
    v = {}
    for name in ("HIPCC", "ARCH", "FLAGS", "SRC"):
        m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M)
        if not m:
            raise SystemExit(f"{tree}: the Makefile sets no {name}")
        v[name] = m.group(1).strip()
    v["HIPCC"] = os.environ.get("HIPCC", v["HIPCC"])
    v["FLAGS"] = v["FLAGS"].replace("$(ARCH)", os.environ.get("ARCH", v["ARCH"])).split()
    v["SRC"] = v["SRC"].split()
    return v


def assembly(tree, src, out):
    v = makefile_vars(tree)
    subprocess.run([v["HIPCC"], *v["FLAGS"], "-S", "--cuda-device-only", "-o", out, src], cwd=os.path.join(tree, PKG), check=True)
    return open(out).read()


LABEL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")


def normal(line):
    line = line.split(";", 1)[0].strip()
    if not line:
        return None
    if line.startswith(".") and not line.endswith(":") and not line.startswith(".amdhsa_"):
        return None                                                   # a directive (labels end in ':')
    return LABEL.sub(lambda m: ".L%sN%s" % (m.group(1), m.group(3) or ""), line)


def kernels(asm):
    """{kernel symbol: [normalised lines of its body, then of its .amdhsa_ block]}"""
    lines = asm.split("\n")
    out = {l.split()[1]: [] for l in lines if l.strip().startswith(".amdhsa_kernel ")}
    body = resource = None                                            # the kernel whose body / descriptor the line belongs to
    for l in lines:
        s = l.split(";", 1)[0].strip()
        if s.startswith(".amdhsa_kernel "):
            resource = s.split()[1]
        elif s.startswith(".end_amdhsa_kernel"):
            resource = None
        elif s.startswith(".Lfunc_end") and s.endswith(":"):
            body = None
        elif s.endswith(":") and s[:-1] in out:
            body = s[:-1]
        elif resource or body:
            n = normal(l)
            if n:
                out[resource or body].append(n)
    return out


def compare(parent, src, tmp):
    base = os.path.basename(src)
    new = kernels(assembly(ROOT, src, os.path.join(tmp, "new_" + base + ".s")))
    old = kernels(assembly(parent, src, os.path.join(tmp, "old_" + base + ".s")))
    report, bad = [], 0
    for name in sorted(set(old) - set(new)):
        report.append(f"  only in the parent: {name}")
        bad += 1
    for name in sorted(set(new) - set(old)):
        report.append(f"  only in this tree: {name}")
        bad += 1
    for name in sorted(set(new) & set(old)):
        a, b = old[name], new[name]
        if a != b:
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            report.append(f"  differs: {name}\n    line {at}: parent `{a[at] if at < len(a) else '<end>'}` | here `{b[at] if at < len(b) else '<end>'}`")
            bad += 1
    lines_compared = sum(len(new[n]) for n in set(new) & set(old))
    empty = [n for n in new if not new[n]]
    if empty:
        report.append(f"  no text found for: {', '.join(sorted(empty))}")
        bad += len(empty)
    return base, len(new), len(old), lines_compared, bad, report


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_tree")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--only", nargs="*", default=None, help="file names of csrc/ to compare (default: all of SRC but the pinned files)")
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_tree)
    src = [s for s in makefile_vars(ROOT)["SRC"] if os.path.basename(s) not in PINNED]
    if sorted(src) != sorted(s for s in makefile_vars(parent)["SRC"] if os.path.basename(s) not in PINNED):
        raise SystemExit("the two Makefiles list different translation units")
    if a.only is not None:
        src = [s for s in src if os.path.basename(s) in a.only]
    print("# tools/kernel_code_diff.py: device code of this tree against the parent's, kernel by kernel")
    print("# flags: " + " ".join(makefile_vars(ROOT)["FLAGS"]) + " -S --cuda-device-only")
    print("# file  kernels here / in the parent  lines compared  kernels that differ")
    total = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        for base, n_new, n_old, n_lines, bad, report in pool.map(lambda s: compare(parent, s, tmp), src):
            print(f"{base:24s} {n_new:4d} / {n_old:<4d} {n_lines:9d} {bad:4d}")
            for r in report:
                print(r)
            total += bad
            sys.stdout.flush()
    print(f"# {'IDENTICAL' if total == 0 else 'DIFFERENT'}: {total} kernels differ in {len(src)} files")
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
