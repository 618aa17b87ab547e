#!/usr/bin/env python3
"""Are the kernels of two builds the same code, when a change renames kernels, gives them template parameters or moves them
between files?  No GPU needed.

    tools/compare_kernels.py OLD NEW [--rename 'k_old<$1, $2> = kmg::k_new<$1, true, $2, kmg::MapOffsets>' ...] [--renames FILE]

OLD and NEW are device assembly files, or directories of them (*.s, all pooled), made with the Makefile's flags plus
`-S --cuda-device-only`.  tools/kernel_code_diff.py compiles two trees itself and pairs by symbol and file, which is enough for a
change that must touch no kernel; this tool takes the text of a kernel from it (comments and directives dropped, the .amdhsa_
resource lines kept, function numbers taken out of the local labels) and pairs kernels by their DEMANGLED name without the
parameter list, i.e. `kmg::k_apply<8, true, false, false, unsigned int>`, anonymous namespaces dropped.  A rename rule rewrites a
name of OLD before pairing: on the left a kernel name with $1, $2, ... for its template arguments, on the right the name it has
in NEW.  --renames FILE: one rule per line, # comments.

Prints, per pair, identical / DIFFERENT with the instruction counts of both sides, the number of lines a diff marks and the
registers and scratch of the .amdhsa_ lines, then the kernels on one side only.  A plain text comparison: it knows no
instruction.  Exit status 0 when every kernel is paired and identical, 1 otherwise."""
import argparse
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_code_diff import kernels  # noqa: E402


def split_args(s):
    """the top-level comma-separated items of a template argument list"""
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += (ch in "<(") - (ch in ">)")
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()] if cur.strip() else out


def name_of(demangled):
    """`void kmg::(anonymous namespace)::k<1, unsigned int>(float, ...)` -> `kmg::k<1, unsigned int>`"""
    s = demangled.replace("(anonymous namespace)::", "")
    depth = 0
    for i, ch in enumerate(s):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            s = s[:i]
            break
    s = s.strip()
    return s[5:] if s.startswith("void ") else s                     # (a template instance is demangled with its return type)


def base_and_args(name):
    m = re.match(r"([^<]+)(?:<(.*)>)?$", name)
    return m.group(1).strip(), split_args(m.group(2) or "")


def load(path, filt):
    """{name: (file, lines)} of every kernel of an assembly file or a directory of them"""
    files = sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit(f"{path}: no assembly files")
    out = {}
    for f in files:
        ks = kernels(open(f).read())
        symbols = list(ks)
        names = subprocess.run([filt], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.split("\n")
        for sym, dem in zip(symbols, names):
            name = name_of(dem)
            if name in out:
                name += f" [{os.path.basename(f)}]"                  # the same name in two files (internal linkage)
            out[name] = (os.path.basename(f), [l.replace(sym, "SELF") for l in ks[sym]])
    return out


def rename(name, rules):
    base, args = base_and_args(name)
    for (lbase, largs), right in rules:
        if lbase.split("::")[-1] == base.split("::")[-1] and len(largs) == len(args):
            new = right
            for i in sorted(range(len(args)), reverse=True):
                new = new.replace("$%d" % (i + 1), args[i])
            return new
    return name


def resources(lines):
    r = {}
    for l in lines:
        m = re.match(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size)\s+(\d+)", l)
        if m:
            r[{"next_free_vgpr": "vgpr", "next_free_sgpr": "sgpr", "private_segment_fixed_size": "scratch"}[m.group(1)]] = int(m.group(2))
    return r


def instructions(lines):
    return [l for l in lines if not l.endswith(":") and not l.startswith(".amdhsa_")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--renames", help="a file of rename rules")
    ap.add_argument("--quiet", action="store_true", help="do not list the identical kernels")
    ap.add_argument("--show", metavar="TEXT", help="print the diff of the differing kernels whose name contains TEXT")
    a = ap.parse_args()
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    texts = list(a.rename)
    if a.renames:
        texts += [l.split("#", 1)[0].strip() for l in open(a.renames)]
    rules = []
    for t in filter(None, texts):
        left, right = (s.strip() for s in t.split("=", 1))
        rules.append((base_and_args(left), right))
    old = {rename(n, rules): v for n, v in load(a.old, filt).items()}
    new = load(a.new, filt)
    same = diff = 0
    for name in sorted(set(old) & set(new)):
        (fo, lo), (fn, ln) = old[name], new[name]
        io, in_ = instructions(lo), instructions(ln)
        where = fo if fo == fn else f"{fo} -> {fn}"
        if lo == ln:
            same += 1
            if not a.quiet:
                print(f"identical  {len(in_):6d}            {name}  ({where})")
            continue
        diff += 1
        marked = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, lo, ln, autojunk=False).get_opcodes() if tag != "equal")
        ro, rn = resources(lo), resources(ln)
        res = " ".join(f"{k} {ro.get(k)} -> {rn.get(k)}" for k in ("vgpr", "sgpr", "scratch"))
        print(f"DIFFERENT  {len(io):6d} -> {len(in_):<6d}  {name}  ({where}): {marked} lines differ; {res}")
        if a.show is not None and a.show in name:
            print("\n".join(difflib.unified_diff(lo, ln, a.old, a.new, lineterm="", n=2)))
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    for name in only_old:
        print(f"only in {a.old}: {name}  ({old[name][0]})")
    for name in only_new:
        print(f"only in {a.new}: {name}  ({new[name][0]})")
    print(f"# {same} identical, {diff} different, {len(only_old)} only in the first, {len(only_new)} only in the second")
    return 1 if diff or only_old or only_new else 0


if __name__ == "__main__":
    sys.exit(main())
