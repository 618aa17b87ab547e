"""The host arithmetic of the batches (csrc/kmg_batch_layout.h, csrc/kmg_apply_route.h batch_apply_joins) in a
stand-alone program of its own (tests/native/check_batch_layout.cpp): no device, nothing loaded into Python.  Built twice: plain,
and with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_layout_and_join_rule(tmp_path, flags):
    """offsets 16-byte aligned and disjoint for every format and pixel counts 1 .. 40 in mixed order; the grid's sum; the cuts at the
    piece bound; totals that overflow refused; the cuts of a batch into sub-batches (batch_cuts: the greedy rule, [0, n) covered once,
    bound 0 = 2^30, no wrap from 2^63 on); the join rule over the grid of apply_route_table.txt"""
    exe = str(tmp_path / "check_batch_layout")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", *flags, "-I", os.path.join(ROOT, "kmeans-gpu_amd", "csrc"),
                    os.path.join(NATIVE, "check_batch_layout.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, os.path.join(NATIVE, "apply_route_table.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "layout ok" in r.stdout and "cuts ok" in r.stdout and "rows 264 " in r.stdout and "join_mismatches 0" in r.stdout, r.stdout + r.stderr
