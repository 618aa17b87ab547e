"""The lock-step schedule of kmg_reduce_quality_batch (csrc/kmg_quality_search.h) in a stand-alone program of its own
(tests/native/check_quality_search.cpp): no device, nothing loaded into Python.  Built twice: plain, and with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_lock_step_schedule_is_the_sequential_bisection(tmp_path, flags):
    """every (k_min, k_max) with 1 <= k_min <= k_max <= 40: every monotone threshold (the never-accepted one included), periodic and
    pseudo-random non-monotone acceptance -- the counts asked for, k*, reached and the evaluation kept equal kmg_reduce_quality's
    loop, within 1 + ceil(log2(k_max - k_min + 1)) evaluations; 64 searches advanced round by round end as they do alone"""
    exe = str(tmp_path / "check_quality_search")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "kmeans-gpu_amd", "csrc"),
                    os.path.join(NATIVE, "check_quality_search.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "search ok" in r.stdout and "failures 0" in r.stdout, r.stdout + r.stderr
