"""The runtime-to-template dispatch of the kernel launchers (csrc/kmg_dispatch.h) in a stand-alone program of its own
(tests/native/check_dispatch.cpp): no device, nothing loaded into Python.  Built twice: plain, and with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_every_helper_and_every_nest(tmp_path, flags):
    """every helper calls its lambda exactly once with the tag of a listed input and not at all for an unlisted one (and reports
    which); the nests of launch_apply (36 tuples), launch_dither_lists (24) and the diffusion launchers (36) reach as many distinct
    template tuples, each equal to its runtime inputs"""
    exe = str(tmp_path / "check_dispatch")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "kmeans-gpu_amd", "csrc"),
                    os.path.join(NATIVE, "check_dispatch.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "dispatch ok" in r.stdout and "failures 0" in r.stdout, r.stdout + r.stderr
