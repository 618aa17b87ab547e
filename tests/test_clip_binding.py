"""The clip calls (include/kmeans_hip.h at kmg_dev_frame_delta_clip and kmg_clip_report) through every layer that needs no device:
header and Python binding agree, the report is 16 bytes, the constants match, the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "kmeans-gpu_amd", "lib")
CALLS = ("kmg_dev_frame_delta_clip", "kmg_sequence_output_frames")


def _header():
    text = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_header_and_binding_declare_the_same_calls():
    import kmeans_gpu_amd as kg
    header = _header()
    L = kg.lib()
    for name in CALLS:
        m = re.search(r"KMG_API\s+int\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in include/kmeans_hip.h"
        assert name in kg.SYMBOLS
        assert hasattr(L, name), f"{name} is not exported by the library"
        assert len(m.group(1).split(",")) == len(getattr(L, name).argtypes), name
    assert [len(getattr(L, n).argtypes) for n in CALLS] == [16, 10]


def test_clip_report_is_sixteen_bytes_in_header_and_binding():
    import kmeans_gpu_amd as kg
    fields = re.search(r"typedef struct kmg_clip_report \{(.*?)\} kmg_clip_report;", _header(), flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", fields)
    assert [n for _, n in fields] == ["launches", "batched", "per_image", "sub_clips"]
    assert all(t == "uint32_t" for t, _ in fields)
    assert C.sizeof(kg.ClipReport) == 16
    assert [n for n, _ in kg.ClipReport._fields_] == [n for _, n in fields]
    assert kg.ClipReport(1, 2, 3, 4).as_tuple() == (1, 2, 3, 4)


def test_constants_match_the_header():
    import kmeans_gpu_amd as kg
    header = _header()
    assert int(re.search(r"#define KMG_CLIP_FULL_ON_CLEAR (\d+)u", header).group(1)) == kg.CLIP_FULL_ON_CLEAR
    assert int(re.search(r"#define KMG_CLIP_FRAMES (\d+)u", header).group(1)) == kg.CLIP_FRAMES
    assert int(re.search(r"#define KMG_CLIP_MIN_FRAMES (\d+)u", header).group(1)) == kg.CLIP_MIN_FRAMES
    assert C.sizeof(kg.FrameHold) == 48


def test_python_surface():
    import kmeans_gpu_amd as kg
    assert callable(kg.Sequence.frames) and callable(kg.ImageProcessor.frame_delta_clip)
    for name in ("ClipReport", "CLIP_FULL_ON_CLEAR", "CLIP_FRAMES", "CLIP_MIN_FRAMES"):
        assert name in kg.__all__


def test_null_sequence_is_refused_first():
    import kmeans_gpu_amd as kg
    L = kg.lib()
    assert L.kmg_sequence_output_frames(None, 0, None, 0, None, 0, None, None, None, None) == -1
    assert b"sequence is NULL" in L.kmg_last_error()
    assert L.kmg_dev_frame_delta_clip(None, 0, None, None, None, None, 0, 0, 0, 0, None, 0, None, None, None, None) == -1
    assert b"RGBA8" in L.kmg_last_error()                            # the order of kmg_dev_frame_delta_lossy: the format first


def _build(tmp_path):
    exe = str(tmp_path / "check_clip_api")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "kmeans-gpu_amd", "host"),
                    os.path.join(ROOT, "tests", "native", "check_clip_api.cpp"), "-o", exe,
                    "-L", LIBDIR, "-lkmeans_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_device(tmp_path):
    import torch
    r = subprocess.run([_build(tmp_path), "nogpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    if not torch.cuda.is_available():
        assert r.stdout.startswith("error ") and len(r.stdout.split(None, 2)[2].strip()) > 0


@pytest.mark.gpu
def test_cpp_frames_agree_with_frame_and_frame_lossy(torch_cuda, tmp_path):
    r = subprocess.run([_build(tmp_path), "nogpu"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("clip ok "), r.stdout + r.stderr
