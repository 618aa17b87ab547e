"""The batched quality calls (include/kmeans_hip.h at kmg_batch_quality_report) through every layer that needs no device: header
and Python binding agree, the report is 32 bytes, the CLI takes `batch --max-error`, the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "kmeans-gpu_amd", "lib")
CALLS = ("kmg_dev_palette_batch_counts", "kmg_dev_apply_batch_counts", "kmg_dev_compare_batch", "kmg_reduce_quality_batch")
FIELDS = ["rounds", "palette_runs", "launches", "measure_launches", "batched", "per_image", "sub_batches", "fallback"]


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
    assert [len(getattr(L, n).argtypes) for n in CALLS] == [10, 12, 12, 17]


def test_quality_report_is_thirty_two_bytes_in_header_binding_and_rust():
    import kmeans_gpu_amd as kg
    fields = re.search(r"typedef struct kmg_batch_quality_report \{(.*?)\} kmg_batch_quality_report;", _header(), flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", fields)
    assert [n for _, n in fields] == FIELDS
    assert all(t == "uint32_t" for t, _ in fields)
    assert C.sizeof(kg.BatchQualityReport) == 32
    assert [n for n, _ in kg.BatchQualityReport._fields_] == FIELDS
    rust = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    rfields = re.search(r"pub struct kmg_batch_quality_report \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):\s*(\w+),", rfields) == [(n, "u32") for n in FIELDS]
    for name in CALLS:
        assert re.search(r"pub\s+fn\s+" + name + r"\s*\(", rust), name


def test_processor_has_the_batched_quality_methods():
    import kmeans_gpu_amd as kg
    for name in ("reduce_quality_batch", "palette_batch_counts_device", "apply_batch_counts_device", "compare_batch_device"):
        assert callable(getattr(kg.ImageProcessor, name))
    assert "BatchQualityReport" in kg.__all__
    assert "rounds=1" in repr(kg.BatchQualityReport(1, 2, 3, 4, 5, 6, 7, 8)) and "fallback=8" in repr(kg.BatchQualityReport(1, 2, 3, 4, 5, 6, 7, 8))


def test_cli_parser_accepts_batch_max_error(capsys):
    from kmeans_gpu_amd import cli
    args = cli.build_parser().parse_args(["batch", "-i", "a", "b", "-c", "40", "-o", "d", "--max-error", "2.5", "--min-colors", "3"])
    assert (args.command, args.input, args.colorcount, args.max_error, args.min_colors, args.indexed) == ("batch", ["a", "b"], 40, 2.5, 3, False)
    args = cli.build_parser().parse_args(["batch", "-i", "a", "-c", "8", "-o", "d"])
    assert (args.max_error, args.min_colors) == (None, None)
    # what the sub-command refuses before it loads an image
    for argv, words in ((["batch", "-i", "a", "-c", "8", "-o", "d", "--min-colors", "3"], "--min-colors belongs to --max-error"),
                        (["batch", "-i", "a", "-c", "8", "-o", "d", "--max-error", "2", "--min-colors", "9"], "--min-colors 9 is above -c 8"),
                        (["batch", "-i", "a", "-c", "8", "-o", "d", "-a", "octree", "--max-error", "2"], "octree"),
                        (["batch", "-i", "a", "-c", "8", "--palette", "--max-error", "2"], "not with --palette")):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert words in capsys.readouterr().err, argv


def test_search_header_is_host_only():
    """csrc/kmg_quality_search.h includes nothing of the device or the library: tests/native/check_quality_search.cpp builds with g++"""
    text = open(os.path.join(ROOT, "kmeans-gpu_amd", "csrc", "kmg_quality_search.h")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["stdint.h"]


def test_cpp_mirror_compiles_with_the_batched_quality_call(tmp_path):
    """as tests/test_batch_binding.py builds its program; run: a device-less box fails loudly, a box with a device compares the
    batch with the per-image calls"""
    exe = str(tmp_path / "check_batch_quality_api")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "kmeans-gpu_amd", "host"),
                    os.path.join(ROOT, "tests", "native", "check_batch_quality_api.cpp"), "-o", exe,
                    "-L", LIBDIR, "-lkmeans_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe, "nogpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("error ") or r.stdout.startswith("batch quality ok "), r.stdout
