"""The batched output calls (include/kmeans_hip.h at kmg_batch_apply_report) through every layer that needs no device: header and
Python binding agree, the report is 16 bytes, the CLI takes `batch --indexed`, the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "kmeans-gpu_amd", "lib")
CALLS = ("kmg_dev_apply_batch", "kmg_find_batch", "kmg_reduce_indexed_batch")


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
    assert [len(getattr(L, n).argtypes) for n in CALLS] == [13, 12, 15]


def test_apply_report_is_sixteen_bytes_in_header_binding_and_rust():
    import kmeans_gpu_amd as kg
    fields = re.search(r"typedef struct kmg_batch_apply_report \{(.*?)\} kmg_batch_apply_report;", _header(), flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", fields)
    assert [n for _, n in fields] == ["launches", "batched", "per_image", "sub_batches"]
    assert all(t == "uint32_t" for t, _ in fields)
    assert C.sizeof(kg.BatchApplyReport) == 16
    assert [n for n, _ in kg.BatchApplyReport._fields_] == [n for _, n in fields]
    rust = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    rfields = re.search(r"pub struct kmg_batch_apply_report \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):\s*(\w+),", rfields) == [(n, "u32") for _, n in fields]
    for name in CALLS:
        assert re.search(r"pub\s+fn\s+" + name + r"\s*\(", rust), name


def test_processor_has_the_batched_output_methods():
    import kmeans_gpu_amd as kg
    for name in ("find_batch", "reduce_indexed_batch", "apply_batch_device"):
        assert callable(getattr(kg.ImageProcessor, name))
    assert "BatchApplyReport" in kg.__all__
    assert kg.BatchApplyReport(1, 2, 3, 4).as_tuple() == (1, 2, 3, 4)


def test_cli_parser_accepts_batch_indexed():
    from kmeans_gpu_amd import cli
    args = cli.build_parser().parse_args(["batch", "-i", "a", "b", "-c", "8", "-o", "d", "--indexed"])
    assert (args.command, args.input, args.colorcount, args.output, args.mode, args.indexed) == ("batch", ["a", "b"], 8, "d", "replace", True)
    args = cli.build_parser().parse_args(["batch", "-i", "a.png", "-c", "4", "-m", "dither", "-o", "d", "--alpha-cutoff", "9"])
    assert (args.mode, args.indexed, args.alpha_cutoff) == ("dither", False, 9)


def test_cpp_mirror_compiles_with_the_batched_output_calls(tmp_path):
    """as tests/test_batch_binding.py builds its program; run: a device-less box fails loudly, a box with a device compares the
    batch with the per-image calls"""
    exe = str(tmp_path / "check_batch_apply_api")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "kmeans-gpu_amd", "host"),
                    os.path.join(ROOT, "tests", "native", "check_batch_apply_api.cpp"), "-o", exe,
                    "-L", LIBDIR, "-lkmeans_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe, "nogpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("error ") or r.stdout.startswith("batch apply ok "), r.stdout
