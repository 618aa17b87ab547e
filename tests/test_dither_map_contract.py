"""The dither maps (include/kmeans_hip.h at kmg_dither_map) through every layer that needs no device: the test-side reference
(tests/dither_map_ref.py) against the oracle's dither with the reference's matrix, the built-in tables, the blue-noise map, the
refusals of kmg_dither_map_values, the CLI's argument errors, and header, binding, C++ mirror and Rust shim side by side."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dither_map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"kmg_processor_set_dither": 3, "kmg_processor_set_dither_custom": 6, "kmg_dither_map_values": 5}
BLUE64_SHA256 = "cb918acacb48574deb4d4847b60fd36ed24516d148d8e07dab2d7fe2035b9635"


@pytest.mark.parametrize("w,h,k", [(7, 5, 2), (64, 33, 8), (257, 131, 64), (300, 200, 256), (130, 70, 700)])
def test_reference_equals_the_oracle_with_the_reference_matrix(oracle, w, h, k):
    rng = np.random.default_rng(1000 * k + w)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    pal = rng.integers(0, 256, (k, 3), dtype=np.uint8)
    cent = oracle.centroids4(np.stack([oracle.palette_srgb8_to_lab(c) for c in pal]))
    want = oracle.dither(oracle.rgb_to_lab(img), w, h, cent).reshape(h, w)
    got = R.labels(oracle, img, cent, R.BAYER4, 16, 1.0)
    assert int((got != want).sum()) == 0


def test_one_colour_is_replace(oracle):
    img = np.random.default_rng(3).integers(0, 256, (9, 11, 4), dtype=np.uint8)
    cent = np.array([[50.0, 10.0, -10.0, 1.0]], np.float32)
    assert not R.labels(oracle, img, cent, R.bayer(8), 64).any()


def test_bayer_maps_are_the_recursion_and_map_0_the_reference_matrix():
    import kmeans_gpu_amd as kg
    for m, side in ((kg.DitherMap.Bayer2, 2), (kg.DitherMap.Bayer4, 4), (kg.DitherMap.Bayer8, 8), (kg.DitherMap.Bayer16, 16)):
        levels, n = kg.dither_map_values(m)
        assert n == side * side and levels.dtype == np.uint16 and levels.shape == (side, side)
        assert np.array_equal(levels, R.bayer(side)), side
    assert kg.dither_map_values(0)[0].ravel().tolist() == [0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5]   # mix_colors.wgsl:14-17
    assert np.array_equal(R.bayer(4), R.BAYER4)
    assert kg.dither_map_values("bayer16")[1] == 256 and kg.dither_map_values("BLUE")[1] == 4096
    assert list(kg.DITHER_MAP_NAMES) == ["bayer4", "bayer2", "bayer8", "bayer16", "blue"]
    assert [int(kg.DitherMap[n]) for n in ("Bayer4", "Bayer2", "Bayer8", "Bayer16", "Blue64", "Custom")] == list(range(6))


def test_blue64_is_a_pinned_permutation():
    import kmeans_gpu_amd as kg
    levels, n = kg.dither_map_values(kg.DitherMap.Blue64)
    assert levels.shape == (64, 64) and n == 4096
    assert sorted(levels.ravel().tolist()) == list(range(4096))
    assert hashlib.sha256(levels.astype("<u2").tobytes()).hexdigest() == BLUE64_SHA256


def _low_frequency_power(table):
    """mean power of the mean-free spectrum at radial frequencies 0 < r <= 8 cycles per map"""
    t = table.astype(np.float64)
    n = t.shape[0]
    power = np.abs(np.fft.fft2(t - t.mean())) ** 2 / t.size
    f = np.minimum(np.arange(n), n - np.arange(n))
    r = np.hypot(f[:, None], f[None, :])
    return power[(r > 0) & (r <= 8)].mean()


def test_blue64_is_blue():
    """below the smallest low-frequency power among 16 seeded random permutations of the same size (a void-and-cluster map sits near
    3e-4 of that)"""
    import kmeans_gpu_amd as kg
    blue = _low_frequency_power(kg.dither_map_values("blue")[0])
    white = min(_low_frequency_power(np.random.default_rng(seed).permutation(4096).reshape(64, 64)) for seed in range(16))
    print("low-frequency power: blue64", blue, "smallest of 16 random permutations", white)
    assert blue < white


def test_the_generator_reproduces_the_committed_table():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_blue_noise.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_dither_map_values_refusals():
    import kmeans_gpu_amd as kg
    L = kg.lib()
    w, h, n = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    buf = (C.c_uint16 * 4096)(*([9] * 4096))
    for bad in (-1, int(kg.DitherMap.Custom), 6, 99):
        assert L.kmg_dither_map_values(bad, C.byref(w), C.byref(h), C.byref(n), buf) == -1
        assert b"dither map" in L.kmg_last_error()
    assert L.kmg_dither_map_values(0, None, C.byref(h), C.byref(n), buf) == -1
    assert L.kmg_dither_map_values(0, C.byref(w), None, C.byref(n), buf) == -1
    assert L.kmg_dither_map_values(0, C.byref(w), C.byref(h), None, buf) == -1
    assert L.kmg_dither_map_values(0, C.byref(w), C.byref(h), C.byref(n), None) == -1
    assert (w.value, h.value, n.value) == (7, 7, 7) and set(buf[:]) == {9}           # nothing written
    assert L.kmg_processor_set_dither(None, 0, C.c_float(1.0)) == -1
    assert L.kmg_processor_set_dither_custom(None, buf, 4, 4, 16, C.c_float(1.0)) == -1
    with pytest.raises(ValueError):
        kg.dither_map_values("bayer3")


def _cli_error(argv):
    from kmeans_gpu_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    return e.value.code


def test_cli_argument_errors(tmp_path, capsys):
    from PIL import Image
    img = str(tmp_path / "in.png")
    Image.fromarray(np.zeros((8, 8, 4), np.uint8)).save(img)
    # both options are errors without -m dither
    for sub in (["reduce", "-i", img, "-c", "4"], ["find", "-i", img, "-p", "#000000,#ffffff"], ["sequence", "-i", img, "-c", "4"],
                ["batch", "-i", img, "-c", "4", "-o", str(tmp_path)]):
        for mode in ([], ["-m", "replace"], ["-m", "diffuse"], ["-m", "meld"] if sub[0] != "sequence" else ["-m", "replace"]):
            assert _cli_error(sub + mode + ["--dither-map", "bayer8"]) == 2
            assert "need -m dither" in capsys.readouterr().err
            assert _cli_error(sub + mode + ["--dither-strength", "0.5"]) == 2
            assert "need -m dither" in capsys.readouterr().err
    base = ["reduce", "-i", img, "-c", "4", "-m", "dither"]
    for bad in ("-1", "4.5", "nan", "inf", "x"):
        assert _cli_error(base + ["--dither-strength", bad]) == 2
    capsys.readouterr()
    assert _cli_error(base + ["--dither-map", "bayer3"]) == 2
    assert "neither one of" in capsys.readouterr().err
    assert _cli_error(base + ["--dither-map", str(tmp_path / "missing.png")]) == 2
    assert "cannot read" in capsys.readouterr().err
    rgb = str(tmp_path / "rgb.png")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(rgb)
    assert _cli_error(base + ["--dither-map", rgb]) == 2
    assert "grey 8-bit" in capsys.readouterr().err
    for shape in ((8, 12), (128, 8), (3, 4)):
        odd = str(tmp_path / "odd.png")
        Image.fromarray(np.zeros(shape, np.uint8)).save(odd)
        assert _cli_error(base + ["--dither-map", odd]) == 2
        assert "power of two" in capsys.readouterr().err
    assert _cli_error(["--devices", "0,1"] + base + ["--dither-map", "blue"]) == 2
    assert "--devices" in capsys.readouterr().err
    # `palette` has no mode and takes neither option
    assert _cli_error(["palette", "-i", img, "-c", "4", "--dither-map", "blue"]) == 2


def test_cli_reads_a_png_map(tmp_path):
    """check_dither turns a grey PNG into (levels, strength, 256)"""
    import argparse
    from PIL import Image
    from kmeans_gpu_amd import cli
    levels = np.random.default_rng(5).integers(0, 256, (2, 16), dtype=np.uint8)
    path = str(tmp_path / "map.png")
    Image.fromarray(levels).save(path)
    args = argparse.Namespace(dither_map=path, dither_strength=None, mode="dither", devices=None)
    cli.check_dither(args, cli.build_parser())
    assert np.array_equal(args.dither[0], levels) and args.dither[0].dtype == np.uint16 and args.dither[1:] == (1.0, 256)
    args = argparse.Namespace(dither_map=None, dither_strength=2.0, mode="dither", devices=None)
    cli.check_dither(args, cli.build_parser())
    assert args.dither == ("bayer4", 2.0, None)


def _header():
    text = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_header_binding_mirror_and_shim_declare_the_same_calls():
    import kmeans_gpu_amd as kg
    header = _header()
    L = kg.lib()
    hpp = open(os.path.join(ROOT, "kmeans-gpu_amd", "host", "kmeans_color_gpu.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    for name, n_args in CALLS.items():
        m = re.search(r"KMG_API\s+int\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in include/kmeans_hip.h"
        assert "[" not in m.group(1), f"{name}: pointer parameters, not array parameters"
        assert name in kg.SYMBOLS and hasattr(L, name)
        assert len(m.group(1).split(",")) == len(getattr(L, name).argtypes) == n_args, name
        assert name + "(" in hpp, f"{name} is not used by the C++ mirror"
        assert re.search(r"pub\s+fn\s+" + name + r"\s*\(", ffi), f"{name} is not declared in rust-shim/src/ffi.rs"
    enum = re.search(r"typedef enum kmg_dither_map \{(.*?)\} kmg_dither_map;", header, flags=re.S).group(1)
    values = dict((n, int(v)) for n, v in re.findall(r"(KMG_DITHER_\w+)\s*=\s*(\d+)", enum))
    assert values == {"KMG_DITHER_BAYER4": 0, "KMG_DITHER_BAYER2": 1, "KMG_DITHER_BAYER8": 2, "KMG_DITHER_BAYER16": 3, "KMG_DITHER_BLUE64": 4,
                      "KMG_DITHER_CUSTOM": 5, "KMG_DITHER_COUNT": 6}
    for n, v in values.items():
        assert re.search(r"pub const " + n + r": c_int = " + str(v) + ";", ffi), n
    for n, v in values.items():
        if n != "KMG_DITHER_COUNT":
            assert int(kg.DitherMap(v)) == v
    for name in ("DitherMap", "DITHER_MAP_NAMES", "dither_map_values"):
        assert name in kg.__all__
    assert callable(kg.ImageProcessor.set_dither)


def test_cpp_mirror_compiles_with_the_dither_calls(tmp_path):
    """a translation unit that uses the three wrappers compiles against the mirror (host compiler only)"""
    src = tmp_path / "use_dither.cpp"
    src.write_text('#include "kmeans_color_gpu.hpp"\n'
                   "int main() {\n"
                   "    uint32_t w = 0, h = 0, n = 0;\n"
                   "    const std::vector<uint16_t> levels = kmeans_color_gpu::ImageProcessor::dither_map_values(KMG_DITHER_BAYER8, &w, &h, &n);\n"
                   "    void (kmeans_color_gpu::ImageProcessor::*a)(int, float) const = &kmeans_color_gpu::ImageProcessor::set_dither;\n"
                   "    void (kmeans_color_gpu::ImageProcessor::*b)(const std::vector<uint16_t> &, uint32_t, uint32_t, uint32_t, float) const =\n"
                   "        &kmeans_color_gpu::ImageProcessor::set_dither;\n"
                   "    return (a && b && levels.size() == 64 && w == 8 && h == 8 && n == 64) ? 0 : 1;\n"
                   "}\n")
    libdir = os.path.join(ROOT, "kmeans-gpu_amd", "lib")
    exe = str(tmp_path / "use_dither")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "kmeans-gpu_amd", "host"), str(src), "-o", exe,
                    "-L", libdir, "-lkmeans_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([exe]).returncode == 0
