"""The filters of KMG_MODE_DIFFUSE (kmg_diffusion) without a device: the test-side reference (tests/diffusion_ref.py) against the
literal raster loop for every filter, filter 0 against the Floyd-Steinberg reference, the table and the refusals of the two new
functions, their names in every mirror of the C ABI, the CLI's --diffusion, and the mean of a flat grey."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import diffuse_ref
import diffusion_ref


def _palette(k, seed):
    rng = np.random.default_rng(seed)
    pal = np.full((k, 4), 255, np.uint8)
    pal[:, :3] = rng.integers(0, 256, (k, 3))
    return pal


def _library_weights(f):
    import kmeans_gpu_amd as kg
    return kg.diffusion_weights(f)


@pytest.mark.parametrize("f", range(8))
def test_diagonal_reference_equals_the_serial_raster_loop(oracle, f):
    weights, divisor = _library_weights(f)
    replace = diffuse_ref.oracle_find_replace(oracle, _palette(5, 5))
    near = diffuse_ref.Nearest(replace)
    for h, w in [(1, 1), (1, 5), (2, 1), (3, 2), (7, 9), (5, 17)]:
        img = np.random.default_rng(100 * h + w + f).integers(0, 256, (h, w, 4), dtype=np.uint8)
        # (one table of nearest colours for both roads: the diagonals ask the oracle in batches, the loop then finds them there)
        got = diffusion_ref.diffuse(img, replace, weights, divisor, nearest=near)
        assert np.array_equal(got, diffusion_ref.diffuse_serial(img, replace, weights, divisor, nearest=near)), (h, w)
        keep = img[..., 3] >= 128                               # alpha mode's mask takes the same two roads
        got = diffusion_ref.diffuse(img, replace, weights, divisor, keep=keep, nearest=near)
        assert np.array_equal(got, diffusion_ref.diffuse_serial(img, replace, weights, divisor, keep=keep, nearest=near)), (h, w)


def test_filter_0_is_the_floyd_steinberg_reference(oracle):
    weights, divisor = _library_weights(0)
    img = np.random.default_rng(4050).integers(0, 256, (40, 50, 4), dtype=np.uint8)
    replace = diffuse_ref.oracle_find_replace(oracle, _palette(7, 7))
    assert np.array_equal(diffusion_ref.diffuse(img, replace, weights, divisor), diffuse_ref.diffuse(img, replace))


def test_weights_table_and_refusals_need_no_device():
    import kmeans_gpu_amd as kg
    L = kg.lib()
    for f in range(8):
        weights, divisor = _library_weights(f)
        want, d = diffusion_ref.table_weights(f)
        assert divisor == d and np.array_equal(weights, want), f
        assert divisor % 2 == 0                                  # D/2 is an integer for every filter
        assert weights.sum() == (6 if f == 2 else divisor)       # Atkinson passes on 6/8, every other filter all of it
        by_name = _library_weights(diffusion_ref.NAMES[f])       # the CLI's name reaches the same filter
        assert by_name[1] == divisor and np.array_equal(by_name[0], weights)
        assert kg.Diffusion(f) == f and kg.DIFFUSION_NAMES[diffusion_ref.NAMES[f]] == f
    w = (C.c_int32 * 12)(*([77] * 12))
    d = C.c_int32(77)
    for bad in (-1, 8, 1 << 20):
        assert L.kmg_diffusion_weights(bad, w, C.byref(d)) == -1
        assert list(w) == [77] * 12 and d.value == 77
    assert L.kmg_diffusion_weights(1, None, C.byref(d)) == -1
    assert L.kmg_diffusion_weights(1, w, None) == -1
    for f in (-1, 0, 3, 8):
        assert L.kmg_processor_set_diffusion(None, f) == -1
    with pytest.raises(ValueError):
        kg.diffusion_weights("floyd")


def test_the_kernels_reciprocal_division_is_the_floor_for_every_sum():
    """kmg_diffuse_wide.hip divides by the wave-uniform D as umulhi(S + D/2 + 4096 D, ceil(2^32 / D)) - 4096: the mathematical
    floor of (S + D/2) / D for every S the contract admits (|S| <= 4080 D), for every divisor of the table"""
    for f in range(8):
        _, D = _library_weights(f)
        S = np.arange(-4080 * D, 4080 * D + 1, dtype=np.int64)
        u = S + D // 2 + 4096 * D
        assert u.min() >= 0 and u.max() < 1 << 32
        magic = ((1 << 32) + D - 1) // D
        assert magic < 1 << 32
        assert np.array_equal(((u * magic) >> 32) - 4096, (S + D // 2) // D), D


def test_names_in_every_mirror():
    import kmeans_gpu_amd as kg
    header = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    names = ["FLOYD_STEINBERG", "SIERRA_LITE", "ATKINSON", "BURKES", "SIERRA2", "SIERRA3", "JARVIS", "STUCKI"]
    for value, name in enumerate(names):
        assert re.search(r"\bKMG_DIFFUSION_%s\s*=\s*%d\b" % (name, value), header), name
        assert re.search(r"pub const KMG_DIFFUSION_%s: c_int = %d;" % (name, value), ffi), name
        assert diffusion_ref.NAMES[value] == name.lower().replace("_", "-")
    assert re.search(r"\bKMG_DIFFUSION_COUNT\s*=\s*8\b", header)
    assert re.search(r"KMG_API\s+int\s+kmg_processor_set_diffusion\s*\(\s*kmg_processor\s*\*p,\s*int\s+filter\s*\)\s*;", header)
    assert re.search(r"KMG_API\s+int\s+kmg_diffusion_weights\s*\(\s*int\s+filter,\s*int32_t\s*\*weights,\s*int32_t\s*\*divisor\s*\)\s*;", header)
    L = kg.lib()
    for fn in ("kmg_processor_set_diffusion", "kmg_diffusion_weights"):
        assert fn in kg.SYMBOLS and hasattr(L, fn), fn
        assert re.search(r"pub fn %s\(" % fn, ffi), fn
    lib_rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    assert "pub fn set_diffusion" in lib_rs and "ffi::kmg_processor_set_diffusion" in lib_rs
    hpp = open(os.path.join(ROOT, "kmeans-gpu_amd", "host", "kmeans_color_gpu.hpp")).read()
    assert "set_diffusion" in hpp and "kmg_processor_set_diffusion" in hpp


def test_cli_takes_diffusion_with_mode_diffuse_only(capsys):
    from kmeans_gpu_amd import cli
    ap = cli.build_parser()
    args = ap.parse_args(["find", "-i", "gfx/tokyo.png", "-p", "#050505,#ffffff", "-m", "diffuse", "--diffusion", "atkinson"])
    assert args.diffusion == "atkinson" and args.mode == "diffuse"
    cli.check_diffusion(args, ap)                                # accepted
    for argv in (["reduce", "-i", "gfx/tokyo.png", "-c", "8", "--diffusion", "sierra-lite", "-m", "diffuse"],
                 ["sequence", "-i", "a.png", "b.png", "-c", "8", "--diffusion", "sierra3", "-m", "diffuse"],
                 ["batch", "-i", "a.png", "-c", "8", "-o", "out", "--diffusion", "floyd-steinberg", "-m", "diffuse"]):
        args = ap.parse_args(argv)
        cli.check_diffusion(args, ap)
        assert args.diffusion in diffusion_ref.NAMES
    for argv in (["find", "-i", "gfx/tokyo.png", "-p", "#050505,#ffffff", "--diffusion", "atkinson"],
                 ["reduce", "-i", "gfx/tokyo.png", "-c", "8", "-m", "dither", "--diffusion", "jarvis"],
                 ["batch", "-i", "a.png", "-c", "8", "-o", "out", "--diffusion", "stucki"],
                 ["sequence", "-i", "a.png", "b.png", "-c", "8", "--diffusion", "burkes"]):
        with pytest.raises(SystemExit) as e:                     # the whole command: refused before any file is read
            cli.main(argv)
        assert e.value.code == 2
        assert "--diffusion" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ap.parse_args(["find", "-i", "gfx/tokyo.png", "-p", "#050505", "-m", "diffuse", "--diffusion", "floyd"])
    with pytest.raises(SystemExit):
        ap.parse_args(["palette", "-i", "gfx/tokyo.png", "-c", "8", "--diffusion", "atkinson"])


@pytest.fixture(scope="module")
def black_and_white(oracle):
    """the nearest colours of the black / white palette: one table for the seven cases below"""
    pal = np.array([[0, 0, 0, 255], [255, 255, 255, 255]], np.uint8)
    return diffuse_ref.Nearest(diffuse_ref.oracle_find_replace(oracle, pal))


@pytest.mark.parametrize("f", [0, 1, 3, 4, 5, 6, 7])               # Atkinson drops a quarter of the error by definition
def test_flat_grey_keeps_its_mean_on_black_and_white(black_and_white, f):
    weights, divisor = _library_weights(f)
    img = np.full((512, 512, 4), (128, 128, 128, 255), np.uint8)
    out = diffusion_ref.diffuse(img, None, weights, divisor, nearest=black_and_white)
    assert set(np.unique(out[..., :3])) <= {0, 255}
    assert abs(float(out[..., :3].mean()) - 128.0) <= 2.0
