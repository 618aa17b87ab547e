"""KMG_MODE_DIFFUSE without a device: the test-side reference (tests/diffuse_ref.py) against the literal raster loop of the
contract, the mode's value in every mirror of the C ABI, and the CLI's `-m diffuse`."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import diffuse_ref


def _palette(k, seed):
    rng = np.random.default_rng(seed)
    pal = np.full((k, 4), 255, np.uint8)
    pal[:, :3] = rng.integers(0, 256, (k, 3))
    return pal


@pytest.mark.parametrize("h,w", [(1, 1), (1, 17), (17, 1), (7, 5), (40, 33)])
@pytest.mark.parametrize("k", [1, 2, 5, 64])
def test_diagonal_reference_equals_the_serial_raster_loop(oracle, h, w, k):
    rng = np.random.default_rng(1000 * h + 10 * w + k)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    replace = diffuse_ref.oracle_find_replace(oracle, _palette(k, k))
    want = diffuse_ref.diffuse_serial(img, replace)
    got = diffuse_ref.diffuse(img, replace)
    assert np.array_equal(got, want)
    assert (got[..., 3] == 255).all()
    if k == 1:                                                   # one colour: every pixel is pal[0]'s replace bytes
        one = oracle.find(img[:1, :1], _palette(1, 1), oracle.MODE_REPLACE)[0, 0]
        assert (got.reshape(-1, 4) == one).all()


def test_mode_value_in_every_mirror():
    import kmeans_gpu_amd as kg
    header = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    assert re.search(r"\bKMG_MODE_DIFFUSE\s*=\s*3\b", header)
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    assert re.search(r"pub const KMG_MODE_DIFFUSE: c_int = 3;", ffi)
    lib_rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    assert "ReduceMode::Diffuse => ffi::KMG_MODE_DIFFUSE" in lib_rs and 'ReduceMode::Diffuse => "diffuse"' in lib_rs
    hpp = open(os.path.join(ROOT, "kmeans-gpu_amd", "host", "kmeans_color_gpu.hpp")).read()
    assert "Diffuse = KMG_MODE_DIFFUSE" in hpp and '"diffuse"' in hpp
    assert kg.ReduceMode.Diffuse == 3 and kg.ReduceMode(3).name == "Diffuse"


class _FakeProcessor:
    calls = []

    def __init__(self, *a, **kw):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def find(self, image, palette, mode):
        _FakeProcessor.calls.append(("find", int(mode)))
        return np.zeros_like(image)

    def reduce(self, k, image, algo, mode):
        _FakeProcessor.calls.append(("reduce", int(mode)))
        return np.zeros_like(image)


def test_cli_accepts_diffuse_and_names_the_output(monkeypatch):
    from kmeans_gpu_amd import cli
    saved = []
    monkeypatch.setattr(cli, "ImageProcessor", _FakeProcessor)
    monkeypatch.setattr(cli, "_load", lambda path: np.zeros((2, 3, 4), np.uint8))
    monkeypatch.setattr(cli, "_save", lambda path, out: saved.append(path))
    _FakeProcessor.calls = []
    assert cli.main(["reduce", "-i", "gfx/tokyo.png", "-c", "8", "-m", "diffuse"]) == 0
    assert cli.main(["find", "-i", "gfx/tokyo.png", "-p", "#050505,#ffffff", "-m", "diffuse"]) == 0
    assert _FakeProcessor.calls == [("reduce", 3), ("find", 3)]
    assert saved[0] == os.path.join("gfx", "tokyo-reduce-c8-kmeans-diffuse.png")
    assert saved[1].startswith(os.path.join("gfx", "tokyo-find-diffuse-"))
    assert cli.reduce_file_path(8, "kmeans", "diffuse", None, "gfx/tokyo.png") == "gfx/tokyo-reduce-c8-kmeans-diffuse.png"
    with pytest.raises(SystemExit):
        cli.main(["reduce", "-i", "gfx/tokyo.png", "-c", "8", "-m", "floyd"])
