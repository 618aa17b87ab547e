"""Alpha mode (kmg_options.alpha_cutoff) without a device: the test-side reference (tests/alpha_ref.py) against the literal loop and
against the oracle's own default pipeline where the two must agree, and the option's validation through the built library, which
runs before the device query of kmg_processor_create_ex / kmg_group_create."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import alpha_ref
import diffuse_ref


def _palette(k, seed):
    rng = np.random.default_rng(seed)
    pal = np.full((k, 4), 255, np.uint8)
    pal[:, :3] = rng.integers(0, 256, (k, 3))
    return pal


@pytest.mark.parametrize("h,w", [(1, 1), (1, 17), (17, 1), (7, 5), (31, 26)])
@pytest.mark.parametrize("t", [1, 128, 255])
def test_diffuse_restatement_equals_the_literal_loop(oracle, h, w, t):
    rng = np.random.default_rng(100 * h + w + t)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = rng.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (h, w))
    replace = diffuse_ref.oracle_find_replace(oracle, _palette(6, t))
    got = alpha_ref.diffuse(img, replace, t)
    assert np.array_equal(got, alpha_ref.diffuse_serial(img, replace, t))
    assert np.array_equal(got[..., 3], img[..., 3])
    # an excluded pixel is the replace colour of its own unmodified colour
    excl = img[..., 3] < t
    assert np.array_equal(got[excl][:, :3], oracle.find(img, _palette(6, t), oracle.MODE_REPLACE)[excl][:, :3])


def test_diffuse_restatement_with_every_pixel_kept_is_the_diffusion(oracle):
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (40, 33, 4), dtype=np.uint8)
    img[..., 3] = rng.integers(1, 256, (40, 33))
    replace = diffuse_ref.oracle_find_replace(oracle, _palette(9, 3))
    got = alpha_ref.diffuse(img, replace, 1)
    want = diffuse_ref.diffuse(img, replace)
    assert np.array_equal(got[..., :3], want[..., :3]) and np.array_equal(got[..., 3], img[..., 3])


def test_all_kept_palette_is_the_default_pipeline(oracle, tokyo):
    """an opaque image: the restatement (shrink, rgb_to_lab, init_centroids, lloyd) is the oracle's extract_palette_kmeans"""
    cent = alpha_ref.kmeans_centroids(oracle, tokyo, 8, 1)
    want, _ = oracle.extract_palette_kmeans(tokyo, 8)
    assert np.array_equal(cent.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(alpha_ref.palette_kmeans(oracle, tokyo, 8, 255), oracle.palette(tokyo, 8))
    assert np.array_equal(alpha_ref.palette_octree(oracle, tokyo, 8, 1), oracle.palette_octree(tokyo, 8))
    assert np.array_equal(alpha_ref.reduce_kmeans(oracle, tokyo, 8, oracle.MODE_DITHER, 1), oracle.reduce(tokyo, 8, oracle.MODE_DITHER))


def test_kept_pixels_are_a_row_in_raster_order(oracle):
    img = alpha_ref.sprite()
    px, w, h = alpha_ref.kept_pixels(img, 1)
    assert h == 1 and w == int((img[..., 3] >= 1).sum()) < img.shape[0] * img.shape[1]
    order = [(y, x) for y in range(img.shape[0]) for x in range(img.shape[1]) if img[y, x, 3] >= 1]
    assert np.array_equal(px, np.array([img[y, x] for y, x in order]))
    assert alpha_ref.kept_pixels(np.zeros((3, 4, 4), np.uint8), 1) is None
    # c_0 of the compacted image: K[floor(n_kept * 0.5625)]
    cent = alpha_ref.kmeans_centroids(oracle, img, 1, 1)
    c0 = oracle.init_centroids(oracle.rgb_to_lab(px), w, 1, 1)
    assert np.array_equal(c0[0, :3], oracle.rgb_to_lab(px[int(np.float32(w) * np.float32(0.5625))])[0])
    assert cent.shape == (1, 4)


def test_compaction_reference():
    img = np.arange(4 * 10, dtype=np.uint8).reshape(10, 4)
    img[:, 3] = [0, 1, 2, 255, 0, 128, 127, 3, 0, 200]
    assert np.array_equal(alpha_ref.compact(img, 128), img[[3, 5, 9]])
    assert alpha_ref.compact(img, 0).shape == (10, 4)


def _create(opt):
    import kmeans_gpu_amd as kg
    h = C.c_void_p()
    rc = kg.lib().kmg_processor_create_ex(C.byref(opt), C.byref(h))
    if rc == 0:
        kg.lib().kmg_processor_destroy(h)
    return rc, kg.lib().kmg_last_error().decode()


def test_option_validation_runs_before_the_device_query():
    import kmeans_gpu_amd as kg
    o = kg.default_options()
    assert o.alpha_cutoff == 0 and o.struct_size == C.sizeof(kg.Options)
    o.alpha_cutoff = 256
    rc, msg = _create(o)
    assert rc == -1 and "alpha_cutoff" in msg and "256" in msg
    # the current size and both older sizes (without alpha_cutoff, without strategy) pass validation: without a device
    # the call then fails with KMG_ERR_NO_DEVICE, with one it succeeds
    for size, cutoff in ((C.sizeof(kg.Options), 1), (kg.Options.alpha_cutoff.offset, 999), (kg.Options.strategy.offset, 999)):
        o = kg.default_options()
        o.alpha_cutoff = cutoff                                   # (beyond an older size: never read)
        o.struct_size = size
        rc, msg = _create(o)
        assert rc in (0, -2), (size, rc, msg)
        if rc == -2:
            assert "no CPU path" in msg
    o = kg.default_options()
    o.struct_size = kg.Options.alpha_cutoff.offset + 2
    assert _create(o)[0] == -1
    assert kg.lib().kmg_processor_set_alpha_cutoff(None, 1) == -1


def test_group_refuses_alpha_mode_and_accepts_the_older_sizes():
    import kmeans_gpu_amd as kg
    L = kg.lib()
    o = kg.GroupOptions()
    L.kmg_default_group_options(o)
    assert o.processor.alpha_cutoff == 0
    o.processor.alpha_cutoff = 1
    h = C.c_void_p()
    assert L.kmg_group_create(C.byref(o), C.byref(h)) == -1 and b"alpha_cutoff" in L.kmg_last_error()
    # older sizes: past the size check (alpha_cutoff = 1 lies beyond them), stopped by the device-list check that follows it
    o.n_devices = 17
    base = kg.GroupOptions.processor.offset
    for size in (base + kg.Options.alpha_cutoff.offset, base + kg.Options.strategy.offset):
        o.struct_size = size
        assert L.kmg_group_create(C.byref(o), C.byref(h)) == -1 and b"KMG_MAX_DEVICES" in L.kmg_last_error()
    o.struct_size = base + kg.Options.alpha_cutoff.offset + 2
    assert L.kmg_group_create(C.byref(o), C.byref(h)) == -1 and b"struct_size" in L.kmg_last_error()


def test_dev_alpha_compact_argument_checks():
    import kmeans_gpu_amd as kg
    L = kg.lib()
    assert L.kmg_dev_alpha_compact(None, None, 1, 1, None, None, None) == -1


def test_option_in_every_mirror():
    header = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    assert re.search(r"uint32_t alpha_cutoff;", header) and "kmg_processor_set_alpha_cutoff" in header
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    assert "pub alpha_cutoff: u32," in ffi and "pub fn kmg_processor_set_alpha_cutoff" in ffi
    assert "pub fn set_alpha_cutoff" in open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    assert "kmg_processor_set_alpha_cutoff" in open(os.path.join(ROOT, "kmeans-gpu_amd", "host", "kmeans_color_gpu.hpp")).read()


class _FakeProcessor:
    made = []

    def __init__(self, *a, **kw):
        _FakeProcessor.made.append(kw)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def find(self, image, palette, mode):
        return np.zeros_like(image)

    def reduce(self, k, image, algo, mode):
        return np.zeros_like(image)

    def palette(self, k, image, algo):
        return np.zeros((k, 4), np.uint8)


def test_cli_alpha_cutoff_flag(monkeypatch):
    from kmeans_gpu_amd import cli
    saved = []
    monkeypatch.setattr(cli, "ImageProcessor", _FakeProcessor)
    monkeypatch.setattr(cli, "_load", lambda path: np.zeros((2, 3, 4), np.uint8))
    monkeypatch.setattr(cli, "_save", lambda path, out: saved.append(path))
    _FakeProcessor.made = []
    assert cli.main(["reduce", "-i", "gfx/s.png", "-c", "8", "--alpha-cutoff", "1"]) == 0
    assert cli.main(["find", "-i", "gfx/s.png", "-p", "#050505,#ffffff", "--alpha-cutoff", "255"]) == 0
    assert cli.main(["palette", "-i", "gfx/s.png", "-c", "4", "--alpha-cutoff", "7"]) == 0
    assert cli.main(["reduce", "-i", "gfx/s.png", "-c", "8"]) == 0
    assert _FakeProcessor.made == [{"alpha_cutoff": 1}, {"alpha_cutoff": 255}, {"alpha_cutoff": 7}, {}]
    assert saved[0] == os.path.join("gfx", "s-reduce-c8-kmeans-replace.png")          # output names unchanged
    for bad in ("256", "-1", "x"):
        with pytest.raises(SystemExit):
            cli.main(["reduce", "-i", "gfx/s.png", "-c", "8", "--alpha-cutoff", bad])
    with pytest.raises(SystemExit):
        cli.main(["--devices", "0", "reduce", "-i", "gfx/s.png", "-c", "8", "--alpha-cutoff", "1"])
