"""Alpha mode (kmg_options.alpha_cutoff) on the device, bit for bit against tests/alpha_ref.py: kmg_dev_alpha_compact against
numpy (also with empty trailing workgroups and unaligned input and output), kmg_palette / kmg_reduce (k-means and octree) / kmg_find in all four modes under both strategies, the edge cases of the
contract (every pixel kept, fewer kept than k, none kept), a diffusion through an apply plan in two bands, an 8192^2 image with
random alpha, the Python and CLI layers, and the palette step at full resolution (shrink_max_dim = 0), up to more than 2^24
kept pixels.  tests/test_gpu_alpha_routes.py runs every output route in alpha mode."""
import ctypes as C
import os

import numpy as np
import pytest

import alpha_ref
from conftest import load_rgba, set_strategy

pytestmark = pytest.mark.gpu

MODES = [0, 1, 2, 3]                                  # replace, dither, meld, diffuse


@pytest.fixture(scope="module")
def images(tokyo):
    return {"tokyo_disc": alpha_ref.soft_disc(tokyo), "sprite": alpha_ref.sprite()}


@pytest.fixture(scope="module")
def aproc(torch_cuda):
    import kmeans_gpu_amd as kg
    p = kg.ImageProcessor(alpha_cutoff=1)
    yield p
    p.close()


def _compact_on_device(proc, torch, px, cutoff):
    n = px.shape[0]
    d_in = torch.from_numpy(np.ascontiguousarray(px)).cuda()
    d_out = torch.full((n + 64, 4), 0xAB, dtype=torch.uint8, device="cuda")     # (a margin: nothing may be written past n_kept)
    d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    proc.alpha_compact(d_in.data_ptr(), n, cutoff, d_out.data_ptr(), d_n.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n_kept = int(d_n.item())
    out = d_out.cpu().numpy()
    return n_kept, out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097, (1 << 20) + 7])
@pytest.mark.parametrize("pattern", ["random", "all", "none"])
def test_compact_matches_numpy(processor, torch_cuda, n, pattern):
    rng = np.random.default_rng(n)
    px = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    px[:, 3] = {"random": px[:, 3], "all": 200, "none": 3}[pattern]
    n_kept, out = _compact_on_device(processor, torch_cuda, px, 128)
    want = alpha_ref.compact(px, 128)
    assert n_kept == want.shape[0]
    assert np.array_equal(out[:n_kept], want)
    assert (out[n_kept:] == 0xAB).all()


def _edge_alpha(layout, n, t, rng):
    if layout == "random":                                  # random bytes, half of them t - 1 or t
        a = rng.integers(0, 256, n).astype(np.uint8)
        pick = rng.random(n) < 0.5
        a[pick] = np.array([t - 1, t], np.uint8)[rng.integers(0, 2, int(pick.sum()))]
        return a
    a = np.zeros(n, np.uint8)
    if layout == "runs":                                    # 1024 kept, 4096 not, 1024 kept, ...: whole tiles and chunks empty
        run = np.arange(n) % 5120
        a[run < 1024] = 255
    elif layout == "first":
        a[0] = 255
    else:
        a[-1] = 255
    return a


@pytest.mark.parametrize("n", [2048 * 1024 - 1, 2048 * 1024 + 1, 2049 * 1024 + 3, 3 * 2048 * 1024 + 5])
@pytest.mark.parametrize("layout", ["random", "runs", "first", "last"])
def test_compact_at_its_grid_edges(processor, torch_cuda, n, layout):
    """more tiles (1024 pixels) than the 2048-workgroup cap, unevenly (empty trailing workgroups); the input 1, 2 or 3 pixels into
    a device buffer (the unaligned loads) and the output 1 pixel into a sentinel-filled one; cutoffs 1, 2, 254, 255"""
    torch = torch_cuda
    rng = np.random.default_rng(n + len(layout))
    st = torch.cuda.current_stream().cuda_stream
    for i, t in enumerate((1, 2, 254, 255)):
        off = 1 + i % 3
        px = rng.integers(0, 256, (n, 4), dtype=np.uint8)
        px[:, 3] = _edge_alpha(layout, n, t, rng)
        buf = np.zeros((n + 4, 4), np.uint8)
        buf[off:off + n] = px
        d_in = torch.from_numpy(buf).cuda()
        d_out = torch.full((n + 65, 4), 0xAB, dtype=torch.uint8, device="cuda")
        d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        processor.alpha_compact(d_in.data_ptr() + 4 * off, n, t, d_out.data_ptr() + 4, d_n.data_ptr(), st)
        torch.cuda.synchronize()
        n_kept = int(d_n.item())
        out = d_out.cpu().numpy()
        want = alpha_ref.compact(px, t)
        assert n_kept == want.shape[0], (t, off)
        assert np.array_equal(out[1:1 + n_kept], want), (t, off)
        assert (out[0] == 0xAB).all() and (out[1 + n_kept:] == 0xAB).all(), (t, off)


def test_compact_cutoff_zero_copies_and_256_is_refused(processor, torch_cuda):
    import kmeans_gpu_amd as kg
    px = np.random.default_rng(3).integers(0, 256, (5000, 4), dtype=np.uint8)
    n_kept, out = _compact_on_device(processor, torch_cuda, px, 0)
    assert n_kept == 5000 and np.array_equal(out[:5000], px)
    with pytest.raises(kg.KmgError) as e:
        _compact_on_device(processor, torch_cuda, px, 256)
    assert e.value.status == -1


@pytest.mark.parametrize("strategy", ["scan", "table"])
@pytest.mark.parametrize("t", [1, 128, 255])
@pytest.mark.parametrize("name", ["tokyo_disc", "sprite"])
def test_palette_kmeans_and_octree(oracle, aproc, images, name, t, strategy):
    import kmeans_gpu_amd as kg
    set_strategy(strategy)
    img = images[name]
    aproc.set_alpha_cutoff(t)
    try:
        assert np.array_equal(aproc.palette(8, img), alpha_ref.palette_kmeans(oracle, img, 8, t))
        assert np.array_equal(aproc.palette(8, img, kg.Algorithm.Octree), alpha_ref.palette_octree(oracle, img, 8, t))
    finally:
        aproc.set_alpha_cutoff(1)


@pytest.mark.parametrize("strategy", ["scan", "table"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["tokyo_disc", "sprite"])
def test_reduce_kmeans_every_mode(oracle, aproc, images, name, mode, strategy):
    set_strategy(strategy)
    img = images[name]
    got = aproc.reduce(8, img, reduce_mode=mode)
    assert np.array_equal(got, alpha_ref.reduce_kmeans(oracle, img, 8, mode, 1))


@pytest.mark.parametrize("mode", MODES)
def test_reduce_octree_and_find_every_mode(oracle, aproc, images, mode):
    import kmeans_gpu_amd as kg
    img = images["tokyo_disc"]
    assert np.array_equal(aproc.reduce(6, img, kg.Algorithm.Octree, mode), alpha_ref.reduce_octree(oracle, img, 6, mode, 1))
    pal = np.array([[5, 5, 5, 255], [255, 255, 255, 255], [255, 0, 0, 255], [30, 90, 200, 255]], np.uint8)
    assert np.array_equal(aproc.find(img, pal, mode), alpha_ref.find(oracle, img, pal, mode, 1))


@pytest.mark.parametrize("strategy", ["scan", "table"])
def test_reduce_at_cutoff_128_and_large_k(oracle, aproc, images, strategy):
    """t = 128 (the half-transparent edges are excluded) and k = 300 (the output routes of k > 256)"""
    set_strategy(strategy)
    img = images["tokyo_disc"]
    aproc.set_alpha_cutoff(128)
    try:
        for mode in (0, 1, 3):
            assert np.array_equal(aproc.reduce(8, img, reduce_mode=mode), alpha_ref.reduce_kmeans(oracle, img, 8, mode, 128))
        cent = alpha_ref.kmeans_centroids(oracle, img, 300, 128)
        for mode in (0, 1, 2, 3):
            assert np.array_equal(aproc.reduce(300, img, reduce_mode=mode), alpha_ref.apply(oracle, img, cent, mode, 128))
    finally:
        aproc.set_alpha_cutoff(1)


@pytest.mark.parametrize("mode", MODES)
def test_opaque_image_is_the_default_call(oracle, processor, aproc, tokyo, mode):
    import kmeans_gpu_amd as kg
    assert np.array_equal(aproc.palette(8, tokyo), processor.palette(8, tokyo))
    assert np.array_equal(aproc.palette(8, tokyo, kg.Algorithm.Octree), processor.palette(8, tokyo, kg.Algorithm.Octree))
    got = aproc.reduce(8, tokyo, reduce_mode=mode)
    assert np.array_equal(got, processor.reduce(8, tokyo, reduce_mode=mode))
    if mode < 3:
        assert np.array_equal(got, oracle.reduce(tokyo, 8, mode))
    # the reference's bit-exact `find` goldens (samples.sh:6-8)
    pal3 = np.array([[5, 5, 5, 255], [255, 255, 255, 255], [255, 0, 0, 255]], np.uint8)
    golden = {0: "tokyo-find-replace-dark-white-red.png", 1: "tokyo-find-dither-dark-white-red.png"}
    if mode in golden:
        assert np.array_equal(aproc.find(tokyo, pal3, mode), load_rgba(golden[mode]))


def test_fewer_kept_pixels_than_k(oracle, aproc):
    img = np.zeros((20, 30, 4), np.uint8)
    rng = np.random.default_rng(11)
    where = [(2, 3), (5, 29), (11, 0), (19, 17), (7, 7)]
    for y, x in where:
        img[y, x] = list(rng.integers(0, 256, 3)) + [255]
    assert np.array_equal(aproc.palette(8, img), alpha_ref.palette_kmeans(oracle, img, 8, 1))
    for mode in MODES:
        assert np.array_equal(aproc.reduce(8, img, reduce_mode=mode), alpha_ref.reduce_kmeans(oracle, img, 8, mode, 1))


def test_nothing_kept(oracle, aproc):
    import kmeans_gpu_amd as kg
    img = np.random.default_rng(2).integers(0, 256, (40, 50, 4), dtype=np.uint8)
    img[..., 3] = 0
    for algo in (kg.Algorithm.Kmeans, kg.Algorithm.Octree):
        with pytest.raises(kg.KmgError) as e:
            aproc.palette(4, img, algo)
        assert e.value.status == -1 and "no pixel reaches alpha_cutoff" in str(e.value)
        out = np.full_like(img, 7)
        with pytest.raises(kg.KmgError) as e:
            aproc.reduce(4, img, algo, kg.ReduceMode.Replace, out=out)
        assert e.value.status == -1 and (out == 7).all()
    pal = np.array([[0, 0, 0, 255], [250, 250, 250, 255]], np.uint8)
    for mode in MODES:
        assert np.array_equal(aproc.find(img, pal, mode), alpha_ref.find(oracle, img, pal, mode, 1))


@pytest.mark.parametrize("strategy", ["scan", "table"])
def test_diffuse_plan_in_two_bands(oracle, aproc, torch_cuda, images, strategy):
    torch = torch_cuda
    set_strategy(strategy)
    img = images["tokyo_disc"]
    h, w = img.shape[:2]
    cent = alpha_ref.kmeans_centroids(oracle, img, 16, 1)
    want = alpha_ref.apply(oracle, img, cent, 3, 1)
    st = torch.cuda.current_stream().cuda_stream
    d_in = torch.from_numpy(img).cuda()
    whole = torch.zeros_like(d_in)
    aproc.apply(d_in.data_ptr(), w, h, 0, cent, 3, whole.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(whole.cpu().numpy(), want)
    bands = torch.zeros_like(d_in)
    split = 200
    plan = aproc.apply_plan(cent, 3, w * h, st)
    try:
        plan.run(d_in.data_ptr(), w, split, 0, bands.data_ptr(), st)
        plan.run(d_in[split:].data_ptr(), w, h - split, split, bands[split:].data_ptr(), st)
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert np.array_equal(bands.cpu().numpy(), want)


def test_large_image_with_random_alpha(processor, aproc, torch_cuda):
    """8192^2, random alpha: the compaction against numpy, and the output passes of alpha mode = the default's RGB + alpha"""
    torch = torch_cuda
    from kmeans_gpu_amd import synth
    rng = np.random.default_rng(8192)
    img = synth.uniform_rgba_numpy(99, 8192 * 8192).reshape(8192, 8192, 4)
    img[..., 3] = rng.integers(0, 256, (8192, 8192), dtype=np.uint8)
    n_kept, out = _compact_on_device(processor, torch, img.reshape(-1, 4), 128)
    want = alpha_ref.compact(img, 128)
    assert n_kept == want.shape[0] and np.array_equal(out[:n_kept], want)
    del out, want
    pal = rng.integers(0, 256, (32, 4), dtype=np.uint8)
    pal[:, 3] = 255
    for mode in (0, 1):
        got = aproc.find(img, pal, mode)
        ref = processor.find(img, pal, mode)
        ref[..., 3] = img[..., 3]
        assert np.array_equal(got, ref)


def test_python_and_cli_round_trip_alpha(oracle, torch_cuda, tmp_path):
    from PIL import Image
    import kmeans_gpu_amd as kg
    from kmeans_gpu_amd import cli
    img = alpha_ref.sprite(60, 80, seed=9)
    src = str(tmp_path / "sprite.png")
    Image.fromarray(img, "RGBA").save(src)
    dst = str(tmp_path / "out.png")
    assert cli.main(["reduce", "-i", src, "-c", "6", "-m", "dither", "--alpha-cutoff", "1", "-o", dst]) == 0
    got = np.array(Image.open(dst).convert("RGBA"))
    assert np.array_equal(got, alpha_ref.reduce_kmeans(oracle, img, 6, 1, 1))
    assert np.array_equal(got[..., 3], img[..., 3])
    with kg.ImageProcessor() as p:
        assert (p.reduce(6, img, reduce_mode=kg.ReduceMode.Dither)[..., 3] == 255).all()      # the default ignores alpha
        p.set_alpha_cutoff(1)
        assert np.array_equal(p.reduce(6, img, reduce_mode=kg.ReduceMode.Dither), got)
        with pytest.raises(kg.KmgError):
            p.set_alpha_cutoff(256)


def test_group_create_refuses_alpha_mode(torch_cuda):
    import kmeans_gpu_amd as kg
    L = kg.lib()
    o = kg.GroupOptions()
    L.kmg_default_group_options(o)
    o.n_devices = 1
    o.devices[0] = 0
    o.processor.alpha_cutoff = 1
    h = C.c_void_p()
    assert L.kmg_group_create(C.byref(o), C.byref(h)) == -1 and b"alpha_cutoff" in L.kmg_last_error()


# ---- the palette step at full resolution (shrink_max_dim = 0): the kept pixels as one row of n_kept pixels ----------------------
FULL_T = 128
_full_refs = {}


@pytest.fixture(scope="module")
def full_disc(tokyo):
    """the photograph tiled to 1536 x 1024 under a soft disc: about 0.53 M kept pixels, an image of 0.53 M x 1"""
    return alpha_ref.soft_disc(np.ascontiguousarray(np.tile(tokyo, (2, 2, 1))[:1024, :1536]))


@pytest.fixture(scope="module")
def full_proc(torch_cuda):
    import kmeans_gpu_amd as kg
    p = kg.ImageProcessor(shrink_max_dim=0, alpha_cutoff=FULL_T)
    yield p
    p.close()


def _full_centroids(oracle, img, k):
    if k not in _full_refs:
        _full_refs[k] = alpha_ref.kmeans_centroids(oracle, img, k, FULL_T, shrink_max_dim=0)
    return _full_refs[k]


def _palette_of(oracle, cent):
    pal = np.full((cent.shape[0], 4), 255, np.uint8)
    for j in range(cent.shape[0]):
        pal[j, :3] = oracle.palette_lab_to_srgb8(cent[j, :3])
    return alpha_ref.sorted_by_L(oracle, pal)


@pytest.mark.parametrize("strategy", ["scan", "table", "auto"])
@pytest.mark.parametrize("k", [8, 64])
def test_full_resolution_palette(oracle, full_proc, full_disc, k, strategy):
    set_strategy(strategy)
    assert np.array_equal(full_proc.palette(k, full_disc), _palette_of(oracle, _full_centroids(oracle, full_disc, k)))


@pytest.mark.parametrize("mode", MODES)
def test_full_resolution_reduce(oracle, full_proc, full_disc, mode):
    want = alpha_ref.apply(oracle, full_disc, _full_centroids(oracle, full_disc, 8), mode, FULL_T)
    assert np.array_equal(full_proc.reduce(8, full_disc, reduce_mode=mode), want)


def test_full_resolution_more_than_2_24_kept(oracle, torch_cuda):
    """n_kept = 17000023 > 2^24: (float)n_kept is rounded, and the first key of the initialisation, pixel
    (int)((float)width * 0.5625f), is two pixels before floor(9 width / 16)"""
    import kmeans_gpu_amd as kg
    w, h, n_kept = 5000, 4000, 17000023
    assert int(np.float32(n_kept) * np.float32(0.5625)) == n_kept * 9 // 16 + 2
    rng = np.random.default_rng(24)
    n = w * h
    c = rng.integers(0, 256, (40, 3))
    img = np.empty((n, 4), np.uint8)
    img[:, :3] = np.clip(c[rng.integers(0, 40, n)] + rng.normal(0, 12, (n, 3)), 0, 255).astype(np.uint8)
    img[:, 3] = rng.integers(FULL_T, 256, n, dtype=np.uint8)
    img[rng.permutation(n)[:n - n_kept], 3] = rng.integers(0, FULL_T, n - n_kept, dtype=np.uint8)
    img = img.reshape(h, w, 4)
    assert int((img[..., 3] >= FULL_T).sum()) == n_kept
    with kg.ImageProcessor(shrink_max_dim=0, alpha_cutoff=FULL_T) as p:
        assert np.array_equal(p.palette(8, img), alpha_ref.palette_kmeans(oracle, img, 8, FULL_T, shrink_max_dim=0))


def test_full_resolution_every_pixel_kept_is_the_default_call(torch_cuda, tokyo):
    import kmeans_gpu_amd as kg
    img = np.ascontiguousarray(np.tile(tokyo, (2, 2, 1))[:1024, :1536])
    img[..., 3] = np.random.default_rng(4).integers(FULL_T, 256, img.shape[:2], dtype=np.uint8)
    with kg.ImageProcessor(shrink_max_dim=0, alpha_cutoff=FULL_T) as pa, kg.ImageProcessor(shrink_max_dim=0) as pd:
        assert np.array_equal(pa.palette(16, img), pd.palette(16, img))
        got, ref = pa.reduce(16, img, reduce_mode=kg.ReduceMode.Dither), pd.reduce(16, img, reduce_mode=kg.ReduceMode.Dither)
        assert np.array_equal(got[..., :3], ref[..., :3]) and np.array_equal(got[..., 3], img[..., 3])
