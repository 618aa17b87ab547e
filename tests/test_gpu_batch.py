"""Batched palettes (include/kmeans_hip.h at kmg_batch_report; kmg_batch.hip): many small images per launch on one device.

The yardstick is always the per-image call of the library -- kmg_lloyd_init_centroids + kmg_lloyd_run + kmg_lloyd_get_centroids,
kmg_palette, kmg_reduce -- plus the CPU oracle for a subset; never the batch code itself.  Everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
SENTINEL = 0xA5


def _rgba(rgb):
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = rgb
    return out


def _noise(seed, h, w):
    return _rgba(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


@pytest.fixture(scope="module")
def edge_images(oracle, tokyo):
    """1, 2, 255, 256, 257, 511 and 513 pixels and one of 256 x 171; 1 x n and n x 1 among them; varied widths and heights, so that
    first_pixel differs; the 511-pixel image has three distinct colours, the 1- and 2-pixel images fewer pixels than most k"""
    three = np.array([[10, 200, 30], [250, 250, 250], [90, 20, 160]], np.uint8)
    few = _rgba(three[np.random.default_rng(5).integers(0, 3, (7, 73))])                     # 73 x 7 = 511
    nw, nh = oracle.resized_dims(tokyo.shape[1], tokyo.shape[0])
    assert (nw, nh) == (256, 171)
    return [_noise(1, 1, 1), _noise(2, 1, 2), _noise(3, 255, 1), _noise(4, 1, 256), _noise(5, 1, 257), few, _noise(6, 19, 27),
            np.ascontiguousarray(oracle.resize(tokyo, nw, nh))]


def _on_device(torch, images):
    return [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in images]


def _per_image(torch, proc, d_img, im, k):
    """the per-image Lloyd calls: (centroids (k, 4), iterations)"""
    import kmeans_gpu_amd as kg
    stream = torch.cuda.current_stream().cuda_stream
    h, w = im.shape[:2]
    s = kg.Lloyd(proc, k)
    try:
        s.init_centroids(d_img.data_ptr(), w, h, stream)
        it = s.run(d_img.data_ptr(), w * h, 0, stream)
        return s.get_centroids(stream).copy(), it
    finally:
        s.close()


def _device_batch(torch, proc, d_imgs, images, k):
    stream = torch.cuda.current_stream().cuda_stream
    cent, its = proc.palette_batch_device([d.data_ptr() for d in d_imgs], [im.shape[1] for im in images], [im.shape[0] for im in images],
                                          k, stream)
    return cent, its, proc.last_batch_report


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- 1. tile edges and tiny images -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 8, 31, 32, 33, 256, 300])
def test_tile_edges_and_tiny_images(torch_cuda, processor, edge_images, k):
    d_imgs = _on_device(torch_cuda, edge_images)
    cent, its, rep = _device_batch(torch_cuda, processor, d_imgs, edge_images, k)
    assert rep.fallback == 0 and rep.sub_batches == 1
    for i, (d, im) in enumerate(zip(d_imgs, edge_images)):
        want_c, want_it = _per_image(torch_cuda, processor, d, im, k)
        assert int(its[i]) == want_it, (i, im.shape, int(its[i]), want_it)
        assert _same_bits(cent[i], want_c), (i, im.shape)
    assert rep.iterations == int(its.max())
    got = processor.palette_batch(k, edge_images)
    assert processor.last_batch_report.launches > 0                  # (eight images: the batched kernels, not the per-image loop)
    for i, im in enumerate(edge_images):
        want = processor.palette(k, im)
        assert got[i].shape == want.shape and np.array_equal(got[i], want), (i, im.shape)


# ---- 2. the CPU oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 64])
def test_three_images_match_the_oracle(torch_cuda, processor, oracle, edge_images, k):
    images = [edge_images[5], edge_images[6], edge_images[7]]        # 73 x 7 (three colours), 27 x 19, 256 x 171
    cent, its, _ = _device_batch(torch_cuda, processor, _on_device(torch_cuda, images), images, k)
    for i, im in enumerate(images):
        want_c, want_it = oracle.extract_palette_kmeans(im, k)
        assert int(its[i]) == want_it, (i, int(its[i]), want_it)
        assert _same_bits(cent[i][:, :3], want_c[:, :3]), i


# ---- 3. images stop at different times --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def staggered(oracle):
    """images whose loops stop at different checks with check_period = 4, max_iterations = 20 (k = 8), chosen with the oracle's
    lloyd: {iteration count: image}.  A flat and a two-colour image never converge (an empty cluster counts as not converged):
    they run to the cap, as the noise does."""
    yy, xx = np.mgrid[0:48, 0:64]
    cands = [_rgba(np.full((20, 30, 3), 77, np.uint8)),
             _rgba(np.where(np.arange(40)[None, :, None] < 17, np.uint8(20), np.uint8(220)) * np.ones((25, 40, 3), np.uint8)),
             _noise(7, 64, 64), _rgba(np.stack([xx * 4, yy * 5, (xx + yy) * 2], -1).astype(np.uint8))]
    for s in range(8):
        r = np.random.default_rng(s)
        cands.append(_rgba((r.integers(0, 6, (32, 32, 1)) * 50 + r.integers(0, 12, (32, 32, 3))).astype(np.uint8)))
        cands.append(_noise(100 + s, 12, 12))
    by_count = {}
    for im in cands:
        h, w = im.shape[:2]
        lab = oracle.rgb_to_lab(im)
        _, _, it = oracle.lloyd(lab, oracle.init_centroids(lab, w, h, 8), max_iterations=20, check_period=4)
        by_count.setdefault(it, im)
    return by_count


def test_images_stop_at_different_times(torch_cuda, staggered):
    import kmeans_gpu_amd as kg
    assert len(staggered) >= 3 and 19 in staggered and min(staggered) < 19, sorted(staggered)
    counts = sorted(staggered)
    early, cap = staggered[counts[0]], staggered[19]
    mids = [staggered[c] for c in counts[1:-1]]
    images = [early, cap] + mids + [early, cap] + mids[::-1] + [early]   # the early stopper first, in the middle and last
    with kg.ImageProcessor(check_period=4, max_iterations=20) as proc:
        d_imgs = _on_device(torch_cuda, images)
        want = [_per_image(torch_cuda, proc, d, im, 8) for d, im in zip(d_imgs, images)]
        spread = sorted({it for _, it in want})
        assert len(spread) >= 3 and spread[-1] == 19, spread          # (not vacuous: three stops at least, one of them the cap)
        cent, its, rep = _device_batch(torch_cuda, proc, d_imgs, images, 8)
        for i, (want_c, want_it) in enumerate(want):
            assert int(its[i]) == want_it, (i, int(its[i]), want_it)
            assert _same_bits(cent[i], want_c), i
        assert rep.iterations == 19
        # the loop's launches: the initial assignment and one per iteration up to the cap; the initialisation's: k
        assert rep.launches == 8 + 1 + 20


# ---- 4. no leakage between images ------------------------------------------------------------------------------------------
def test_no_leakage_between_images(torch_cuda, processor, edge_images):
    k = 8
    a = edge_images[6]
    d_a = _on_device(torch_cuda, [a])[0]
    want_c, want_it = _per_image(torch_cuda, processor, d_a, a, k)
    cent, its, _ = _device_batch(torch_cuda, processor, [d_a] * 32, [a] * 32, k)
    for i in range(32):
        assert int(its[i]) == want_it and _same_bits(cent[i], want_c), i
    d_imgs = _on_device(torch_cuda, edge_images)
    cent0, its0, _ = _device_batch(torch_cuda, processor, d_imgs, edge_images, k)
    perm = [3, 7, 0, 5, 1, 6, 2, 4]
    cent1, its1, _ = _device_batch(torch_cuda, processor, [d_imgs[p] for p in perm], [edge_images[p] for p in perm], k)
    for j, p in enumerate(perm):
        assert int(its1[j]) == int(its0[p]) and _same_bits(cent1[j], cent0[p]), (j, p)
    # A between two different neighbours
    cent2, its2, _ = _device_batch(torch_cuda, processor, [d_imgs[7], d_a, d_imgs[5]], [edge_images[7], a, edge_images[5]], k)
    assert int(its2[1]) == want_it and _same_bits(cent2[1], want_c)


# ---- 5. the launch count does not grow with the number of images -------------------------------------------------------
@pytest.mark.parametrize("k", [8, 33])
def test_launch_count_does_not_grow_with_the_batch(torch_cuda, processor, edge_images, k):
    d_imgs = _on_device(torch_cuda, edge_images)
    single = []
    for d, im in zip(d_imgs, edge_images):
        _, its, rep = _device_batch(torch_cuda, processor, [d], [im], k)
        assert rep.fallback == 0
        assert rep.launches >= k + 1
        single.append(rep.launches)
    _, _, rep32 = _device_batch(torch_cuda, processor, [d_imgs[6]] * 32, [edge_images[6]] * 32, k)
    assert rep32.launches == single[6] and rep32.fallback == 0
    _, _, mixed = _device_batch(torch_cuda, processor, d_imgs, edge_images, k)
    assert mixed.launches == max(single) and mixed.fallback == 0
    assert len(set(single)) > 1                                      # (the images do stop at different times)


# ---- the raw C calls, for the tests that look at the output buffers after a refusal -------------------------------------
def _raw(proc, images, k, algo=0, mode=None, bound=0, n_images=None, null=(), widths=None, heights=None, null_out_entry=None,
         null_in_entry=None):
    """kmg_palette_batch (mode None) or kmg_reduce_batch with sentinel-filled outputs: (status, outputs, counts, message)"""
    import kmeans_gpu_amd as kg
    L = kg.lib()
    n = len(images)
    imgs = [np.ascontiguousarray(im) for im in images]
    if mode is None:
        outs = [np.full((max(k, 1), 4), SENTINEL, np.uint8) for _ in imgs]
    else:
        outs = [np.full(im.shape, SENTINEL, np.uint8) for im in imgs]
    counts = np.full(max(n, 1), 0xA5A5A5A5, np.uint32)
    src = (C.c_void_p * max(n, 1))(*[im.ctypes.data for im in imgs])
    dst = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    if null_in_entry is not None:
        src[null_in_entry] = None
    if null_out_entry is not None:
        dst[null_out_entry] = None
    ws = (C.c_uint32 * max(n, 1))(*(widths if widths is not None else [im.shape[1] for im in imgs]))
    hs = (C.c_uint32 * max(n, 1))(*(heights if heights is not None else [im.shape[0] for im in imgs]))
    rep = kg.BatchReport()
    a = {"rgba": src, "widths": ws, "heights": hs, "out": dst, "counts": C.c_void_p(counts.ctypes.data)}
    for name in null:
        a[name] = None
    count = n if n_images is None else n_images
    if mode is None:
        rc = L.kmg_palette_batch(proc.handle, count, a["rgba"], a["widths"], a["heights"], k, algo, bound, a["out"], a["counts"], C.byref(rep))
    else:
        rc = L.kmg_reduce_batch(proc.handle, count, a["rgba"], a["widths"], a["heights"], k, algo, mode, bound, a["out"], C.byref(rep))
    return rc, outs, counts, L.kmg_last_error().decode()


def _untouched(outs, counts):
    return all(np.all(o == SENTINEL) for o in outs) and np.all(counts == 0xA5A5A5A5)


# ---- 6. alpha mode -------------------------------------------------------------------------------------------------------------
def test_alpha_mode(torch_cuda):
    import kmeans_gpu_amd as kg
    full = _noise(21, 30, 40)
    half = _noise(22, 30, 40)
    half[:, :20, 3] = 0
    one = _noise(23, 30, 40)
    one[..., 3] = 100
    one[17, 23, 3] = 128
    none = _noise(24, 30, 40)
    none[..., 3] = 127
    images = [full, half, one]
    with kg.ImageProcessor(alpha_cutoff=128) as proc:
        got = proc.palette_batch(8, images)
        assert proc.last_batch_report.launches > 0
        for i, im in enumerate(images):
            assert np.array_equal(got[i], proc.palette(8, im)), i
        for mode in (kg.ReduceMode.Replace, kg.ReduceMode.Dither):
            got = proc.reduce_batch(8, images, reduce_mode=mode)
            for i, im in enumerate(images):
                assert np.array_equal(got[i], proc.reduce(8, im, reduce_mode=mode)), (i, mode)
        for mode in (None, int(kg.ReduceMode.Replace)):
            for bound in (0, 1):                                     # (one sub-batch; one image per sub-batch)
                rc, outs, counts, msg = _raw(proc, images + [none], 8, mode=mode, bound=bound)
                assert rc == INVALID and "image 3" in msg and "alpha_cutoff" in msg, (rc, msg)
                assert _untouched(outs, counts)
        rc, outs, counts, msg = _raw(proc, [full, none, half], 8, algo=int(kg.Algorithm.Octree), mode=int(kg.ReduceMode.Replace), bound=1)
        assert rc == INVALID and "image 1" in msg and _untouched(outs, counts), (rc, msg)


# ---- 7. fallback and mixing ------------------------------------------------------------------------------------------------------
def test_fallback_mixes_with_the_batched_images(torch_cuda, edge_images):
    import kmeans_gpu_amd as kg
    images = [edge_images[6], _noise(31, 600, 1024), edge_images[7], edge_images[5]]
    with kg.ImageProcessor(shrink_max_dim=0) as proc:
        got = proc.palette_batch(8, images)
        rep = proc.last_batch_report
        assert rep.fallback == 1 and rep.launches > 0 and rep.sub_batches == 1
        for i, im in enumerate(images):
            assert np.array_equal(got[i], proc.palette(8, im)), i


# ---- 8. kmg_reduce_batch -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five_images(tokyo):
    return [_noise(41, 64, 64), np.ascontiguousarray(tokyo[50:150, 100:300]), np.ascontiguousarray(tokyo[0:384, 0:512]),
            _noise(42, 257, 129), np.ascontiguousarray(tokyo[200:400, 300:600])]


def _resident(im):
    """include/kmeans_hip.h at max_resident_bytes, for kmg_reduce_batch with the default options: the source, and the shrunk copy"""
    import kmeans_gpu_amd as kg
    h, w = im.shape[:2]
    if w <= 256 and h <= 256:
        return 4 * w * h
    sw, sh = kg.resized_dims(w, h)
    return 4 * w * h + 4 * sw * sh


@pytest.mark.parametrize("k", [8, 64])
@pytest.mark.parametrize("mode", ["Replace", "Dither", "Diffuse"])
def test_reduce_batch_equals_reduce(processor, five_images, mode, k):
    import kmeans_gpu_amd as kg
    mode = kg.ReduceMode[mode]
    got = processor.reduce_batch(k, five_images, reduce_mode=mode)
    rep = processor.last_batch_report
    assert rep.sub_batches == 1 and rep.fallback == 0 and rep.launches > 0
    for i, im in enumerate(five_images):
        assert np.array_equal(got[i], processor.reduce(k, im, reduce_mode=mode)), i


def test_reduce_batch_in_three_sub_batches_and_octree(processor, five_images):
    import kmeans_gpu_amd as kg
    bound = 700_000
    sizes = [_resident(im) for im in five_images]
    cuts, held = 1, 0
    for i, b in enumerate(sizes):
        if held and held + b > bound:
            cuts, held = cuts + 1, 0
        held += b
    assert cuts == 3 and max(sizes) > bound, (sizes, cuts)             # three sub-batches, one image beyond the bound alone
    for k, mode in ((8, kg.ReduceMode.Dither), (64, kg.ReduceMode.Replace)):
        whole = processor.reduce_batch(k, five_images, reduce_mode=mode)
        cut = processor.reduce_batch(k, five_images, reduce_mode=mode, max_resident_bytes=bound)
        assert processor.last_batch_report.sub_batches == 3
        for i in range(5):
            assert np.array_equal(whole[i], cut[i]), (k, i)
    pals = processor.palette_batch(8, five_images, max_resident_bytes=bound)
    for i, im in enumerate(five_images):
        assert np.array_equal(pals[i], processor.palette(8, im)), i
    got = processor.reduce_batch(8, five_images, algo=kg.Algorithm.Octree, reduce_mode=kg.ReduceMode.Dither)
    assert processor.last_batch_report.launches == 0
    pals = processor.palette_batch(8, five_images, algo=kg.Algorithm.Octree)
    for i, im in enumerate(five_images):
        assert np.array_equal(got[i], processor.reduce(8, im, algo=kg.Algorithm.Octree, reduce_mode=kg.ReduceMode.Dither)), i
        assert np.array_equal(pals[i], processor.palette(8, im, algo=kg.Algorithm.Octree)), i


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_one_at_a_time_and_in_pairs(torch_cuda, edge_images):
    import kmeans_gpu_amd as kg
    images = [edge_images[6], edge_images[5], edge_images[3]]
    w = [im.shape[1] for im in images]
    h = [im.shape[0] for im in images]
    red = int(kg.ReduceMode.Replace)
    with kg.ImageProcessor() as proc:
        def refused(want_rc, needle, k=8, **kw):
            for mode in (None, red):                                 # kmg_palette_batch, kmg_reduce_batch
                rc, outs, counts, msg = _raw(proc, images, k, mode=mode, **kw)
                assert rc == want_rc and msg and needle in msg, (kw, mode, rc, msg)
                assert _untouched(outs, counts), (kw, mode)

        # one at a time
        refused(INVALID, "empty", n_images=0)
        for name in ("rgba", "widths", "heights", "out"):
            refused(INVALID, "array is NULL", null=(name,))
        rc, outs, counts, msg = _raw(proc, images, 8, null=("counts",))
        assert rc == INVALID and "array is NULL" in msg and all(np.all(o == SENTINEL) for o in outs)
        refused(INVALID, "image 1: image pointer is NULL", null_in_entry=1)
        refused(INVALID, "image 2: output pointer is NULL", null_out_entry=2)
        refused(INVALID, "image 1 has zero width or height", widths=[w[0], 0, w[2]])
        refused(INVALID, "image 0 has zero width or height", heights=[0, h[1], h[2]])
        refused(INVALID, "higher than 0", k=0)
        refused(INVALID, "unknown algorithm", algo=2)
        rc, outs, counts, msg = _raw(proc, images, 8, mode=4)
        assert rc == INVALID and "unknown mode" in msg and _untouched(outs, counts)
        rc, outs, counts, msg = _raw(proc, images, 8, mode=-1)
        assert rc == INVALID and "unknown mode" in msg and _untouched(outs, counts)
        refused(UNSUPPORTED, "KMG_MAX_K", k=3073)
        proc.set_fixed_colors([[255, 0, 0]])
        refused(INVALID, "fixed colours")
        # pairs: which refusal wins (the order of include/kmeans_hip.h)
        refused(INVALID, "unknown algorithm", algo=7)                               # algorithm before fixed colours
        refused(UNSUPPORTED, "KMG_MAX_K", k=3073)                                   # the colour limit before fixed colours
        proc.set_alpha_weight(True)
        refused(INVALID, "fixed colours")                                           # fixed colours before weighting
        proc.set_fixed_colors(None)
        refused(INVALID, "alpha weighting")
        refused(INVALID, "higher than 0", k=0)                                      # the colour count before weighting
        proc.set_alpha_weight(False)
        refused(INVALID, "empty", n_images=0, null=("rgba",))                       # the empty batch before a NULL array
        refused(INVALID, "array is NULL", null=("heights",), null_in_entry=0)       # a NULL array before a NULL entry
        refused(INVALID, "image 0 has zero width", widths=[0, w[1], w[2]], null_in_entry=1)   # image 0 before image 1
        refused(INVALID, "image 1: image pointer", widths=[w[0], w[1], 0], null_in_entry=1)
        refused(INVALID, "image 1: image pointer", null_in_entry=1, k=0)            # the images before the colour count
        refused(INVALID, "higher than 0", k=0, algo=5)                              # the colour count before the algorithm
        # fixed colours and weighting cleared: the call works again
        got = proc.palette_batch(8, images)
        for i, im in enumerate(images):
            assert np.array_equal(got[i], proc.palette(8, im)), i


# ---- 10. a warm processor ------------------------------------------------------------------------------------------------------
def test_warm_processor_reuses_its_blocks(torch_cuda, edge_images, five_images):
    import kmeans_gpu_amd as kg
    with kg.ImageProcessor() as proc:
        first = proc.palette_batch(33, edge_images)
        between = proc.reduce(8, five_images[1], reduce_mode=kg.ReduceMode.Dither)
        second = proc.palette_batch(33, edge_images)
        mallocs_2 = proc.debug_block_counts()[0]
        third = proc.palette_batch(33, edge_images)
        assert proc.debug_block_counts()[0] == mallocs_2               # no hipMalloc for the third batch
        for a, b, c in zip(first, second, third):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        assert np.array_equal(between, proc.reduce(8, five_images[1], reduce_mode=kg.ReduceMode.Dither))
        red_1 = proc.reduce_batch(8, five_images[:3])
        mallocs_r = proc.debug_block_counts()[0]
        red_2 = proc.reduce_batch(8, five_images[:3])
        assert proc.debug_block_counts()[0] == mallocs_r
        for a, b in zip(red_1, red_2):
            assert np.array_equal(a, b)
