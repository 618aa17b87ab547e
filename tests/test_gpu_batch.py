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


# ---- 11. a warm processor whose blocks hold other batches' words ---------------------------------------------------------
def test_warm_processor_runs_each_batch_in_another_batchs_blocks(torch_cuda, edge_images, five_images):
    """nine images at k = 300, then two others at k = 3, then those two reversed plus one at k = 33, on one processor: n, k and the
    sizes shrink and change, so every word a recycled block still holds (stop, slots, dist, centroids, records, gather buffer,
    tables) differs from the one the next batch needs.  Every result against the per-image calls of a FRESH processor; a second
    round of the three batches allocates nothing"""
    import kmeans_gpu_amd as kg
    a = list(edge_images) + [five_images[0]]
    b = [five_images[1], five_images[3]]
    c = [b[1], b[0], five_images[4]]
    batches = [(a, 300), (b, 3), (c, 33)]
    assert len(a) == 9
    dither = kg.ReduceMode.Dither
    with kg.ImageProcessor() as fresh:
        want = []
        for images, k in batches:
            pals = [fresh.palette(k, im) for im in images]
            reds = [fresh.reduce_indexed(k, im, reduce_mode=dither) for im in images]
            finds = [fresh.find_indexed(im, reds[0][0], reduce_mode=dither) for im in images]
            want.append((pals, reds, finds))
    with kg.ImageProcessor() as proc:
        def one_round(tag):
            for (images, k), (pals, reds, finds) in zip(batches, want):
                got = proc.palette_batch(k, images)
                assert proc.last_batch_report.launches > 0 and proc.last_batch_report.fallback == 0
                for i in range(len(images)):
                    assert got[i].shape == pals[i].shape and np.array_equal(got[i], pals[i]), (tag, k, i, "palette_batch")
                got = proc.reduce_indexed_batch(k, images, reduce_mode=dither)
                for i in range(len(images)):
                    assert got[i][1].dtype == (np.uint8 if k <= 256 else np.uint16) == reds[i][1].dtype
                    assert np.array_equal(got[i][0], reds[i][0]), (tag, k, i, "palette of reduce_indexed_batch")
                    assert np.array_equal(got[i][1], reds[i][1]), (tag, k, i, "map of reduce_indexed_batch")
                got = proc.find_batch(images, reds[0][0], reduce_mode=dither)
                for i in range(len(images)):
                    assert got[i].dtype == finds[i].dtype and np.array_equal(got[i], finds[i]), (tag, k, i, "find_batch")
        one_round("first")
        mallocs = proc.debug_block_counts()[0]
        one_round("second")
        assert proc.debug_block_counts()[0] == mallocs                 # no hipMalloc in the second round


# ---- 12. more tiles than one chain of launches takes -------------------------------------------------------------------
BATCH_MAX_TILES = 1 << 20          # include/kmeans_hip.h at kmg_dev_palette_batch: "up to 2^20 tiles of 256 pixels in all"


def _chains(pixel_counts):
    """the pieces the documented limit cuts a device batch into: consecutive entries whose tiles of 256 pixels sum to 2^20 at most"""
    pieces, held = [[]], 0
    for i, n in enumerate(pixel_counts):
        tiles = (n + 255) // 256
        if pieces[-1] and held + tiles > BATCH_MAX_TILES:
            pieces.append([])
            held = 0
        pieces[-1].append(i)
        held += tiles
    return pieces


def test_more_tiles_than_one_chain_takes(torch_cuda):
    """4 100 device views of ONE resident 256 x 256 image (256 tiles each: 2^20 tiles after 4 096 views), k = 2: the batch runs as two
    chains, and the second chain's results go back through its own index list.  The last entry of the first chain, the first of
    the second and the last of the batch are three OTHER images (two colours each: they stop at the first check, the noise runs to
    the cap), so a result stored at an index counted from 0, or one piece's results in the other's place, shows.
    Batched state by the header's figure (12 bytes per working pixel + 128 k per view): 4 096 x (12 x 65 536 + 256) = 3 222 274 048
    bytes = 3.0 GiB for the first chain, 3 146 752 bytes for the second; under 4 GiB."""
    import kmeans_gpu_amd as kg
    k, side, n_views = 2, 256, 4100
    state_bytes = 4096 * (12 * side * side + 128 * k)
    assert state_bytes == 3222274048 and state_bytes < 4 << 30
    base = _noise(51, side, side)

    def two_colours(seed, lo, hi):
        m = np.random.default_rng(seed).random((side, side, 1)) < 0.4
        return _rgba(np.where(m, np.uint8(lo), np.uint8(hi)) * np.ones((side, side, 3), np.uint8))
    odd = [two_colours(52, 30, 220), two_colours(53, 90, 160), two_colours(54, 5, 120)]
    pieces = _chains([side * side] * n_views)
    assert [len(p) for p in pieces] == [4096, 4] and sum(256 * len(p) for p in pieces) > BATCH_MAX_TILES
    where = {pieces[0][-1]: 0, pieces[1][0]: 1, pieces[1][-1]: 2}       # entry -> which odd image
    assert sorted(where) == [4095, 4096, 4099]
    with kg.ImageProcessor(max_iterations=3, check_period=1) as proc:
        d_base, d_odd = _on_device(torch_cuda, [base])[0], _on_device(torch_cuda, odd)
        want_base = _per_image(torch_cuda, proc, d_base, base, k)
        want_odd = [_per_image(torch_cuda, proc, d, im, k) for d, im in zip(d_odd, odd)]
        assert len({want_base[1]} | {it for _, it in want_odd}) > 1, (want_base[1], [it for _, it in want_odd])
        d_imgs = [d_odd[where[i]] if i in where else d_base for i in range(n_views)]
        images = [odd[where[i]] if i in where else base for i in range(n_views)]
        want = [want_odd[where[i]] if i in where else want_base for i in range(n_views)]
        cent, its, rep = _device_batch(torch_cuda, proc, d_imgs, images, k)
        assert rep.fallback == 0
        # two chains, each k launches of the initialisation, the initial assignment and one launch per iteration up to its slowest
        assert rep.launches == sum(k + 2 + max(want[i][1] for i in p) for p in pieces), (rep, [max(want[i][1] for i in p) for p in pieces])
        assert rep.iterations == max(it for _, it in want)
        for i in sorted(where) + [0, 1, 2048, 4097, 4098]:             # the three odd entries; 0, 1 and one in the middle of each piece
            assert int(its[i]) == want[i][1], (i, int(its[i]), want[i][1])
            assert _same_bits(cent[i], want[i][0]), i


# ---- 13. the loop's options at their edges --------------------------------------------------------------------------------
EVERYTHING_CONVERGES = 1.0e6       # far above every CIE94 distance: every centroid with a pixel counts as converged at once
OPTION_EDGES = [(1, 1, None), (1, 8, None), (2, 1, None), (5, 1, None), (20, 4, EVERYTHING_CONVERGES), (9, 2, 0.0)]
_oracle_counts = {}


def _oracle_lloyd(oracle, im, k, max_iterations, check_period, convergence):
    h, w = im.shape[:2]
    lab = oracle.rgb_to_lab(im)
    cent, _, it = oracle.lloyd(lab, oracle.init_centroids(lab, w, h, k), max_iterations=max_iterations, check_period=check_period,
                               convergence=1.0 if convergence is None else convergence)
    return cent, it


def _oracle_count_table(oracle, images, max_iterations, check_period, convergence):
    """{k: iteration counts of the images} by the oracle, for the three k of the test; computed once per row of OPTION_EDGES"""
    key = (max_iterations, check_period, convergence)
    if key not in _oracle_counts:
        _oracle_counts[key] = {k: [_oracle_lloyd(oracle, im, k, *key)[1] for im in images] for k in (1, 8, 33)}
    return _oracle_counts[key]


@pytest.fixture(scope="module")
def edge_and_early_images(edge_images):
    """edge_images, which all run to the cap under (max_iterations 5, check_period 1) at k = 8 and 33, and three images that stop
    earlier there (the test asserts it with the oracle): forty colours with a little noise, twice, and three grey levels with noise"""
    def forty(seed):
        r = np.random.default_rng(seed)
        pal = r.integers(0, 256, (40, 3), dtype=np.uint8)
        return _rgba(np.clip(pal[r.integers(0, 40, (30, 30))].astype(int) + r.integers(-2, 3, (30, 30, 3)), 0, 255).astype(np.uint8))
    r = np.random.default_rng(5)
    levels = _rgba((r.integers(0, 3, (32, 32, 1)) * 83 + r.integers(0, 20, (32, 32, 3))).astype(np.uint8))
    return list(edge_images) + [forty(0), levels, forty(5)]


@pytest.mark.parametrize("k", [1, 8, 33])
@pytest.mark.parametrize("max_iterations,check_period,convergence", OPTION_EDGES)
def test_options_at_their_edges(torch_cuda, oracle, edge_and_early_images, max_iterations, check_period, convergence, k):
    """max_iterations = 1 never reaches a check (its = max_iterations - 1 through stop = max_iterations + 1); check_period = 1 checks
    after every iteration but the first; a threshold above every distance stops an image at the first check (iteration 4), unless
    it has fewer colours than k -- an empty cluster never counts as converged, so that image runs to the cap; threshold 0.0: no
    centroid ever counts, every image runs to the cap.  Not vacuous, by the oracle, for every batch: the counts of ITS images take
    at least two values -- (5, 1): 1, 2 and 4 at k = 8 and at k = 33; the large threshold: 4 and 19 -- unless the options
    force one: max_iterations 1 and 2, threshold 0.0, and k = 1 in every row (one centroid with a pixel has converged at the
    first check, whatever the image)."""
    import kmeans_gpu_amd as kg
    edge_images = edge_and_early_images
    table = _oracle_count_table(oracle, edge_images, max_iterations, check_period, convergence)
    spread = sorted(set(table[k]))
    forced = {(1, 1): [0], (1, 8): [0], (2, 1): [1], (9, 2): [8]}.get((max_iterations, check_period))
    if forced is None and k == 1:
        forced = [1 if check_period == 1 else check_period]
    if forced is not None:
        assert spread == forced, spread
    else:
        assert len(spread) >= 2, spread
        if (max_iterations, check_period) == (5, 1):
            assert min(spread) < 3 and max(spread) == 4, spread          # (an early stop, a later one and the cap in one batch)
    if convergence == EVERYTHING_CONVERGES:
        for im, it in zip(edge_images, table[k]):
            colours = len(np.unique(im.reshape(-1, 4), axis=0))
            assert it == (4 if colours >= k else max_iterations - 1), (k, im.shape, it, colours)
    opts = {} if convergence is None else {"convergence": convergence}
    with kg.ImageProcessor(max_iterations=max_iterations, check_period=check_period, **opts) as proc:
        d_imgs = _on_device(torch_cuda, edge_images)
        cent, its, rep = _device_batch(torch_cuda, proc, d_imgs, edge_images, k)
        assert rep.fallback == 0 and rep.sub_batches == 1
        for i, (d, im) in enumerate(zip(d_imgs, edge_images)):
            want_c, want_it = _per_image(torch_cuda, proc, d, im, k)
            assert int(its[i]) == want_it, (i, im.shape, int(its[i]), want_it)
            assert _same_bits(cent[i], want_c), (i, im.shape)
        assert rep.iterations == int(its.max())
        assert rep.launches == k + 2 + int(its.max())
        if k == 8:
            for i in (5, 6, 7):                                          # 73 x 7 (three colours), 27 x 19, 256 x 171
                want_c, want_it = _oracle_lloyd(oracle, edge_images[i], k, max_iterations, check_period, convergence)
                assert int(its[i]) == want_it == table[8][i], (i, int(its[i]), want_it)
                assert _same_bits(cent[i][:, :3], want_c[:, :3]), i


# ---- 14. a sub-batch of one image -----------------------------------------------------------------------------------------
def test_a_sub_batch_of_one_image_reports_its_iterations(torch_cuda, processor, edge_images):
    """include/kmeans_hip.h: a sub-batch of ONE image takes the per-image palette step -- no batched launch -- and `iterations`
    covers it all the same (it was 0 for such a sub-batch: the per-image step dropped the count)"""
    images = [edge_images[7], edge_images[5], edge_images[6]]        # 256 x 171, 73 x 7 (runs to the cap), 27 x 19: none is shrunk
    k = 8
    want = [_per_image(torch_cuda, processor, d, im, k)[1] for d, im in zip(_on_device(torch_cuda, images), images)]
    assert max(want) not in (want[0], want[-1]), want                 # (neither the first nor the last image's count is the answer)
    for i, im in enumerate(images):
        got = processor.palette_batch(k, [im])
        assert np.array_equal(got[0], processor.palette(k, im))
        assert processor.last_batch_report.as_tuple() == (0, want[i], 1, 0), (i, processor.last_batch_report)
    got = processor.palette_batch(k, images, max_resident_bytes=1)
    assert processor.last_batch_report.as_tuple() == (0, max(want), 3, 0), processor.last_batch_report
    whole = processor.palette_batch(k, images)
    assert processor.last_batch_report.as_tuple() == (k + 2 + max(want), max(want), 1, 0), processor.last_batch_report
    for a, b in zip(got, whole):
        assert np.array_equal(a, b)
