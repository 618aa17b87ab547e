"""Batched quality targets (include/kmeans_hip.h at kmg_batch_quality_report): the batched kernels with a colour
count per image -- kmg_dev_palette_batch_counts, kmg_dev_apply_batch_counts, kmg_dev_compare_batch -- and kmg_reduce_quality_batch on
top of them.

The yardstick is always the per-image call of the library -- the kmg_lloyd_* calls, kmg_dev_apply_format, kmg_dev_compare,
kmg_reduce_quality --, never the batch code itself.  Everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
SENTINEL = 0xA5
GUARD = 64
RGBA8, INDEX8, INDEX16 = 0, 1, 2
REPLACE, DITHER, MELD, DIFFUSE = 0, 1, 2, 3
BPP = {RGBA8: 4, INDEX8: 1, INDEX16: 2}
RGB, LAB = 1, 2
PASS_TILE = 1024                                                     # kPassTile (kmg_pass.h): the pixels of one workgroup of a record pass
MAX_FIELDS = (9, 10, 11, 13)                                         # kmg_error_stats: max_abs[3] and lab_max are maxima, the rest sums


def _rgba(rgb):
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = rgb
    return out


def _noise(seed, h, w):
    return _rgba(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def _palette(seed, k):
    pal = np.random.default_rng(1000 + seed).integers(0, 256, (k, 4), dtype=np.uint8)
    pal[:, 3] = 255
    return pal


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _on_device(torch, images):
    """(as bytes: index maps of uint16 travel like the others)"""
    return [torch.from_numpy(np.ascontiguousarray(im).reshape(-1).view(np.uint8)).cuda() for im in images]


def _dims(images):
    return [im.shape[1] for im in images], [im.shape[0] for im in images]


# the shapes of the device tests: one pixel, a partial tile of the 256-pixel palette pass, two tiles, several, 64 tiles, and one
# pixel again for a count above the pixel count; the counts: the k = 1 pick, both sides of the scan's switch at 32
SHAPES = [(1, 1), (15, 16), (16, 17), (48, 64), (256, 256), (1, 1)]
KS = [1, 2, 31, 32, 33, 5]


@pytest.fixture(scope="module")
def shape_images():
    return [_noise(40 + i, h, w) for i, (h, w) in enumerate(SHAPES)]


# ---- 1. the palette chain with a count per image --------------------------------------------------------------------------------
def _lloyd_alone(torch, proc, d_img, im, k):
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


def _chain(torch, proc, d_imgs, images, ks):
    stream = torch.cuda.current_stream().cuda_stream
    ws, hs = _dims(images)
    tables, its = proc.palette_batch_counts_device([d.data_ptr() for d in d_imgs], ws, hs, ks, stream)
    return tables, its, proc.last_batch_report


@pytest.mark.parametrize("ks", [KS, KS[::-1], [33, 33, 1, 2, 40, 31]], ids=["as listed", "reversed", "mixed"])
def test_palette_chain_with_a_count_per_image(torch_cuda, processor, shape_images, ks):
    d_imgs = _on_device(torch_cuda, shape_images)
    tables, its, rep = _chain(torch_cuda, processor, d_imgs, shape_images, ks)
    assert [t.shape for t in tables] == [(k, 4) for k in ks]
    for i, (d, im) in enumerate(zip(d_imgs, shape_images)):
        want_c, want_it = _lloyd_alone(torch_cuda, processor, d, im, ks[i])
        assert int(its[i]) == want_it, (i, im.shape, ks[i], int(its[i]), want_it)
        assert _same_bits(tables[i], want_c), (i, im.shape, ks[i])
    assert (rep.fallback, rep.sub_batches, rep.iterations) == (0, 1, int(its.max()))
    assert rep.launches == max(ks) + 2 + int(its.max()), (rep, its)


@pytest.mark.parametrize("k", [1, 5, 32, 33])
def test_equal_counts_are_the_palette_batch(torch_cuda, processor, shape_images, k):
    stream = torch_cuda.cuda.current_stream().cuda_stream
    d_imgs = _on_device(torch_cuda, shape_images)
    ws, hs = _dims(shape_images)
    cent, its_one = processor.palette_batch_device([d.data_ptr() for d in d_imgs], ws, hs, k, stream)
    one = processor.last_batch_report.as_tuple()
    tables, its, rep = _chain(torch_cuda, processor, d_imgs, shape_images, [k] * len(shape_images))
    assert rep.as_tuple() == one and np.array_equal(its, its_one)
    assert all(_same_bits(t, c) for t, c in zip(tables, cent))


def test_a_stopped_image_keeps_its_table_while_others_run(torch_cuda):
    """check_period = 2: a flat image at k = 1 and a two-colour image at k = 2 stop at the first check (every cluster has pixels and
    does not move), the noise runs on; later launches leave the stopped tables alone"""
    import kmeans_gpu_amd as kg
    flat = _rgba(np.full((20, 30, 3), (200, 30, 90), np.uint8))
    two = _rgba(np.array([[10, 20, 30], [240, 200, 90]], np.uint8)[np.random.default_rng(8).integers(0, 2, (20, 30))])
    images = [flat, _noise(3, 48, 64), two, _noise(4, 16, 17)]
    ks = [1, 40, 2, 8]
    with kg.ImageProcessor(check_period=2, max_iterations=20) as proc:
        d_imgs = _on_device(torch_cuda, images)
        tables, its, rep = _chain(torch_cuda, proc, d_imgs, images, ks)
        want = [_lloyd_alone(torch_cuda, proc, d, im, k) for d, im, k in zip(d_imgs, images, ks)]
        assert [int(v) for v in its] == [it for _, it in want]
        assert int(its[0]) < int(its[1]) and int(its[2]) < int(its[1]), its    # (they stopped while the noise ran)
        assert all(_same_bits(t, c) for t, (c, _) in zip(tables, want))
        assert rep.launches == max(ks) + 2 + int(its.max())


# ---- 2. the output pass with a table per image of its own size --------------------------------------------------------------------
def _device_outputs(torch, images, fmt):
    """guarded device outputs: (tensors, addresses of the bodies)"""
    outs = [torch.full((im.shape[0] * im.shape[1] * BPP[fmt] + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for im in images]
    return outs, [o.data_ptr() + GUARD for o in outs]


def _device_body(out, im, fmt):
    raw = out.cpu().numpy()
    assert np.all(raw[:GUARD] == SENTINEL) and np.all(raw[-GUARD:] == SENTINEL)
    body = raw[GUARD:-GUARD]
    return body.reshape(im.shape) if fmt == RGBA8 else body.view(np.uint16 if fmt == INDEX16 else np.uint8).reshape(im.shape[:2])


@pytest.fixture(scope="module")
def output_images(shape_images):
    """the shapes above with alpha bytes on both sides of 128, and a 2000 x 2000 image for k = 600: its own plan takes the mask
    words (dither, from 4 000 000 pixels on above k = 512) or the colour table (replace), so it keeps its per-image pass"""
    images = [im.copy() for im in shape_images] + [_noise(50, 2000, 2000)]
    for i, im in enumerate(images):
        im[..., 3] = np.random.default_rng(60 + i).integers(0, 256, im.shape[:2], dtype=np.uint8)
    images[5][..., 3] = 255
    return images


@pytest.mark.parametrize("cutoff", [0, 128])
@pytest.mark.parametrize("fmt", [RGBA8, INDEX8, INDEX16])
@pytest.mark.parametrize("mode", [REPLACE, DITHER])
def test_output_with_a_table_per_image(torch_cuda, output_images, mode, fmt, cutoff):
    import kmeans_gpu_amd as kg
    stream = torch_cuda.cuda.current_stream().cuda_stream
    images = output_images if fmt != INDEX8 else output_images[:-1]       # (INDEX8 holds no 600 colours)
    ks = (KS + [600])[:len(images)]
    tables = [kg.palette_to_centroids(_palette(7 * k + i, k)) for i, k in enumerate(ks)]
    ws, hs = _dims(images)
    with kg.ImageProcessor(alpha_cutoff=cutoff) as proc:
        d_imgs = _on_device(torch_cuda, images)
        outs, ptrs = _device_outputs(torch_cuda, images, fmt)
        rep = proc.apply_batch_counts_device([d.data_ptr() for d in d_imgs], ws, hs, tables, mode, fmt, ptrs, stream)
        assert rep.batched + rep.per_image == len(images) and rep.sub_batches == 1, rep
        assert 1 <= rep.launches <= 2, rep                                 # the joined set: k < 32 and k >= 32
        if len(images) == 7:
            assert (rep.batched, rep.per_image, rep.launches) == (6, 1, 2), rep
        if len(images) == 6:
            assert (rep.batched, rep.per_image, rep.launches) == (6, 0, 2), rep
        for i, im in enumerate(images):
            want, wptr = _device_outputs(torch_cuda, [im], fmt)
            proc.apply(d_imgs[i].data_ptr(), ws[i], hs[i], 0, tables[i], mode, wptr[0], stream, format=kg.OutputFormat(fmt))
            torch_cuda.cuda.synchronize()
            assert np.array_equal(_device_body(outs[i], im, fmt), _device_body(want[0], im, fmt)), (i, im.shape, ks[i])
        # counts on one side of 32 only: one launch
        few = [0, 1, 5]
        outs, ptrs = _device_outputs(torch_cuda, [images[i] for i in few], fmt)
        rep = proc.apply_batch_counts_device([d_imgs[i].data_ptr() for i in few], [ws[i] for i in few], [hs[i] for i in few],
                                             [tables[i] for i in few], mode, fmt, ptrs, stream)
        assert (rep.launches, rep.batched, rep.per_image) == (1, 3, 0), rep


# ---- 3. the batched error record ---------------------------------------------------------------------------------------------------
def _records(torch, n):
    return torch.zeros((n, 14), dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("what", [RGB, LAB, RGB | LAB])
@pytest.mark.parametrize("fmt", [RGBA8, INDEX8, INDEX16])
def test_batched_records_equal_the_per_image_records(torch_cuda, processor, fmt, what):
    """images of 1, kPassTile - 1, kPassTile + 1 and 5000 pixels (the last: five workgroups that combine into one record), a count
    per image, alpha bytes around the cutoff, and one map with indices >= its k"""
    import kmeans_gpu_amd as kg
    stream = torch_cuda.cuda.current_stream().cuda_stream
    pixels = [1, PASS_TILE - 1, PASS_TILE + 1, 5000]
    ks = [1, 31, 200, 33]
    cutoff = 100
    rng = np.random.default_rng(5)
    srcs = [rng.integers(0, 256, (n, 4), dtype=np.uint8) for n in pixels]
    pals = [_palette(300 + i, k) for i, k in enumerate(ks)]
    if fmt == RGBA8:
        outs = [np.where(rng.random((n, 1)) < 0.3, s, rng.integers(0, 256, (n, 4), dtype=np.uint8)).astype(np.uint8) for n, s in zip(pixels, srcs)]
    else:
        outs = [rng.integers(0, k, n).astype(np.uint8 if fmt == INDEX8 else np.uint16) for n, k in zip(pixels, ks)]
        outs[1][::7] = ks[1] + 3                                           # invalid indices: counted apart, they add nothing else
    d_src, d_out = _on_device(torch_cuda, srcs), _on_device(torch_cuda, outs)
    rec = _records(torch_cuda, len(pixels))
    palettes = None if fmt == RGBA8 else pals

    def batch():
        processor.compare_batch_device([d.data_ptr() for d in d_src], [d.data_ptr() for d in d_out], pixels, fmt, palettes, cutoff, what,
                                       rec.data_ptr(), stream)
        torch_cuda.cuda.synchronize()
        return rec.cpu().numpy().view(np.uint64)

    got = batch()
    want = np.zeros((len(pixels), 14), np.uint64)
    for i, n in enumerate(pixels):
        one = _records(torch_cuda, 1)
        processor.compare_device(d_src[i].data_ptr(), d_out[i].data_ptr(), n, one.data_ptr(), format=kg.OutputFormat(fmt),
                                 palette=None if fmt == RGBA8 else pals[i], alpha_cutoff=cutoff, what=what, stream=stream)
        torch_cuda.cuda.synchronize()
        want[i] = one.cpu().numpy().view(np.uint64)[0]
    assert np.array_equal(got, want), (got, want)
    assert all(want[i, 0] + want[i, 2] == int((srcs[i][:, 3] >= cutoff).sum()) for i in range(len(pixels)))
    if fmt != RGBA8:
        assert want[1, 2] > 0 and want[0, 2] == want[2, 2] == want[3, 2] == 0
    # a second call COMBINES: the sums double, the maxima stay
    twice = batch()
    for f in range(14):
        assert np.array_equal(twice[:, f], want[:, f] if f in MAX_FIELDS else 2 * want[:, f]), f


# ---- 4. kmg_reduce_quality_batch = kmg_reduce_quality per image -------------------------------------------------------------------
K_MIN, K_MAX = 2, 40
# dE 3.0 in units of 1/4096 dE^2.  Chosen with the CPU reference (tests/error_ref.py Working.search over quality_images()), for both
# cutoffs: k* = 2 (flat), 24 (the ramp, twice), 33 (36 colours), and the other images do not reach it at 40.
TARGET = 36864


class Guarded:
    """a host buffer of n bytes between two runs of guard bytes"""

    def __init__(self, n):
        self.n = n
        self.raw = np.full(n + 2 * GUARD, SENTINEL, np.uint8)
        self.ptr = self.raw.ctypes.data + GUARD

    def guards_ok(self):
        return bool(np.all(self.raw[:GUARD] == SENTINEL) and np.all(self.raw[GUARD + self.n:] == SENTINEL))

    def untouched(self):
        return bool(np.all(self.raw == SENTINEL))

    def body(self):
        return self.raw[GUARD:GUARD + self.n]


def quality_images():
    """a flat colour, two gradients, noise, a 300 x 200 image that is shrunk, 36 colours in random tiles, and the ramp and the noise
    a second time; four of them partly transparent (alpha mode compacts those)"""
    flat = _rgba(np.full((20, 30, 3), (40, 120, 200), np.uint8))
    x = np.arange(64, dtype=np.uint32)[None, :].repeat(48, 0)
    y = np.arange(48, dtype=np.uint32)[:, None].repeat(64, 1)
    ramp = _rgba(np.stack([x * 4, x * 2 + 60, 255 - x * 3], -1).astype(np.uint8))
    plane = _rgba(np.stack([x * 4, y * 5, (x + y) * 2], -1).astype(np.uint8))
    noise = _noise(7, 30, 40)
    xx = np.arange(300, dtype=np.uint32)[None, :].repeat(200, 0)
    yy = np.arange(200, dtype=np.uint32)[:, None].repeat(300, 1)
    big = _rgba(np.stack([(xx * 255) // 299, (yy * 255) // 199, ((xx // 30 + yy // 25) % 4) * 80], -1).astype(np.uint8))
    colours = np.random.default_rng(11).integers(0, 256, (36, 3), dtype=np.uint8)
    tiles = _rgba(colours[np.random.default_rng(12).integers(0, 36, (45, 37))])
    images = [flat, ramp, plane, noise, big, ramp.copy(), noise.copy(), tiles]
    images[2][:, :20, 3] = 0
    images[3][::3, :, 3] = 100
    images[4][150:, :, 3] = 127
    images[7][:, 30:, 3] = 60
    images[6][::3, :, 3] = 100
    return [np.ascontiguousarray(im) for im in images]


def quality_one(proc, im, k_min, k_max, target, mode, fmt):
    """kmg_reduce_quality of one image in an explicit format: (k*, palette bytes, output bytes, record, reached)"""
    import kmeans_gpu_amd as kg
    buf, pal = Guarded(im.shape[0] * im.shape[1] * BPP[fmt]), Guarded(4 * k_max)
    cnt, reached, stats = C.c_uint32(), C.c_int(), kg.ErrorStats()
    rc = kg.lib().kmg_reduce_quality(proc.handle, C.c_void_p(im.ctypes.data), im.shape[1], im.shape[0], k_min, k_max, target, mode, fmt,
                                     C.c_void_p(pal.ptr), C.byref(cnt), C.c_void_p(buf.ptr), C.byref(stats), C.byref(reached))
    assert rc == 0 and buf.guards_ok() and pal.guards_ok(), kg.lib().kmg_last_error().decode()
    return cnt.value, pal.body()[:4 * cnt.value].copy(), buf.body().copy(), stats.as_tuple(), reached.value


def raw_quality_batch(proc, images, k_min, k_max, target, mode, fmt, bound=0, n_images=None, null=(), widths=None, heights=None, null_in=None,
                      null_out=None, null_pal=None):
    """kmg_reduce_quality_batch into guarded buffers: (status, palettes, counts, outputs, records, reached, report, message)"""
    import kmeans_gpu_amd as kg
    L = kg.lib()
    n = max(len(images), 1)
    bufs = [Guarded(im.shape[0] * im.shape[1] * BPP.get(fmt, 4)) for im in images]
    pals = [Guarded(4 * max(min(k_max, 4096), 1)) for _ in images]
    counts = np.full(n, 0xA5A5A5A5, np.uint32)
    stats = (kg.ErrorStats * n)()
    reached = (C.c_int * n)(*([-7] * n))
    src = (C.c_void_p * n)(*[im.ctypes.data for im in images])
    if null_in is not None:
        src[null_in] = None

    def ptrs(gs, null_entry):
        a = (C.c_void_p * n)(*[g.ptr for g in gs])
        if null_entry is not None:
            a[null_entry] = None
        return a

    a = {"rgba": src, "widths": (C.c_uint32 * n)(*(widths if widths is not None else [im.shape[1] for im in images])),
         "heights": (C.c_uint32 * n)(*(heights if heights is not None else [im.shape[0] for im in images])),
         "out": ptrs(bufs, null_out), "palettes": ptrs(pals, null_pal), "counts": C.c_void_p(counts.ctypes.data)}
    for name in null:
        a[name] = None
    rep = kg.BatchQualityReport()
    rc = L.kmg_reduce_quality_batch(proc.handle, len(images) if n_images is None else n_images, a["rgba"], a["widths"], a["heights"], k_min, k_max,
                                    target, mode, fmt, bound, a["palettes"], a["counts"], a["out"], stats, reached, C.byref(rep))
    return rc, pals, counts, bufs, stats, reached, rep, L.kmg_last_error().decode()


def quality_batch(proc, images, k_min, k_max, target, mode, fmt, bound=0):
    """[(k*, palette bytes, output bytes, record, reached)], report"""
    rc, pals, counts, bufs, stats, reached, rep, msg = raw_quality_batch(proc, images, k_min, k_max, target, mode, fmt, bound)
    assert rc == 0, msg
    assert all(b.guards_ok() for b in bufs) and all(q.guards_ok() for q in pals)
    return [(int(counts[i]), pals[i].body()[:4 * int(counts[i])].copy(), bufs[i].body().copy(), stats[i].as_tuple(), reached[i])
            for i in range(len(images))], rep


def _same_results(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want))
            if not (g[0] == w[0] and np.array_equal(g[1], w[1]) and np.array_equal(g[2], w[2]) and g[3] == w[3] and g[4] == w[4])]


@pytest.mark.parametrize("mode,fmt,cutoff", [(REPLACE, INDEX8, 0), (DITHER, RGBA8, 0), (DITHER, INDEX8, 128), (REPLACE, RGBA8, 128)])
def test_quality_batch_equals_quality_per_image(torch_cuda, mode, fmt, cutoff):
    import kmeans_gpu_amd as kg
    images = quality_images()
    n = len(images)
    with kg.ImageProcessor(alpha_cutoff=cutoff) as proc:
        want = [quality_one(proc, im, K_MIN, K_MAX, TARGET, mode, fmt) for im in images]
        # the batch has something to get wrong: counts that differ, on both sides of the scan's switch, and a search that fails
        stars = [w[0] for w in want]
        assert len(set(stars)) >= 3, stars
        assert any(w[4] == 0 for w in want), stars
        assert any(k < 32 for k in stars) and any(k > 32 for k, w in zip(stars, want) if w[4]), stars
        got, rep = quality_batch(proc, images, K_MIN, K_MAX, TARGET, mode, fmt)
        assert _same_results(got, want) == []
        bound = 1 + int(np.ceil(np.log2(K_MAX - K_MIN + 1)))
        assert 1 < rep.rounds <= bound, rep
        assert (rep.batched + rep.per_image, rep.sub_batches, rep.fallback) == (n, 1, 0), rep
        assert rep.batched == n                                            # (replace and dither on small images: all join)
        assert n <= rep.palette_runs <= n * bound and rep.measure_launches == rep.rounds and rep.launches > 0, rep
        # the order of the batch and a cut change nothing
        back, _ = quality_batch(proc, images[::-1], K_MIN, K_MAX, TARGET, mode, fmt)
        assert _same_results(back[::-1], want) == []
        # max_resident_bytes cuts the 300 x 200 image off alone: its sub-batch of one takes the per-image search
        small = sum(im.shape[0] * im.shape[1] for im in images[:4]) * (4 + 4 + 4 + 2 + BPP[fmt])
        cut, rep = quality_batch(proc, images, K_MIN, K_MAX, TARGET, mode, fmt, bound=small)
        assert _same_results(cut, want) == []
        assert rep.sub_batches == 3 and rep.per_image == 1 and rep.batched == n - 1 and rep.fallback == 0, rep
        # no image reaches a target of 0 except the flat one: without it, one round
        hard = [images[3], images[6], images[2]]
        got0, rep0 = quality_batch(proc, hard, K_MIN, K_MAX, 0, mode, fmt)
        assert all(g[0] == K_MAX and g[4] == 0 for g in got0) and rep0.rounds == 1 and rep0.palette_runs == 3, rep0
        assert _same_results(got0, [quality_one(proc, im, K_MIN, K_MAX, 0, mode, fmt) for im in hard]) == []


def test_quality_batch_python_layer_and_strategy(torch_cuda, processor):
    import kmeans_gpu_amd as kg
    images = quality_images()[:4]
    want = [processor.reduce_quality(im, 3.0, K_MIN, K_MAX, kg.ReduceMode.Dither, indexed=True) for im in images]
    for strategy in ("auto", "table"):
        kg.set_strategy(strategy)
        try:
            got = processor.reduce_quality_batch(images, 3.0, K_MIN, K_MAX, kg.ReduceMode.Dither, indexed=True)
        finally:
            kg.set_strategy("auto")
        for g, w in zip(got, want):
            assert g[0] == w[0] and np.array_equal(g[1], w[1]) and np.array_equal(g[2], w[2]) and g[3].as_tuple() == w[3].as_tuple() and g[4] == w[4]
    assert processor.last_quality_report.rounds >= 1


def test_quality_batch_fallback_and_single_image(torch_cuda):
    import kmeans_gpu_amd as kg
    with kg.ImageProcessor(shrink_max_dim=0) as proc:
        big = _rgba(np.random.default_rng(2).integers(0, 4, (512, 1024, 3), dtype=np.uint8) * 60)     # 2^19 pixels: the per-image search
        images = [_noise(1, 20, 30), big, _noise(2, 9, 11)]
        got, rep = quality_batch(proc, images, 2, 8, TARGET, REPLACE, INDEX8)
        assert (rep.fallback, rep.per_image, rep.batched) == (1, 1, 2), rep
        assert _same_results(got, [quality_one(proc, im, 2, 8, TARGET, REPLACE, INDEX8) for im in images]) == []
        # a batch of one image: the per-image search
        got, rep = quality_batch(proc, images[:1], 2, 8, TARGET, DITHER, RGBA8)
        assert (rep.rounds, rep.launches, rep.per_image, rep.batched, rep.fallback) == (0, 0, 1, 0, 0) and rep.palette_runs >= 1, rep
        assert _same_results(got, [quality_one(proc, images[0], 2, 8, TARGET, DITHER, RGBA8)]) == []


def test_warm_quality_batch_allocates_nothing(torch_cuda):
    import kmeans_gpu_amd as kg
    images = quality_images()
    with kg.ImageProcessor() as proc:
        first, _ = quality_batch(proc, images, K_MIN, K_MAX, TARGET, DITHER, INDEX8)
        mallocs = proc.debug_block_counts()[0]
        again, _ = quality_batch(proc, images, K_MIN, K_MAX, TARGET, DITHER, INDEX8)
        assert proc.debug_block_counts()[0] == mallocs                     # no hipMalloc in the warm call
        assert _same_results(again, first) == []


def test_quality_batch_image_without_a_kept_pixel(torch_cuda):
    import kmeans_gpu_amd as kg
    images = quality_images()[:3]
    empty = _noise(26, 30, 41)
    empty[..., 3] = 127
    with kg.ImageProcessor(alpha_cutoff=128) as proc:
        for bound in (0, 1):
            rc, pals, counts, bufs, _, reached, _, msg = raw_quality_batch(proc, images + [empty], 2, 8, TARGET, REPLACE, INDEX8, bound=bound)
            assert rc == INVALID and "image 3" in msg and "alpha_cutoff" in msg, (bound, rc, msg)
            assert all(b.untouched() for b in bufs + pals) and np.all(counts == 0xA5A5A5A5) and all(r == -7 for r in reached), bound


# ---- 5. the refusals of the four calls, in order ------------------------------------------------------------------------------------
def test_refusals_one_at_a_time_and_in_pairs(torch_cuda):
    import kmeans_gpu_amd as kg
    L = kg.lib()
    images = [_noise(1, 5, 7), _noise(2, 16, 15), _noise(3, 3, 9)]
    w, h = _dims(images)
    with kg.ImageProcessor() as proc:
        def refused(want_rc, needle, k_min=2, k_max=8, mode=REPLACE, fmt=INDEX8, **kw):
            rc, pals, counts, bufs, _, reached, _, msg = raw_quality_batch(proc, images, k_min, k_max, TARGET, mode, fmt, **kw)
            assert rc == want_rc and msg and needle in msg, (kw, rc, msg)
            assert all(b.untouched() for b in bufs + pals) and np.all(counts == 0xA5A5A5A5) and all(r == -7 for r in reached), kw

        # kmg_reduce_quality_batch, one at a time in the order of include/kmeans_hip.h, then each with the next
        assert L.kmg_reduce_quality_batch(None, 1, None, None, None, 2, 8, 0, 0, 0, 0, None, None, None, None, None, None) == INVALID
        assert b"processor is NULL" in L.kmg_last_error()
        refused(INVALID, "empty", n_images=0)
        for name in ("rgba", "widths", "heights", "out", "palettes", "counts"):
            refused(INVALID, "array is NULL", null=(name,))
        refused(INVALID, "image 1: image pointer is NULL", null_in=1)
        refused(INVALID, "image 2: output pointer is NULL", null_out=2)
        refused(INVALID, "image 0: output pointer is NULL", null_pal=0)
        refused(INVALID, "image 1 has zero width or height", widths=[w[0], 0, w[2]])
        refused(INVALID, "colour counts", k_min=0)
        refused(INVALID, "colour counts", k_min=9)
        refused(INVALID, "colour counts", k_max=3073, fmt=INDEX16)
        refused(INVALID, "unknown mode", mode=4)
        refused(INVALID, "unknown output format", fmt=3)
        refused(INVALID, "no index output", mode=MELD)
        refused(INVALID, "INDEX8", k_max=257)
        proc.set_alpha_cutoff(1)
        refused(INVALID, "transparent slot", k_max=256)
        proc.set_alpha_cutoff(0)
        proc.set_fixed_colors([[255, 0, 0]])
        refused(INVALID, "fixed colours")
        proc.set_alpha_weight(True)
        refused(INVALID, "fixed colours")                                                   # fixed colours before weighting
        refused(INVALID, "INDEX8", k_max=257)                                               # the room of INDEX8 before fixed colours
        proc.set_fixed_colors(None)
        refused(INVALID, "alpha weighting")
        proc.set_alpha_weight(False)
        refused(INVALID, "empty", n_images=0, null=("rgba",))                               # the empty batch before a NULL array
        refused(INVALID, "array is NULL", null=("heights",), null_in=0)                     # a NULL array before a NULL entry
        refused(INVALID, "image 1: image pointer", null_in=1, k_min=0)                      # the images before the colour counts
        refused(INVALID, "colour counts", k_min=0, mode=9)                                  # the colour counts before the mode
        refused(INVALID, "unknown mode", mode=7, fmt=9)                                     # the mode before the format
        refused(INVALID, "unknown output format", fmt=5, mode=REPLACE, k_max=300)           # the format before the index rules
        refused(INVALID, "no index output", mode=MELD, k_max=257)                           # meld before the room of INDEX8

        # the device calls
        stream = torch_cuda.cuda.current_stream().cuda_stream
        d_imgs = _on_device(torch_cuda, images)
        ks_ok = [3, 8, 33]
        tables = np.concatenate([kg.palette_to_centroids(_palette(i, k)) for i, k in enumerate(ks_ok)]).astype(np.float32)
        far = tables.copy()
        far[5, 1] = 400.0                                                                   # image 1's table leaves the box of the index formats

        def dev(call, want_rc, needle, ks=ks_ok, c4=tables, mode=REPLACE, fmt=INDEX8, n_images=3, null=(), widths=None, null_in=None, null_out=None,
                odd=None):
            outs, ptrs = _device_outputs(torch_cuda, images, fmt if fmt in BPP else INDEX8)
            if odd is not None:
                ptrs[odd] += 1
            src = (C.c_void_p * 3)(*[d.data_ptr() for d in d_imgs])
            dst = (C.c_void_p * 3)(*ptrs)
            if null_in is not None:
                src[null_in] = None
            if null_out is not None:
                dst[null_out] = None
            counts = np.array(ks, np.uint32)
            c4 = np.ascontiguousarray(c4, np.float32)
            got = np.full((int(sum(ks_ok)), 4), 7.0, np.float32)
            a = {"rgba": src, "widths": (C.c_uint32 * 3)(*(widths or w)), "heights": (C.c_uint32 * 3)(*h), "out": dst,
                 "centroids": C.c_void_p(c4.ctypes.data if call == "apply" else got.ctypes.data), "ks": C.c_void_p(counts.ctypes.data)}
            for name in null:
                a[name] = None
            if call == "apply":
                rc = L.kmg_dev_apply_batch_counts(proc.handle, n_images, a["rgba"], a["widths"], a["heights"], a["centroids"], a["ks"], mode, fmt,
                                                  a["out"], None, C.c_void_p(stream))
            else:
                rc = L.kmg_dev_palette_batch_counts(proc.handle, n_images, a["rgba"], a["widths"], a["heights"], a["ks"], a["centroids"], None, None,
                                                    C.c_void_p(stream))
            msg = L.kmg_last_error().decode()
            assert rc == want_rc and needle in msg, (call, rc, msg)
            torch_cuda.cuda.synchronize()
            assert all(bool((o == SENTINEL).all()) for o in outs) and np.all(got == 7.0)

        for call in ("palette", "apply"):
            dev(call, INVALID, "empty", n_images=0)
            for name in ("rgba", "widths", "heights", "centroids", "ks") + (("out",) if call == "apply" else ()):
                dev(call, INVALID, "NULL" if call == "apply" else "bad palette_batch arguments", null=(name,))
            dev(call, INVALID, "image 2: image pointer is NULL", null_in=2)
            dev(call, INVALID, "image 1 has zero width", widths=[w[0], 0, w[2]])
            dev(call, INVALID, "higher than 0", ks=[3, 0, 33])
            dev(call, UNSUPPORTED, "KMG_MAX_K", ks=[3, 8, 3073], fmt=INDEX16)
            dev(call, INVALID, "empty", n_images=0, null=("ks",))                             # the empty batch before a NULL array
            dev(call, INVALID, "image 0: image pointer", null_in=0, ks=[0, 8, 33])            # the images before the counts
        dev("palette", INVALID, "higher than 0", ks=[3, 0, 3073])                             # image 1's count before image 2's
        dev("apply", INVALID, "image 0: output pointer is NULL", null_out=0)
        dev("apply", INVALID, "unknown mode", mode=5)
        dev("apply", INVALID, "unknown output format", fmt=-1)
        dev("apply", INVALID, "no index output", mode=MELD)
        dev("apply", INVALID, "INDEX8", ks=[3, 8, 257], c4=np.zeros((268, 4), np.float32))
        dev("apply", INVALID, "outside", c4=far)
        dev("apply", INVALID, "2-byte aligned", fmt=INDEX16, odd=1)
        dev("apply", INVALID, "higher than 0", ks=[3, 0, 33], mode=5)                         # a zero count before the mode
        dev("apply", INVALID, "unknown mode", mode=7, fmt=9)                                  # the mode before the format
        dev("apply", INVALID, "unknown output format", fmt=5, ks=[3, 8, 3073])                # the format before the colour limit
        dev("apply", UNSUPPORTED, "KMG_MAX_K", ks=[3, 8, 3073], mode=MELD)                    # the colour limit before the index rules
        dev("apply", INVALID, "outside", c4=far, fmt=INDEX16, odd=0)                          # the index rules before the alignment

        # kmg_dev_compare_batch
        pixels = [im.shape[0] * im.shape[1] for im in images]
        maps = _on_device(torch_cuda, [np.zeros(n + 1, np.uint16) for n in pixels])
        pal = np.concatenate([_palette(i, k) for i, k in enumerate(ks_ok)])
        rec = _records(torch_cuda, 3)

        def cmp(want_rc, needle, fmt=INDEX16, what=RGB | LAB, cutoff=0, ks=ks_ok, n_images=3, null=(), npx=None, null_in=None, odd=None, rec_off=0):
            src = (C.c_void_p * 3)(*[d.data_ptr() for d in d_imgs])
            dst = (C.c_void_p * 3)(*[m.data_ptr() + (1 if odd == i else 0) for i, m in enumerate(maps)])
            if null_in is not None:
                src[null_in] = None
            counts = np.array(ks, np.uint32)
            a = {"src": src, "out": dst, "pixels": (C.c_uint64 * 3)(*(npx or pixels)), "palettes": C.c_void_p(pal.ctypes.data),
                 "ks": C.c_void_p(counts.ctypes.data), "stats": C.c_void_p(rec.data_ptr() + rec_off)}
            for name in null:
                a[name] = None
            rc = L.kmg_dev_compare_batch(proc.handle, n_images, a["src"], a["out"], a["pixels"], fmt, a["palettes"], a["ks"], cutoff, what, a["stats"],
                                         C.c_void_p(stream))
            msg = L.kmg_last_error().decode()
            assert rc == want_rc and needle in msg, (rc, msg)
            torch_cuda.cuda.synchronize()
            assert bool((rec == 0).all())

        assert L.kmg_dev_compare_batch(None, 1, None, None, None, 0, None, None, 0, 3, None, None) == INVALID
        cmp(INVALID, "empty", n_images=0)
        for name in ("src", "out", "pixels", "stats"):
            cmp(INVALID, "array is NULL", null=(name,))
        cmp(INVALID, "unknown output format", fmt=3)
        cmp(INVALID, "what = 0", what=0)
        cmp(INVALID, "above 255", cutoff=256)
        cmp(INVALID, "needs the palettes", null=("palettes",))
        cmp(INVALID, "needs the palettes", null=("ks",))
        cmp(INVALID, "image 1: image or output pointer is NULL", null_in=1)
        cmp(INVALID, "image 2 has no pixel", npx=[pixels[0], pixels[1], 0])
        cmp(UNSUPPORTED, "2^32-1", npx=[pixels[0], 1 << 32, pixels[2]])
        cmp(INVALID, "image 0: an index format needs a palette", ks=[0, 8, 33])
        cmp(INVALID, "INDEX8", fmt=INDEX8, ks=[3, 8, 257])
        cmp(INVALID, "image 1: INDEX16 output is not 2-byte aligned", odd=1)
        cmp(INVALID, "not 8-byte aligned", rec_off=4)
        cmp(INVALID, "empty", n_images=0, null=("src",))                                    # in pairs: the earlier one wins
        cmp(INVALID, "array is NULL", null=("stats",), fmt=7)
        cmp(INVALID, "unknown output format", fmt=7, what=0)
        cmp(INVALID, "what = 8", what=8, cutoff=300)
        cmp(INVALID, "above 255", cutoff=300, null=("palettes",))
        cmp(INVALID, "needs the palettes", null=("ks",), null_in=0)
        cmp(INVALID, "image 0: image or output", null_in=0, npx=[pixels[0], 0, pixels[2]])
        cmp(INVALID, "image 1 has no pixel", npx=[pixels[0], 0, pixels[2]], ks=[3, 8, 0])
        cmp(INVALID, "image 2: an index format", ks=[3, 8, 0], rec_off=4)
        # the processor is usable afterwards
        got, rep = quality_batch(proc, images, 2, 8, TARGET, DITHER, INDEX8)
        assert _same_results(got, [quality_one(proc, im, 2, 8, TARGET, DITHER, INDEX8) for im in images]) == []
