"""Batched output (include/kmeans_hip.h at kmg_batch_apply_report; kmg_batch_apply.hip): kmg_find_batch, kmg_reduce_indexed_batch
and kmg_dev_apply_batch -- the output passes of many small images in one launch.

The yardstick is always the per-image call of the library -- kmg_find_indexed, kmg_reduce_indexed, kmg_dev_apply_format -- plus
the CPU oracle for a subset; never the batch code itself.  Everything is compared bit for bit, and every host output buffer lies
between guard bytes that must survive."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
SENTINEL = 0xA5
GUARD = 64
RGBA8, INDEX8, INDEX16 = 0, 1, 2
REPLACE, DITHER, MELD, DIFFUSE = 0, 1, 2, 3
BPP = {RGBA8: 4, INDEX8: 1, INDEX16: 2}


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

    def view(self, im, fmt):
        body = self.raw[GUARD:GUARD + self.n]
        return body.reshape(im.shape) if fmt == RGBA8 else body.view(np.uint16 if fmt == INDEX16 else np.uint8).reshape(im.shape[:2])


def _arrays(images, widths=None, heights=None, null_in=None):
    n = max(len(images), 1)
    src = (C.c_void_p * n)(*[im.ctypes.data for im in images])
    if null_in is not None:
        src[null_in] = None
    ws = (C.c_uint32 * n)(*(widths if widths is not None else [im.shape[1] for im in images]))
    hs = (C.c_uint32 * n)(*(heights if heights is not None else [im.shape[0] for im in images]))
    return src, ws, hs


def _ptrs(bufs, null_entry=None):
    a = (C.c_void_p * max(len(bufs), 1))(*[b.ptr for b in bufs])
    if null_entry is not None:
        a[null_entry] = None
    return a


def raw_find_batch(proc, images, pal, mode, fmt, bound=0, n_images=None, null=(), widths=None, heights=None, null_in=None, null_out=None,
                   n_colors=None):
    """kmg_find_batch into guarded buffers: (status, buffers, report, message)"""
    import kmeans_gpu_amd as kg
    L = kg.lib()
    images = [np.ascontiguousarray(im) for im in images]
    bufs = [Guarded(im.shape[0] * im.shape[1] * BPP.get(fmt, 4)) for im in images]
    src, ws, hs = _arrays(images, widths, heights, null_in)
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 4)
    a = {"rgba": src, "widths": ws, "heights": hs, "out": _ptrs(bufs, null_out), "palette": C.c_void_p(pal.ctypes.data)}
    for name in null:
        a[name] = None
    rep = kg.BatchApplyReport()
    rc = L.kmg_find_batch(proc.handle, len(images) if n_images is None else n_images, a["rgba"], a["widths"], a["heights"], a["palette"],
                          pal.shape[0] if n_colors is None else n_colors, mode, fmt, bound, a["out"], C.byref(rep))
    return rc, bufs, rep, L.kmg_last_error().decode()


def find_batch(proc, images, pal, mode, fmt, bound=0):
    rc, bufs, rep, msg = raw_find_batch(proc, images, pal, mode, fmt, bound)
    assert rc == 0, msg
    assert all(b.guards_ok() for b in bufs)
    return [b.view(im, fmt) for b, im in zip(bufs, images)], rep


def find_one(proc, im, pal, mode, fmt):
    """kmg_find_indexed of one image in an explicit format (KMG_FORMAT_RGBA8: the bytes of kmg_find)"""
    import kmeans_gpu_amd as kg
    im = np.ascontiguousarray(im)
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 4)
    buf = Guarded(im.shape[0] * im.shape[1] * BPP[fmt])
    rc = kg.lib().kmg_find_indexed(proc.handle, C.c_void_p(im.ctypes.data), im.shape[1], im.shape[0], C.c_void_p(pal.ctypes.data), pal.shape[0],
                                   mode, fmt, C.c_void_p(buf.ptr))
    assert rc == 0 and buf.guards_ok(), kg.lib().kmg_last_error().decode()
    return buf.view(im, fmt)


def raw_reduce_batch(proc, images, k, mode, fmt, algo=0, bound=0, n_images=None, null=(), widths=None, heights=None, null_in=None,
                     null_out=None, null_pal=None):
    """kmg_reduce_indexed_batch into guarded buffers: (status, palette buffers, counts, output buffers, reports, message)"""
    import kmeans_gpu_amd as kg
    L = kg.lib()
    images = [np.ascontiguousarray(im) for im in images]
    bufs = [Guarded(im.shape[0] * im.shape[1] * BPP.get(fmt, 4)) for im in images]
    pals = [Guarded(4 * max(k, 1)) for _ in images]
    counts = np.full(max(len(images), 1), 0xA5A5A5A5, np.uint32)
    src, ws, hs = _arrays(images, widths, heights, null_in)
    a = {"rgba": src, "widths": ws, "heights": hs, "out": _ptrs(bufs, null_out), "palettes": _ptrs(pals, null_pal),
         "counts": C.c_void_p(counts.ctypes.data)}
    for name in null:
        a[name] = None
    brep, arep = kg.BatchReport(), kg.BatchApplyReport()
    rc = L.kmg_reduce_indexed_batch(proc.handle, len(images) if n_images is None else n_images, a["rgba"], a["widths"], a["heights"], k, algo,
                                    mode, fmt, bound, a["palettes"], a["counts"], a["out"], C.byref(brep), C.byref(arep))
    return rc, pals, counts, bufs, (brep, arep), L.kmg_last_error().decode()


def reduce_batch(proc, images, k, mode, fmt, algo=0, bound=0):
    """[(palette, output)], (batch report, apply report)"""
    rc, pals, counts, bufs, reps, msg = raw_reduce_batch(proc, images, k, mode, fmt, algo, bound)
    assert rc == 0, msg
    assert all(b.guards_ok() for b in bufs) and all(q.guards_ok() for q in pals)
    return [(q.raw[GUARD:GUARD + 4 * int(c)].reshape(-1, 4), b.view(im, fmt)) for q, c, b, im in zip(pals, counts, bufs, images)], reps


def reduce_one(proc, im, k, mode, fmt, algo=0):
    import kmeans_gpu_amd as kg
    im = np.ascontiguousarray(im)
    buf, pal, cnt = Guarded(im.shape[0] * im.shape[1] * BPP[fmt]), Guarded(4 * k), C.c_uint32()
    rc = kg.lib().kmg_reduce_indexed(proc.handle, C.c_void_p(im.ctypes.data), im.shape[1], im.shape[0], k, algo, mode, fmt, C.c_void_p(pal.ptr),
                                     C.byref(cnt), C.c_void_p(buf.ptr))
    assert rc == 0 and buf.guards_ok() and pal.guards_ok(), kg.lib().kmg_last_error().decode()
    return pal.raw[GUARD:GUARD + 4 * cnt.value].reshape(-1, 4), buf.view(im, fmt)


def _same_pairs(got, want):
    return all(np.array_equal(gp, wp) and np.array_equal(go, wo) for (gp, go), (wp, wo) in zip(got, want))


@pytest.fixture(scope="module")
def edge_images(oracle, tokyo):
    """1 .. 2049 pixels around the group of four, the tiles of 1024 and 2048 pixels and the workgroup of 256 threads; 1 x n and
    n x 1 among them, and widths 2, 3, 5 and 7, so that a group of four pixels crosses row ends and the Bayer index wraps inside
    it; one image twice; the 256 x 171 shrunk tokyo image"""
    shapes = [(1, 1), (1, 2), (3, 1), (2, 2), (1, 5), (85, 3), (128, 2), (1, 257), (341, 3), (1024, 1), (205, 5), (89, 23), (1, 2048),
              (683, 3), (37, 7)]
    assert [h * w for h, w in shapes[:14]] == [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049]
    images = [_noise(10 + i, h, w) for i, (h, w) in enumerate(shapes)]
    nw, nh = oracle.resized_dims(tokyo.shape[1], tokyo.shape[0])
    assert (nw, nh) == (256, 171)
    return images + [images[8], np.ascontiguousarray(oracle.resize(tokyo, nw, nh))]


# ---- 1. tile and group edges ---------------------------------------------------------------------------------------------------
CASES = [(k, f) for k in (1, 2, 31, 32, 33, 255, 256) for f in (RGBA8, INDEX8, INDEX16)] + [(k, f) for k in (257, 3072) for f in (RGBA8, INDEX16)]


@pytest.mark.parametrize("mode", [REPLACE, DITHER])
@pytest.mark.parametrize("k,fmt", CASES)
def test_tile_and_group_edges(processor, edge_images, k, fmt, mode):
    pal = _palette(k, k)
    got, rep = find_batch(processor, edge_images, pal, mode, fmt)
    assert (rep.batched, rep.per_image, rep.sub_batches) == (len(edge_images), 0, 1) and rep.launches >= 1, rep
    for i, im in enumerate(edge_images):
        assert np.array_equal(got[i], find_one(processor, im, pal, mode, fmt)), (i, im.shape)
    if fmt != RGBA8 and k == 33:
        # the Python layer: the format find_indexed chooses
        maps = processor.find_batch(edge_images, pal, reduce_mode=mode)
        assert all(np.array_equal(m, processor.find_indexed(im, pal, reduce_mode=mode)) for m, im in zip(maps, edge_images))


# ---- 2. shared and per-image tables on device-resident images ------------------------------------------------------------------
def _device_outputs(torch, images, fmt):
    """guarded device outputs: (tensors, addresses of the bodies)"""
    outs = [torch.full((im.shape[0] * im.shape[1] * BPP[fmt] + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for im in images]
    return outs, [o.data_ptr() + GUARD for o in outs]


def _device_body(out, im, fmt):
    raw = out.cpu().numpy()
    assert np.all(raw[:GUARD] == SENTINEL) and np.all(raw[-GUARD:] == SENTINEL)
    body = raw[GUARD:-GUARD]
    return body.reshape(im.shape) if fmt == RGBA8 else body.view(np.uint16 if fmt == INDEX16 else np.uint8).reshape(im.shape[:2])


@pytest.mark.parametrize("k,fmt,mode", [(8, RGBA8, DITHER), (8, INDEX8, REPLACE), (33, INDEX16, DITHER), (64, INDEX8, DITHER), (300, RGBA8, REPLACE)])
def test_shared_and_per_image_tables(torch_cuda, processor, edge_images, k, fmt, mode):
    import kmeans_gpu_amd as kg
    stream = torch_cuda.cuda.current_stream().cuda_stream
    images = edge_images
    n = len(images)
    d_imgs = [torch_cuda.from_numpy(im).cuda() for im in images]
    tables = np.stack([kg.palette_to_centroids(_palette(50 * k + t, k)) for t in range(n)])
    ws, hs = [im.shape[1] for im in images], [im.shape[0] for im in images]
    for c4 in (tables[0], tables):
        outs, ptrs = _device_outputs(torch_cuda, images, fmt)
        rep = processor.apply_batch_device([d.data_ptr() for d in d_imgs], ws, hs, c4, mode, fmt, ptrs, stream)
        assert (rep.batched, rep.per_image, rep.sub_batches) == (n, 0, 1) and rep.launches >= 1
        for i, im in enumerate(images):
            want, wptr = _device_outputs(torch_cuda, [im], fmt)
            processor.apply(d_imgs[i].data_ptr(), ws[i], hs[i], 0, c4 if c4.ndim == 2 else c4[i], mode, wptr[0], stream, format=kg.OutputFormat(fmt))
            torch_cuda.cuda.synchronize()
            assert np.array_equal(_device_body(outs[i], im, fmt), _device_body(want[0], im, fmt)), (i, im.shape, c4.ndim)


# ---- 3. alpha mode -------------------------------------------------------------------------------------------------------------
def _alpha_images():
    full = _noise(21, 30, 41)
    half = _noise(22, 30, 41)
    half[:, :20, 3] = 0
    mixed = _noise(23, 17, 7)
    mixed[..., 3] = np.random.default_rng(9).integers(0, 256, (17, 7), dtype=np.uint8)
    one = _noise(24, 9, 5)
    one[..., 3] = 0
    one[4, 3, 3] = 200
    return [full, half, mixed, one, _noise(25, 1, 3)]


@pytest.mark.parametrize("cutoff", [1, 128])
def test_alpha_mode(torch_cuda, cutoff):
    import kmeans_gpu_amd as kg
    images = _alpha_images()
    k = 8
    pal = _palette(77, k)
    with kg.ImageProcessor(alpha_cutoff=cutoff) as proc:
        for mode in (REPLACE, DITHER):
            for fmt in (RGBA8, INDEX8, INDEX16):
                got, rep = find_batch(proc, images, pal, mode, fmt)
                assert (rep.batched, rep.per_image) == (len(images), 0)
                for i, im in enumerate(images):
                    assert np.array_equal(got[i], find_one(proc, im, pal, mode, fmt)), (i, mode, fmt)
                    dropped = im[..., 3] < cutoff
                    if fmt == RGBA8:
                        assert np.array_equal(got[i][..., 3], im[..., 3])                 # the source's alpha
                    else:
                        assert np.all(got[i][dropped] == k) and np.all(got[i][~dropped] < k)
                        assert dropped.any() or i in (0, 4)
                res, (brep, arep) = reduce_batch(proc, images, k, mode, fmt)
                assert arep.batched == len(images) and brep.launches > 0
                assert _same_pairs(res, [reduce_one(proc, im, k, mode, fmt) for im in images]), (mode, fmt)
        # INDEX8 holds 256 indices: 255 colours and the transparent slot
        rc, bufs, _, msg = raw_find_batch(proc, images, _palette(5, 256), REPLACE, INDEX8)
        assert rc == INVALID and "INDEX8" in msg and all(b.untouched() for b in bufs), (rc, msg)
        got, rep = find_batch(proc, images, _palette(5, 255), DITHER, INDEX8)
        assert rep.batched == len(images)
        for i, im in enumerate(images):
            assert np.array_equal(got[i], find_one(proc, im, _palette(5, 255), DITHER, INDEX8)), i
        rc, pals, counts, bufs, _, msg = raw_reduce_batch(proc, images, 256, REPLACE, INDEX8)
        assert rc == INVALID and "INDEX8" in msg and all(b.untouched() for b in bufs + pals), (rc, msg)


# ---- 4. fallbacks keep the bytes -----------------------------------------------------------------------------------------------
def test_fallbacks_keep_the_bytes(torch_cuda, processor, edge_images):
    import kmeans_gpu_amd as kg
    images = edge_images[3:9] + edge_images[-1:]
    n = len(images)
    pal = _palette(3, 16)
    # meld and diffusion: their own passes
    for mode, fmt in ((MELD, RGBA8), (DIFFUSE, RGBA8), (DIFFUSE, INDEX8)):
        got, rep = find_batch(processor, images, pal, mode, fmt)
        assert (rep.launches, rep.batched, rep.per_image) == (0, 0, n), (mode, rep)
        for i, im in enumerate(images):
            assert np.array_equal(got[i], find_one(processor, im, pal, mode, fmt)), (mode, fmt, i)
        res, (_, arep) = reduce_batch(processor, images, 8, mode, fmt)
        assert (arep.batched, arep.per_image) == (0, n)
        assert _same_pairs(res, [reduce_one(processor, im, 8, mode, fmt) for im in images]), (mode, fmt)
    # a forced colour table / candidate lists
    want = {mode: [find_one(processor, im, pal, mode, INDEX8) for im in images] for mode in (REPLACE, DITHER)}
    kg.set_strategy("table")
    try:
        for mode in (REPLACE, DITHER):
            got, rep = find_batch(processor, images, pal, mode, INDEX8)
            assert (rep.launches, rep.batched, rep.per_image) == (0, 0, n), (mode, rep)
            assert all(np.array_equal(g, w) for g, w in zip(got, want[mode])), mode
    finally:
        kg.set_strategy("auto")
    # Dither images that a plan of their own sends to the candidate lists.  The join rule is widened by one case (kmg_apply_route.h,
    # measured in the `pruned` rows of profiles/r10_batch_apply_time.txt: joined, such images take 0.23 - 0.37 of their own passes):
    # from k = 128 a plan prunes from 16384 pixels on for the latency of ONE image's scan, which a batched launch pays once -- so
    # the 128 x 128 image at k = 128 joins, and an image prunes inside a batch only where the lists win on throughput:
    # n (0.255 k - 0.3) > 45e6, 600 x 600 at k = 512.  A batch of ONE image is its own plan: the 128 x 128 image alone prunes.
    tiny = [_noise(60 + i, 8, 8) for i in range(4)]
    for k, big, per_image in ((128, _noise(70, 128, 128), 0), (512, _noise(71, 600, 600), 1)):
        batch = tiny[:2] + [big] + tiny[2:]
        pal_k = _palette(k, k)
        got, rep = find_batch(processor, batch, pal_k, DITHER, INDEX16)
        assert (rep.batched, rep.per_image) == (len(batch) - per_image, per_image), (k, rep)
        for i, im in enumerate(batch):
            assert np.array_equal(got[i], find_one(processor, im, pal_k, DITHER, INDEX16)), (k, i)
    alone = _noise(70, 128, 128)
    got, rep = find_batch(processor, [alone], _palette(128, 128), DITHER, INDEX16)
    assert (rep.launches, rep.batched, rep.per_image) == (0, 0, 1), rep
    assert np.array_equal(got[0], find_one(processor, alone, _palette(128, 128), DITHER, INDEX16))
    # the octree: the host algorithm and the per-image output pass
    octree = int(kg.Algorithm.Octree)
    res, (brep, arep) = reduce_batch(processor, images, 8, DITHER, INDEX8, algo=octree)
    assert (arep.launches, arep.batched, arep.per_image) == (0, 0, n) and brep.launches == 0
    assert _same_pairs(res, [reduce_one(processor, im, 8, DITHER, INDEX8, algo=octree) for im in images])


# ---- 5. kmg_reduce_indexed_batch = kmg_reduce_indexed per image ------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [RGBA8, INDEX8, INDEX16])
@pytest.mark.parametrize("k", [8, 64])
def test_reduce_indexed_batch_equivalences(processor, edge_images, k, fmt):
    images = edge_images
    n = len(images)
    for mode in (REPLACE, DITHER):
        want = [reduce_one(processor, im, k, mode, fmt) for im in images]
        got, (brep, arep) = reduce_batch(processor, images, k, mode, fmt)
        assert (arep.batched, arep.per_image, arep.sub_batches) == (n, 0, 1) and arep.launches >= 1 and brep.launches > 0
        assert _same_pairs(got, want), mode
        assert all(len(p) == k for p, _ in got)
        if mode == DITHER:
            continue
        back, _ = reduce_batch(processor, images[::-1], k, mode, fmt)                  # the batch reversed
        assert _same_pairs(back[::-1], want)
        cut, (_, arep) = reduce_batch(processor, images, k, mode, fmt, bound=1)          # a sub-batch per image
        assert arep.sub_batches == n and arep.batched == n and _same_pairs(cut, want)
    # a cut after every second image: six images of one size, the bound two images' source and output
    same = [_noise(90 + i, 30, 40) for i in range(6)]
    want = [reduce_one(processor, im, k, DITHER, fmt) for im in same]
    cut, (brep, arep) = reduce_batch(processor, same, k, DITHER, fmt, bound=2 * 1200 * (4 + BPP[fmt]))
    assert (brep.sub_batches, arep.sub_batches, arep.batched) == (3, 3, 6) and _same_pairs(cut, want)
    if fmt != RGBA8 and k == 8:
        pairs = processor.reduce_indexed_batch(k, same, reduce_mode=DITHER)            # the Python layer
        assert processor.last_batch_apply_report.batched == 6
        assert _same_pairs(pairs, [processor.reduce_indexed(k, im, reduce_mode=DITHER) for im in same])


# ---- 6. the CPU oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 64])
def test_three_images_match_the_oracle(processor, oracle, edge_images, k):
    three = np.array([[10, 200, 30], [250, 250, 250], [90, 20, 160]], np.uint8)
    few = _rgba(three[np.random.default_rng(5).integers(0, 3, (7, 73))])                 # 73 x 7, three colours
    images = [few, _noise(6, 19, 27), edge_images[-1]]                                   # 27 x 19, 256 x 171
    pal = _palette(k + 1, k)
    for mode, omode in ((REPLACE, oracle.MODE_REPLACE), (DITHER, oracle.MODE_DITHER)):
        got, rep = find_batch(processor, images, pal, mode, RGBA8)
        res, (_, arep) = reduce_batch(processor, images, k, mode, RGBA8)
        idx, _ = reduce_batch(processor, images, k, mode, INDEX16)
        assert rep.batched == 3 and arep.batched == 3
        for i, im in enumerate(images):
            want = oracle.find(im, pal, omode)
            assert np.array_equal(got[i], want), (mode, i)
            want = oracle.reduce(im, k, omode)
            assert np.array_equal(res[i][1], want), (mode, i)
            p, m = idx[i]
            assert np.array_equal(p[m], want), (mode, i)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_one_at_a_time_and_in_pairs(torch_cuda, edge_images):
    import kmeans_gpu_amd as kg
    images = [edge_images[14], edge_images[5], edge_images[7]]
    w = [im.shape[1] for im in images]
    h = [im.shape[0] for im in images]
    pal = _palette(1, 8)
    with kg.ImageProcessor() as proc:
        def refused(want_rc, needle, which=("find", "reduce"), mode=REPLACE, fmt=INDEX8, k=8, algo=0, **kw):
            if "find" in which:
                fkw = {a: b for a, b in kw.items() if a != "null_pal"}
                if k != 8:
                    fkw["n_colors"] = k
                rc, bufs, _, msg = raw_find_batch(proc, images, _palette(1, max(k, 1)), mode, fmt, **fkw)
                assert rc == want_rc and msg and needle in msg, ("find", kw, rc, msg)
                assert all(b.untouched() for b in bufs), ("find", kw)
            if "reduce" in which:
                rkw = {a: ("palettes" if b == "palette" else b) for a, b in kw.items()}
                rc, pals, counts, bufs, _, msg = raw_reduce_batch(proc, images, k, mode, fmt, algo=algo, **rkw)
                assert rc == want_rc and msg and needle in msg, ("reduce", kw, rc, msg)
                assert all(b.untouched() for b in bufs + pals) and np.all(counts == 0xA5A5A5A5), ("reduce", kw)

        # one at a time, in the order of include/kmeans_hip.h
        L = kg.lib()
        assert L.kmg_find_batch(None, 1, None, None, None, None, 1, 0, 0, 0, None, None) == INVALID and b"processor is NULL" in L.kmg_last_error()
        assert L.kmg_reduce_indexed_batch(None, 1, None, None, None, 8, 0, 0, 0, 0, None, None, None, None, None) == INVALID
        assert L.kmg_dev_apply_batch(None, 1, None, None, None, None, 1, 8, 0, 0, None, None, None) == INVALID
        refused(INVALID, "empty", n_images=0)
        for name in ("rgba", "widths", "heights", "out"):
            refused(INVALID, "array is NULL", null=(name,))
        refused(INVALID, "array is NULL", which=("reduce",), null=("palettes",))
        refused(INVALID, "array is NULL", which=("reduce",), null=("counts",))
        refused(INVALID, "image 1: image pointer is NULL", null_in=1)
        refused(INVALID, "image 2: output pointer is NULL", null_out=2)
        refused(INVALID, "image 0: output pointer is NULL", which=("reduce",), null_pal=0)
        refused(INVALID, "image 1 has zero width or height", widths=[w[0], 0, w[2]])
        refused(INVALID, "image 0 has zero width or height", heights=[0, h[1], h[2]])
        refused(INVALID, "higher than 0", which=("reduce",), k=0)
        refused(INVALID, "palette is empty", which=("find",), k=0)
        refused(INVALID, "palette is empty", which=("find",), null=("palette",))
        refused(INVALID, "unknown algorithm", which=("reduce",), algo=2)
        refused(INVALID, "unknown mode", mode=4)
        refused(INVALID, "unknown mode", mode=-1)
        refused(INVALID, "unknown output format", fmt=3)
        refused(UNSUPPORTED, "KMG_MAX_K", k=3073, fmt=INDEX16)
        refused(INVALID, "no index output", mode=MELD)
        refused(INVALID, "INDEX8", k=257)
        proc.set_fixed_colors([[255, 0, 0]])
        refused(INVALID, "fixed colours", which=("reduce",))
        got, _ = find_batch(proc, images, pal, REPLACE, INDEX8)                            # kmg_find_batch ignores them, as kmg_find does
        assert all(np.array_equal(g, find_one(proc, im, pal, REPLACE, INDEX8)) for g, im in zip(got, images))
        # pairs: the earlier refusal wins
        refused(INVALID, "unknown algorithm", which=("reduce",), algo=7)                    # algorithm before fixed colours
        refused(INVALID, "INDEX8", which=("reduce",), k=257)                                # the index rules before fixed colours
        refused(INVALID, "no index output", which=("reduce",), mode=MELD)
        proc.set_alpha_weight(True)
        refused(INVALID, "fixed colours", which=("reduce",))                                # fixed colours before weighting
        proc.set_fixed_colors(None)
        refused(INVALID, "alpha weighting", which=("reduce",))
        got, _ = find_batch(proc, images, pal, DITHER, INDEX8)
        assert all(np.array_equal(g, find_one(proc, im, pal, DITHER, INDEX8)) for g, im in zip(got, images))
        proc.set_alpha_weight(False)
        refused(INVALID, "empty", n_images=0, null=("rgba",))                               # the empty batch before a NULL array
        refused(INVALID, "array is NULL", null=("heights",), null_in=0)                     # a NULL array before a NULL entry
        refused(INVALID, "image 0 has zero width", widths=[0, w[1], w[2]], null_in=1)       # image 0 before image 1
        refused(INVALID, "image 1: image pointer", null_in=1, k=0)                          # the images before the colour count
        refused(INVALID, "higher than 0", which=("reduce",), k=0, algo=5)                   # the colour count before the algorithm
        refused(INVALID, "palette is empty", which=("find",), k=0, mode=9)                  # ... and before the mode
        refused(INVALID, "unknown mode", mode=7, fmt=9)                                     # the mode before the format
        refused(INVALID, "unknown output format", fmt=5, k=3073)                            # the format before the colour limit
        refused(UNSUPPORTED, "KMG_MAX_K", k=3073, mode=MELD)                                # the colour limit before the index rules
        refused(INVALID, "no index output", mode=MELD, k=257)                               # meld before the room of INDEX8

        # kmg_dev_apply_batch
        stream = torch_cuda.cuda.current_stream().cuda_stream
        d_imgs = [torch_cuda.from_numpy(im).cuda() for im in images]
        c4 = kg.palette_to_centroids(pal)
        far = c4.copy()
        far[3, 1] = 400.0                                                                   # outside the box of the index formats

        def dev(want_rc, needle, tables=c4, n_tables=1, k=8, mode=REPLACE, fmt=INDEX8, n_images=3, null=(), widths=None, null_in=None,
                null_out=None, odd=None):
            outs, ptrs = _device_outputs(torch_cuda, images, fmt if fmt in BPP else INDEX8)
            if odd is not None:
                ptrs[odd] += 1
            src = (C.c_void_p * 3)(*[d.data_ptr() for d in d_imgs])
            dst = (C.c_void_p * 3)(*ptrs)
            if null_in is not None:
                src[null_in] = None
            if null_out is not None:
                dst[null_out] = None
            tables = np.ascontiguousarray(tables, np.float32)
            a = {"rgba": src, "widths": (C.c_uint32 * 3)(*(widths or w)), "heights": (C.c_uint32 * 3)(*h), "out": dst,
                 "centroids": C.c_void_p(tables.ctypes.data)}
            for name in null:
                a[name] = None
            rc = L.kmg_dev_apply_batch(proc.handle, n_images, a["rgba"], a["widths"], a["heights"], a["centroids"], n_tables, k, mode, fmt, a["out"],
                                       None, C.c_void_p(stream))
            msg = L.kmg_last_error().decode()
            assert rc == want_rc and needle in msg, (rc, msg)
            torch_cuda.cuda.synchronize()
            assert all(bool((o == SENTINEL).all()) for o in outs)

        dev(INVALID, "empty", n_images=0)
        for name in ("rgba", "widths", "heights", "out", "centroids"):
            dev(INVALID, "array is NULL", null=(name,))
        dev(INVALID, "image 2: image pointer is NULL", null_in=2)
        dev(INVALID, "image 0: output pointer is NULL", null_out=0)
        dev(INVALID, "image 1 has zero width", widths=[w[0], 0, w[2]])
        dev(INVALID, "higher than 0", k=0)
        dev(INVALID, "unknown mode", mode=5)
        dev(INVALID, "unknown output format", fmt=-1)
        dev(UNSUPPORTED, "KMG_MAX_K", k=3073)
        dev(INVALID, "no index output", mode=MELD)
        dev(INVALID, "outside", tables=far)
        dev(INVALID, "n_tables", n_tables=2, tables=np.stack([c4, c4]))
        dev(INVALID, "n_tables", n_tables=0)
        dev(INVALID, "2-byte aligned", fmt=INDEX16, odd=1)
        dev(INVALID, "outside", tables=np.stack([c4, far]), n_tables=2)                     # the index rules before n_tables
        dev(INVALID, "no index output", mode=MELD, n_tables=2, tables=np.stack([c4, c4]))
        dev(INVALID, "n_tables", n_tables=2, tables=np.stack([c4, c4]), fmt=INDEX16, odd=0)  # n_tables before the alignment
        dev(INVALID, "higher than 0", k=0, mode=5)
        # the processor is usable afterwards
        got, rep = find_batch(proc, images, pal, DITHER, INDEX8)
        assert rep.batched == 3 and all(np.array_equal(g, find_one(proc, im, pal, DITHER, INDEX8)) for g, im in zip(got, images))


# ---- 8. more workgroups than one launch takes --------------------------------------------------------------------------------------
def test_more_workgroups_than_one_launch_takes(torch_cuda, processor, edge_images):
    """24 400 views of the 256 x 171 image: 43 tiles of 1024 pixels each, 1 049 200 workgroups -- past the 2^20 of one launch (the
    cut itself: tests/native/check_batch_layout.cpp).  All views but the last two write the same bytes into one output."""
    import kmeans_gpu_amd as kg
    stream = torch_cuda.cuda.current_stream().cuda_stream
    im = edge_images[-1]
    views = 24_400
    d_img = torch_cuda.from_numpy(im).cuda()
    c4 = kg.palette_to_centroids(_palette(4, 4))
    outs, ptrs = _device_outputs(torch_cuda, [im] * 3, INDEX8)
    rep = processor.apply_batch_device([d_img.data_ptr()] * views, [im.shape[1]] * views, [im.shape[0]] * views, c4, DITHER, INDEX8,
                                       [ptrs[0]] * (views - 2) + ptrs[1:], stream)
    assert rep.launches >= 2 and (rep.batched, rep.per_image) == (views, 0), rep
    want = find_one(processor, im, _palette(4, 4), DITHER, INDEX8)
    for o in outs:
        assert np.array_equal(_device_body(o, im, INDEX8), want)


# ---- 9. the command line ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", [0, 128])
def test_cli_batch_indexed_writes_palette_pngs(torch_cuda, tmp_path, capsys, cutoff):
    import kmeans_gpu_amd as kg
    from PIL import Image
    from kmeans_gpu_amd import cli
    images = [_noise(80, 20, 31), _noise(81, 7, 5)]
    images[0][:, :9, 3] = 10
    paths = []
    for i, im in enumerate(images):
        paths.append(str(tmp_path / f"in{i}.png"))
        Image.fromarray(im, "RGBA").save(paths[-1])
    out = str(tmp_path / "out")
    argv = ["batch", "-i", *paths, "-c", "8", "-m", "dither", "-o", out, "--indexed"] + (["--alpha-cutoff", str(cutoff)] if cutoff else [])
    assert cli.main(argv) == 0
    said = capsys.readouterr().out
    assert "Batch: 2 images" in said and "Batch output: 1 launches for 2 images, 0 on the per-image pass" in said, said
    with kg.ImageProcessor(alpha_cutoff=cutoff) as proc:
        for i, im in enumerate(images):
            png = Image.open(os.path.join(out, f"in{i}-reduce-c8-kmeans-dither.png"))
            assert png.mode == "P"
            got = np.array(png.convert("RGBA"))
            want = proc.reduce(8, im, reduce_mode=kg.ReduceMode.Dither)
            kept = im[..., 3] >= cutoff
            assert np.array_equal(got[kept][:, :3], want[kept][:, :3]) and np.all(got[kept][:, 3] == 255), i
            assert np.all(got[~kept][:, 3] == 0), i


# ---- 10. sub-batches: the cuts of kmg_find_batch, the up-front alpha pass, the octree image by image --------------------------------
@pytest.mark.parametrize("fmt", [RGBA8, INDEX8, INDEX16])
def test_find_batch_in_several_sub_batches(processor, fmt):
    """six images of one size: a cut after every second image (the bound two images' source and output), then one after every image"""
    same = [_noise(90 + i, 30, 40) for i in range(6)]
    pal = _palette(8, 8)
    want = [find_one(processor, im, pal, DITHER, fmt) for im in same]
    got, rep = find_batch(processor, same, pal, DITHER, fmt, bound=2 * 1200 * (4 + BPP[fmt]))
    assert (rep.sub_batches, rep.batched, rep.per_image) == (3, 6, 0), rep
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    got, rep = find_batch(processor, same, pal, DITHER, fmt, bound=1)
    assert rep.sub_batches == 6 and rep.batched + rep.per_image == 6, rep
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("algo", [0, 1], ids=["kmeans", "octree"])
def test_reduce_indexed_batch_image_without_a_kept_pixel(torch_cuda, algo):
    """an image that keeps no pixel refuses the whole call before any output is written, in one sub-batch and in one per image (the
    up-front alpha pass); without it, a sub-batch per image gives the bytes of kmg_reduce_indexed"""
    import kmeans_gpu_amd as kg
    images = _alpha_images()
    empty = _noise(26, 30, 41)
    empty[..., 3] = 127
    k = 8
    with kg.ImageProcessor(alpha_cutoff=128) as proc:
        for bound in (0, 1):
            rc, pals, counts, bufs, _, msg = raw_reduce_batch(proc, images[:3] + [empty] + images[3:], k, DITHER, INDEX8, algo=algo, bound=bound)
            assert rc == INVALID and "image 3" in msg, (bound, rc, msg)
            assert all(b.untouched() for b in bufs + pals) and np.all(counts == 0xA5A5A5A5), bound
        got, (brep, arep) = reduce_batch(proc, images, k, DITHER, INDEX8, algo=algo, bound=1)
        assert (brep.sub_batches, arep.sub_batches) == (len(images), len(images))
        assert _same_pairs(got, [reduce_one(proc, im, k, DITHER, INDEX8, algo=algo) for im in images])


def test_octree_reduce_indexed_batch_image_by_image(processor, edge_images):
    """the octree at a sub-batch per image: the host algorithm and the per-image output pass, nothing batched"""
    images = edge_images[3:9] + edge_images[-1:]
    n = len(images)
    got, (brep, arep) = reduce_batch(processor, images, 8, DITHER, INDEX8, algo=1, bound=1)
    assert (arep.per_image, arep.batched, arep.launches, arep.sub_batches) == (n, 0, 0, n), arep
    assert (brep.sub_batches, brep.launches) == (n, 0), brep
    assert _same_pairs(got, [reduce_one(processor, im, 8, DITHER, INDEX8, algo=1) for im in images])
