"""Palette-index output (include/kmeans_hip.h kmg_output_format) on every route of the output pass.

The routes are those of the table in tests/test_gpu_alpha_routes.py, for the modes with an index (replace 0, dither 1, diffuse 3):
`scan` and `table` at k = 1, 5, 24, 40, 256, 300, 600 (k_apply unchunked / chunked, the label tables u8 / u16, the Lab lists of one
and two halves, the mask words above 512, kDiffuseScan / Pairs / Cells), and the mask-word column `table+mask_words` for dither at
k = 40, 100, 150, 200, 256 (k_dither_sorted and k_dither_pruned<W> with the identity palette, then k_narrow_index).

Every cell runs on the 1001 x 300 image of the alpha route test through kmg_dev_apply_format on the whole image and through one plan
in three bands on two streams (the later bands start on odd pixel offsets: the `aligned == 0` paths), in INDEX8 where k <= 256 and
in INDEX16, and checks that
  - P[index] is the RGBA8 call's RGB, byte for byte (P = lab_to_rgb.wgsl of the centroids, the output pass's palette);
  - every index is < k; in alpha mode (cutoff 128) exactly the pixels with alpha < 128 are k, the others keep their index
    (diffusion: P[index] = the RGBA8 call's RGB in alpha mode);
  - the index is the same across strategies, and in replace mode equals the oracle's orc_assign labels."""
import numpy as np
import pytest

from conftest import set_strategy
from test_gpu_alpha_routes import BANDS, H, W, _image

pytestmark = pytest.mark.gpu

FMT8, FMT16 = 1, 2
T = 128
KS = (1, 5, 24, 40, 256, 300, 600)
ROUTES = ([(s, k, m) for s in ("scan", "table") for k in KS for m in (0, 1, 3)] +
          [("table+mask_words", k, 1) for k in (40, 100, 150, 200, 256)])


@pytest.fixture(scope="module")
def image(oracle):
    return _image(oracle)


@pytest.fixture(scope="module")
def procs(torch_cuda):
    import kmeans_gpu_amd as kg
    ps = {0: kg.ImageProcessor(), T: kg.ImageProcessor(alpha_cutoff=T)}
    yield ps
    for p in ps.values():
        p.close()


_palettes, _seen, _labels = {}, {}, {}


def _centroids(oracle, k):
    import kmeans_gpu_amd as kg
    if k not in _palettes:
        pal = np.array(sorted(set(map(tuple, oracle.synth_uniform(k + 9, k)))), np.uint8)
        assert pal.shape[0] == k
        _palettes[k] = kg.palette_to_centroids(pal)
    return _palettes[k]


def _rgba(torch, proc, d_in, cent, mode):
    out = torch.full_like(d_in, 0x5A)
    proc.apply(d_in.data_ptr(), W, H, 0, cent, mode, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(H, W, 4)


def _dtype(fmt):
    return np.uint8 if fmt == FMT8 else np.uint16


def _whole(torch, proc, d_in, cent, mode, fmt):
    t = torch.uint8 if fmt == FMT8 else torch.int16
    out = torch.full((H * W + 64,), 0x5A, dtype=t, device="cuda")
    proc.apply(d_in.data_ptr(), W, H, 0, cent, mode, out.data_ptr(), torch.cuda.current_stream().cuda_stream, format=fmt)
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(_dtype(fmt))
    assert (host[H * W:] == 0x5A).all(), "written past the end"
    return host[:H * W].reshape(H, W)


def _banded(torch, proc, d_in, cent, mode, fmt):
    t = torch.uint8 if fmt == FMT8 else torch.int16
    size = 1 if fmt == FMT8 else 2
    out = torch.full((H * W,), 0x5A, dtype=t, device="cuda")
    torch.cuda.synchronize()
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    plan = proc.apply_plan(cent, mode, W * H, streams[0].cuda_stream, format=fmt)
    try:
        for i in range(len(BANDS) - 1):
            r0, r1 = BANDS[i], BANDS[i + 1]
            plan.run(d_in.data_ptr() + 4 * r0 * W, W, r1 - r0, r0, out.data_ptr() + size * r0 * W, streams[i % 2].cuda_stream)
        torch.cuda.synchronize()
        plan.status()
    finally:
        plan.close()
    return out.cpu().numpy().view(_dtype(fmt)).reshape(H, W)


def _orc_labels(oracle, image, cent, k):
    if k not in _labels:
        _labels[k] = oracle.assign(oracle.rgb_to_lab(image.reshape(-1, 4)), cent).reshape(H, W)
    return _labels[k]


@pytest.mark.parametrize("strategy,k,mode", ROUTES)
def test_route_index(oracle, torch_cuda, procs, image, strategy, k, mode):
    torch = torch_cuda
    set_strategy(strategy)
    cent = _centroids(oracle, k)
    P = oracle.lab_to_rgba8(cent[:, :3])
    d_in = torch.from_numpy(image.reshape(-1, 4)).cuda()
    rgba = _rgba(torch, procs[0], d_in, cent, mode)
    rgba_t = _rgba(torch, procs[T], d_in, cent, mode)
    drop = image[..., 3] < T
    ref = None
    for fmt in ((FMT8, FMT16) if k <= 256 else (FMT16,)):
        idx = _whole(torch, procs[0], d_in, cent, mode, fmt)
        assert int(idx.max()) < k, f"format {fmt}: index {int(idx.max())} >= k"
        assert np.array_equal(P[idx][..., :3], rgba[..., :3]), f"format {fmt}: P[index] is not the RGBA8 output"
        assert np.array_equal(_banded(torch, procs[0], d_in, cent, mode, fmt), idx), f"format {fmt}: plan in bands"
        ref = idx.astype(np.uint32) if ref is None else ref
        assert np.array_equal(idx, ref), "INDEX8 and INDEX16 differ"
        if fmt == FMT8 and k == 256:
            continue                                          # (no room for the transparent slot)
        for got in (_whole(torch, procs[T], d_in, cent, mode, fmt), _banded(torch, procs[T], d_in, cent, mode, fmt)):
            assert np.array_equal(got == k, drop), f"format {fmt}: index k exactly where alpha < {T}"
            kept = ~drop
            if mode == 3:
                assert np.array_equal(P[got[kept]][:, :3], rgba_t[kept][:, :3]), f"format {fmt}: alpha-mode diffusion"
            else:
                assert np.array_equal(got[kept], idx[kept]), f"format {fmt}: alpha mode changed a kept pixel's index"
    key = (k, mode)
    if key in _seen:
        assert np.array_equal(_seen[key], ref), "the index differs between strategies"
    _seen[key] = ref
    if mode == 0:
        assert np.array_equal(ref, _orc_labels(oracle, image, cent, k)), "replace index differs from orc_assign"


@pytest.mark.parametrize("k,mode,fmt", [(256, 0, FMT8), (256, 1, FMT8), (600, 0, FMT16)])
def test_full_resolution(oracle, torch_cuda, procs, k, mode, fmt):
    """8192^2 (the flagship image size) through a plan sized for it: the label-table route for replace, the list route for dither"""
    torch = torch_cuda
    n = 8192 * 8192
    d_in = torch.from_numpy(oracle.synth_uniform(8192, n)).cuda()
    cent = _centroids(oracle, k)
    pal = torch.from_numpy(oracle.lab_to_rgba8(cent[:, :3]).view(np.int32).reshape(-1)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    rgba = torch.empty_like(d_in)
    plan = procs[0].apply_plan(cent, mode, n, st)
    plan.run(d_in.data_ptr(), 8192, 8192, 0, rgba.data_ptr(), st)
    plan.close()
    idx = torch.empty(n, dtype=torch.uint8 if fmt == FMT8 else torch.int16, device="cuda")
    plan = procs[0].apply_plan(cent, mode, n, st, format=fmt)
    plan.run(d_in.data_ptr(), 8192, 8192, 0, idx.data_ptr(), st)
    plan.close()
    torch.cuda.synchronize()
    lab = idx.long() if fmt == FMT8 else idx.long() & 0xFFFF
    assert int(lab.max()) < k
    got = pal[lab] & 0x00FFFFFF
    want = rgba.view(torch.int32).reshape(-1) & 0x00FFFFFF
    assert bool((got == want).all()), f"{int((got != want).sum())} pixels differ"


def test_find_and_reduce_indexed(torch_cuda, processor, tokyo):
    import kmeans_gpu_amd as kg
    from conftest import sorted_palette
    colors = sorted_palette("apollo-1x.png")                   # more than 8 colours: a real palette of the golden tests
    for mode in (kg.ReduceMode.Replace, kg.ReduceMode.Dither, kg.ReduceMode.Diffuse):
        idx = processor.find_indexed(tokyo, colors, mode)
        assert idx.dtype == (np.uint8 if colors.shape[0] <= 256 else np.uint16) and idx.shape == tokyo.shape[:2]
        want = processor.find(tokyo, colors, mode)
        assert np.array_equal(colors[idx][..., :3], want[..., :3]), f"find_indexed, mode {int(mode)}"
        for algo in (kg.Algorithm.Kmeans, kg.Algorithm.Octree):
            pal, idx = processor.reduce_indexed(8, tokyo, algo, mode)
            want = processor.reduce(8, tokyo, algo, mode)
            assert idx.dtype == np.uint8 and int(idx.max()) < pal.shape[0]
            assert np.array_equal(pal[idx], want), f"reduce_indexed, algo {int(algo)}, mode {int(mode)}"
            ref = processor.palette(8, tokyo, algo)
            assert sorted(map(tuple, pal)) == sorted(map(tuple, ref)), f"reduce_indexed's palette is not kmg_palette's set, algo {int(algo)}"
    # the RGBA8 format of the new calls: the bytes of the existing ones
    out = np.empty_like(tokyo)
    lib = kg.lib()
    h, w = tokyo.shape[:2]
    import ctypes as C
    assert lib.kmg_find_indexed(processor.handle, tokyo.ctypes.data, w, h, colors.ctypes.data, colors.shape[0], 1, 0,
                                out.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(out, processor.find(tokyo, colors, kg.ReduceMode.Dither))
    pal = np.empty((8, 4), np.uint8)
    cnt = C.c_uint32()
    assert lib.kmg_reduce_indexed(processor.handle, tokyo.ctypes.data, w, h, 8, 0, 0, 0, pal.ctypes.data, C.byref(cnt),
                                  out.ctypes.data_as(C.c_void_p)) == 0
    assert cnt.value == 8 and np.array_equal(out, processor.reduce(8, tokyo))


def test_reduce_indexed_alpha_mode(torch_cuda, tokyo):
    import kmeans_gpu_amd as kg
    img = tokyo.copy()
    img[::3, :, 3] = 0
    with kg.ImageProcessor(alpha_cutoff=1) as p:
        pal, idx = p.reduce_indexed(16, img, kg.Algorithm.Kmeans, kg.ReduceMode.Dither)
        want = p.reduce(16, img, kg.Algorithm.Kmeans, kg.ReduceMode.Dither)
        drop = img[..., 3] == 0
        assert np.array_equal(idx == 16, drop)
        assert np.array_equal(pal[idx[~drop]][:, :3], want[~drop][:, :3])


def test_errors(torch_cuda, processor, oracle):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    cent = _centroids(oracle, 24)
    d_in = torch.zeros((64, 4), dtype=torch.uint8, device="cuda")
    out = torch.zeros(256, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def apply(c, mode, fmt, ptr=None):
        processor.apply(d_in.data_ptr(), 8, 8, 0, c, mode, out.data_ptr() if ptr is None else ptr, st, format=fmt)

    apply(cent, 0, FMT8)                                     # (the valid call)
    for mode, fmt in ((2, FMT8), (2, FMT16)):
        with pytest.raises(kg.KmgError, match="meld"):
            apply(cent, mode, fmt)
    with pytest.raises(kg.KmgError):
        kg.ImageProcessor.apply_plan(processor, cent, 2, 64, st, format=FMT16)
    bad = cent.copy()
    bad[3, 1] = np.nan
    with pytest.raises(kg.KmgError, match="outside"):
        apply(bad, 0, FMT8)
    for j, v in ((0, 200.5), (0, -100.5), (1, 300.5), (2, -300.5), (1, np.inf)):
        bad = cent.copy()
        bad[5, j] = v
        with pytest.raises(kg.KmgError, match="outside"):
            apply(bad, 1, FMT16)
        apply(bad, 1, None)                                   # RGBA8 takes any table, as before
    corner = cent.copy()
    corner[0, :3] = (200.0, -300.0, 300.0)                    # the box itself is accepted
    apply(corner, 1, FMT8)
    with pytest.raises(kg.KmgError, match="aligned"):
        apply(cent, 0, FMT16, out.data_ptr() + 1)
    with pytest.raises(kg.KmgError):
        apply(_centroids(oracle, 300), 0, FMT8)               # k > 256 needs INDEX16
    with pytest.raises(kg.KmgError):
        apply(cent, 0, 3)                                     # no such format
    with kg.ImageProcessor(alpha_cutoff=10) as p:
        with pytest.raises(kg.KmgError, match="INDEX16"):
            p.apply(d_in.data_ptr(), 8, 8, 0, _centroids(oracle, 256), 0, out.data_ptr(), st, format=FMT8)
        p.apply(d_in.data_ptr(), 8, 8, 0, _centroids(oracle, 256), 0, out.data_ptr(), st, format=FMT16)
    torch.cuda.synchronize()


def test_dither_lists_with_equal_centroids_in_both_halves(oracle, procs):
    """A palette step with more centroids than the image has colours leaves equal centroids, and with k = 300 some pairs lie in
    different halves of the Lab lists (indices below and from 256).  A pixel whose dithered colour is exactly such a centroid has
    key 0 for both: the scan takes the first, and so must the list pass -- its packed keys then differ in the index byte alone,
    which orders the second half's index 256 (byte 0) first, and the tie threshold of a key of 0 is 0.  Found by the random sessions
    (tests/session_harness.py, surface 4: a batch of nine images at k = 300 under the forced table strategy)."""
    import kmeans_gpu_amd as kg
    rng = np.random.default_rng(11)
    pal = rng.integers(0, 256, (7, 4), dtype=np.uint8)
    img = np.ascontiguousarray(pal[rng.integers(0, 7, 50 * 80)].reshape(50, 80, 4))
    img[..., 3] = 255
    k = 300
    cent, _ = oracle.extract_palette_kmeans(img, k)
    want = oracle.dither(oracle.rgb_to_lab(img), 80, 50, cent).reshape(50, 80)
    pairs = [m for m in range(256) if (cent[256:] == cent[m]).all(axis=1).any()]
    on_a_pair = np.isin(want, pairs)
    assert pairs and on_a_pair.any() and want.max() < 256        # (not vacuous: the scan labels pixels with the first of such a pair)
    got = {}
    for strategy in ("scan", "table"):
        set_strategy(strategy)
        p, idx = procs[0].reduce_indexed(k, img, reduce_mode=kg.ReduceMode.Dither)
        assert idx.dtype == np.uint16 and p.shape == (k, 4)
        got[strategy] = idx
    assert np.array_equal(got["scan"], want)
    bad = np.flatnonzero(got["table"].reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (bad.size, bad[:4], got["table"].reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]])


# ---- every instantiation and alignment branch of the launchers at a small size ------------------------------------------------
# The route tests above leave gaps in the launchers' (format x alpha x route) products: their bands move the source and the output
# off alignment TOGETHER, and the diffusion filters other than Floyd-Steinberg meet alpha mode in RGBA8 / INDEX8 at one k only
# (tests/test_gpu_diffusion_filters.py).  Here: a 67 x 41 noise image with random alpha (2 747 pixels: no multiple of four, odd
# width, three workgroups of k_apply's 1 024-pixel tiles), the source aligned and the output at its base AND one element in (bit 0
# of the kernels' flag word 0 for the format's own vector store: 16 bytes RGBA8, 4 u8, 8 u16), k = 5 / 40 / 300 / 600 (unchunked,
# chunked, two list halves and INDEX16 only, mask words), both forced strategies, cutoff 0 and 128, every format the k admits,
# replace, dither, and diffusion under Floyd-Steinberg, Atkinson (skew 2) and Burkes (skew 3) -- against the oracle (replace,
# dither) and the diffusion references.
SW, SH = 67, 41
ATKINSON, BURKES = 2, 3
_small_want, _small_near = {}, {}


def _small_image():
    rng = np.random.default_rng(6741)
    return rng.integers(0, 256, (SH, SW, 4), dtype=np.uint8)


def _small_reference(oracle, img, cent, k, mode, f, cutoff):
    """the RGBA8 bytes of (mode, filter, cutoff), alpha = the source's in alpha mode; computed once per k"""
    import alpha_ref
    import diffuse_ref
    import diffusion_ref
    import kmeans_gpu_amd as kg
    key = (k, mode, f, cutoff)
    if key not in _small_want:
        keep = img[..., 3] >= cutoff
        if mode != 3:
            want = oracle.apply(img, cent, mode)
        else:
            if k not in _small_near:
                _small_near[k] = diffuse_ref.Nearest(diffuse_ref.oracle_apply_replace(oracle, cent))
            if f == 0:
                want = alpha_ref.diffuse(img, None, cutoff, nearest=_small_near[k]) if cutoff else diffuse_ref.diffuse(img, None, nearest=_small_near[k])
            else:
                weights, divisor = kg.diffusion_weights(f)
                want = diffusion_ref.diffuse(img, None, weights, divisor, keep=keep if cutoff else None, nearest=_small_near[k])
        if cutoff:
            want = alpha_ref.with_alpha(want, img)
        _small_want[key] = want
    return _small_want[key]


def _small_run(torch, proc, d_in, cent, mode, fmt, offset):
    """the call with the output `offset` elements into a buffer filled with 0x5A; nothing outside the image is written"""
    n = SW * SH
    if fmt is None:
        buf = torch.full((n + 8, 4), 0x5A, dtype=torch.uint8, device="cuda")
        size, view = 4, np.uint8
    else:
        buf = torch.full((n + 8,), 0x5A, dtype=torch.uint8 if fmt == FMT8 else torch.int16, device="cuda")
        size, view = (1, np.uint8) if fmt == FMT8 else (2, np.uint16)
    assert buf.data_ptr() % 16 == 0 and d_in.data_ptr() % 16 == 0
    proc.apply(d_in.data_ptr(), SW, SH, 0, cent, mode, buf.data_ptr() + size * offset, torch.cuda.current_stream().cuda_stream, format=fmt)
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(view)
    assert (host[:offset] == 0x5A).all() and (host[offset + n:] == 0x5A).all(), "written outside the image"
    return host[offset:offset + n].reshape((SH, SW, 4) if fmt is None else (SH, SW))


@pytest.mark.parametrize("strategy", ("scan", "table"))
@pytest.mark.parametrize("k", (5, 40, 300, 600))
def test_small_image_every_format_alpha_and_alignment(oracle, torch_cuda, procs, strategy, k):
    torch = torch_cuda
    set_strategy(strategy)
    img = _small_image()
    cent = _centroids(oracle, k)
    P = oracle.lab_to_rgba8(cent[:, :3])
    d_in = torch.from_numpy(img.reshape(-1, 4)).cuda()
    try:
        for mode, f in ((0, 0), (1, 0), (3, 0), (3, ATKINSON), (3, BURKES)):
            for cutoff in (0, T):
                proc = procs[cutoff]
                proc.set_diffusion(f)
                want = _small_reference(oracle, img, cent, k, mode, f, cutoff)
                keep = img[..., 3] >= cutoff
                for fmt in (None, FMT8, FMT16) if k <= 255 else (None, FMT16):
                    for offset in (0, 1):
                        got = _small_run(torch, proc, d_in, cent, mode, fmt, offset)
                        where = f"mode {mode}, filter {f}, cutoff {cutoff}, format {fmt}, output offset {offset}"
                        if fmt is None:
                            assert np.array_equal(got, want), where
                            continue
                        assert np.array_equal(got == k, ~keep), where + ": index k exactly where alpha is below the cutoff"
                        assert int(got[keep].max()) < k, where
                        assert np.array_equal(P[got[keep]][:, :3], want[keep][:, :3]), where + ": P[index] is not the reference's RGB"
    finally:
        for proc in procs.values():
            proc.set_diffusion(0)
