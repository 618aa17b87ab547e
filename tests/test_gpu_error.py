"""Error statistics and the quality-targeted colour count on the device (include/kmeans_hip.h at kmg_error_stats).
Every comparison is exact, integer for integer, against the model tests/error_ref.py (the oracle's Lab, numpy integers).

  - kmg_dev_compare on random images: 1 x 1, odd widths, bands that start at odd pixel offsets (the one-load-per-pixel paths),
    4096^2; every field for what = RGB, LAB and both; RGBA8 / INDEX8 / INDEX16 with k in {1, 2, 255, 256, 3072}; cutoffs 0, 1,
    128, 255 with random alpha; planted invalid indices; a record that already holds values (the combination rule, the fields of a
    part that is not requested); row bands on two streams into one record.
  - kmg_compare on the outputs of reduce, find and reduce_indexed, all four modes, alpha mode on and off.
  - kmg_reduce_quality: the three tokyo.png cases of tests/test_error_contract.py, an image that is not shrunk, alpha mode, E(k)
    through public calls only, both strategies; output, palette and count against reduce_indexed(k*).
  - one 8192^2 run: reduce_indexed at k = 256 in dither mode, then compare."""
import ctypes as C

import numpy as np
import pytest

import alpha_ref
import error_ref as R
from conftest import set_strategy
from test_error_contract import tokyo_cases

pytestmark = pytest.mark.gpu

RGBA8, INDEX8, INDEX16 = 0, 1, 2
_SIZE = {RGBA8: 4, INDEX8: 1, INDEX16: 2}


@pytest.fixture(scope="module")
def procs(torch_cuda):
    import kmeans_gpu_amd as kg
    ps = {0: kg.ImageProcessor(), 128: kg.ImageProcessor(alpha_cutoff=128), "raw": kg.ImageProcessor(shrink_max_dim=0)}
    yield ps
    for p in ps.values():
        p.close()


def _to_device(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a.reshape(-1)).cuda()


def _record(d_stats):
    return tuple(int(v) for v in d_stats.cpu().numpy().view(np.uint64))


def _dev(torch, proc, src, out, fmt, pal, cutoff, what, prior=None):
    d_src, d_out = _to_device(torch, src), _to_device(torch, out)
    d_stats = torch.from_numpy(np.array(prior if prior is not None else R.ZERO, np.uint64).view(np.int64)).cuda()
    proc.compare_device(d_src.data_ptr(), d_out.data_ptr(), src.reshape(-1, 4).shape[0], d_stats.data_ptr(), fmt, pal, cutoff, what,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return _record(d_stats)


def _case(rng, n, fmt, k, cutoff, plant=True):
    """(src (n, 4), out, palette or None): random pixels with random alpha, a share of them unchanged; index forms: the transparent
    slot on uncounted pixels and -- where the format has room above k -- planted invalid indices on counted ones"""
    src = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    if fmt == RGBA8:
        out = rng.integers(0, 256, (n, 4), dtype=np.uint8)
        same = rng.random(n) < 0.3
        out[same, :3] = src[same, :3]
        return src, out, None
    pal = rng.integers(0, 256, (k, 4), dtype=np.uint8)
    dtype = np.uint8 if fmt == INDEX8 else np.uint16
    idx = rng.integers(0, k, n).astype(dtype)
    same = rng.random(n) < 0.3
    src[same, :3] = pal[idx[same].astype(np.int64)][:, :3]
    top = 256 if fmt == INDEX8 else 65536
    if k < top:
        idx[src[:, 3] < cutoff] = k
        if plant:
            bad = rng.random(n) < 0.05
            idx[bad] = rng.integers(k, top, int(bad.sum())).astype(dtype)
    return src, idx, pal


def _ks(fmt, cutoff):
    if fmt == RGBA8:
        return (0,)
    if fmt == INDEX8:
        return (1, 2, 255) + ((256,) if cutoff == 0 else ())
    return (1, 2, 255, 256, 3072)


@pytest.mark.parametrize("what", [R.RGB, R.LAB, R.RGB | R.LAB])
@pytest.mark.parametrize("fmt", [RGBA8, INDEX8, INDEX16])
def test_compare_device_random(oracle, torch_cuda, procs, fmt, what):
    rng = np.random.default_rng(100 * fmt + what)
    for n in (1, 7, 143, 3 * 1001, 1024, 257 * 129):
        for cutoff in (0, 1, 128, 255):
            for k in _ks(fmt, cutoff):
                src, out, pal = _case(rng, n, fmt, k, cutoff)
                want = R.stats(oracle, src, out, palette=pal, cutoff=cutoff, what=what)
                got = _dev(torch_cuda, procs[0], src, out, fmt, pal, cutoff, what)
                assert got == want, (n, cutoff, k, dict(zip(R.FIELDS, zip(got, want))))
                if fmt != RGBA8 and k < (256 if fmt == INDEX8 else 65536) and n >= 1024 and cutoff <= 128:
                    assert want[2] > 0
    # a record that already holds values: sums are added, maxima are maxed, the fields of the other part are left alone
    src, out, pal = _case(rng, 5000, fmt, 200, 64)
    prior = tuple(int(v) for v in rng.integers(1, 1 << 40, 14))
    model = R.stats(oracle, src, out, palette=pal, cutoff=64, what=what)
    got = _dev(torch_cuda, procs[0], src, out, fmt, pal, 64, what, prior=prior)
    assert got == R.combine(prior, model)
    if what == R.RGB:
        assert got[12:] == prior[12:]
    if what == R.LAB:
        assert got[3:12] == prior[3:12]


@pytest.mark.parametrize("fmt", [RGBA8, INDEX8, INDEX16])
def test_unaligned_bands_on_two_streams(oracle, torch_cuda, procs, fmt):
    """row bands of a 1001-pixel-wide image start at odd pixel offsets: both pointers are then unaligned for the vector loads; the
    bands accumulate into one record from two streams, in either order, and give the whole image's"""
    torch = torch_cuda
    rng = np.random.default_rng(7 + fmt)
    w, h, k, cutoff = 1001, 301, 256 if fmt != INDEX8 else 255, 100
    src, out, pal = _case(rng, w * h, fmt, k, cutoff)
    whole = R.stats(oracle, src, out, palette=pal, cutoff=cutoff)
    assert _dev(torch, procs[0], src, out, fmt, pal, cutoff, 3) == whole
    d_src, d_out = _to_device(torch, src), _to_device(torch, out)
    rows = [0, 1, 38, 39, 140, 277, 301]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for order in (range(len(rows) - 1), reversed(range(len(rows) - 1))):
        d_stats = torch.zeros(14, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for j, i in enumerate(order):
            p0, p1 = rows[i] * w, rows[i + 1] * w
            procs[0].compare_device(d_src.data_ptr() + 4 * p0, d_out.data_ptr() + _SIZE[fmt] * p0, p1 - p0, d_stats.data_ptr(), fmt, pal,
                                    cutoff, 3, streams[j % 2].cuda_stream)
        torch.cuda.synchronize()
        assert _record(d_stats) == whole
    # a band that starts one pixel in, on its own: the model of that range
    got = torch.zeros(14, dtype=torch.int64, device="cuda")
    procs[0].compare_device(d_src.data_ptr() + 4, d_out.data_ptr() + _SIZE[fmt], w * h - 1, got.data_ptr(), fmt, pal, cutoff, 3,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _record(got) == R.stats(oracle, src[1:], out[1:], palette=pal, cutoff=cutoff)


@pytest.mark.parametrize("fmt,k,cutoff", [(RGBA8, 0, 0), (INDEX8, 256, 0), (INDEX16, 3072, 128)])
def test_compare_device_4096_squared(oracle, torch_cuda, procs, fmt, k, cutoff):
    rng = np.random.default_rng(40 + fmt)
    src, out, pal = _case(rng, 4096 * 4096, fmt, k, cutoff)
    want = R.stats(oracle, src, out, palette=pal, cutoff=cutoff)
    got = _dev(torch_cuda, procs[0], src, out, fmt, pal, cutoff, 3)
    assert got == want, dict(zip(R.FIELDS, zip(got, want)))
    assert want[0] > 1 << 22 and want[12] > 1 << 40


@pytest.mark.parametrize("n", [2048 * 1024 - 1, 2048 * 1024 + 1, 2049 * 1024 + 3])
def test_compare_device_at_its_grid_edges(oracle, torch_cuda, procs, n):
    """the partition of the tiles into the workgroups' runs where it is uneven: 2048 tiles with a ragged last one (one each); 2049
    tiles (two per workgroup: 1024 full runs, one of a single ragged tile, 1023 empty ones); 2050 tiles, the last one ragged"""
    rng = np.random.default_rng(n)
    src, out, pal = _case(rng, n, INDEX8, 255, 128)
    want = R.stats(oracle, src, out, palette=pal, cutoff=128)
    got = _dev(torch_cuda, procs[0], src, out, INDEX8, pal, 128, R.RGB | R.LAB)
    assert got == want, dict(zip(R.FIELDS, zip(got, want)))
    assert want[0] > n // 4 and want[2] > 0


def test_refusals_on_the_device(torch_cuda, procs):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    pal = np.zeros((256, 4), np.uint8)
    for kwargs in (dict(what=0), dict(what=4), dict(alpha_cutoff=256), dict(format=INDEX8, palette=pal, alpha_cutoff=1),
                   dict(format=INDEX8), dict(format=7)):
        with pytest.raises(kg.KmgError) as e:
            procs[0].compare_device(d.data_ptr(), d.data_ptr() + 256, 8, d.data_ptr() + 384, **kwargs)
        assert e.value.status == -1
    with pytest.raises(kg.KmgError) as e:                     # the record is 8-byte aligned
        procs[0].compare_device(d.data_ptr(), d.data_ptr() + 256, 8, d.data_ptr() + 388)
    assert e.value.status == -1
    torch.cuda.synchronize()
    assert int(d.abs().sum()) == 0


# ---- kmg_compare on what the library itself writes --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def disc(tokyo):
    return alpha_ref.soft_disc(np.ascontiguousarray(tokyo))


@pytest.mark.parametrize("t", [0, 128])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_compare_on_library_outputs(oracle, procs, disc, mode, t):
    import kmeans_gpu_amd as kg
    proc = procs[t]
    pal = np.array(sorted(set(map(tuple, oracle.synth_uniform(31, 12)))), np.uint8)
    for out in (proc.reduce(9, disc, reduce_mode=mode), proc.find(disc, pal, mode)):
        got = proc.compare(disc, out)
        assert got.as_tuple() == R.stats(oracle, disc, out, cutoff=t)
        assert got.pixels == int((disc[..., 3] >= t).sum()) and got.changed > 0
        for what in (R.RGB, R.LAB):
            assert proc.compare(disc, out, what=what).as_tuple() == R.stats(oracle, disc, out, cutoff=t, what=what)
    if mode != 2:
        colours, index = proc.reduce_indexed(9, disc, reduce_mode=mode)
        got = proc.compare(disc, index, palette=colours)
        want = R.stats(oracle, disc, index, palette=colours, cutoff=t)
        assert got.as_tuple() == want and want[2] == 0
        # ... which is the record of the RGBA8 output of the same call
        assert want == R.stats(oracle, disc, proc.reduce(9, disc, reduce_mode=mode), cutoff=t)
        index = proc.find_indexed(disc, pal, mode)
        assert proc.compare(disc, index, palette=pal).as_tuple() == R.stats(oracle, disc, index, palette=pal, cutoff=t)
        assert isinstance(got, kg.ErrorStats) and got.psnr > 10 and got.delta_e_rms > 0


# ---- kmg_reduce_quality ------------------------------------------------------------------------------------------------------------
def _reduce_quality(proc, img, k_min, k_max, target, mode, fmt):
    """the C call with an integer target: (k, palette, output, record, reached)"""
    import kmeans_gpu_amd as kg
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    out = np.empty((h, w, 4), np.uint8) if fmt == RGBA8 else np.empty((h, w), np.uint8 if fmt == INDEX8 else np.uint16)
    pal = np.zeros((k_max, 4), np.uint8)
    cnt, reached, stats = C.c_uint32(), C.c_int(-1), kg.ErrorStats()
    rc = kg.lib().kmg_reduce_quality(proc.handle, C.c_void_p(img.ctypes.data), w, h, k_min, k_max, int(target), mode, fmt,
                                     C.c_void_p(pal.ctypes.data), C.byref(cnt), C.c_void_p(out.ctypes.data), C.byref(stats), C.byref(reached))
    assert rc == 0, kg.lib().kmg_last_error()
    return int(cnt.value), pal[:cnt.value].copy(), out, stats.as_tuple(), reached.value


def _check_search(proc, img, W, k_min, k_max, target, modes=((0, INDEX8), (1, INDEX8), (3, RGBA8))):
    want_k, want_reached, want_rec, _ = W.search(k_min, k_max, target)
    for mode, fmt in modes:
        k, pal, out, rec, reached = _reduce_quality(proc, img, k_min, k_max, target, mode, fmt)
        assert (k, reached) == (want_k, int(want_reached)), (k, reached, want_k, want_reached)
        assert rec == want_rec, dict(zip(R.FIELDS, zip(rec, want_rec)))
        assert np.array_equal(pal, W.record(k)[1])
        if fmt == RGBA8:
            ref_pal, _ = proc.reduce_indexed(k, img, reduce_mode=0)
            ref_out = proc.reduce(k, img, reduce_mode=mode)
        else:
            ref_pal, ref_out = proc.reduce_indexed(k, img, reduce_mode=mode)
        assert out.dtype == ref_out.dtype and np.array_equal(out, ref_out) and np.array_equal(pal, ref_pal)
    return want_k, want_reached, want_rec


def test_reduce_quality_tokyo(oracle, procs, tokyo):
    W = R.Working(oracle, tokyo)
    got = {name: _check_search(procs[0], tokyo, W, 2, 64, target) for name, target in tokyo_cases(W)}
    assert 2 < got["interior"][0] < 64 and got["interior"][1]
    assert got["not_reached"][:2] == (64, False)
    assert got["k_min"][:2] == (2, True)


def test_reduce_quality_python_wrapper(oracle, procs, tokyo):
    W = R.Working(oracle, tokyo)
    de = 4.5
    target = int(np.floor(4096.0 * de * de))
    want_k, want_reached, want_rec, _ = W.search(2, 32, target)
    k, colours, index, stats, reached = procs[0].reduce_quality(tokyo, de, k_min=2, k_max=32, reduce_mode=1, indexed=True)
    assert (k, reached, stats.as_tuple()) == (want_k, want_reached, want_rec)
    ref_pal, ref_idx = procs[0].reduce_indexed(k, tokyo, reduce_mode=1)
    assert np.array_equal(colours, ref_pal) and np.array_equal(index, ref_idx) and index.dtype == np.uint8
    k2, colours2, image, stats2, reached2 = procs[0].reduce_quality(tokyo, de, k_min=2, k_max=32, reduce_mode=2)
    assert (k2, reached2, stats2.as_tuple()) == (k, reached, stats.as_tuple()) and np.array_equal(colours2, colours)
    assert np.array_equal(image, procs[0].reduce(k, tokyo, reduce_mode=2))
    if reached:
        assert stats.delta_e_rms <= de


def test_reduce_quality_without_shrink(oracle, procs, tokyo):
    img = np.ascontiguousarray(tokyo[120:320, 200:440])
    assert max(img.shape[:2]) <= 256
    W = R.Working(oracle, img, shrink_max_dim=0)
    assert W.n == 200 * 240
    for _, target in tokyo_cases(W):
        _check_search(procs["raw"], img, W, 2, 64, target, modes=((0, INDEX8), (1, RGBA8)))
    # W is the image itself: `achieved` is the record of the full output in replace mode
    k, pal, out, rec, _ = _reduce_quality(procs["raw"], img, 2, 64, tokyo_cases(W)[0][1], 0, INDEX8)
    assert rec == procs["raw"].compare(img, out, palette=pal).as_tuple()


def test_reduce_quality_alpha_mode(oracle, procs, disc):
    W = R.Working(oracle, disc, cutoff=128)
    assert W.h == 1 and W.n < 256 * 171
    for _, target in tokyo_cases(W):
        k, _, rec = _check_search(procs[128], disc, W, 2, 64, target)
        assert rec[0] == W.n
    # a wider search in INDEX16, the transparent slot above 255 colours
    target = tokyo_cases(W)[0][1]
    want_k, want_reached, want_rec, _ = W.search(1, 300, target)
    k, pal, out, rec, reached = _reduce_quality(procs[128], disc, 1, 300, target, 0, INDEX16)
    assert (k, reached, rec) == (want_k, int(want_reached), want_rec)
    ref_pal, ref_out = procs[128].reduce_indexed(k, disc, reduce_mode=0)
    assert np.array_equal(pal, ref_pal) and np.array_equal(out.astype(np.uint16), ref_out.astype(np.uint16))


@pytest.mark.parametrize("t", [0, 128])
def test_E_through_public_calls_only(oracle, torch_cuda, procs, disc, t):
    """W from kmg_dev_resize and kmg_dev_alpha_compact, C_k and the labels from kmg_reduce_indexed in replace mode on W (a processor
    without shrink and without alpha mode), E(k) from kmg_compare: the record kmg_reduce_quality reports"""
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    h, w = disc.shape[:2]
    sw, sh = kg.resized_dims(w, h)
    st = torch.cuda.current_stream().cuda_stream
    d_img = torch.from_numpy(disc.reshape(-1)).cuda()
    d_small = torch.zeros(sw * sh * 4, dtype=torch.uint8, device="cuda")
    procs[0].resize(d_img.data_ptr(), w, h, sw, sh, d_small.data_ptr(), st)
    if t:
        d_kept = torch.zeros(sw * sh * 4, dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        procs[0].alpha_compact(d_small.data_ptr(), sw * sh, t, d_kept.data_ptr(), d_n.data_ptr(), st)
        torch.cuda.synchronize()
        n = int(d_n.cpu()[0])
        assert 0 < n < sw * sh
        Wimg = d_kept.cpu().numpy()[:4 * n].reshape(1, n, 4)
    else:
        torch.cuda.synchronize()
        Wimg = d_small.cpu().numpy().reshape(sh, sw, 4)
    model = R.Working(oracle, disc, cutoff=t)
    assert np.array_equal(Wimg.reshape(-1, 4), model.px)
    target = tokyo_cases(model)[0][1]
    k, pal, _, rec, reached = _reduce_quality(procs[t], disc, 2, 64, target, 0, INDEX8)
    pal_w, idx_w = procs["raw"].reduce_indexed(k, Wimg, reduce_mode=0)
    assert np.array_equal(pal_w, pal)
    got = procs["raw"].compare(Wimg, idx_w, palette=pal_w)
    assert got.as_tuple() == rec and reached == int(got.lab_sse <= target * model.n)


def test_both_strategies_give_identical_results(oracle, procs, tokyo, disc):
    W = R.Working(oracle, tokyo)
    target = tokyo_cases(W)[0][1]
    got = {}
    for strategy in ("scan", "table"):
        set_strategy(strategy)
        k, pal, out, rec, reached = _reduce_quality(procs[0], tokyo, 2, 64, target, 1, INDEX8)
        cmp_idx = procs[0].compare(tokyo, out, palette=pal).as_tuple()
        cmp_rgba = procs[128].compare(disc, procs[128].reduce(7, disc, reduce_mode=3)).as_tuple()
        got[strategy] = (k, pal.tobytes(), out.tobytes(), rec, reached, cmp_idx, cmp_rgba)
    assert got["scan"] == got["table"]
    assert got["scan"][3] == W.search(2, 64, target)[2]


def test_full_size_dither_then_compare(oracle, torch_cuda, tokyo):
    """8192^2 tiled photograph: reduce_indexed at k = 256 in dither mode, then compare against the model evaluated in chunks"""
    import kmeans_gpu_amd as kg
    big = np.ascontiguousarray(np.tile(tokyo, (16, 11, 1))[:8192, :8192])
    with kg.ImageProcessor() as proc:
        colours, index = proc.reduce_indexed(256, big, reduce_mode=1)
        assert index.dtype == np.uint8 and colours.shape == (256, 4)
        got = proc.compare(big, index, palette=colours)
    want = R.stats(oracle, big, index, palette=colours)
    assert got.as_tuple() == want, dict(zip(R.FIELDS, zip(got.as_tuple(), want)))
    assert want[0] == 8192 * 8192 and want[2] == 0 and 20.0 < got.psnr < 60.0
