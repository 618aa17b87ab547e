"""KMG_MODE_DITHER with a threshold map on the device (the MapOffsets instantiations of k_apply and k_dither_lists) against the
test-side reference of the contract (tests/dither_map_ref.py), byte for byte: every built-in map and three custom ones on both
routes, in every format, with and without alpha mode; the LDS bound; bands; strengths; a workgroup that walks two tiles in each
kernel; the custom copy of the reference's matrix against the kernels of the default; the sticky rules; the refusals.

The base image is 67 x 70: the width is odd and no multiple of 4 (groups of four pixels wrap rows), wider than the widest map (x
wraps) and there are more than 64 rows (every map wraps in y).

The module has a processor of its own: the choice is sticky, and the session's processor stays at the default."""
import ctypes as C

import numpy as np
import pytest

import dither_map_ref as R

pytestmark = pytest.mark.gpu

W, H = 67, 70


@pytest.fixture(scope="module")
def dproc(torch_cuda):
    import kmeans_gpu_amd as kg
    p = kg.ImageProcessor()
    yield p
    p.close()


@pytest.fixture(autouse=True)
def _back_to_the_default(dproc):
    yield
    dproc.set_dither(0, 1.0)
    dproc.set_alpha_cutoff(0)


def _palette(k, seed):
    rng = np.random.default_rng(seed)
    pal = np.full((k, 4), 255, np.uint8)
    pal[:, :3] = rng.integers(0, 256, (k, 3))
    return pal


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _maps():
    """name -> (what set_dither takes, levels (mh, mw), n_levels)"""
    import kmeans_gpu_amd as kg
    rng = np.random.default_rng(77)
    out = {}
    for name in ("bayer2", "bayer8", "bayer16", "blue"):
        levels, n = kg.dither_map_values(name)
        out[name] = (name, levels, n)
    out["custom8x2"] = (None, rng.integers(0, 5, (2, 8)).astype(np.uint16), 5)              # 8 wide, 2 high
    out["custom1x1"] = (None, np.array([[3]], np.uint16), 7)
    out["custom64x64"] = (None, rng.integers(0, 65536, (64, 64)).astype(np.uint16), 65536)
    return out


MAP_NAMES = ["bayer2", "bayer8", "bayer16", "blue", "custom8x2", "custom1x1", "custom64x64"]


def _set(proc, entry, strength=1.0):
    what, levels, n = entry
    if what is None:
        proc.set_dither(levels, strength, levels=n)
    else:
        proc.set_dither(what, strength)


_FORMATS = {"rgba8": (None, np.uint8, 4), "index8": (1, np.uint8, 1), "index16": (2, np.uint16, 1)}


def _apply(torch, proc, host, cent, fmt, row0=0, rows=None):
    """kmg_dev_apply[_format] of rows [row0, row0 + rows) of `host` in KMG_MODE_DITHER; (rows, w[, 4]) array"""
    import kmeans_gpu_amd as kg
    h, w = host.shape[:2]
    rows = h - row0 if rows is None else rows
    format, dtype, chans = _FORMATS[fmt]
    d_in = torch.from_numpy(np.ascontiguousarray(host[row0:row0 + rows])).cuda()
    d_out = torch.zeros(rows * w * chans * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
    proc.apply(d_in.data_ptr(), w, rows, row0, cent, kg.ReduceMode.Dither, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream,
               format=None if format is None else kg.OutputFormat(format))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(dtype)
    return out.reshape(rows, w, 4) if chans == 4 else out.reshape(rows, w)


def _want(oracle, host, cent, lab, fmt, cutoff):
    k = cent.shape[0]
    if fmt == "rgba8":
        return R.rgba8(oracle, host, cent, lab, cutoff)
    return R.index_map(host, lab, k, cutoff, _FORMATS[fmt][1])


# ---- 1. every map x k x strategy x format x alpha cutoff ------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAP_NAMES)
def test_maps_on_both_routes_in_every_format_equal_the_reference(torch_cuda, dproc, oracle, name):
    import kmeans_gpu_amd as kg
    entry = _maps()[name]
    host = _noise(H, W, 6770)
    _set(dproc, entry)
    for k in (2, 8, 257):                                            # (257: the list route takes both halves)
        cent = kg.palette_to_centroids(_palette(k, 31 * k))
        lab = R.labels(oracle, host, cent, entry[1], entry[2])
        for cutoff in (0, 128):
            dproc.set_alpha_cutoff(cutoff)
            for fmt in ("rgba8", "index8", "index16"):
                if fmt == "index8" and k > 255:
                    continue
                outs = {}
                for strategy in ("scan", "table"):                   # (table: the candidate lists at any size)
                    kg.set_strategy(strategy)                        # (back to auto after every test: conftest)
                    outs[strategy] = _apply(torch_cuda, dproc, host, cent, fmt)
                assert np.array_equal(outs["scan"], outs["table"]), (k, cutoff, fmt)
                assert np.array_equal(outs["scan"], _want(oracle, host, cent, lab, fmt, cutoff)), (k, cutoff, fmt)


# ---- 2. k = 1 is replace -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bayer8", "blue", "custom8x2"])
def test_one_colour_is_the_replace_output(torch_cuda, dproc, oracle, name):
    import kmeans_gpu_amd as kg
    host, pal = _noise(H, W, 11), _palette(1, 5)
    _set(dproc, _maps()[name], 2.0)
    for strategy in ("scan", "table"):
        kg.set_strategy(strategy)
        got = dproc.find(host, pal, kg.ReduceMode.Dither)
        assert np.array_equal(got, dproc.find(host, pal, kg.ReduceMode.Replace))
        assert np.array_equal(got, oracle.find(host, pal, oracle.MODE_REPLACE))


# ---- 3. the LDS bound: k = KMG_MAX_K with the 64 x 64 map ---------------------------------------------------------------------------
def test_largest_k_with_the_largest_map_scans_under_every_strategy(torch_cuda, dproc, oracle):
    """48 KiB of centroids + 1 KiB + 16 KiB of offsets: above the 64 KiB every device has.  TABLE (k > 512: the mask words) and
    MASK_WORDS must fall back to the scan"""
    import kmeans_gpu_amd as kg
    entry = _maps()["custom64x64"]
    host = _noise(H, W, 3072)
    cent = kg.palette_to_centroids(_palette(3072, 3072))
    _set(dproc, entry)
    lab = R.labels(oracle, host, cent, entry[1], entry[2])
    for strategy in ("scan", "table", "scan+mask_words", "table+mask_words", "mask_words"):
        kg.set_strategy(strategy)
        for fmt in ("rgba8", "index16"):
            assert np.array_equal(_apply(torch_cuda, dproc, host, cent, fmt), _want(oracle, host, cent, lab, fmt, 0)), (strategy, fmt)
    # MASK_WORDS sends every k to the mask words: a small k under it scans as well
    cent8 = kg.palette_to_centroids(_palette(8, 8))
    kg.set_strategy("table+mask_words")
    assert np.array_equal(_apply(torch_cuda, dproc, host, cent8, "index8"), R.labels(oracle, host, cent8, entry[1], entry[2]).astype(np.uint8))


# ---- 4. bands of one plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["scan", "table"])
def test_bands_of_one_plan_equal_the_whole_image(torch_cuda, dproc, oracle, strategy):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    kg.set_strategy(strategy)
    host = _noise(H, W, 404)
    cent = kg.palette_to_centroids(_palette(24, 24))
    st = torch.cuda.current_stream().cuda_stream
    img = torch.from_numpy(host.reshape(-1, 4)).cuda()
    for name in ("bayer16", "blue", "custom8x2"):
        entry = _maps()[name]
        _set(dproc, entry)
        whole = _apply(torch, dproc, host, cent, "index8")
        assert np.array_equal(whole, R.labels(oracle, host, cent, entry[1], entry[2]).astype(np.uint8))
        out = torch.zeros(H * W, dtype=torch.uint8, device="cuda")
        plan = dproc.apply_plan(cent, kg.ReduceMode.Dither, H * W, st, format=kg.OutputFormat.Index8)
        for r0, r1 in ((0, 3), (3, 37), (37, 70)):                  # row0 = 3 and 37: no multiple of any map height but 1
            plan.run(img[r0 * W:].data_ptr(), W, r1 - r0, r0, out[r0 * W:].data_ptr(), st)
        torch.cuda.synchronize()
        plan.close()
        assert np.array_equal(out.cpu().numpy().reshape(H, W), whole), name
        # kmg_dev_apply_format on a band of its own
        assert np.array_equal(_apply(torch, dproc, host, cent, "index8", 37, 33), whole[37:]), name


# ---- 5. strength -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strength", [0.0, 0.5, 2.0])
def test_strengths_equal_the_reference(torch_cuda, dproc, oracle, strength):
    import kmeans_gpu_amd as kg
    host = _noise(H, W, 55)
    cent = kg.palette_to_centroids(_palette(8, 88))
    labs = []
    for name in ("bayer8", "blue"):
        entry = _maps()[name]
        _set(dproc, entry, strength)
        lab = R.labels(oracle, host, cent, entry[1], entry[2], strength)
        labs.append(lab)
        for strategy in ("scan", "table"):
            kg.set_strategy(strategy)
            assert np.array_equal(_apply(torch_cuda, dproc, host, cent, "index8"), lab.astype(np.uint8)), (name, strategy)
    # the reference's matrix at another strength runs the map instantiations too
    dproc.set_dither("bayer4", strength)
    lab4 = R.labels(oracle, host, cent, R.BAYER4, 16, strength)
    for strategy in ("scan", "table"):
        kg.set_strategy(strategy)
        assert np.array_equal(_apply(torch_cuda, dproc, host, cent, "index8"), lab4.astype(np.uint8)), strategy
    if strength == 0.0:                                              # no offset: every map gives the same labels
        assert np.array_equal(labs[0], labs[1]) and np.array_equal(labs[0], lab4)


# ---- 6. a workgroup that walks two tiles ---------------------------------------------------------------------------------------------------
# k_apply: the grid is capped at 2048 workgroups of 256 threads x 8 pixels (kApplyGridCap, kmg_kernels.hip), so some workgroup
# takes a second tile from 2048 * 2048 + 1 = 4 194 305 pixels on; 2049 x 2048 = 4 196 352 is the smallest image of odd width 2049
# above that (2049 tiles).  k_dither_lists: 8192 workgroups of 256 x 4 pixels (kDitherListsGridCap, kmg_lists.hip), a second tile
# from 8192 * 1024 + 1 = 8 388 609 pixels on; 2049 x 4095 = 8 390 655 is the smallest of that width (8194 tiles).  A map and the
# default choice are instantiations of the same two kernels behind the same two launchers: both walk.
@pytest.mark.parametrize("strategy,w,h,choice", [pytest.param("scan", 2049, 2048, "blue", id="scan-2049-2048"),
                                                 pytest.param("table", 2049, 4095, "blue", id="table-2049-4095"),
                                                 pytest.param("scan", 2049, 2048, "default", id="scan-2049-2048-default"),
                                                 pytest.param("table", 2049, 4095, "default", id="table-2049-4095-default")])
def test_a_workgroup_walks_two_tiles(torch_cuda, dproc, oracle, strategy, w, h, choice):
    import kmeans_gpu_amd as kg
    tile = 2048 if strategy == "scan" else 1024
    cap = 2048 if strategy == "scan" else 8192
    assert (w * h + tile - 1) // tile > cap >= ((w * (h - 1)) + tile - 1) // tile and w % 2 == 1
    kg.set_strategy(strategy)
    host = _noise(h, w, w + h)
    cent = kg.palette_to_centroids(_palette(8, 808))
    if choice == "default":
        dproc.set_dither(0, 1.0)
        want = oracle.dither(oracle.rgb_to_lab(host), w, h, cent).reshape(h, w).astype(np.uint8)
    else:
        entry = _maps()[choice]
        _set(dproc, entry)
        want = R.labels(oracle, host, cent, entry[1], entry[2]).astype(np.uint8)
    got = _apply(torch_cuda, dproc, host, cent, "index8")
    assert np.array_equal(got, want)


# ---- 7. the custom copy of the reference's matrix through the map instantiations = the default through the Bayer ones ---------------------------
@pytest.mark.parametrize("strategy", ["scan", "table"])
def test_custom_copy_of_the_reference_matrix_equals_a_fresh_default_processor(torch_cuda, dproc, oracle, strategy):
    import kmeans_gpu_amd as kg
    kg.set_strategy(strategy)
    host = _noise(H, W, 707)
    with kg.ImageProcessor() as fresh:
        for k in (2, 8, 257):
            cent = kg.palette_to_centroids(_palette(k, 7 * k))
            for cutoff in (0, 128):
                fresh.set_alpha_cutoff(cutoff)
                dproc.set_alpha_cutoff(cutoff)
                for fmt in ("rgba8", "index16"):
                    dproc.set_dither(0, 1.0)
                    old = _apply(torch_cuda, fresh, host, cent, fmt)
                    assert np.array_equal(_apply(torch_cuda, dproc, host, cent, fmt), old)          # the default choice: the Bayer instantiations
                    dproc.set_dither(R.BAYER4, 1.0, levels=16)
                    assert dproc.dither_map == kg.DitherMap.Custom
                    assert np.array_equal(_apply(torch_cuda, dproc, host, cent, fmt), old), (k, cutoff, fmt)
            lab = oracle.dither(oracle.rgb_to_lab(host), W, H, cent).reshape(H, W)
            assert np.array_equal(_apply(torch_cuda, dproc, host, cent, "index16"), R.index_map(host, lab, k, 128, np.uint16))


# ---- 8. sticky rules ---------------------------------------------------------------------------------------------------------------------
def test_a_plan_keeps_the_map_it_was_made_under(torch_cuda, dproc, oracle):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    host = _noise(H, W, 808)
    cent = kg.palette_to_centroids(_palette(12, 12))
    img = torch.from_numpy(host.reshape(-1, 4)).cuda()
    out = torch.zeros(H * W, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dproc.set_dither(kg.DitherMap.Bayer8)
    plan = dproc.apply_plan(cent, kg.ReduceMode.Dither, H * W, st, format=kg.OutputFormat.Index8)
    plan.run(img.data_ptr(), W, 30, 0, out.data_ptr(), st)
    dproc.set_dither(0)                                              # the plan keeps Bayer 8
    assert dproc.dither_map == kg.DitherMap.Bayer4 and dproc.dither_strength == 1.0
    plan.run(img[30 * W:].data_ptr(), W, H - 30, 30, out[30 * W:].data_ptr(), st)
    torch.cuda.synchronize()
    plan.close()
    levels, n = kg.dither_map_values("bayer8")
    assert np.array_equal(out.cpu().numpy().reshape(H, W), R.labels(oracle, host, cent, levels, n).astype(np.uint8))
    lab0 = oracle.dither(oracle.rgb_to_lab(host), W, H, cent).reshape(H, W)
    assert np.array_equal(_apply(torch, dproc, host, cent, "index8"), lab0.astype(np.uint8))
    with kg.ImageProcessor(dither_map="bayer8", dither_strength=1.0) as p2:   # the constructor's arguments are the same switch
        assert p2.dither_map == kg.DitherMap.Bayer8
        assert np.array_equal(_apply(torch, p2, host, cent, "index8"), out.cpu().numpy().reshape(H, W))


def test_the_other_modes_ignore_the_choice(dproc):
    import kmeans_gpu_amd as kg
    img, pal = _noise(40, 50, 31), _palette(10, 31)
    modes = (kg.ReduceMode.Replace, kg.ReduceMode.Meld, kg.ReduceMode.Diffuse)
    before = [dproc.find(img, pal, m) for m in modes]
    dproc.set_dither("blue", 3.0)
    for m, b in zip(modes, before):
        assert np.array_equal(dproc.find(img, pal, m), b), int(m)


def test_host_calls_follow_the_processor(torch_cuda, dproc, oracle):
    """find against the reference; reduce, reduce_indexed, reduce_quality and reduce_indexed_batch against each other, against the
    default (they must differ) and -- the palette step does not read the choice, so the centroids are the same -- under the custom
    copy of the reference's matrix (the map instantiations) against the default (the Bayer instantiations), which they must equal"""
    import kmeans_gpu_amd as kg
    D = kg.ReduceMode.Dither
    k = 6
    images = [_noise(40 + 7 * i, 61 - 4 * i, 900 + i) for i in range(3)]
    pal = _palette(k, 66)
    levels, n = kg.dither_map_values("bayer8")

    def calls():
        out = {"reduce": [dproc.reduce(k, im, reduce_mode=D) for im in images],
               "indexed": [dproc.reduce_indexed(k, im, reduce_mode=D) for im in images],
               "quality": [dproc.reduce_quality(im, 1.0, k, k, D, indexed=True) for im in images],
               "batch": dproc.reduce_indexed_batch(k, images, reduce_mode=D)}
        return out

    default = calls()
    dproc.set_dither("bayer8")
    for im in images:
        cent = kg.palette_to_centroids(pal)
        want = R.rgba8(oracle, im, cent, R.labels(oracle, im, cent, levels, n))
        assert np.array_equal(dproc.find(im, pal, D), want)
        assert np.array_equal(pal[dproc.find_indexed(im, pal, D)][..., :3], want[..., :3])
    mapped = calls()
    dproc.set_dither(R.BAYER4, 1.0, levels=16)
    copied = calls()
    for i in range(3):
        colors, index = mapped["indexed"][i]
        assert np.array_equal(colors[index][..., :3], mapped["reduce"][i][..., :3])
        assert np.array_equal(mapped["batch"][i][0], colors) and np.array_equal(mapped["batch"][i][1], index)
        assert mapped["quality"][i][0] == k and np.array_equal(mapped["quality"][i][2], index)
        assert not np.array_equal(index, default["indexed"][i][1])
        assert np.array_equal(copied["reduce"][i], default["reduce"][i])
        assert np.array_equal(copied["indexed"][i][1], default["indexed"][i][1])
        assert np.array_equal(copied["quality"][i][2], default["quality"][i][2])
        assert np.array_equal(copied["batch"][i][1], default["batch"][i][1])
    assert dproc.last_batch_apply_report.per_image == 3 and dproc.last_batch_apply_report.batched == 0


def test_an_open_sequence_output_keeps_its_map(torch_cuda, dproc, oracle):
    """every frame's map is kmg_dev_apply_format with the sequence's centroids under the map the output was opened with, whatever the
    processor says later; a clip of eight 32 x 32 frames equals the single frames; per-frame palettes likewise"""
    import kmeans_gpu_amd as kg
    h = w = 32
    k = 12
    frames = [_noise(h, w, 600 + t) for t in range(8)]
    for fr in frames:
        fr[..., 3] = 255
    entry = _maps()["blue"]
    _set(dproc, entry)
    with dproc.sequence() as seq:
        for fr in frames:
            seq.add(fr)
        cent = seq.centroids(k)
        seq.output(k, kg.ReduceMode.Dither, kg.OutputFormat.Index8, w, h)
        want = [R.labels(oracle, fr, cent, entry[1], entry[2]).astype(np.uint8) for fr in frames]
        assert np.array_equal(_apply(torch_cuda, dproc, frames[0], cent, "index8"), want[0])
        dproc.set_dither("bayer2", 0.5)                              # the open output keeps the blue-noise map
        for fr, I in zip(frames, want):
            got, _, full = seq.frame(fr, delta=False)
            assert full and np.array_equal(got, I)
        clip = seq.frames(frames, delta=False)
        for (got, _, full), I in zip(clip, want):
            assert full and np.array_equal(got, I)
        assert seq.last_clip_report.per_image == 8 and seq.last_clip_report.batched == 0

    def local_maps(opened_under, switched_to):
        dproc.set_dither(opened_under)
        with dproc.sequence() as seq:
            seq.output_local(k, kg.ReduceMode.Dither, kg.OutputFormat.Index8, w, h)
            dproc.set_dither(switched_to)
            return [seq.frame_local(fr, delta=False)[0] for fr in frames[:2]]
    kept, plain, other = local_maps("blue", "bayer2"), local_maps("blue", "blue"), local_maps("bayer2", "bayer2")
    assert all(np.array_equal(a, b) for a, b in zip(kept, plain))
    assert not all(np.array_equal(a, b) for a, b in zip(kept, other))


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(torch_cuda, dproc, oracle):
    import kmeans_gpu_amd as kg
    L = kg.lib()
    host = _noise(H, W, 99)
    cent = kg.palette_to_centroids(_palette(8, 99))
    dproc.set_dither("bayer16", 1.5)
    levels, n = kg.dither_map_values("bayer16")
    want = R.labels(oracle, host, cent, levels, n, 1.5).astype(np.uint8)
    assert np.array_equal(_apply(torch_cuda, dproc, host, cent, "index8"), want)
    ok = np.zeros((4, 4), np.uint16)
    ptr = ok.ctypes.data_as(C.POINTER(C.c_uint16))
    f = C.c_float
    refused = [
        lambda: L.kmg_processor_set_dither(None, 1, f(1.0)),
        lambda: L.kmg_processor_set_dither(dproc.handle, -1, f(1.0)),
        lambda: L.kmg_processor_set_dither(dproc.handle, 6, f(1.0)),
        lambda: L.kmg_processor_set_dither(dproc.handle, int(kg.DitherMap.Custom), f(1.0)),
        lambda: L.kmg_processor_set_dither(dproc.handle, 1, f(-0.5)),
        lambda: L.kmg_processor_set_dither(dproc.handle, 1, f(4.5)),
        lambda: L.kmg_processor_set_dither(dproc.handle, 1, f(float("nan"))),
        lambda: L.kmg_processor_set_dither(dproc.handle, 1, f(float("inf"))),
        lambda: L.kmg_processor_set_dither_custom(None, ptr, 4, 4, 16, f(1.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, None, 4, 4, 16, f(1.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, ptr, 0, 4, 16, f(1.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, ptr, 4, 0, 16, f(1.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, ptr, 3, 4, 16, f(1.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, ptr, 4, 12, 16, f(1.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, ptr, 128, 1, 16, f(1.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, ptr, 1, 128, 16, f(1.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, ptr, 4, 4, 0, f(1.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, ptr, 4, 4, 65537, f(1.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, ptr, 4, 4, 16, f(5.0)),
        lambda: L.kmg_processor_set_dither_custom(dproc.handle, ptr, 4, 4, 16, f(float("nan"))),
    ]
    for i, call in enumerate(refused):
        assert call() == -1, i
        assert len(L.kmg_last_error()) > 0
        assert np.array_equal(_apply(torch_cuda, dproc, host, cent, "index8"), want), i
    bad = np.zeros((4, 4), np.uint16)
    bad[3, 2] = 16                                                   # a level that is not below n_levels
    assert L.kmg_processor_set_dither_custom(dproc.handle, bad.ctypes.data_as(C.POINTER(C.c_uint16)), 4, 4, 16, f(1.0)) == -1
    assert np.array_equal(_apply(torch_cuda, dproc, host, cent, "index8"), want)
    for call in (lambda: dproc.set_dither("bayer3"), lambda: dproc.set_dither(np.zeros(4, np.uint16)), lambda: dproc.set_dither(np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            call()
    assert dproc.dither_map == kg.DitherMap.Bayer16 and dproc.dither_strength == 1.5
    assert np.array_equal(_apply(torch_cuda, dproc, host, cent, "index8"), want)
    # the largest n_levels and the largest level are accepted
    top = np.full((1, 2), 65535, np.uint16)
    dproc.set_dither(top, 1.0, levels=65536)
    assert np.array_equal(_apply(torch_cuda, dproc, host, cent, "index8"), R.labels(oracle, host, cent, top, 65536).astype(np.uint8))


def test_a_group_refuses_a_member_whose_choice_is_not_the_default(torch_cuda, oracle):
    import kmeans_gpu_amd as kg
    img, pal = _noise(40, 50, 41), _palette(6, 41)
    with kg.Group(devices=[0]) as group:
        want = group.find(img, pal, kg.ReduceMode.Dither)
        assert np.array_equal(want, oracle.find(img, pal, oracle.MODE_DITHER))
        member = group.processor(0)
        member.set_dither("bayer8")
        for call in (lambda: group.find(img, pal, kg.ReduceMode.Dither), lambda: group.reduce(6, img, reduce_mode=kg.ReduceMode.Dither),
                     lambda: group.reduce_batch(6, [img, img], reduce_mode=kg.ReduceMode.Dither)):
            with pytest.raises(kg.KmgError) as e:
                call()
            assert e.value.status == -1 and "dither" in str(e.value)
        # the other modes do not read the choice
        assert np.array_equal(group.find(img, pal, kg.ReduceMode.Replace), oracle.find(img, pal, oracle.MODE_REPLACE))
        member.set_dither(R.BAYER4, 1.0, levels=16)                   # a custom copy of the default is not the default
        with pytest.raises(kg.KmgError):
            group.find(img, pal, kg.ReduceMode.Dither)
        member.set_dither(0, 1.0)
        assert np.array_equal(group.find(img, pal, kg.ReduceMode.Dither), want)
