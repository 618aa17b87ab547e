"""Alpha-weighted k-means on the device (include/kmeans_hip.h at kmg_processor_set_weighting / kmg_lloyd_set_weighting), bit for bit
against tests/weight_ref.py:
  1. the weighted sums of every per-pixel route (k_assign at 1 / 2 / 4 / 8 pixels per thread, plain and chunked scan, unaligned
     loads; the two-step partial sums; the fused update), with the labels of an unweighted object;
  2. the loops: the one-launch-per-iteration kernel of small images, the per-pixel loop with fused updates, and the latter after an
     initialisation that bound the image;
  3. the host-buffer calls against the model: palette, reduce, reduce_indexed at t = 0 and 128, fixed colours, sequences,
     per-frame palettes cold and warm, the quality search, and the default bytes after the weighting is taken back;
  4. the refusals, with the objects usable afterwards;
  5. the sums at the bound: 2^28 pixels made on the device, sums between 2^62 and 2^63 against exact integer arithmetic."""
import numpy as np
import pytest

import alpha_ref
import diffuse_ref
import error_ref
import fixed_ref
import weight_ref as W
from conftest import set_strategy

pytestmark = pytest.mark.gpu

PINS = np.array([[0, 0, 0, 255], [200, 30, 30, 255]], np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pixels(n, seed):
    """n RGBA8 pixels: noise, then flat runs of 1 .. 40 pixels; random alpha that includes 0 and 255 (inside the runs too)"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    half = n // 2
    runs = rng.integers(1, 41, n - half)
    colours = rng.integers(0, 256, (runs.shape[0], 3), dtype=np.uint8)
    px[half:, :3] = np.repeat(colours, runs, axis=0)[:n - half]
    px[::7, 3] = 0
    px[3::11, 3] = 255
    return px


_problems = {}


def _problem(oracle, n, k):
    """(pixels, Lab, centroids, labels, weighted sums) of one case, computed once"""
    if (n, k) not in _problems:
        if ("px", n) not in _problems:
            px = _pixels(n, n)
            lab = oracle.rgb_to_lab(px)
            _problems[("px", n)] = (px, lab, W.pixel_q(oracle, lab))
        px, lab, q = _problems[("px", n)]
        cent = oracle.centroids4(lab[np.linspace(0, n - 1, k).astype(int)])
        labels = oracle.assign(lab, cent)
        _problems[(n, k)] = (px, lab, cent, labels, W.accumulate(q, px[:, 3], labels, k))
    return _problems[(n, k)]


class _Dev:
    def __init__(self, torch, px, k, offset=0):
        """offset = 1: the pixels start 4 bytes into their buffer (the unaligned loads of k_assign)"""
        self.torch = torch
        self.n = px.shape[0]
        self.st = torch.cuda.current_stream().cuda_stream
        words = np.zeros(self.n + offset, np.uint32)
        words[offset:] = np.ascontiguousarray(px).view(np.uint32).reshape(-1)
        self.buf = torch.from_numpy(words.view(np.int32)).cuda()
        self.ptr = self.buf.data_ptr() + 4 * offset
        self.labels = torch.zeros(self.n, dtype=torch.int32, device="cuda")
        self.acc = torch.zeros((k, 4), dtype=torch.int64, device="cuda")

    def lab(self):
        self.torch.cuda.synchronize()
        return self.labels.cpu().numpy().view(np.uint32)

    def sums(self):
        self.torch.cuda.synchronize()
        return self.acc.cpu().numpy()


# the smallest pixel count of each pixels-per-thread class of k_assign plus a ragged tail; k = 8: plain scan, k = 40: chunked scan
@pytest.mark.parametrize("k", [8, 40])
@pytest.mark.parametrize("n", [1000, (1 << 19) + 3, (1 << 20) + 3, (1 << 21) + 5])
def test_sums_by_route(torch_cuda, processor, oracle, n, k):
    import kmeans_gpu_amd as kg
    px, lab, cent, labels, want = _problem(oracle, n, k)
    assert px[:, 3].min() == 0 and px[:, 3].max() == 255
    assert not np.array_equal(want, oracle.accumulate(lab, labels, k))
    want_cent, want_conv = oracle.finalize(want, cent)
    set_strategy("table")                                            # (whatever the strategy says: weighted sums scan the pixels)
    s, u = kg.Lloyd(processor, k), kg.Lloyd(processor, k)
    try:
        s.set_weighting(kg.WEIGHT_ALPHA)
        for offset in (0, 1):
            d = _Dev(torch_cuda, px, k, offset)
            s.set_centroids(cent, d.st)
            assert s.prepare(d.ptr, n, True, d.st) == "scan"
            s.assign_accumulate(d.ptr, n, d.labels.data_ptr(), d.acc.data_ptr(), d.st)
            assert np.array_equal(d.sums(), want), offset
            assert np.array_equal(d.lab(), labels), offset
        # the labels do not depend on the weights: those of an unweighted object, whose sums are the default ones
        got_labels = d.lab().copy()
        u.set_centroids(cent, d.st)
        d.labels.zero_(); d.acc.zero_()
        u.assign_accumulate(d.ptr, n, d.labels.data_ptr(), d.acc.data_ptr(), d.st)
        assert np.array_equal(d.lab(), got_labels) and np.array_equal(d.sums(), oracle.accumulate(lab, labels, k))
        # sums only (no label map), and the two halves
        d.acc.zero_()
        s.assign_accumulate(d.ptr, n, 0, d.acc.data_ptr(), d.st)
        assert np.array_equal(d.sums(), want)
        d.acc.zero_(); d.labels.zero_()
        s.assign_partials(d.ptr, n, d.labels.data_ptr(), d.st)
        s.reduce_partials(n, d.acc.data_ptr(), d.st)
        assert np.array_equal(d.sums(), want) and np.array_equal(d.lab(), labels)
        # the fused update reads the weighted sums
        d.acc.zero_()
        s.assign_update(d.ptr, n, d.labels.data_ptr(), d.acc.data_ptr(), True, d.st)
        assert np.array_equal(d.sums(), want)
        assert np.array_equal(_bits(s.get_centroids(d.st)[:, :3]), _bits(want_cent[:, :3]))
        assert s.converged_count(d.st) == want_conv
        # iterate: update first (from the sums in place), then the weighted sums of the new assignment
        s.set_centroids(cent, d.st)
        s.iterate(d.ptr, n, d.labels.data_ptr(), d.acc.data_ptr(), True, d.st)
        s.flush(d.st)
        labels2 = oracle.assign(lab, want_cent)
        assert np.array_equal(d.lab(), labels2)
        assert np.array_equal(d.sums(), W.accumulate(_problems[("px", n)][2], px[:, 3], labels2, k))
        # back to unit weights: the default sums again
        s.set_weighting(kg.WEIGHT_NONE)
        s.set_centroids(cent, d.st)
        d.acc.zero_()
        s.assign_accumulate(d.ptr, n, 0, d.acc.data_ptr(), d.st)
        assert np.array_equal(d.sums(), oracle.accumulate(lab, labels, k))
    finally:
        s.close()
        u.close()


@pytest.fixture(scope="module")
def sprite_working(oracle):
    px, w, h = W.working_pixels(oracle, W.weighted_sprite(), 0)
    return np.ascontiguousarray(px)


@pytest.mark.parametrize("k", [4, 8, 16, 40])
def test_run_small_image_loop(torch_cuda, processor, oracle, sprite_working, k):
    """the compaction of the weighted sprite: the single-launch loop (k = 40: its chunked variant)"""
    import kmeans_gpu_amd as kg
    px = sprite_working
    lab = oracle.rgb_to_lab(px)
    cent0 = oracle.init_centroids(lab, px.shape[0], 1, k)
    want, want_labels, want_it = W.lloyd(oracle, lab, px[:, 3], cent0)
    plain, _, _ = oracle.lloyd(lab, cent0)
    assert not np.array_equal(_bits(want), _bits(plain))
    d = _Dev(torch_cuda, px, k)
    s = kg.Lloyd(processor, k)
    try:
        s.set_weighting(kg.WEIGHT_ALPHA)
        s.init_centroids(d.ptr, d.n, 1, d.st)                          # unweighted, unchanged
        assert np.array_equal(_bits(s.get_centroids(d.st)[:, :3]), _bits(cent0[:, :3]))
        it = s.run(d.ptr, d.n, d.labels.data_ptr(), d.st)
        assert it == want_it
        assert np.array_equal(_bits(s.get_centroids(d.st)[:, :3]), _bits(want[:, :3]))
        assert np.array_equal(d.lab(), want_labels)
    finally:
        s.close()


def test_run_per_pixel_loop_and_dropped_binding(torch_cuda, oracle):
    """2^19 + 3 pixels, nine iterations: the loop of assign passes with fused updates; then the same problem from an initialisation
    that ran over the colour table and left the image bound -- the weighted loop drops that binding instead of inheriting it"""
    import kmeans_gpu_amd as kg
    n, k = (1 << 19) + 3, 8
    px, lab, _, _, _ = _problem(oracle, n, k)
    cent0 = oracle.init_centroids(lab, n, 1, k)
    want, want_labels, want_it = W.lloyd(oracle, lab, px[:, 3], cent0, max_iterations=9)
    plain, _, _ = oracle.lloyd(lab, cent0, max_iterations=9)
    assert not np.array_equal(_bits(want), _bits(plain))
    d = _Dev(torch_cuda, px, k)
    with kg.ImageProcessor(max_iterations=9) as proc:
        s = kg.Lloyd(proc, k)
        try:
            s.set_weighting(kg.WEIGHT_ALPHA)
            for strategy in ("scan", "table"):
                proc.set_strategy(strategy)
                s.init_centroids(d.ptr, n, 1, d.st)
                assert np.array_equal(_bits(s.get_centroids(d.st)[:, :3]), _bits(cent0[:, :3])), strategy
                d.labels.zero_()
                it = s.run(d.ptr, n, d.labels.data_ptr(), d.st)
                assert it == want_it, strategy
                assert np.array_equal(_bits(s.get_centroids(d.st)[:, :3]), _bits(want[:, :3])), strategy
                assert np.array_equal(d.lab(), want_labels), strategy
                assert s.prepare(d.ptr, n, True, d.st) == "scan"
        finally:
            s.close()


# ---- the host-buffer calls ------------------------------------------------------------------------------------------------------
@pytest.fixture()
def wproc(torch_cuda):
    import kmeans_gpu_amd as kg
    p = kg.ImageProcessor(alpha_weight=True)
    yield p
    p.close()


def _big():
    """300 x 210, shrunk to 256 x 179 first: the weights are the alpha AFTER the shrink"""
    rng = np.random.default_rng(77)
    img = rng.integers(0, 256, (210, 300, 4), dtype=np.uint8)
    img[::2, :, :3] //= 3
    img[60:150, 80:220, 3] = 0
    return img


IMAGES = {"sprite": W.weighted_sprite, "big": _big}


def _expected_output(oracle, img, cent, mode, t):
    """the output step is unchanged: alpha mode's at t, the default one at t = 0 (alpha 255)"""
    if t:
        return alpha_ref.apply(oracle, img, cent, int(mode), t)
    if int(mode) == alpha_ref.MODE_DIFFUSE:
        return diffuse_ref.diffuse(img, diffuse_ref.oracle_apply_replace(oracle, cent))
    return oracle.apply(img, cent, int(mode))


def _sorted_palette(oracle, cent):
    pal = np.full((cent.shape[0], 4), 255, np.uint8)
    for j in range(cent.shape[0]):
        pal[j, :3] = oracle.palette_lab_to_srgb8(cent[j, :3])
    return alpha_ref.sorted_by_L(oracle, pal)


@pytest.mark.parametrize("name,k", [("sprite", 8), ("sprite", 40), ("big", 6)])
@pytest.mark.parametrize("t", [0, 128])
def test_palette_reduce_and_reduce_indexed(wproc, oracle, name, k, t):
    import kmeans_gpu_amd as kg
    img = IMAGES[name]()
    wproc.set_alpha_cutoff(t)
    cent = W.kmeans_centroids(oracle, img, k, t)
    unweighted = alpha_ref.kmeans_centroids(oracle, img, k, max(t, 1))
    assert not np.array_equal(_bits(cent), _bits(unweighted))
    assert np.array_equal(wproc.palette(k, img), _sorted_palette(oracle, cent))
    keep = img[..., 3] >= t
    for mode in (kg.ReduceMode.Replace, kg.ReduceMode.Dither, kg.ReduceMode.Diffuse):
        want = _expected_output(oracle, img, cent, mode, t)
        assert np.array_equal(wproc.reduce(k, img, reduce_mode=mode), want), mode
        pal, index = wproc.reduce_indexed(k, img, reduce_mode=mode)
        assert np.array_equal(pal, fixed_ref.palette_bytes(oracle, cent)), mode
        assert np.array_equal(pal[index[keep]][:, :3], want[keep][:, :3]) and (index[~keep] == k).all(), mode
    # the strategy switch changes nothing: weighted sums always scan the pixels
    wproc.set_strategy("table")
    assert np.array_equal(wproc.palette(k, img), _sorted_palette(oracle, cent))
    wproc.set_strategy("auto")
    # the weighting taken back: the default bytes again
    wproc.set_alpha_weight(False)
    if t:
        assert np.array_equal(wproc.reduce(k, img), alpha_ref.reduce_kmeans(oracle, img, k, oracle.MODE_REPLACE, t))
    else:
        assert np.array_equal(wproc.reduce(k, img), oracle.reduce(img, k, oracle.MODE_REPLACE))


@pytest.mark.parametrize("t", [0, 128])
def test_fixed_colours(wproc, oracle, t):
    img = W.weighted_sprite()
    k = 7
    wproc.set_alpha_cutoff(t)
    wproc.set_fixed_colors(PINS)
    cent = W.kmeans_centroids(oracle, img, k, t, colours=PINS)
    assert np.array_equal(_bits(cent[:2]), _bits(fixed_ref.pins_lab(oracle, PINS)))
    pal, index = wproc.reduce_indexed(k, img)
    assert np.array_equal(pal, fixed_ref.palette_bytes(oracle, cent)) and np.array_equal(pal[:2, :3], PINS[:, :3])
    keep = img[..., 3] >= t
    assert np.array_equal(pal[index[keep]][:, :3], _expected_output(oracle, img, cent, 0, t)[keep][:, :3])
    assert np.array_equal(wproc.palette(k, img), _sorted_palette(oracle, cent))


def test_sequence(wproc, oracle):
    """two frames of different sizes; the weighting in force at an add decides the frame's cutoff, the one in force at the palette
    call whether the loop is weighted"""
    import kmeans_gpu_amd as kg
    k = 6
    a = W.weighted_sprite()
    b = np.ascontiguousarray(W.weighted_sprite(seed=12)[5:60, 10:71])
    for t in (0, 128):
        wproc.set_alpha_weight(True)
        wproc.set_alpha_cutoff(t)
        with wproc.sequence() as seq:
            seq.add(a); seq.add(b)
            cent = W.sequence_centroids(oracle, [a, b], [max(t, 1)] * 2, k)
            assert seq.info()[1] == int((a[..., 3] >= max(t, 1)).sum() + (b[..., 3] >= max(t, 1)).sum())
            assert np.array_equal(_bits(seq.centroids(k)[:, :3]), _bits(cent[:, :3])), t
            assert np.array_equal(seq.palette(k), _sorted_palette(oracle, cent)), t
            pal = seq.output(k, kg.ReduceMode.Replace, kg.OutputFormat.Index8, a.shape[1], a.shape[0])
            assert np.array_equal(pal, fixed_ref.palette_bytes(oracle, cent)), t
            index, _, _ = seq.frame(a, delta=False)
            keep = a[..., 3] >= t
            assert np.array_equal(pal[index[keep]][:, :3], _expected_output(oracle, a, cent, 0, t)[keep][:, :3]), t
            seq.end_output()
            # the loop unweighted on the same W: alpha mode's sequence at the adds' cutoff
            wproc.set_alpha_weight(False)
            px = np.concatenate([alpha_ref.compact(a, max(t, 1)), alpha_ref.compact(b, max(t, 1))])
            lab = oracle.rgb_to_lab(px)
            plain, _, _ = oracle.lloyd(lab, oracle.init_centroids(lab, px.shape[0], 1, k))
            assert np.array_equal(_bits(seq.centroids(k)[:, :3]), _bits(plain[:, :3])), t
    # a frame added without weighting at t = 0 keeps its pixels of weight 0: in W, in the initialisation, and nothing in the sums
    wproc.set_alpha_cutoff(0)
    wproc.set_alpha_weight(False)
    with wproc.sequence() as seq:
        seq.add(a)
        wproc.set_alpha_weight(True)
        seq.add(b)
        assert seq.info()[1] == a.shape[0] * a.shape[1] + int((b[..., 3] >= 1).sum())
        cent = W.sequence_centroids(oracle, [a, b], [0, 1], k)
        assert np.array_equal(_bits(seq.centroids(k)[:, :3]), _bits(cent[:, :3]))


@pytest.mark.parametrize("warm", [False, True])
def test_per_frame_palettes(wproc, oracle, warm):
    import kmeans_gpu_amd as kg
    k, t = 6, 0
    base = W.weighted_sprite()
    frames = [base, np.roll(base, 7, axis=1), np.roll(base, 5, axis=0)]
    frames[2][..., :3] = 255 - frames[2][..., :3]
    h, w = base.shape[:2]
    with wproc.sequence() as seq:
        seq.output_local(k, kg.ReduceMode.Replace, kg.OutputFormat.Index8, w, h, warm=warm)
        prev = None
        for i, f in enumerate(frames):
            warm4 = None
            if warm and prev is not None:
                warm4 = np.ones((k, 4), np.float32)
                warm4[:, :3] = prev[:, :3]
            cent = W.kmeans_centroids(oracle, f, k, t, warm4=warm4)
            index, pal, _, _ = seq.frame_local(f, delta=False)
            assert np.array_equal(pal, fixed_ref.palette_bytes(oracle, cent)), (warm, i)
            assert np.array_equal(pal[index][..., :3], oracle.apply(f, cent, oracle.MODE_REPLACE)[..., :3]), (warm, i)
            prev = cent
        seq.end_output()


class _WeightedWorking(error_ref.Working):
    """the model of kmg_reduce_quality under weighting: W cut at max(t, 1), the weighted palette at every k, the UNWEIGHTED record"""

    def centroids(self, k):
        return W.centroids_of_working(self.oracle, self.px, self.w, self.h, k)[0]


def test_reduce_quality(wproc, oracle):
    img = W.weighted_sprite()
    work = _WeightedWorking(oracle, img, W.cutoff(0))
    # a target between the model's errors at 6 and 5 colours, so that the bisection has to find its way
    target = (work.E(6) + work.E(5)) // (2 * work.n)
    delta_e = float(np.sqrt((target + 0.5) / 4096.0))
    assert int(np.floor(4096.0 * delta_e * delta_e)) == target
    want_k, want_reached, want_rec, _ = work.search(2, 16, target)
    k, pal, index, stats, reached = wproc.reduce_quality(img, delta_e, k_min=2, k_max=16, indexed=True)
    assert (k, reached) == (want_k, want_reached)
    assert np.array_equal(pal, work.record(k)[1])
    assert stats.as_tuple() == want_rec
    want_pal, want_index = wproc.reduce_indexed(k, img)
    assert np.array_equal(pal, want_pal) and np.array_equal(index, want_index)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_processor_refusals(wproc, oracle):
    import kmeans_gpu_amd as kg
    L = kg.lib()
    img = W.weighted_sprite()
    for bad in (2, -1, 255):
        assert L.kmg_processor_set_weighting(wproc.handle, bad) == -1
    for call in (lambda: wproc.palette(8, img, kg.Algorithm.Octree), lambda: wproc.reduce(8, img, kg.Algorithm.Octree),
                 lambda: wproc.reduce_indexed(8, img, kg.Algorithm.Octree)):
        with pytest.raises(kg.KmgError) as e:
            call()
        assert e.value.status == -1
    out = np.full(img.shape, 0xA5, np.uint8)
    with pytest.raises(kg.KmgError):
        wproc.reduce(8, img, algo=kg.Algorithm.Octree, out=out)
    assert (out == 0xA5).all()                                       # nothing written
    # no pixel is kept: alpha mode's error, at t = 0 too
    none = img.copy()
    none[..., 3] = 0
    for call in (lambda: wproc.palette(4, none), lambda: wproc.reduce(4, none, out=out), lambda: wproc.reduce_indexed(4, none)):
        with pytest.raises(kg.KmgError) as e:
            call()
        assert e.value.status == -1
    assert (out == 0xA5).all()
    # the refused value left the weighting on, and the processor works
    cent = W.kmeans_centroids(oracle, img, 5, 0)
    assert np.array_equal(wproc.reduce_indexed(5, img)[0], fixed_ref.palette_bytes(oracle, cent))
    # find takes the caller's palette: untouched; octree works again once the weighting is off
    assert np.array_equal(wproc.find(img, PINS), oracle.find(img, PINS, oracle.MODE_REPLACE))
    wproc.set_alpha_weight(False)
    assert np.array_equal(wproc.palette(8, img, kg.Algorithm.Octree), oracle.palette_octree(img, 8))
    # the group layer has no weighted sums
    with kg.Group(devices=[0]) as group:
        member = group.processor(0)
        opaque = img.copy()
        opaque[..., 3] = 255
        member.set_alpha_weight(True)
        for call in (lambda: group.palette(4, opaque), lambda: group.reduce(4, opaque), lambda: group.reduce_batch(4, [opaque])):
            with pytest.raises(kg.KmgError) as e:
                call()
            assert e.value.status == -1
        member.set_alpha_weight(False)
        assert np.array_equal(group.reduce(4, opaque), oracle.reduce(opaque, 4, oracle.MODE_REPLACE))


def test_lloyd_refusals(torch_cuda, processor, oracle):
    import kmeans_gpu_amd as kg
    L = kg.lib()
    n, k = (1 << 19) + 3, 8
    px, lab, cent, labels, want = _problem(oracle, n, k)
    d = _Dev(torch_cuda, px, k)
    s = kg.Lloyd(processor, k)
    try:
        for bad in (2, -1):
            assert L.kmg_lloyd_set_weighting(s._h, bad) == -1
        s.set_centroids(cent, d.st)
        # a caller's binding: the weighting cannot change under it
        set_strategy("table")
        assert s.prepare(d.ptr, n, True, d.st) == "table"
        with pytest.raises(kg.KmgError) as e:
            s.set_weighting(kg.WEIGHT_ALPHA)
        assert e.value.status == -1
        s.assign_accumulate(d.ptr, n, 0, d.acc.data_ptr(), d.st)
        assert np.array_equal(d.sums(), oracle.accumulate(lab, labels, k))       # still unweighted, still bound
        s.unbind_image()
        s.set_weighting(kg.WEIGHT_ALPHA)
        # a weighted object has no colour-table route
        for call in (lambda: s.bind_image(d.ptr, n, d.st), lambda: s.set_cell_share(0, 2, d.st),
                     lambda: s.accumulate_into(d.ptr, n, d.acc.data_ptr(), d.st),
                     lambda: s.labels_from_tables_update(d.ptr, n, d.labels.data_ptr(), d.acc.data_ptr(), d.st)):
            with pytest.raises(kg.KmgError) as e:
                call()
            assert e.value.status == -1
        assert s.prepare(d.ptr, n, True, d.st) == "scan"
        # ... and works
        d.acc.zero_()
        s.assign_accumulate(d.ptr, n, d.labels.data_ptr(), d.acc.data_ptr(), d.st)
        assert np.array_equal(d.sums(), want) and np.array_equal(d.lab(), labels)
        # unweighted again: the caller may bind again
        s.set_weighting(kg.WEIGHT_NONE)
        s.bind_image(d.ptr, n, d.st)
        d.acc.zero_()
        s.assign_accumulate(d.ptr, n, 0, d.acc.data_ptr(), d.st)
        assert np.array_equal(d.sums(), oracle.accumulate(lab, labels, k))
    finally:
        s.close()


# ---- the sums at the bound ----------------------------------------------------------------------------------------------------------
N_BOUND = 1 << 28
TILE = 4093                                                          # prime: every repetition meets the 4-pixel groups at another phase


def _bound_problem(oracle):
    """the host side of test_sums_at_the_pixel_bound, no device needed: 64 RGBA words, a tile of TILE indices into them in runs of
    1 .. 5, and -- the image being the tile repeated, cut at N_BOUND -- the per-colour counts in closed form:
    count_c = (N_BOUND // TILE) (occurrences of c in the tile) + (occurrences in its first N_BOUND % TILE entries).
    About 70 % of the pixels are opaque near-whites, 25 % opaque pure green (what is left of 72 % and 24 % of the runs once
    neighbours must differ), the rest 55 random colours with alpha bytes that
    include 0, 1, 2, 127, 128, 254 and 255."""
    rng = np.random.default_rng(228)
    pal = rng.integers(0, 256, (64, 4), dtype=np.uint8)
    pal[:8, :3] = 255 - rng.integers(0, 3, (8, 3))
    pal[0, :3] = 255
    pal[:9, 3] = 255
    pal[8, :3] = (0, 255, 0)
    pal[9:16, 3] = (0, 1, 2, 127, 128, 254, 255)
    runs = rng.integers(1, 6, TILE)
    colour, other = [], 0
    for r in rng.random(TILE):
        while True:                                                  # (neighbours differ, so that no two runs make a longer one)
            c = int(rng.integers(0, 8)) if r < 0.72 else 8 if r < 0.96 else 9 + other % 55
            if not colour or c != colour[-1]:
                break
            r = rng.random()
        other += c > 8                                               # the 55 others in turn: each of them is there
        colour.append(c)
    tile = np.repeat(colour, runs)[:TILE].astype(np.int64)
    reps, tail = divmod(N_BOUND, TILE)
    counts = reps * np.bincount(tile, minlength=64).astype(object) + np.bincount(tile[:tail], minlength=64).astype(object)
    assert sum(counts) == N_BOUND
    lab = oracle.rgb_to_lab(pal)
    q = W.pixel_q(oracle, lab)
    problem = dict(pal=pal, tile=tile, counts=counts, lab=lab)
    for k, rows in ((8, [0, 8, 9, 10, 11, 12, 13, 14]), (40, list(range(40)))):
        cent = oracle.centroids4(lab[rows])
        labels = oracle.assign(lab, cent)
        sums = [[0, 0, 0, 0] for _ in range(k)]                      # exact Python integers
        for c in range(64):
            a = int(pal[c, 3])
            for j in range(3):
                sums[labels[c]][j] += int(counts[c]) * a * int(q[c, j])
            sums[labels[c]][3] += int(counts[c]) * a
        problem[k] = (cent, labels, sums)
    return problem


def _bound_feasible(P):
    """what the palette of _bound_problem must give, asserted on the expected values before any launch (and, without a device, by
    tests/test_weight_contract.py): a sum of a qL of at least 2^62, a sum of a qa or a qb of at most -2^60, every |sum| below 2^63,
    weights 0, 1 and 255 present"""
    sums = P[8][2]
    flat = [v for row in sums for v in row]
    print("largest sum 2^%.3f, lowest -2^%.3f" % (np.log2(float(max(flat))), np.log2(float(-min(flat)))))
    assert max(row[0] for row in sums) >= 1 << 62
    assert min(min(row[1], row[2]) for row in sums) <= -(1 << 60)
    assert all(abs(v) < (1 << 63) for v in flat) and all(abs(v) < (1 << 63) for row in P[40][2] for v in row)
    assert {0, 1, 255} <= set(P["pal"][np.unique(P["tile"]), 3].tolist())


def test_sums_at_the_pixel_bound(torch_cuda, processor, oracle):
    """2^28 pixels exactly, the most a weighted pass takes: sums between 2^62 and 2^63 and below -2^60 through the int64 run
    registers, the unsigned 64-bit LDS bins, the partial slabs and the double division of the update, bit for bit against exact
    integer arithmetic; one pixel more is KMG_ERR_UNSUPPORTED and touches nothing.  The pixels are made on the device (a tile
    broadcast into the buffer); the counts are in closed form (_bound_problem).  1 GiB of pixels, 1 GiB of labels."""
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    P = _bound_problem(oracle)
    n, pal, tile = N_BOUND, P["pal"], P["tile"]
    cent, labels_of, sums = P[8]
    _bound_feasible(P)
    want = np.array(sums, np.int64)
    want_cent, want_conv = oracle.finalize(want, cent)

    st = torch.cuda.current_stream().cuda_stream
    words = torch.from_numpy(np.ascontiguousarray(pal).view(np.uint32).reshape(-1).astype(np.int64)).cuda().to(torch.int32)
    tile_words = words[torch.from_numpy(tile).cuda()]
    reps, tail = divmod(n, TILE)
    buf = torch.empty(n + 1, dtype=torch.int32, device="cuda")      # one pixel more than the bound, for the refusal
    buf[:reps * TILE].view(reps, TILE).copy_(tile_words.expand(reps, TILE))
    buf[reps * TILE:n] = tile_words[:tail]
    buf[n] = words[0]                                                # opaque white: a pass that read it would show in every sum
    labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    acc = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    tile_labels = torch.from_numpy(labels_of.astype(np.int64)).cuda().to(torch.int32)[torch.from_numpy(tile).cuda()]

    def got():
        torch.cuda.synchronize()
        return acc.cpu().numpy()

    s = kg.Lloyd(processor, 8)
    try:
        s.set_weighting(kg.WEIGHT_ALPHA)
        s.set_centroids(cent, st)
        s.assign_accumulate(buf.data_ptr(), n, 0, acc.data_ptr(), st)
        assert np.array_equal(got(), want)
        # one pixel more: refused before anything is enqueued, the sums buffer untouched, the object usable
        acc.fill_(0x5A5A5A5A5A5A5A5A)
        for call in (lambda: s.assign_accumulate(buf.data_ptr(), n + 1, 0, acc.data_ptr(), st), lambda: s.run(buf.data_ptr(), n + 1, 0, st)):
            with pytest.raises(kg.KmgError) as e:
                call()
            assert e.value.status == -5
        assert (got() == 0x5A5A5A5A5A5A5A5A).all()
        assert np.array_equal(_bits(s.get_centroids(st)), _bits(cent))
        # the two halves, with the label map
        acc.zero_()
        s.assign_partials(buf.data_ptr(), n, labels.data_ptr(), st)
        s.reduce_partials(n, acc.data_ptr(), st)
        assert np.array_equal(got(), want)
        assert bool((labels[:reps * TILE].view(reps, TILE) == tile_labels).all()) and bool((labels[reps * TILE:] == tile_labels[:tail]).all())
        # the fused update: the double division of sums far above 2^53
        acc.zero_()
        s.assign_update(buf.data_ptr(), n, 0, acc.data_ptr(), True, st)
        assert np.array_equal(got(), want)
        assert np.array_equal(_bits(s.get_centroids(st)[:, :3]), _bits(want_cent[:, :3]))
        assert s.converged_count(st) == want_conv
    finally:
        s.close()
    # the chunked scan: sums only
    cent40, _, sums40 = P[40]
    acc = torch.zeros((40, 4), dtype=torch.int64, device="cuda")
    s = kg.Lloyd(processor, 40)
    try:
        s.set_weighting(kg.WEIGHT_ALPHA)
        s.set_centroids(cent40, st)
        s.assign_accumulate(buf.data_ptr(), n, 0, acc.data_ptr(), st)
        assert np.array_equal(got(), np.array(sums40, np.int64))
    finally:
        s.close()
