"""Fixed palette colours on the device (include/kmeans_hip.h at kmg_processor_set_fixed_colors, kmg_lloyd_init_centroids_seeded,
kmg_lloyd_set_fixed), bit for bit against tests/fixed_ref.py:
  1. the seeded initialisation: shapes around the block of 16 and the workgroup, ties, a pin equal to an image colour, duplicate
     pins, f below / at / above the multi-pick width and f = k, k across the cube-pass shapes, both routes (pixels, colour cells);
  2. every update route with n_fixed set: update, assign_update, iterate + flush, run, labels_from_tables_update;
  3. end to end: palette, reduce_indexed in three modes, reduce_quality, alpha mode, a sequence across clear, the refusals."""
import numpy as np
import pytest

import alpha_ref
import diffuse_ref
import fixed_ref as R
from conftest import set_strategy

pytestmark = pytest.mark.gpu

PINS = np.array([[0, 0, 0, 255], [255, 255, 255, 255], [200, 30, 30, 7], [200, 30, 30, 255], [12, 200, 90, 255], [0, 0, 0, 0],
                 [40, 80, 160, 255], [250, 240, 10, 255]], np.uint8)                 # (entries 2 / 3 and 0 / 5: duplicates)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _two_colours(w, h):
    img = np.empty((h, w, 4), np.uint8)
    img[...] = (30, 60, 200, 255)
    img.reshape(-1, 4)[1::3] = (220, 210, 40, 255)
    return img


def _flat(w, h):
    img = np.empty((h, w, 4), np.uint8)
    img[...] = (90, 120, 30, 255)
    return img


_cache = {}


def _model_init(oracle, name, img, k, seeds4):
    key = (name, k, seeds4.tobytes())
    if key not in _cache:
        h, w = img.shape[:2]
        _cache[key] = R.init_centroids(oracle, oracle.rgb_to_lab(img), w, h, k, seeds4)
    return _cache[key]


class _Dev:
    def __init__(self, torch, img, k):
        self.torch = torch
        self.h, self.w = img.shape[:2]
        self.n = self.h * self.w
        self.k = k
        self.st = torch.cuda.current_stream().cuda_stream
        self.px = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).cuda()
        self.labels = torch.zeros(self.n, dtype=torch.int32, device="cuda")
        self.acc = torch.zeros((k, 4), dtype=torch.int64, device="cuda")

    def lab(self):
        return self.labels.cpu().numpy().view(np.uint32)


def _gpu_init(torch, processor, img, k, seeds4, strategy="scan"):
    import kmeans_gpu_amd as kg
    set_strategy(strategy)
    d = _Dev(torch, img, k)
    s = kg.Lloyd(processor, k)
    try:
        s.init_centroids_seeded(d.px.data_ptr(), d.w, d.h, seeds4, d.st)
        return s.get_centroids(d.st)
    finally:
        s.close()


IMAGES = {
    "odd": lambda: _noise(1, 97, 61),          # 5917 pixels: no multiple of 16, 24 workgroups
    "tiny": lambda: _noise(2, 5, 2),           # n < 16
    "flat": lambda: _flat(33, 7),              # every distance ties
    "two": lambda: _two_colours(50, 9),
    "small": lambda: _noise(3, 40, 23),        # 920 pixels for the large k
}


@pytest.mark.parametrize("name,k,f", [
    ("odd", 8, 1), ("odd", 8, 3), ("odd", 8, 5), ("odd", 8, 8), ("odd", 2, 1), ("odd", 2, 2), ("odd", 33, 5), ("odd", 33, 1),
    ("tiny", 8, 3), ("tiny", 2, 1), ("flat", 8, 3), ("flat", 2, 1), ("two", 8, 5), ("two", 2, 1), ("small", 300, 5), ("small", 300, 1),
])
def test_seeded_init(torch_cuda, processor, oracle, name, k, f):
    img = IMAGES[name]()
    seeds = R.pins_lab(oracle, PINS[:f])
    want = _model_init(oracle, name, img, k, seeds)
    got = _gpu_init(torch_cuda, processor, img, k, seeds)
    assert np.array_equal(_bits(got[:, :3]), _bits(want[:, :3])), (name, k, f)
    assert np.array_equal(_bits(got[:f, :3]), _bits(seeds[:, :3]))


def test_seed_equal_to_an_image_colour(torch_cuda, processor, oracle):
    # distance 0 at pixels of the image, and -- flat image -- at every pixel: Candidate(0, 0.0), pixel 0
    for name in ("odd", "flat"):
        img = IMAGES[name]()
        seeds = np.ones((2, 4), np.float32)
        seeds[:, :3] = oracle.rgb_to_lab(img.reshape(-1, 4)[[7, 20]])
        want = _model_init(oracle, name, img, 6, seeds)
        for strategy in ("scan", "table"):
            got = _gpu_init(torch_cuda, processor, img, 6, seeds, strategy)
            assert np.array_equal(_bits(got[:, :3]), _bits(want[:, :3])), (name, strategy)


@pytest.mark.parametrize("name", ["noise", "tokyo"])
def test_seeded_init_both_routes(torch_cuda, processor, oracle, tokyo, name):
    img = _noise(9, 256, 192) if name == "noise" else np.ascontiguousarray(tokyo[100:292, 200:456])
    assert img.shape[:2] == (192, 256)
    seeds = R.pins_lab(oracle, PINS[:3])
    want = _model_init(oracle, name, img, 8, seeds)
    scan = _gpu_init(torch_cuda, processor, img, 8, seeds, "scan")
    table = _gpu_init(torch_cuda, processor, img, 8, seeds, "table")
    assert np.array_equal(_bits(scan), _bits(table))
    assert np.array_equal(_bits(scan[:, :3]), _bits(want[:, :3]))


@pytest.mark.parametrize("name,k,f", [("odd", 33, 5), ("odd", 8, 8), ("two", 8, 5), ("tiny", 8, 3), ("small", 300, 4)])
def test_seeded_init_over_the_cells(torch_cuda, processor, oracle, name, k, f):
    img = IMAGES[name]()
    seeds = R.pins_lab(oracle, PINS[:f])
    want = _model_init(oracle, name, img, k, seeds)
    got = _gpu_init(torch_cuda, processor, img, k, seeds, "table")
    assert np.array_equal(_bits(got[:, :3]), _bits(want[:, :3]))


@pytest.mark.parametrize("strategy", ["scan", "table"])
@pytest.mark.parametrize("k", [2, 8, 33, 300])
def test_no_seed_is_init_centroids(torch_cuda, processor, strategy, k):
    import kmeans_gpu_amd as kg
    img = IMAGES["odd"]()
    set_strategy(strategy)
    d = _Dev(torch_cuda, img, k)
    out = []
    for seeded in (False, True):
        s = kg.Lloyd(processor, k)
        if seeded:
            s.init_centroids_seeded(d.px.data_ptr(), d.w, d.h, np.zeros((0, 4), np.float32), d.st)
        else:
            s.init_centroids(d.px.data_ptr(), d.w, d.h, d.st)
        out.append(s.get_centroids(d.st).tobytes())
        s.close()
    assert out[0] == out[1]


def test_seeds_move_unless_fixed(torch_cuda, processor, oracle):
    import kmeans_gpu_amd as kg
    img = IMAGES["odd"]()
    k, f = 8, 3
    seeds = R.pins_lab(oracle, PINS[:f])
    lab = oracle.rgb_to_lab(img)
    c0 = _model_init(oracle, "odd", img, k, seeds)
    d = _Dev(torch_cuda, img, k)
    for fixed in (0, f):
        s = kg.Lloyd(processor, k)
        s.init_centroids_seeded(d.px.data_ptr(), d.w, d.h, seeds, d.st)
        s.set_fixed(fixed)
        it = s.run(d.px.data_ptr(), d.n, d.labels.data_ptr(), d.st)
        got = s.get_centroids(d.st)
        s.close()
        wc, wl, wit = R.lloyd(oracle, lab, c0, fixed)
        assert np.array_equal(_bits(got[:, :3]), _bits(wc[:, :3])) and it == wit and np.array_equal(d.lab(), wl)
        assert np.array_equal(_bits(got[:f, :3]), _bits(seeds[:, :3])) == (fixed == f)


def _start(torch, processor, oracle, img, k, f, strategy):
    """a Lloyd object with k centroids spread over the image's pixels, n_fixed = f; the model's view of it"""
    import kmeans_gpu_amd as kg
    set_strategy(strategy)
    d = _Dev(torch, img, k)
    lab = oracle.rgb_to_lab(img)
    cent = oracle.centroids4(lab[np.linspace(0, lab.shape[0] - 1, k).astype(int)])
    s = kg.Lloyd(processor, k)
    s.set_centroids(cent, d.st)
    s.set_fixed(f)
    return d, s, lab, cent


UPDATE_SHAPES = [(8, 3, "scan"), (8, 3, "table"), (33, 5, "scan"), (33, 5, "table"), (300, 4, "scan"), (300, 4, "table"), (8, 8, "scan"),
                 (2, 1, "table")]


@pytest.mark.parametrize("k,f,strategy", UPDATE_SHAPES)
def test_update_routes(torch_cuda, processor, oracle, k, f, strategy):
    torch = torch_cuda
    img = _noise(21, 256, 192) if strategy == "table" else IMAGES["odd"]()
    d, s, lab, cent = _start(torch, processor, oracle, img, k, f, strategy)
    try:
        labels = oracle.assign(lab, cent)
        acc = oracle.accumulate(lab, labels, k)
        want, conv = R.step(oracle, acc, cent, f)
        assert np.array_equal(_bits(want[:f]), _bits(cent[:f]))
        if strategy == "table":
            assert s.prepare(d.px.data_ptr(), d.n, True, d.st) == "table"

        def check(what, sums=True):
            torch.cuda.synchronize()
            got = s.get_centroids(d.st)
            assert np.array_equal(_bits(got[:, :3]), _bits(want[:, :3])), what
            assert s.converged_count(d.st) == conv, what
            if sums:
                assert np.array_equal(d.acc.cpu().numpy(), acc), what          # pinned clusters' sums included
            s.set_centroids(cent, d.st)
            if strategy == "table":
                assert s.prepare(d.px.data_ptr(), d.n, True, d.st) == "table"

        # kmg_lloyd_update
        d.acc.copy_(torch.from_numpy(acc))
        s.update(d.acc.data_ptr(), d.st)
        check("update")
        # kmg_lloyd_assign_update(do_update), with and without a label map (the tail's two carriers)
        for lab_ptr in (d.labels.data_ptr(), 0):
            d.acc.zero_()
            s.assign_update(d.px.data_ptr(), d.n, lab_ptr, d.acc.data_ptr(), True, d.st)
            check("assign_update")
        assert np.array_equal(d.lab(), labels)
        # kmg_lloyd_iterate + flush: sums of the first assignment, then update-first
        d.acc.zero_()
        s.iterate(d.px.data_ptr(), d.n, d.labels.data_ptr(), d.acc.data_ptr(), False, d.st)
        s.iterate(d.px.data_ptr(), d.n, d.labels.data_ptr(), d.acc.data_ptr(), True, d.st)
        s.flush(d.st)
        torch.cuda.synchronize()
        assert np.array_equal(d.lab(), oracle.assign(lab, want))
        check("iterate", sums=False)
        # kmg_lloyd_labels_from_tables_update (k <= 256, a bound image)
        if strategy == "table" and k <= 256:
            d.acc.zero_()
            s.accumulate_into(d.px.data_ptr(), d.n, d.acc.data_ptr(), d.st)
            s.labels_from_tables_update(d.px.data_ptr(), d.n, d.labels.data_ptr(), d.acc.data_ptr(), d.st)
            torch.cuda.synchronize()
            assert np.array_equal(d.lab(), labels) and not d.acc.cpu().numpy().any()
            check("labels_from_tables_update", sums=False)
    finally:
        s.close()


@pytest.mark.parametrize("k,f,strategy", [(8, 3, "scan"), (8, 3, "table"), (33, 5, "table"), (300, 4, "scan"), (8, 8, "scan")])
def test_run_route(torch_cuda, processor, oracle, k, f, strategy):
    # 97 x 61: the one-launch-per-iteration loop of small images; 1024 x 600 under "scan": the assign + reduce + update loop
    for img in ((IMAGES["odd"](),) if strategy == "table" or k > 8 else (IMAGES["odd"](), _noise(4, 1024, 600))):
        d, s, lab, cent = _start(torch_cuda, processor, oracle, img, k, f, strategy)
        try:
            it = s.run(d.px.data_ptr(), d.n, d.labels.data_ptr(), d.st)
            got = s.get_centroids(d.st)
        finally:
            s.close()
        wc, wl, wit = R.lloyd(oracle, lab, cent, f)
        assert it == wit
        assert np.array_equal(_bits(got[:, :3]), _bits(wc[:, :3])) and np.array_equal(d.lab(), wl)
        assert np.array_equal(_bits(got[:f]), _bits(cent[:f]))


def test_lloyd_refusals(torch_cuda, processor):
    import kmeans_gpu_amd as kg
    img = IMAGES["odd"]()
    d = _Dev(torch_cuda, img, 4)
    s = kg.Lloyd(processor, 4)
    try:
        with pytest.raises(kg.KmgError):
            s.set_fixed(5)
        with pytest.raises(kg.KmgError):
            s.init_centroids_seeded(d.px.data_ptr(), d.w, d.h, np.zeros((5, 4), np.float32), d.st)
        with pytest.raises(kg.KmgError):
            s.init_centroids_seeded(d.px.data_ptr(), d.w, d.h, np.full((1, 4), np.nan, np.float32), d.st)
        s.set_fixed(4)
        s.set_fixed(0)
        set_strategy("table")
        s.init_centroids(d.px.data_ptr(), d.w, d.h, d.st)
        assert s.prepare(d.px.data_ptr(), d.n, True, d.st) == "table"
        s.set_cell_share(0, 2, d.st)
        with pytest.raises(kg.KmgError):
            s.set_fixed(1)
        s.set_cell_share(0, 1, d.st)
        s.set_fixed(1)
    finally:
        s.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fproc(torch_cuda):
    import kmeans_gpu_amd as kg
    p = kg.ImageProcessor()
    yield p
    p.close()


def _working(oracle, img, t=0):
    px, w, h = alpha_ref.kept_pixels(alpha_ref.shrink(oracle, img, 256), t)
    return px, w, h


@pytest.mark.parametrize("k,f", [(8, 3), (6, 6), (40, 5)])
def test_palette_and_reduce_indexed(fproc, oracle, k, f):
    import kmeans_gpu_amd as kg
    img = IMAGES["odd"]()
    h, w = img.shape[:2]
    fproc.set_fixed_colors(PINS[:f])
    cent, _ = R.palette_centroids(oracle, img.reshape(-1, 4), w, h, k, PINS[:f])
    assert np.array_equal(_bits(cent[:f]), _bits(R.pins_lab(oracle, PINS[:f])))
    want_pal = np.full((k, 4), 255, np.uint8)
    for j in range(k):
        want_pal[j, :3] = oracle.palette_lab_to_srgb8(cent[j, :3])
    assert np.array_equal(fproc.palette(k, img), alpha_ref.sorted_by_L(oracle, want_pal))
    for mode in (kg.ReduceMode.Replace, kg.ReduceMode.Dither, kg.ReduceMode.Diffuse):
        pal, index = fproc.reduce_indexed(k, img, reduce_mode=mode)
        assert np.array_equal(pal, R.palette_bytes(oracle, cent)), mode
        assert np.array_equal(pal[:f, :3], PINS[:f, :3]) and (pal[:, 3] == 255).all(), mode       # the pins, byte-exact, in order
        assert int(index.max()) < k
        if mode == kg.ReduceMode.Diffuse:
            want = diffuse_ref.diffuse(img, diffuse_ref.oracle_apply_replace(oracle, cent))
        else:
            want = oracle.apply(img, cent, int(mode))
        assert np.array_equal(pal[index][..., :3], want[..., :3]), mode
    # the RGBA8 call writes the same colours
    out = fproc.reduce(k, img)
    assert np.array_equal(out, oracle.apply(img, cent, oracle.MODE_REPLACE))
    # cleared: the default call again, byte for byte
    fproc.set_fixed_colors(None)
    assert np.array_equal(fproc.reduce(k, img), oracle.reduce(img, k, oracle.MODE_REPLACE))


def test_constructor_and_shrunk_image(torch_cuda, oracle):
    import kmeans_gpu_amd as kg
    img = _noise(31, 300, 420)                                      # shrunk to 182 x 256 first
    with kg.ImageProcessor(fixed_colors=PINS[:2, :3]) as p:         # (n, 3) colours
        px, w, h = _working(oracle, img)
        cent, _ = R.palette_centroids(oracle, px, w, h, 5, PINS[:2])
        pal, index = p.reduce_indexed(5, img)
        assert np.array_equal(pal, R.palette_bytes(oracle, cent))
        assert np.array_equal(pal[index], oracle.apply(img, cent, oracle.MODE_REPLACE))


def test_reduce_quality(fproc, oracle):
    img = IMAGES["odd"]()
    h, w = img.shape[:2]
    f = 3
    fproc.set_fixed_colors(PINS[:f])
    k, pal, index, stats, reached = fproc.reduce_quality(img, 30.0, k_min=3, k_max=12, indexed=True)
    assert 3 <= k <= 12
    want_pal, want_index = fproc.reduce_indexed(k, img)             # byte for byte what kmg_reduce_indexed(k*) writes
    assert np.array_equal(pal, want_pal) and np.array_equal(index, want_index)
    cent, _ = R.palette_centroids(oracle, img.reshape(-1, 4), w, h, k, PINS[:f])
    assert np.array_equal(pal, R.palette_bytes(oracle, cent)) and np.array_equal(pal[:f, :3], PINS[:f, :3])
    # an unreachable target: k* = k_max, pins still first
    k, pal, _, _, reached = fproc.reduce_quality(img, 0.0, k_min=3, k_max=4, indexed=True)
    assert k == 4 and not reached and np.array_equal(pal[:f, :3], PINS[:f, :3])


def test_alpha_mode(fproc, oracle):
    img = alpha_ref.sprite()
    f, k, t = 2, 6, 128
    fproc.set_fixed_colors(PINS[:f])
    fproc.set_alpha_cutoff(t)
    px, w, h = _working(oracle, img, t)
    assert h == 1 and w < img.shape[0] * img.shape[1]
    cent, _ = R.palette_centroids(oracle, px, w, h, k, PINS[:f])
    pal, index = fproc.reduce_indexed(k, img)
    assert np.array_equal(pal, R.palette_bytes(oracle, cent)) and np.array_equal(pal[:f, :3], PINS[:f, :3])
    keep = img[..., 3] >= t
    assert np.array_equal(pal[index[keep]][:, :3], oracle.apply(img, cent, oracle.MODE_REPLACE)[keep][:, :3])
    assert (index[~keep] == k).all()


def test_sequence_keeps_the_pins(fproc, oracle):
    import kmeans_gpu_amd as kg
    f, k = 3, 7
    frames = [_noise(40 + i, 61, 37) for i in range(3)]
    fproc.set_fixed_colors(PINS[:f])
    with fproc.sequence() as seq:
        for fr in frames:
            seq.add(fr)
        px = np.concatenate([fr.reshape(-1, 4) for fr in frames])
        cent, _ = R.palette_centroids(oracle, px, px.shape[0], 1, k, PINS[:f])
        assert np.array_equal(_bits(seq.centroids(k)[:, :3]), _bits(cent[:, :3]))
        want_pal = np.full((k, 4), 255, np.uint8)
        for j in range(k):
            want_pal[j, :3] = oracle.palette_lab_to_srgb8(cent[j, :3])
        assert np.array_equal(seq.palette(k), alpha_ref.sorted_by_L(oracle, want_pal))
        pal = seq.output(k, kg.ReduceMode.Replace, kg.OutputFormat.Index8, 61, 37)
        assert np.array_equal(pal, R.palette_bytes(oracle, cent)) and np.array_equal(pal[:f, :3], PINS[:f, :3])
        index, _, _ = seq.frame(frames[1], delta=False)
        assert np.array_equal(pal[index], oracle.apply(frames[1], cent, oracle.MODE_REPLACE))
        seq.end_output()
        # one whole frame: with pins (sw, sh) and |W| x 1 are the same problem, and it is kmg_reduce_indexed of that frame
        seq.clear()
        seq.add(frames[2])
        one = seq.centroids(k)
        c2, _ = R.palette_centroids(oracle, frames[2].reshape(-1, 4), 61, 37, k, PINS[:f])
        assert np.array_equal(_bits(one[:, :3]), _bits(c2[:, :3])) and np.array_equal(_bits(one[:f, :3]), _bits(cent[:f, :3]))
        assert np.array_equal(fproc.reduce_indexed(k, frames[2])[0], R.palette_bytes(oracle, c2))
        # a second scene after clear: the pins are held, the rest follows the new frames
        seq.clear()
        seq.add(frames[0]); seq.add(_two_colours(30, 11))
        two = seq.centroids(k)
        assert np.array_equal(_bits(two[:f, :3]), _bits(cent[:f, :3])) and not np.array_equal(_bits(two[f:]), _bits(one[f:]))
        with pytest.raises(kg.KmgError):
            seq.centroids(f - 1)
        assert seq.centroids(f).shape == (f, 4)


def test_refusals(fproc, oracle):
    import ctypes as C
    import kmeans_gpu_amd as kg
    img = IMAGES["odd"]()
    fproc.set_fixed_colors(PINS[:4])
    for call in (lambda: fproc.palette(3, img), lambda: fproc.reduce(3, img), lambda: fproc.reduce_indexed(3, img),
                 lambda: fproc.reduce_quality(img, 5.0, k_min=3, k_max=9),
                 lambda: fproc.palette(8, img, kg.Algorithm.Octree), lambda: fproc.reduce(8, img, kg.Algorithm.Octree),
                 lambda: fproc.reduce_indexed(8, img, kg.Algorithm.Octree)):
        with pytest.raises(kg.KmgError) as e:
            call()
        assert e.value.status == -1
    # nothing written
    out = np.full(img.shape, 0xA5, np.uint8)
    with pytest.raises(kg.KmgError):
        fproc.reduce(3, img, out=out)
    assert (out == 0xA5).all()
    L = kg.lib()
    too_many = np.zeros((3073, 4), np.uint8)
    assert L.kmg_processor_set_fixed_colors(fproc.handle, too_many.ctypes.data_as(C.c_void_p), 3073) == -1
    assert L.kmg_processor_set_fixed_colors(fproc.handle, None, 2) == -1
    assert fproc.reduce(4, img).shape == img.shape                  # the list set before is still in force, and k = f works
    pal, _ = fproc.reduce_indexed(4, img)
    assert np.array_equal(pal[:, :3], PINS[:4, :3])
    # find takes the caller's palette: untouched by the fixed colours
    assert np.array_equal(fproc.find(img, PINS[4:7]), oracle.find(img, PINS[4:7], oracle.MODE_REPLACE))
    # the group layer has no pinned path
    with kg.Group(devices=[0]) as group:
        member = group.processor(0)
        assert group.reduce(4, img).shape == img.shape
        member.set_fixed_colors(PINS[:2])
        for call in (lambda: group.palette(4, img), lambda: group.reduce(4, img), lambda: group.reduce_batch(4, [img])):
            with pytest.raises(kg.KmgError) as e:
                call()
            assert e.value.status == -1
        member.set_fixed_colors(None)
        assert np.array_equal(group.reduce(4, img), oracle.reduce(img, 4, oracle.MODE_REPLACE))
