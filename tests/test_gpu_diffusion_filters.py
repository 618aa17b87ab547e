"""The filters of KMG_MODE_DIFFUSE other than Floyd-Steinberg on the device (kmg_diffuse_wide.hip) against the test-side reference of
the contract (tests/diffusion_ref.py, nearest colours from the oracle's replace pass; weights from kmg_diffusion_weights): shapes
around the chunk, body and reach boundaries, palette sizes of every nearest-colour route, the three strategies, the index formats,
alpha mode, a plan in bands on two streams (bands of one row: the forwarded row), kmg_dev_apply on a band, the switch itself, the
modes that ignore it, the calls that reach diffusion through a plan (sequence output, clip, find_batch), the reuse of the progress
ring, threads, and the watchdog on a chain of waiting chunks.

The module has a processor of its own: the switch is sticky, and the session's processor stays at filter 0."""
import threading

import numpy as np
import pytest

import diffuse_ref
import diffusion_ref

pytestmark = pytest.mark.gpu

SIERRA_LITE, ATKINSON, BURKES, SIERRA2, SIERRA3, JARVIS, STUCKI = range(1, 8)
FILTERS = list(range(1, 8))


@pytest.fixture(scope="module")
def fproc(torch_cuda):
    import kmeans_gpu_amd as kg
    p = kg.ImageProcessor()
    yield p
    p.close()


@pytest.fixture(autouse=True)
def _back_to_floyd_steinberg(fproc):
    yield
    fproc.set_diffusion(0)
    fproc.set_alpha_cutoff(0)


def _palette(k, seed):
    rng = np.random.default_rng(seed)
    pal = np.full((k, 4), 255, np.uint8)
    pal[:, :3] = rng.integers(0, 256, (k, 3))
    return pal


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


_nearest = {}


def _near(oracle, pal):
    """one table of nearest colours per palette, shared by every test that diffuses onto it"""
    key = pal.tobytes()
    if key not in _nearest:
        _nearest[key] = diffuse_ref.Nearest(diffuse_ref.oracle_find_replace(oracle, pal))
    return _nearest[key]


def _want(oracle, img, pal, f, keep=None):
    import kmeans_gpu_amd as kg
    weights, divisor = kg.diffusion_weights(f)
    return diffusion_ref.diffuse(img, None, weights, divisor, keep=keep, nearest=_near(oracle, pal))


SHAPES = [(1, 1), (1, 2), (2, 1), (3, 2), (64, 17), (65, 3), (66, 5), (129, 2), (63, 200), (200, 257), (1, 4099), (4099, 1),
          (700, 300)]


@pytest.mark.parametrize("f", FILTERS)
def test_find_shapes_equal_reference(fproc, oracle, f):
    import kmeans_gpu_amd as kg
    fproc.set_diffusion(f)
    pal = _palette(16, 16)
    for h, w in SHAPES:
        img = _noise(h, w, h * 7 + w)
        got = fproc.find(img, pal, kg.ReduceMode.Diffuse)
        assert np.array_equal(got, _want(oracle, img, pal, f)), (h, w)


@pytest.mark.parametrize("f", [ATKINSON, JARVIS])
@pytest.mark.parametrize("k", [1, 2, 256, 300, 3072])
def test_find_palette_sizes_equal_reference(fproc, oracle, f, k):
    import kmeans_gpu_amd as kg
    fproc.set_diffusion(f)
    img, pal = _noise(70, 90, k), _palette(k, k + 7)
    assert np.array_equal(fproc.find(img, pal, kg.ReduceMode.Diffuse), _want(oracle, img, pal, f))


@pytest.mark.parametrize("f", [SIERRA_LITE, STUCKI])
@pytest.mark.parametrize("k", [2, 64, 300])
def test_scan_table_and_auto_give_identical_bytes(fproc, oracle, f, k):
    import kmeans_gpu_amd as kg
    fproc.set_diffusion(f)
    img, pal = _noise(200, 257, 77 + k), _palette(k, 5 * k)
    outs = {}
    for strategy in ("scan", "table", "auto"):
        kg.set_strategy(strategy)                                 # (back to auto after every test: conftest)
        outs[strategy] = fproc.find(img, pal, kg.ReduceMode.Diffuse)
    assert np.array_equal(outs["scan"], outs["table"]) and np.array_equal(outs["auto"], outs["table"])
    if k == 64:
        assert np.array_equal(outs["table"], _want(oracle, img, pal, f))


@pytest.mark.parametrize("f", FILTERS)
@pytest.mark.parametrize("k", [40, 300])                              # INDEX8 and INDEX16
def test_find_indexed_equals_rgba8_and_reference(fproc, oracle, f, k):
    import kmeans_gpu_amd as kg
    fproc.set_diffusion(f)
    img, pal = _noise(130, 75, 9 * k + f), _palette(k, k)
    idx = fproc.find_indexed(img, pal, kg.ReduceMode.Diffuse)
    assert idx.dtype == (np.uint8 if k <= 256 else np.uint16) and idx.max() < k
    rgba = fproc.find(img, pal, kg.ReduceMode.Diffuse)
    want = _want(oracle, img, pal, f)
    assert np.array_equal(rgba, want)
    assert np.array_equal(pal[idx][..., :3], rgba[..., :3])


@pytest.mark.parametrize("f", FILTERS)
def test_alpha_mode_keeps_alpha_and_leaves_dropped_pixels_out(fproc, oracle, f):
    import kmeans_gpu_amd as kg
    fproc.set_diffusion(f)
    fproc.set_alpha_cutoff(128)
    k = 20
    img, pal = _noise(131, 97, 1280 + f), _palette(k, 28)
    keep = img[..., 3] >= 128
    want = _want(oracle, img, pal, f, keep=keep)
    want[..., 3] = img[..., 3]
    got = fproc.find(img, pal, kg.ReduceMode.Diffuse)
    assert np.array_equal(got, want)
    idx = fproc.find_indexed(img, pal, kg.ReduceMode.Diffuse)
    assert idx.dtype == np.uint8 and (idx[~keep] == k).all() and (idx[keep] < k).all()
    assert np.array_equal(pal[idx[keep]][:, :3], want[keep][:, :3])


@pytest.mark.parametrize("f", [ATKINSON, STUCKI])
def test_plan_in_bands_on_two_streams_equals_the_whole_pass(torch_cuda, fproc, oracle, f):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    fproc.set_diffusion(f)
    w, h, k = 300, 200, 40
    host = _noise(h, w, 4242)
    img = torch.from_numpy(host.reshape(-1, 4)).cuda()
    pal = _palette(k, 9)
    cent = kg.palette_to_centroids(pal)
    st = torch.cuda.current_stream().cuda_stream
    whole = torch.zeros((h * w, 4), dtype=torch.uint8, device="cuda")
    fproc.apply(img.data_ptr(), w, h, 0, cent, kg.ReduceMode.Diffuse, whole.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(whole.cpu().numpy().reshape(h, w, 4), _want(oracle, host, pal, f))
    out = torch.zeros((h * w, 4), dtype=torch.uint8, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    plan = fproc.apply_plan(cent, kg.ReduceMode.Diffuse, h * w, st)
    bounds = [0, 1, 2, 65, 66, 130, 200]                          # [0, 1), [1, 2), [65, 66): bands of one row forward a row
    for i, (r0, r1) in enumerate(zip(bounds[:-1], bounds[1:])):
        plan.run(img[r0 * w:].data_ptr(), w, r1 - r0, r0, out[r0 * w:].data_ptr(), streams[i % 2].cuda_stream)
    plan.status()
    torch.cuda.synchronize()
    plan.close()
    assert torch.equal(out, whole)


@pytest.mark.parametrize("f", [SIERRA_LITE, SIERRA3])
def test_dev_apply_on_a_band_diffuses_the_band_alone(torch_cuda, fproc, oracle, f):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    fproc.set_diffusion(f)
    w, h, r0, rows = 300, 400, 123, 150
    host = _noise(h, w, 5150)
    img = torch.from_numpy(host.reshape(-1, 4)).cuda()
    pal = _palette(24, 3)
    out = torch.zeros((rows * w, 4), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    fproc.apply(img[r0 * w:].data_ptr(), w, rows, r0, kg.palette_to_centroids(pal), kg.ReduceMode.Diffuse, out.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(rows, w, 4), _want(oracle, host[r0:r0 + rows], pal, f))


def test_the_switch(torch_cuda, fproc, oracle):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    w, h = 120, 140
    host, pal = _noise(h, w, 88), _palette(12, 12)
    img = torch.from_numpy(host.reshape(-1, 4)).cuda()
    out = torch.zeros((h * w, 4), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    fproc.set_diffusion("burkes")
    plan = fproc.apply_plan(kg.palette_to_centroids(pal), kg.ReduceMode.Diffuse, h * w, st)
    plan.run(img.data_ptr(), w, 70, 0, out.data_ptr(), st)
    fproc.set_diffusion(kg.Diffusion.Jarvis)                      # the plan keeps the filter it was made under
    plan.run(img[70 * w:].data_ptr(), w, h - 70, 70, out[70 * w:].data_ptr(), st)
    plan.status()
    plan.close()
    assert np.array_equal(out.cpu().numpy().reshape(h, w, 4), _want(oracle, host, pal, BURKES))
    assert np.array_equal(fproc.find(host, pal, kg.ReduceMode.Diffuse), _want(oracle, host, pal, JARVIS))
    for bad in (8, -1):
        with pytest.raises(kg.KmgError) as e:
            fproc.set_diffusion(bad)
        assert e.value.status == -1
    assert fproc.diffusion == kg.Diffusion.Jarvis
    assert np.array_equal(fproc.find(host, pal, kg.ReduceMode.Diffuse), _want(oracle, host, pal, JARVIS))
    fproc.set_diffusion(0)
    want0 = diffuse_ref.diffuse(host, None, nearest=_near(oracle, pal))
    assert np.array_equal(fproc.find(host, pal, kg.ReduceMode.Diffuse), want0)
    with kg.ImageProcessor(diffusion="sierra2") as p2:            # the constructor's argument is the same switch
        assert np.array_equal(p2.find(host, pal, kg.ReduceMode.Diffuse), _want(oracle, host, pal, SIERRA2))


def test_the_other_modes_ignore_the_switch(fproc):
    import kmeans_gpu_amd as kg
    img, pal = _noise(90, 110, 31), _palette(10, 31)
    modes = (kg.ReduceMode.Replace, kg.ReduceMode.Dither, kg.ReduceMode.Meld)
    before = [fproc.find(img, pal, m) for m in modes]
    fproc.set_diffusion(JARVIS)
    for m, b in zip(modes, before):
        assert np.array_equal(fproc.find(img, pal, m), b), int(m)


def test_sequence_output_clip_and_find_batch_follow_the_switch(torch_cuda, fproc, oracle):
    """The sequence output fixes the filter when it is opened: every frame's map is the single-frame call's (kmg_dev_apply_format
    with the sequence's centroids, as tests/test_gpu_sequence.py compares) under that filter, whatever the switch says later; a
    clip of 8 frames equals the single frames; kmg_find_batch equals kmg_find_indexed image by image, and the reference."""
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    st = torch.cuda.current_stream().cuda_stream
    h = w = 32
    k = 12
    frames = [_noise(h, w, 600 + t) for t in range(8)]
    for fr in frames:
        fr[..., 3] = 255
    fproc.set_diffusion(SIERRA3)
    with fproc.sequence() as seq:
        for fr in frames:
            seq.add(fr)
        cent = seq.centroids(k)
        pal = seq.output(k, kg.ReduceMode.Diffuse, kg.OutputFormat.Index8, w, h)
        want = []
        for fr in frames:
            d_in = torch.from_numpy(fr).cuda()
            d_out = torch.zeros(h * w, dtype=torch.uint8, device="cuda")
            fproc.apply(d_in.data_ptr(), w, h, 0, cent, kg.ReduceMode.Diffuse, d_out.data_ptr(), st, format=kg.OutputFormat.Index8)
            torch.cuda.synchronize()
            want.append(d_out.cpu().numpy().reshape(h, w))
        weights, divisor = kg.diffusion_weights(SIERRA3)
        ref = diffusion_ref.diffuse(frames[0], diffuse_ref.oracle_apply_replace(oracle, cent), weights, divisor)
        assert np.array_equal(pal[want[0]][..., :3], ref[..., :3])
        fproc.set_diffusion(ATKINSON)                             # the open output keeps Sierra-3
        for fr, I in zip(frames, want):
            got, _, full = seq.frame(fr, delta=False)
            assert full and np.array_equal(got, I)
        clip = seq.frames(frames, delta=False)
        for (got, _, full), I in zip(clip, want):
            assert full and np.array_equal(got, I)
    # per-frame palettes: the output keeps the filter it was opened under here too
    def local_maps(opened_under, switched_to):
        fproc.set_diffusion(opened_under)
        with fproc.sequence() as seq:
            seq.output_local(k, kg.ReduceMode.Diffuse, kg.OutputFormat.Index8, w, h)
            fproc.set_diffusion(switched_to)
            return [seq.frame_local(fr, delta=False)[0] for fr in frames[:2]]
    kept, plain, other = local_maps(SIERRA3, ATKINSON), local_maps(SIERRA3, SIERRA3), local_maps(ATKINSON, ATKINSON)
    assert all(np.array_equal(a, b) for a, b in zip(kept, plain))
    assert not all(np.array_equal(a, b) for a, b in zip(kept, other))
    fproc.set_diffusion(BURKES)
    images = [_noise(20 + 3 * i, 40 - 2 * i, 700 + i) for i in range(6)]
    pal = _palette(16, 61)
    maps = fproc.find_batch(images, pal, kg.ReduceMode.Diffuse)
    for im, m in zip(images, maps):
        assert np.array_equal(m, fproc.find_indexed(im, pal, kg.ReduceMode.Diffuse))
        assert np.array_equal(pal[m][..., :3], _want(oracle, im, pal, BURKES)[..., :3])


def test_more_chunks_than_progress_slots(fproc, oracle):
    """1 x 65 600: 1 025 chunks of 64 rows, so the ring of 1 024 progress / heartbeat slots is reused"""
    import kmeans_gpu_amd as kg
    fproc.set_diffusion(JARVIS)
    img, pal = _noise(65600, 1, 65600), _palette(16, 16)
    assert np.array_equal(fproc.find(img, pal, kg.ReduceMode.Diffuse), _want(oracle, img, pal, JARVIS))


def test_eight_threads_on_one_processor_share_nothing(fproc):
    import kmeans_gpu_amd as kg
    fproc.set_diffusion(SIERRA3)
    cases = [(_noise(200 + 37 * i, 150 + 11 * i, 900 + i), _palette(3 + 9 * i, 40 + i)) for i in range(8)]
    alone = [fproc.find(img, pal, kg.ReduceMode.Diffuse) for img, pal in cases]
    got = [None] * 8
    errors = []

    def work(i):
        try:
            for _ in range(3):
                got[i] = fproc.find(cases[i][0], cases[i][1], kg.ReduceMode.Diffuse)
                if not np.array_equal(got[i], alone[i]):
                    return
        except Exception as e:                                   # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(8):
        assert np.array_equal(got[i], alone[i]), i


def test_scan_at_the_largest_k_on_a_tall_image(fproc, oracle):
    """128 chunks of 64 rows, each waiting for the last two rows of the one before, at the slowest step there is (a per-lane scan
    of 3072 centroids): while the pipeline fills, the watchdog must read a waiting predecessor's heartbeat as progress of the
    pass -- no timeout, the reference's bytes."""
    import kmeans_gpu_amd as kg
    fproc.set_diffusion(JARVIS)
    img, pal = _noise(8192, 16, 3072), _palette(3072, 11)
    cent = oracle.centroids4(np.stack([oracle.palette_srgb8_to_lab(c) for c in pal]))
    weights, divisor = kg.diffusion_weights(JARVIS)
    kg.set_strategy("scan")                                       # (back to auto after every test: conftest)
    got = fproc.find(img, pal, kg.ReduceMode.Diffuse)
    assert np.array_equal(got, diffusion_ref.diffuse(img, diffuse_ref.oracle_apply_replace(oracle, cent), weights, divisor))
