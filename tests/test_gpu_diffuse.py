"""KMG_MODE_DIFFUSE on the device (kmg_diffuse.hip) against the test-side reference of the contract (tests/diffuse_ref.py, whose
nearest colours come from the oracle's own replace pass): kmg_find, kmg_reduce, both nearest-colour routes, the plan in bands on two
streams, kmg_dev_apply on a band, concurrent calls on one processor, a property no implementation can fake, and one full-size
image.  The kmg_group_* calls keep rejecting the mode."""
import threading

import numpy as np
import pytest

from conftest import load_rgba, sorted_palette
import diffuse_ref

pytestmark = pytest.mark.gpu


def _palette(k, seed):
    rng = np.random.default_rng(seed)
    pal = np.full((k, 4), 255, np.uint8)
    pal[:, :3] = rng.integers(0, 256, (k, 3))
    return pal


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _want_find(oracle, img, pal):
    return diffuse_ref.diffuse(img, diffuse_ref.oracle_find_replace(oracle, pal))


def test_smallest_case_find_equals_reference(processor, oracle):
    import kmeans_gpu_amd as kg
    img, pal = _noise(65, 3, 1), _palette(5, 1)
    assert np.array_equal(processor.find(img, pal, kg.ReduceMode.Diffuse), _want_find(oracle, img, pal))


@pytest.mark.parametrize("case", ["tokyo-dark-white-red", "tokyo-apollo", "tokyo-resurrect"])
def test_find_on_the_golden_images_equals_reference(processor, oracle, tokyo, case):
    import kmeans_gpu_amd as kg
    pal = {"tokyo-dark-white-red": np.array([[5, 5, 5, 255], [255, 255, 255, 255], [255, 0, 0, 255]], np.uint8),
           "tokyo-apollo": sorted_palette("apollo-1x.png"), "tokyo-resurrect": sorted_palette("resurrect_64.png")}[case]
    got = processor.find(tokyo, pal, kg.ReduceMode.Diffuse)
    assert np.array_equal(got, _want_find(oracle, tokyo, pal))


@pytest.mark.parametrize("k", [1, 2, 256, 300, 3072])
def test_find_random_palettes_equals_reference(processor, oracle, k):
    import kmeans_gpu_amd as kg
    img, pal = _noise(70, 90, k), _palette(k, k + 7)
    assert np.array_equal(processor.find(img, pal, kg.ReduceMode.Diffuse), _want_find(oracle, img, pal))


@pytest.mark.parametrize("h,w,kind", [(1, 1, "noise"), (1, 4099, "noise"), (4099, 1, "noise"), (65, 3, "noise"),
                                      (63, 200, "noise"), (1100, 1024, "noise"), (300, 257, "flat")])
def test_find_shapes_equals_reference(processor, oracle, h, w, kind):
    import kmeans_gpu_amd as kg
    img = _noise(h, w, h * 7 + w) if kind == "noise" else np.full((h, w, 4), (90, 140, 200, 255), np.uint8)
    pal = _palette(16, h + w)
    assert np.array_equal(processor.find(img, pal, kg.ReduceMode.Diffuse), _want_find(oracle, img, pal))


@pytest.mark.parametrize("k", [8, 64])
def test_reduce_kmeans_and_octree_equal_reference(processor, oracle, tokyo, k):
    import kmeans_gpu_amd as kg
    cent, _ = oracle.extract_palette_kmeans(tokyo, k)
    want = diffuse_ref.diffuse(tokyo, diffuse_ref.oracle_apply_replace(oracle, cent))
    assert np.array_equal(processor.reduce(k, tokyo, kg.Algorithm.Kmeans, kg.ReduceMode.Diffuse), want)
    opal = oracle.palette_octree(tokyo, k)
    want = _want_find(oracle, tokyo, opal)
    assert np.array_equal(processor.reduce(k, tokyo, kg.Algorithm.Octree, kg.ReduceMode.Diffuse), want)


@pytest.mark.parametrize("k", [2, 64, 300])
def test_scan_table_and_auto_give_identical_bytes(processor, oracle, k):
    import kmeans_gpu_amd as kg
    img, pal = _noise(1100, 1024, 77 + k), _palette(k, 5 * k)
    outs = {}
    try:
        for strategy in ("scan", "table", "auto"):
            kg.set_strategy(strategy)
            outs[strategy] = processor.find(img, pal, kg.ReduceMode.Diffuse)
    finally:
        kg.set_strategy("auto")
    assert np.array_equal(outs["scan"], outs["table"]) and np.array_equal(outs["auto"], outs["table"])
    if k == 64:
        assert np.array_equal(outs["table"], _want_find(oracle, img, pal))


def _palette_centroids(oracle, pal):
    return oracle.centroids4(np.stack([oracle.palette_srgb8_to_lab(c) for c in pal]))


def test_scan_at_the_largest_k_on_a_tall_image(processor, oracle):
    """512 chunks of 64 rows, each waiting for the whole last row of the one before, at the slowest step there is (a per-lane
    scan of 3072 centroids): the pipeline takes seconds to fill, and the watchdog must read a waiting predecessor's heartbeat as
    progress of the pass -- no timeout, the reference's bytes"""
    import kmeans_gpu_amd as kg
    img, pal = _noise(32768, 16, 3072), _palette(3072, 11)
    cent = _palette_centroids(oracle, pal)
    sample = img[:4, :, :].reshape(1, -1, 4).copy(); sample[..., 3] = 255
    assert np.array_equal(oracle.apply(sample, cent, oracle.MODE_REPLACE), oracle.find(sample, pal, oracle.MODE_REPLACE))
    try:
        kg.set_strategy("scan")
        got = processor.find(img, pal, kg.ReduceMode.Diffuse)
    finally:
        kg.set_strategy("auto")
    assert np.array_equal(got, diffuse_ref.diffuse(img, diffuse_ref.oracle_apply_replace(oracle, cent)))


def test_more_chunks_than_progress_slots(processor, oracle):
    """1 x 65 600: 1 025 chunks of 64 rows, so the ring of 1 024 progress / heartbeat slots is reused"""
    import kmeans_gpu_amd as kg
    img, pal = _noise(65600, 1, 65600), _palette(16, 16)
    cent = _palette_centroids(oracle, pal)
    got = processor.find(img, pal, kg.ReduceMode.Diffuse)
    assert np.array_equal(got, diffuse_ref.diffuse(img, diffuse_ref.oracle_apply_replace(oracle, cent)))


def test_plan_status_after_bands(torch_cuda, processor):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    w, h = 300, 200
    img = torch.from_numpy(_noise(h, w, 77).reshape(-1, 4)).cuda()
    out = torch.zeros_like(img)
    st = torch.cuda.current_stream().cuda_stream
    plan = processor.apply_plan(kg.palette_to_centroids(_palette(8, 8)), kg.ReduceMode.Diffuse, w * h, st)
    plan.run(img.data_ptr(), w, 120, 0, out.data_ptr(), st)
    plan.run(img[120 * w:].data_ptr(), w, 80, 120, out[120 * w:].data_ptr(), st)
    plan.status()                                                    # waits for the last band: no band timed out
    plan.close()


def test_apply_plan_in_bands_on_two_streams_equals_the_whole_pass(torch_cuda, processor, oracle):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    w, h, k = 2048, 1536, 40
    n = w * h
    host = _noise(h, w, 4242)
    img = torch.from_numpy(host.reshape(n, 4)).cuda()
    pal = _palette(k, 9)
    cent = kg.palette_to_centroids(pal)
    st = torch.cuda.current_stream().cuda_stream
    whole = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    processor.apply(img.data_ptr(), w, h, 0, cent, kg.ReduceMode.Diffuse, whole.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(whole.cpu().numpy().reshape(h, w, 4), _want_find(oracle, host, pal))
    out = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    plan = processor.apply_plan(cent, kg.ReduceMode.Diffuse, n, st)
    bounds = [0, 100, 101, 640, 1203, h]
    for i, (r0, r1) in enumerate(zip(bounds[:-1], bounds[1:])):
        s = streams[i % 2]
        plan.run(img[r0 * w:].data_ptr(), w, r1 - r0, r0, out[r0 * w:].data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    plan.close()
    assert torch.equal(out, whole)
    # a band that does not continue the image is refused
    plan = processor.apply_plan(cent, kg.ReduceMode.Diffuse, n, st)
    with pytest.raises(kg.KmgError) as e:
        plan.run(img.data_ptr(), w, 10, 5, out.data_ptr(), st)                       # row0 must be 0 first
    assert e.value.status == -1
    plan.run(img.data_ptr(), w, 10, 0, out.data_ptr(), st)
    with pytest.raises(kg.KmgError) as e:
        plan.run(img[20 * w:].data_ptr(), w, 10, 20, out.data_ptr(), st)            # skips rows 10 .. 19
    assert e.value.status == -1
    with pytest.raises(kg.KmgError) as e:
        plan.run(img[10 * w:].data_ptr(), w - 1, 10, 10, out.data_ptr(), st)        # another width
    assert e.value.status == -1
    torch.cuda.synchronize()
    plan.close()


def test_dev_apply_on_a_band_diffuses_the_band_alone(torch_cuda, processor, oracle):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    w, h, r0, rows = 300, 400, 123, 150
    host = _noise(h, w, 5150)
    img = torch.from_numpy(host.reshape(-1, 4)).cuda()
    pal = _palette(24, 3)
    out = torch.zeros((rows * w, 4), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    processor.apply(img[r0 * w:].data_ptr(), w, rows, r0, kg.palette_to_centroids(pal), kg.ReduceMode.Diffuse, out.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(rows, w, 4), _want_find(oracle, host[r0:r0 + rows], pal))


def test_eight_threads_on_one_processor_share_nothing(processor):
    import kmeans_gpu_amd as kg
    cases = [(_noise(200 + 37 * i, 150 + 11 * i, 900 + i), _palette(3 + 9 * i, 40 + i)) for i in range(8)]
    alone = [processor.find(img, pal, kg.ReduceMode.Diffuse) for img, pal in cases]
    got = [None] * 8
    errors = []

    def work(i):
        try:
            for _ in range(3):
                got[i] = processor.find(cases[i][0], cases[i][1], kg.ReduceMode.Diffuse)
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


def test_flat_grey_keeps_its_mean_on_black_and_white(processor):
    import kmeans_gpu_amd as kg
    img = np.full((512, 512, 4), (128, 128, 128, 255), np.uint8)
    pal = np.array([[0, 0, 0, 255], [255, 255, 255, 255]], np.uint8)
    rep = processor.find(img, pal, kg.ReduceMode.Replace)
    assert (rep[..., :3] == 255).all()
    dif = processor.find(img, pal, kg.ReduceMode.Diffuse)
    assert set(np.unique(dif[..., :3])) <= {0, 255} and (dif[..., 3] == 255).all()
    assert abs(float(dif[..., :3].mean()) - 128.0) <= 2.0


def test_full_size_photograph_k64(torch_cuda, processor, oracle):
    import bench
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    w = h = 8192
    n = w * h
    rgba = bench.synthetic_image("photo", n, 0, 64, 0x5EED0B10)
    host = rgba.cpu().numpy().reshape(h, w, 4)
    pal = host.reshape(-1, 4)[np.arange(64, dtype=np.int64) * (n // 64)].copy()
    pal[:, 3] = 255
    cent = kg.palette_to_centroids(pal)
    out = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    processor.apply(rgba.data_ptr(), w, h, 0, cent, kg.ReduceMode.Diffuse, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(h, w, 4)
    del out, rgba
    want = diffuse_ref.diffuse(host, diffuse_ref.oracle_find_replace(oracle, pal))
    assert np.array_equal(got, want)


def test_group_calls_still_reject_mode_3(torch_cuda, tokyo):
    import kmeans_gpu_amd as kg
    with kg.Group(devices=[0]) as g:
        with pytest.raises(kg.KmgError) as e:
            g.find(tokyo, sorted_palette("apollo-1x.png"), kg.ReduceMode.Diffuse)
        assert e.value.status == -1
        with pytest.raises(kg.KmgError) as e:
            g.reduce(8, tokyo, kg.Algorithm.Kmeans, kg.ReduceMode.Diffuse)
        assert e.value.status == -1
        with pytest.raises(kg.KmgError) as e:
            g.reduce_batch(8, [tokyo, tokyo[:100]], kg.Algorithm.Kmeans, kg.ReduceMode.Diffuse)
        assert e.value.status == -1
