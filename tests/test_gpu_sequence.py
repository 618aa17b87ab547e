"""Frame sequences on the device (include/kmeans_hip.h at kmg_sequence), against tests/sequence_ref.py:
  1. k_frame_delta bit for bit: shapes around the 16-byte chunk, the 256-chunk tile and the grid cap, both index types, pointers
     1 - 3 elements into sentinel-filled buffers (apart: the element-wise path; together: the vector path with a partial first
     chunk), four change patterns, and a frame in two bands combined in both orders; the per-lane (x, y) cursor where a workgroup
     walks several tiles (tests/tile_walk.py, tests/probe_run.py): one-pixel frames whose record is known by construction, in bands
     of 4200, 4100, 2101 (INDEX16: 2100), 4102, 4102 and 2049 tiles (tile = 4096 elements INDEX8, 2048 INDEX16) of the widths 1000 tile / 1024
     (step_y = 1), tile (step_x = 0), tile - 1, 300 tile / 1024 (step_y = 3), 3 and 1 (both formats, all six), behind a partial
     first chunk, and as the second of two bands with an odd row0;
  2. refusals, after each of which the processor still works;
  3. the shared palette: one frame = kmg_palette / kmg_reduce_indexed, frames of different sizes, alpha mode, the colour-table
     strategy on a large working sequence, many re-allocations of W -- float bit patterns, under both strategies;
  4. frame output: full maps = kmg_dev_apply_format, deltas replay to them, records = numpy's, the is_full rule;
  5. lifecycle: begin twice, frame without begin, wrong size, destroy with an output open, the block counts stop growing;
  6. the Python Sequence and the CLI end to end, the APNG decoded by the reader of tests/test_sequence_contract.py."""
import ctypes as C

import numpy as np
import pytest

import alpha_ref
import probe_run
import tile_walk
import sequence_ref as R
from conftest import set_strategy
from test_sequence_contract import read_apng

pytestmark = pytest.mark.gpu

FMT8, FMT16 = 1, 2
SHAPES = [(1, 1), (15, 3), (16, 2), (17, 5), (63, 1), (64, 1), (65, 2), (1023, 3), (1025, 3), (4099, 7), (2048 * 1024 + 5, 1)]
# pointers apart (element by element), together (16-byte accesses behind a partial first chunk), and -- beyond the 1 - 3 -- unshifted
OFFSETS = [(1, 2, 3), (3, 3, 3), (2, 2, 2), (0, 0, 0)]
PATTERNS = ("nothing", "everything", "corners", "random")
# 2048 workgroups of 256 lanes x 16 bytes cover 8 Mi bytes per tile round: only a larger band makes a workgroup walk several tiles
# (the prefetch, the per-tile coordinate step)
MANY_TILES = (4099, 2100)
PAD = 8


def _np_dtype(fmt):
    return np.uint8 if fmt == FMT8 else np.uint16


def _sentinel(fmt):
    return 0xA5 if fmt == FMT8 else 0xA5C3


class _Dev:
    """the three buffers of a delta call, each `off` elements into a sentinel-filled allocation, and the record"""

    def __init__(self, torch, fmt, n, offs):
        self.torch, self.fmt, self.n, self.offs = torch, fmt, n, offs
        self.size = 1 if fmt == FMT8 else 2
        t = torch.uint8 if fmt == FMT8 else torch.int16
        s = _sentinel(fmt)
        self.bufs = [torch.from_numpy(np.full(n + 2 * PAD, s, _np_dtype(fmt)).view(np.uint8 if fmt == FMT8 else np.int16)).cuda()
                     for _ in range(3)]
        assert self.bufs[0].dtype == t
        self.info = torch.zeros(4, dtype=torch.int64, device="cuda")

    def ptr(self, i, first=0):
        return self.bufs[i].data_ptr() + self.size * (self.offs[i] + first)

    def put(self, i, a):
        flat = np.ascontiguousarray(a).reshape(-1).view(np.uint8 if self.fmt == FMT8 else np.int16)
        self.bufs[i][self.offs[i]:self.offs[i] + self.n] = self.torch.from_numpy(flat).cuda()

    def get(self, i, shape):
        host = self.bufs[i].cpu().numpy().view(_np_dtype(self.fmt))
        o = self.offs[i]
        assert (host[:o] == _sentinel(self.fmt)).all() and (host[o + self.n:] == _sentinel(self.fmt)).all(), "written outside the band"
        return host[o:o + self.n].reshape(shape)

    def fresh(self):
        import kmeans_gpu_amd as kg
        self.info.copy_(self.torch.from_numpy(np.frombuffer(kg.FrameDelta.fresh_bytes(), np.int64).copy()))

    def record(self):
        import kmeans_gpu_amd as kg
        return kg.FrameDelta.from_array(self.info.cpu().numpy()).as_tuple()


def _pattern(rng, name, rows, width, k, dtype):
    canvas = rng.integers(0, k + 1, (rows, width)).astype(dtype)
    if name == "nothing":
        index = canvas.copy()
    elif name == "everything":
        index = ((canvas.astype(np.int64) + 1 + rng.integers(0, k, (rows, width))) % (k + 1)).astype(dtype)
    elif name == "corners":
        index = canvas.copy()
        for y, x in ((0, 0), (0, width - 1), (rows - 1, 0), (rows - 1, width - 1)):
            index[y, x] = (int(canvas[y, x]) + 1) % (k + 1)
    else:                                                           # a tenth of the pixels, slot k on both sides
        index = np.where(rng.random((rows, width)) < 0.1, rng.integers(0, k + 1, (rows, width)), canvas).astype(dtype)
        index[rng.random((rows, width)) < 0.01] = k
    return index, canvas


def _delta_cases(torch, processor, fmt, width, rows, offsets, patterns):
    st = torch.cuda.current_stream().cuda_stream
    dtype = _np_dtype(fmt)
    rng = np.random.default_rng(width * 7 + rows + fmt)
    for offs in offsets:
        dev = _Dev(torch, fmt, width * rows, offs)
        for name in patterns:
            k = (255 if fmt == FMT8 else 3072) if name != "corners" else (7 if fmt == FMT8 else 300)
            index, canvas = _pattern(rng, name, rows, width, k, dtype)
            want_d, want_c, want_rec = R.delta(index, canvas, k)
            dev.put(0, index); dev.put(1, canvas); dev.put(2, np.full(width * rows, _sentinel(fmt), dtype)); dev.fresh()
            processor.frame_delta(dev.ptr(0), dev.ptr(1), width, rows, 0, fmt, k, dev.ptr(2), dev.info.data_ptr(), st)
            torch.cuda.synchronize()
            what = f"{name}, offsets {offs}"
            assert dev.record() == want_rec, what
            assert np.array_equal(dev.get(2, (rows, width)), want_d), what
            assert np.array_equal(dev.get(1, (rows, width)), want_c), what
            assert np.array_equal(dev.get(0, (rows, width)), index), what
            if name == "nothing":
                assert dev.record() == R.FRESH
            if name != "random" or rows < 2:
                continue
            # the same frame in two bands, in both orders, on two streams: the same maps and the same record
            cut = rows // 2
            other = torch.cuda.Stream()
            for order in ((0, 1), (1, 0)):
                dev.put(1, canvas); dev.put(2, np.full(width * rows, _sentinel(fmt), dtype)); dev.fresh()
                torch.cuda.synchronize()
                for b in order:
                    r0, r1 = (0, cut) if b == 0 else (cut, rows)
                    processor.frame_delta(dev.ptr(0, r0 * width), dev.ptr(1, r0 * width), width, r1 - r0, r0, fmt, k,
                                          dev.ptr(2, r0 * width), dev.info.data_ptr(), st if b == 0 else other.cuda_stream)
                torch.cuda.synchronize()
                assert dev.record() == want_rec, f"{what}, bands {order}"
                assert np.array_equal(dev.get(2, (rows, width)), want_d) and np.array_equal(dev.get(1, (rows, width)), want_c)


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
@pytest.mark.parametrize("width,rows", SHAPES)
def test_delta_kernel(torch_cuda, processor, fmt, width, rows):
    _delta_cases(torch_cuda, processor, fmt, width, rows, OFFSETS[:2] if width * rows > 1 << 20 else OFFSETS, PATTERNS)


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
def test_delta_kernel_many_tiles_per_workgroup(torch_cuda, processor, fmt):
    _delta_cases(torch_cuda, processor, fmt, MANY_TILES[0], MANY_TILES[1], [(3, 3, 3)], ("corners", "random"))


PROBE_BANDS = [(name, 0, 0) for name, _, _, _ in tile_walk.shapes(1024)] + [("below", 3, 0), ("below", 0, tile_walk.BAND_ROW0)]


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
@pytest.mark.parametrize("name,offs,row0", PROBE_BANDS)
def test_delta_box_of_single_pixels_over_several_tiles_per_workgroup(torch_cuda, processor, fmt, name, offs, row0):
    """offs: elements the three pointers lie past a 16-byte boundary (3: a partial first chunk); row0: the band starts there"""
    tile = tile_walk.tile_elems("delta", 1 if fmt == FMT8 else 2)
    _, width, rows, per = next(s for s in tile_walk.shapes(tile) if s[0] == name)
    state = probe_run.DeltaState(torch_cuda, processor, None, fmt, width, rows, offs)
    assert state.shift(0) == offs
    probe_run.drive(state, per, row0)


def test_delta_refusals(torch_cuda, processor):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    st = torch.cuda.current_stream().cuda_stream
    a = torch.zeros(64, dtype=torch.uint8, device="cuda")
    b = torch.full((64,), 3, dtype=torch.uint8, device="cuda")
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    info = torch.zeros(4, dtype=torch.int64, device="cuda")

    def call(index=None, canvas=None, width=8, rows=8, fmt=FMT8, k=5, delta=None, rec=None):
        processor.frame_delta(a.data_ptr() if index is None else index, b.data_ptr() if canvas is None else canvas, width, rows, 0, fmt, k,
                              d.data_ptr() if delta is None else delta, info.data_ptr() if rec is None else rec, st)

    def still_works():
        b.fill_(3)
        info.copy_(torch.from_numpy(np.frombuffer(kg.FrameDelta.fresh_bytes(), np.int64).copy()))
        call()
        torch.cuda.synchronize()
        assert kg.FrameDelta.from_array(info.cpu().numpy()).as_tuple() == (64, 0, 0, 0, 8, 8)
        assert bool((d == 0).all()) and bool((b == 0).all())

    still_works()
    for kwargs, text in (({"fmt": 0}, "RGBA8"), ({"fmt": FMT8, "k": 256}, "INDEX16"), ({"fmt": 3}, "format"), ({"k": 0}, "k = 0"),
                         ({"width": 0}, "zero"), ({"rows": 0}, "zero"), ({"fmt": FMT16, "delta": d.data_ptr() + 1}, "aligned"),
                         ({"rec": info.data_ptr() + 4}, "aligned")):
        with pytest.raises(kg.KmgError, match=text) as e:
            call(**kwargs)
        assert e.value.status == -1
        still_works()
    L = kg.lib()
    for args in ((None, b, d, info), (a, None, d, info), (a, b, None, info), (a, b, d, None)):
        ptrs = [C.c_void_p(x.data_ptr()) if x is not None else None for x in args]
        assert L.kmg_dev_frame_delta(processor.handle, ptrs[0], ptrs[1], 8, 8, 0, FMT8, 5, ptrs[2], ptrs[3], C.c_void_p(st)) == -1
        assert b"NULL" in L.kmg_last_error()
        still_works()
    assert L.kmg_dev_frame_delta(None, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), 8, 8, 0, FMT8, 5, C.c_void_p(d.data_ptr()),
                                 C.c_void_p(info.data_ptr()), C.c_void_p(st)) == -1
    still_works()


# ---- the shared palette ----------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def crops(tokyo):
    return [np.ascontiguousarray(tokyo[10:210, 20:320]), np.ascontiguousarray(tokyo[300:431, 500:597]),
            np.ascontiguousarray(tokyo[200:456, 100:356])]                 # 300x200 (shrunk), 97x131, 256x256


_want = {}


def _reference(oracle, name, frames, k, **kw):
    if (name, k) not in _want:
        _want[(name, k)] = R.centroids(oracle, frames, k, **kw)
    return _want[(name, k)]


@pytest.mark.parametrize("strategy", ["scan", "table"])
def test_one_frame_is_the_single_image_call(torch_cuda, processor, oracle, tokyo, strategy):
    set_strategy(strategy)
    h, w = tokyo.shape[:2]
    with processor.sequence() as seq:
        seq.add(tokyo)
        import kmeans_gpu_amd as kg
        sw, sh = kg.resized_dims(w, h)
        assert seq.info() == (1, sw * sh)
        assert np.array_equal(seq.palette(8), processor.palette(8, tokyo))
        pal, idx = processor.reduce_indexed(8, tokyo)
        assert np.array_equal(seq.output(8, 0, FMT8, w, h), pal)
        got, _, full = seq.frame(tokyo, delta=False)
        assert full and np.array_equal(got, idx)
        assert np.array_equal(_bits(seq.centroids(8)), _bits(_reference(oracle, "tokyo", [tokyo], 8)))


@pytest.mark.parametrize("strategy", ["scan", "table"])
@pytest.mark.parametrize("k", [2, 8, 64])
def test_frames_of_different_sizes(torch_cuda, processor, oracle, crops, strategy, k):
    torch = torch_cuda
    set_strategy(strategy)
    want = _reference(oracle, "crops", crops, k)
    with processor.sequence() as seq:
        seq.add(crops[0])
        d = torch.from_numpy(crops[1]).cuda()                              # one of them from device memory
        seq.add_device(d.data_ptr(), crops[1].shape[1], crops[1].shape[0], torch.cuda.current_stream().cuda_stream)
        seq.add(crops[2])
        import kmeans_gpu_amd as kg
        sw, sh = kg.resized_dims(300, 200)
        assert (sw, sh) != (300, 200) and seq.info() == (3, sw * sh + 97 * 131 + 256 * 256)
        assert np.array_equal(_bits(seq.centroids(k)), _bits(want))
        assert np.array_equal(seq.palette(k), R.sorted_palette(oracle, want))
        seq.clear()
        assert seq.info() == (0, 0)
        seq.add(crops[2])
        assert np.array_equal(seq.palette(k), processor.palette(k, crops[2]))   # after clear: a one-frame sequence again


@pytest.mark.parametrize("strategy", ["scan", "table"])
def test_alpha_mode_sequence(torch_cuda, oracle, strategy):
    import kmeans_gpu_amd as kg
    set_strategy(strategy)
    t = 128
    frames = [alpha_ref.sprite(seed=5), np.zeros((40, 30, 4), np.uint8), alpha_ref.sprite(h=300, w=280, seed=6)]
    want = _reference(oracle, "sprites", frames, 6, t=t)
    n = sum(int((alpha_ref.shrink(oracle, f, 256)[..., 3] >= t).sum()) for f in frames)
    with kg.ImageProcessor(alpha_cutoff=t) as p, p.sequence() as seq:
        with pytest.raises(kg.KmgError, match="no pixel reaches alpha_cutoff") as e:
            seq.centroids(4)
        assert e.value.status == -1
        seq.add(frames[1])
        assert seq.info() == (1, 0)
        with pytest.raises(kg.KmgError, match="no pixel reaches alpha_cutoff"):
            seq.palette(4)
        seq.clear()
        for f in frames:
            seq.add(f)
        assert seq.info() == (3, n)
        assert np.array_equal(_bits(seq.centroids(6)), _bits(want))
        # one frame with every pixel kept, in alpha mode: the image itself, with its own dimensions
        opaque = frames[0].copy()
        opaque[..., 3] = 255
        seq.clear()
        seq.add(opaque)
        assert np.array_equal(seq.palette(5), p.palette(5, opaque))


def test_large_working_sequence_takes_the_colour_table(torch_cuda, oracle):
    import kmeans_gpu_amd as kg
    frames = [oracle.synth_uniform(31 + i, w * h).reshape(h, w, 4) for i, (w, h) in enumerate(((600, 600), (700, 500), (512, 700)))]
    assert sum(f.shape[0] * f.shape[1] for f in frames) >= 1 << 20
    want = R.centroids(oracle, frames, 16, shrink_max_dim=0, max_iterations=4)
    with kg.ImageProcessor(shrink_max_dim=0, max_iterations=4) as p, p.sequence() as seq:
        for f in frames:
            seq.add(f)
        assert seq.info() == (3, 600 * 600 + 700 * 500 + 512 * 700)
        assert np.array_equal(_bits(seq.centroids(16)), _bits(want))


def test_forty_frames_regrow_the_working_sequence(torch_cuda, oracle, tokyo):
    import kmeans_gpu_amd as kg
    frames = [np.ascontiguousarray(tokyo[7 * i:7 * i + 24 + i, 11 * i:11 * i + 30 + 2 * i]) for i in range(40)]
    want = R.centroids(oracle, frames, 12)
    with kg.ImageProcessor() as p, p.sequence() as seq:
        before = p.debug_block_counts()
        for f in frames:
            seq.add(f)
        after = p.debug_block_counts()
        assert sum(after) - sum(before) >= 4, "W was expected to move to a larger block several times"
        assert seq.info() == (40, sum(f.shape[0] * f.shape[1] for f in frames))
        assert np.array_equal(_bits(seq.centroids(12)), _bits(want))


# ---- frame output -----------------------------------------------------------------------------------------------------------------
def _moving_frames(tokyo, n=4, h=96, w=128):
    back = np.ascontiguousarray(tokyo[150:150 + h, 300:300 + w])
    sprite = alpha_ref.sprite(h=40, w=48, seed=3)
    frames = []
    for t in range(n):
        f = back.copy()
        y, x = 10 + 9 * t, 6 + 21 * t
        m = sprite[..., 3] == 255
        f[y:y + 40, x:x + 48][m] = sprite[m]
        frames.append(f)
    return frames


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_frame_output(torch_cuda, processor, tokyo, mode, fmt):
    torch = torch_cuda
    frames = _moving_frames(tokyo)
    h, w = frames[0].shape[:2]
    k = 24
    st = torch.cuda.current_stream().cuda_stream
    with processor.sequence() as seq:
        for f in frames:
            seq.add(f)
        cent = seq.centroids(k)
        pal = seq.output(k, mode, fmt, w, h)
        assert pal.shape == (k, 4)
        full_maps = []
        for f in frames:                                                   # the full maps, against kmg_dev_apply_format
            d_in = torch.from_numpy(f).cuda()
            d_out = torch.zeros(h * w, dtype=torch.uint8 if fmt == FMT8 else torch.int16, device="cuda")
            processor.apply(d_in.data_ptr(), w, h, 0, cent, mode, d_out.data_ptr(), st, format=fmt)
            torch.cuda.synchronize()
            want = d_out.cpu().numpy().view(_np_dtype(fmt)).reshape(h, w)
            got, info, full = seq.frame(f, delta=False)
            assert full and info.as_tuple() == R.FRESH and got.dtype == _np_dtype(fmt)
            assert np.array_equal(got, want)
            full_maps.append(want)
        pal2 = seq.output(k, mode, fmt, w, h)                              # a second begin: a fresh canvas
        assert np.array_equal(pal2, pal)
        coded, canvas = [], np.full((h, w), k, _np_dtype(fmt))
        for f, I in zip(frames + [frames[-1]], full_maps + [full_maps[-1]]):
            got, info, full = seq.frame(f, delta=True)
            want_d, canvas, want_rec = R.delta(I, canvas, k)
            assert not full and info.as_tuple() == want_rec
            assert np.array_equal(got, want_d)
            coded.append((got, full))
        assert np.array_equal(coded[0][0], full_maps[0])                   # the first delta IS I_0
        assert info.rect is None and (got == k).all()                      # the repeated frame: nothing changed
        for shown, I in zip(R.replay(coded, k), full_maps + [full_maps[-1]]):
            assert np.array_equal(shown, I)
        if mode == 0:
            assert 0 < coded[1][0].size and (coded[1][0] != k).sum() < h * w // 2   # a moving sprite changes a part of the frame


def test_a_pixel_that_turns_transparent_sends_the_full_frame(torch_cuda):
    import kmeans_gpu_amd as kg
    a = alpha_ref.sprite(h=96, w=128, seed=5)
    b = np.roll(a, 17, axis=1)
    k = 9
    with kg.ImageProcessor(alpha_cutoff=128) as p, p.sequence() as seq:
        seq.add(a); seq.add(b)
        seq.output(k, 0, FMT8, 128, 96)
        Ia, ia, fa = seq.frame(a)
        assert not fa and ia.changed == int((a[..., 3] >= 128).sum()) and ia.cleared == 0      # (k over a canvas of k: unchanged)
        assert np.array_equal(Ia == k, a[..., 3] < 128)
        Ib, ib, fb = seq.frame(b)
        want_d, _, want_rec = R.delta(Ib, Ia, k)
        assert ib.as_tuple() == want_rec and ib.cleared > 0
        assert fb and np.array_equal(Ib == k, b[..., 3] < 128), "cleared pixels: the full map, is_full = 1"
        Ic, ic, fc = seq.frame(b)                                          # the canvas took the frame all the same
        assert not fc and ic.rect is None and (Ic == k).all()


# ---- lifecycle -----------------------------------------------------------------------------------------------------------------------
def test_lifecycle(torch_cuda, tokyo):
    import kmeans_gpu_amd as kg
    frames = _moving_frames(tokyo, n=2)
    with kg.ImageProcessor() as p:
        seq = p.sequence()
        with pytest.raises(kg.KmgError) as e:
            seq.frame(frames[0])
        assert e.value.status == -1
        out = np.zeros((96, 128), np.uint8)
        rec, full = kg.FrameDelta(), C.c_int()
        L = kg.lib()
        assert L.kmg_sequence_output_frame(seq._h, frames[0].ctypes.data, 1, out.ctypes.data_as(C.c_void_p), C.byref(rec), C.byref(full)) == -1
        assert b"no output is open" in L.kmg_last_error()
        with pytest.raises(kg.KmgError, match="no pixel"):
            seq.output(4, 0, FMT8, 128, 96)                                # nothing added yet
        seq.add(frames[0])
        for bad, text in (((4, 2, FMT8, 128, 96), "meld"), ((256, 0, FMT8, 128, 96), "INDEX16"), ((4, 0, 7, 128, 96), "format"),
                          ((4, 9, FMT8, 128, 96), "mode"), ((4, 0, FMT8, 0, 96), "zero")):
            with pytest.raises(kg.KmgError, match=text):
                seq.output(*bad)
            with pytest.raises(kg.KmgError):
                seq.frame(frames[0])                                       # a refused begin leaves no output open
        pal = seq.output(4, 0, FMT8, 128, 96)
        first = seq.frame(frames[0])
        with pytest.raises(kg.KmgError, match="128 x 96") as e:
            seq.frame(frames[0][:50])
        assert e.value.status == -1
        assert np.array_equal(seq.output(4, 0, FMT8, 128, 96), pal)
        again = seq.frame(frames[0])                                       # begin twice: the second starts from a canvas of k
        assert again[1].changed == 128 * 96 and np.array_equal(again[0], first[0])
        cent = seq.centroids(4)                                            # (of the same W: the centroids of the open output)
        seq.add(frames[1])                                                 # adding while an output is open does not affect it
        assert seq.info()[0] == 2
        assert np.array_equal(seq.frame(frames[0])[0], np.full((96, 128), 4, np.uint8))
        torch = torch_cuda
        d_in = torch.from_numpy(frames[1]).cuda()
        d_out = torch.zeros(96 * 128, dtype=torch.uint8, device="cuda")
        p.apply(d_in.data_ptr(), 128, 96, 0, cent, 0, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream, format=FMT8)
        torch.cuda.synchronize()
        assert np.array_equal(seq.frame(frames[1], delta=False)[0], d_out.cpu().numpy().reshape(96, 128))
        rgba = seq.output(4, 2, 0, 128, 96)                                # RGBA8 takes meld, but no delta
        assert rgba.shape == (4, 4)
        with pytest.raises(kg.KmgError, match="RGBA8"):
            seq.frame(frames[0], delta=True)
        img, _, full = seq.frame(frames[0], delta=False)
        assert full and img.shape == (96, 128, 4)
        seq.end_output()
        with pytest.raises(kg.KmgError):
            seq.frame(frames[0])
        seq.output(4, 3, FMT16, 128, 96)
        seq.frame(frames[1])
        seq.close()                                                        # destroy with an output open
        late = p.sequence()                                                # a sequence that is still alive when its processor closes
        late.add(frames[0])
        # create / add / output / destroy again and again: the blocks are handed out again, none is allocated
        counts = []
        for _ in range(6):
            with p.sequence() as s2:
                for f in frames:
                    s2.add(f)
                s2.output(8, 1, FMT8, 128, 96)
                for f in frames:
                    s2.frame(f)
            counts.append(p.debug_block_counts()[0])
        assert counts[2:] == [counts[2]] * 4, counts


# ---- the Python Sequence and the CLI, end to end -------------------------------------------------------------------------------------
def test_python_sequence_to_apng(torch_cuda, processor, tokyo):
    from kmeans_gpu_amd import apng
    frames = _moving_frames(tokyo)
    k = 16
    with processor.sequence() as seq:
        for f in frames:
            seq.add(f)
        pal = seq.output(k, 1, FMT8, 128, 96)
        full_maps = [seq.frame(f, delta=False)[0] for f in frames]
        seq.output(k, 1, FMT8, 128, 96)
        coded = [(m, info.rect, full) for m, info, full in (seq.frame(f) for f in frames)]
    plte, trns, shown = read_apng(apng.encode(pal, 128, 96, coded))
    assert np.array_equal(plte[:k], pal[:, :3]) and trns == bytes([255] * k + [0])
    for got, want in zip(shown, full_maps):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("alpha", [0, 128])
def test_cli_sequence(torch_cuda, tokyo, tmp_path, capsys, alpha):
    import kmeans_gpu_amd as kg
    from PIL import Image
    from kmeans_gpu_amd import cli
    if alpha:
        a = alpha_ref.sprite(h=96, w=128, seed=5)
        frames = [a, np.roll(a, 17, axis=1), np.roll(a, 17, axis=1)]
    else:
        frames = _moving_frames(tokyo)
    paths = []
    for i, f in enumerate(frames):
        paths.append(str(tmp_path / f"f{i}.png"))
        Image.fromarray(f, "RGBA").save(paths[-1])
    out = str(tmp_path / "anim.png")
    base = ["sequence", "-i", *paths, "-c", "12", "-m", "dither"] + (["--alpha-cutoff", str(alpha)] if alpha else [])
    assert cli.main(base + ["-o", out, "--delay-ms", "50"]) == 0
    assert "Palette: #" in capsys.readouterr().out
    with kg.ImageProcessor(alpha_cutoff=alpha) as p, p.sequence() as seq:
        for f in frames:
            seq.add(f)
        pal = seq.output(12, 1, FMT8, 128, 96)
        full_maps = [seq.frame(f, delta=False)[0] for f in frames]
    plte, trns, shown = read_apng(open(out, "rb").read())
    assert np.array_equal(plte[:12], pal[:, :3])
    assert len(shown) == len(frames)
    for got, want in zip(shown, full_maps):
        assert np.array_equal(got, want)
    full = str(tmp_path / "full.png")
    assert cli.main(base + ["--no-delta", "-o", full]) == 0
    for got, want in zip(read_apng(open(full, "rb").read())[2], full_maps):
        assert np.array_equal(got, want)
