"""Lossy delta frames on the device (include/kmeans_hip.h at kmg_dev_frame_delta_lossy), against tests/hold_ref.py:
  1. k_frame_hold bit for bit -- delta map, canvas, held source and all eight record fields: shapes around the 4-pixel group, the
     1024-pixel tile and the grid cap, both index types, pointers that allow the 16-byte accesses and pointers that force the
     per-pixel path, sentinels around every buffer, five patterns, and a frame in two bands on two streams in both orders; the
     per-lane (x, y) cursor where a workgroup walks several tiles (tests/tile_walk.py, tests/probe_run.py): one-pixel frames, pairs,
     a clear and planted held pixels whose record is known by construction, in bands of 4200, 4100, 2099, 4102, 4102 and 2049 tiles
     of 1024 pixels of the widths 1000 (step_y = 1), 1024 (step_x = 0), 1023, 300 (step_y = 3), 3 and 1 (both formats, all six),
     and as the second of two bands with an odd row0;
  2. refusals, after each of which the processor still works;
  3. the sequence layer: noise under the tolerance in three modes and both formats, exact and lossy frames alternating on one output
     (the held source and the frame buffer swap), a pixel that turns transparent, begin / end / begin at another size;
  4. Sequence.frame(tolerance=) against the C call, and `sequence --lossy` end to end through the APNG reader of
     tests/test_sequence_contract.py."""
import ctypes as C

import numpy as np
import pytest

import alpha_ref
import probe_run
import tile_walk
import hold_ref as H
import sequence_ref
from test_hold_contract import check_invariant
from test_sequence_contract import read_apng

pytestmark = pytest.mark.gpu

FMT8, FMT16 = 1, 2
SHAPES = [(1, 1), (3, 1), (4, 1), (5, 3), (255, 1), (256, 1), (257, 2), (1023, 1), (1024, 1), (1025, 3), (4099, 7)]
# 2048 workgroups x 1024 pixels per tile round: only a larger band makes a workgroup walk several tiles (the prefetch, the
# per-tile coordinate step)
MANY_TILES = (4099, 600)
# elements into the allocations of (source, indices, canvas, held source, delta map).  The 16-byte accesses need the two RGBA8
# buffers at a multiple of 4 words and the three index buffers at a multiple of 4 elements
VECTOR = [(0, 0, 0, 0, 0), (4, 4, 8, 4, 12)]
PER_PIXEL = [(1, 2, 3, 1, 1), (0, 1, 0, 0, 0), (0, 0, 0, 3, 0)]
PATTERNS = ("nothing", "far", "noise", "tenth", "corners")
PAD = 16
WORD = 0xA5C3A5C3


def _np_dtype(fmt):
    return np.uint8 if fmt == FMT8 else np.uint16


def _sentinel(fmt):
    return 0xA5 if fmt == FMT8 else 0xA5C3


class _Dev:
    """the five buffers of a lossy delta call, each `off` elements into a sentinel-filled allocation, and the record"""
    SRC, INDEX, CANVAS, HELD, DELTA = range(5)

    def __init__(self, torch, fmt, n, offs):
        self.torch, self.fmt, self.n, self.offs = torch, fmt, n, offs
        self.bufs = []
        for i in range(5):
            if i in (self.SRC, self.HELD):
                host = np.full(n + 2 * PAD, WORD, np.uint32).view(np.int32)
            else:
                host = np.full(n + 2 * PAD, _sentinel(fmt), _np_dtype(fmt)).view(np.uint8 if fmt == FMT8 else np.int16)
            self.bufs.append(torch.from_numpy(host).cuda())
        self.info = torch.zeros(6, dtype=torch.int64, device="cuda")

    def _words(self, i):
        return i in (self.SRC, self.HELD)

    def ptr(self, i, first=0):
        return self.bufs[i].data_ptr() + self.bufs[i].element_size() * (self.offs[i] + first)

    def put(self, i, a):
        a = np.ascontiguousarray(a)
        flat = a.reshape(-1, 4).view(np.int32).reshape(-1) if self._words(i) else a.reshape(-1).view(np.uint8 if self.fmt == FMT8 else np.int16)
        assert flat.shape[0] == self.n
        self.bufs[i][self.offs[i]:self.offs[i] + self.n] = self.torch.from_numpy(flat).cuda()

    def get(self, i, shape):
        host = self.bufs[i].cpu().numpy()
        host = host.view(np.uint32) if self._words(i) else host.view(_np_dtype(self.fmt))
        o, s = self.offs[i], WORD if self._words(i) else _sentinel(self.fmt)
        assert (host[:o] == s).all() and (host[o + self.n:] == s).all(), "written outside the band"
        body = host[o:o + self.n]
        return body.view(np.uint8).reshape(shape + (4,)) if self._words(i) else body.reshape(shape)

    def fresh(self):
        import kmeans_gpu_amd as kg
        self.info.copy_(self.torch.from_numpy(np.frombuffer(kg.FrameHold.fresh_bytes(), np.int64).copy()))

    def record(self):
        import kmeans_gpu_amd as kg
        return kg.FrameHold.from_array(self.info.cpu().numpy()).as_tuple()


def _near(rng, a, amp):
    out = np.clip(a.astype(np.int64) + rng.integers(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8)
    out[..., 3] = a[..., 3]
    return out


def _pattern(rng, name, rows, width, k, dtype):
    """(source, indices, canvas, held source, tolerance)"""
    held = rng.integers(0, 256, (rows, width, 4)).astype(np.uint8)
    canvas = rng.integers(0, k + 1, (rows, width)).astype(dtype)
    tol = 40000
    if name == "nothing":                                           # every source word equals its held word, no index moves
        return held.copy(), canvas.copy(), canvas, held, tol
    if name == "far":                                               # every pixel far from its anchor: the exact rule
        src = held ^ np.uint8(0x80)
        index = ((canvas.astype(np.int64) + 1 + rng.integers(0, k, (rows, width))) % (k + 1)).astype(dtype)
        return src, index, canvas, held, tol
    if name == "noise":                                             # noise under the tolerance, indices flicker as a dither's do
        canvas = rng.integers(0, k, (rows, width)).astype(dtype)
        flick = rng.random((rows, width)) < 0.6
        index = np.where(flick, (canvas.astype(np.int64) + 1) % k, canvas).astype(dtype)
        return _near(rng, held, 1), index, canvas, held, tol
    if name == "corners":
        src, index = held.copy(), canvas.copy()
        for y, x in ((0, 0), (0, width - 1), (rows - 1, 0), (rows - 1, width - 1)):
            src[y, x, :3] = held[y, x, :3] ^ 0x80
            index[y, x] = (int(canvas[y, x]) + 1) % (k + 1)
        return src, index, canvas, held, tol
    # a tenth far away, the rest still or within the noise; slot k on both sides
    kind = rng.random((rows, width))
    src = np.where((kind < 0.1)[..., None], held ^ np.uint8(0x80), np.where((kind < 0.6)[..., None], _near(rng, held, 2), held)).astype(np.uint8)
    src[..., 3] = rng.integers(0, 256, (rows, width))
    index = np.where(rng.random((rows, width)) < 0.5, rng.integers(0, k + 1, (rows, width)), canvas).astype(dtype)
    index[rng.random((rows, width)) < 0.02] = k
    canvas[rng.random((rows, width)) < 0.02] = k
    return src, index, canvas, held, 3000


def _expectations(oracle, name, case, k, want):
    """what the pattern is there to show, stated on the reference's own result"""
    src, index, canvas, held, tol = case
    d, new_canvas, new_held, rec = want
    if name == "nothing":
        assert rec == H.FRESH and (d == k).all()
    elif name == "far":
        holdable = (canvas != k) & (index != k)
        assert int(H.distance(oracle, src, held).reshape(index.shape)[holdable].min(initial=tol + 1)) > tol
        assert rec[:6] == sequence_ref.delta(index, canvas, k)[2] and rec[6:] == (0, 0)
        assert np.array_equal(new_canvas, index) and np.array_equal(new_held, src)
    elif name == "noise":
        assert int(H.distance(oracle, src, held).max()) <= tol
        assert rec[0] == 0 and rec[:6] == H.FRESH[:6] and rec[6] == int((index != canvas).sum())
        assert (index.size < 8 or rec[6] > 0) and np.array_equal(new_canvas, canvas) and np.array_equal(new_held, held)
    elif name == "corners":
        rows, width = index.shape
        assert rec[2:6] == (0, 0, width, rows) and rec[0] == len({(0, 0), (0, width - 1), (rows - 1, 0), (rows - 1, width - 1)})


_large = {}


def _large_case(oracle, name, rows, width, k):
    """the band of MANY_TILES and its reference, made once for both formats (indices below 256 either way)"""
    if name not in _large:
        case = _pattern(np.random.default_rng(99), name, rows, width, k, np.uint8)
        _large[name] = (case, H.hold(oracle, *case[:4], k, case[4]))
    return _large[name]


def _run(torch, processor, dev, case, k, width, rows, fmt, bands=None):
    st = torch.cuda.current_stream().cuda_stream
    src, index, canvas, held, tol = case
    dtype = _np_dtype(fmt)
    dev.put(dev.SRC, src); dev.put(dev.INDEX, index.astype(dtype)); dev.put(dev.CANVAS, canvas.astype(dtype)); dev.put(dev.HELD, held)
    dev.put(dev.DELTA, np.full(width * rows, _sentinel(fmt), dtype)); dev.fresh()
    torch.cuda.synchronize()
    for r0, r1, stream in (bands or [(0, rows, st)]):
        processor.frame_delta_lossy(dev.ptr(dev.SRC, r0 * width), dev.ptr(dev.INDEX, r0 * width), dev.ptr(dev.CANVAS, r0 * width),
                                    dev.ptr(dev.HELD, r0 * width), width, r1 - r0, r0, fmt, k, tol, dev.ptr(dev.DELTA, r0 * width),
                                    dev.info.data_ptr(), stream)
    torch.cuda.synchronize()


def _check(dev, case, want, width, rows, fmt, what):
    dtype = _np_dtype(fmt)
    assert dev.record() == want[3], what
    assert np.array_equal(dev.get(dev.DELTA, (rows, width)), want[0].astype(dtype)), what
    assert np.array_equal(dev.get(dev.CANVAS, (rows, width)), want[1].astype(dtype)), what
    assert np.array_equal(dev.get(dev.HELD, (rows, width)), want[2]), what
    assert np.array_equal(dev.get(dev.SRC, (rows, width)), case[0]) and np.array_equal(dev.get(dev.INDEX, (rows, width)), case[1].astype(dtype)), what


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
@pytest.mark.parametrize("width,rows", SHAPES)
def test_hold_kernel(torch_cuda, processor, oracle, fmt, width, rows):
    torch = torch_cuda
    dtype = _np_dtype(fmt)
    rng = np.random.default_rng(width * 7 + rows + fmt)
    for offs in VECTOR + PER_PIXEL:
        dev = _Dev(torch, fmt, width * rows, offs)
        for name in PATTERNS:
            k = (255 if fmt == FMT8 else 3072) if name != "corners" else (7 if fmt == FMT8 else 300)
            case = _pattern(rng, name, rows, width, k, dtype)
            want = H.hold(oracle, *case[:4], k, case[4])
            _expectations(oracle, name, case, k, want)
            _run(torch, processor, dev, case, k, width, rows, fmt)
            _check(dev, case, want, width, rows, fmt, f"{name}, offsets {offs}")
            if name != "tenth" or rows < 2:
                continue
            # the same frame in two bands, in both orders, on two streams: the same buffers and the same record
            cut, st, other = rows // 2, torch.cuda.current_stream().cuda_stream, torch.cuda.Stream()
            for order in ((0, 1), (1, 0)):
                bands = [((0, cut, st), (cut, rows, other.cuda_stream))[b] for b in order]
                _run(torch, processor, dev, case, k, width, rows, fmt, bands)
                _check(dev, case, want, width, rows, fmt, f"{name}, offsets {offs}, bands {order}")


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
def test_hold_kernel_many_tiles_per_workgroup(torch_cuda, processor, oracle, fmt):
    width, rows = MANY_TILES
    assert width * rows > 2048 * 1024
    k = 200
    for offs, name in ((VECTOR[1], "tenth"), (PER_PIXEL[0], "noise")):
        case, want = _large_case(oracle, name, rows, width, k)
        _expectations(oracle, name, case, k, want)
        dev = _Dev(torch_cuda, fmt, width * rows, offs)
        _run(torch_cuda, processor, dev, case, k, width, rows, fmt)
        _check(dev, case, want, width, rows, fmt, f"{name}, offsets {offs}")


PROBE_BANDS = [(name, 0) for name, _, _, _ in tile_walk.shapes(1024)] + [("below", tile_walk.BAND_ROW0)]


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
@pytest.mark.parametrize("name,row0", PROBE_BANDS)
def test_hold_box_of_single_pixels_over_several_tiles_per_workgroup(torch_cuda, processor, oracle, fmt, name, row0):
    _, width, rows, per = next(s for s in tile_walk.shapes(1024) if s[0] == name)
    probe_run.drive(probe_run.HoldState(torch_cuda, processor, oracle, fmt, width, rows), per, row0)


def test_tolerance_zero_runs_the_kernel(torch_cuda, processor, oracle):
    rng = np.random.default_rng(4)
    src, index, canvas, held, _ = _pattern(rng, "tenth", 9, 77, 40, np.uint8)
    for tol in (0, H.D_MAX, 0xFFFFFFFF):
        case = (src, index, canvas, held, tol)
        want = H.hold(oracle, src, index, canvas, held, 40, tol)
        dev = _Dev(torch_cuda, FMT8, 9 * 77, VECTOR[0])
        _run(torch_cuda, processor, dev, case, 40, 77, 9, FMT8)
        _check(dev, case, want, 77, 9, FMT8, f"tolerance {tol}")
    assert want[3][0] == int(((index != canvas) & ((canvas == 40) | (index == 40))).sum())   # everything holdable is held


def test_hold_refusals(torch_cuda, processor):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    st = torch.cuda.current_stream().cuda_stream
    s = torch.zeros(64, dtype=torch.int32, device="cuda")
    h = torch.zeros(64, dtype=torch.int32, device="cuda")
    a = torch.zeros(64, dtype=torch.uint8, device="cuda")
    b = torch.full((64,), 5, dtype=torch.uint8, device="cuda")
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    info = torch.zeros(6, dtype=torch.int64, device="cuda")

    def call(src=None, index=None, canvas=None, held=None, width=8, rows=8, fmt=FMT8, k=5, delta=None, rec=None):
        processor.frame_delta_lossy(s.data_ptr() if src is None else src, a.data_ptr() if index is None else index,
                                    b.data_ptr() if canvas is None else canvas, h.data_ptr() if held is None else held, width, rows, 0, fmt, k,
                                    100, d.data_ptr() if delta is None else delta, info.data_ptr() if rec is None else rec, st)

    def still_works():
        b.fill_(5); h.fill_(7); s.fill_(9)
        info.copy_(torch.from_numpy(np.frombuffer(kg.FrameHold.fresh_bytes(), np.int64).copy()))
        call()
        torch.cuda.synchronize()
        assert kg.FrameHold.from_array(info.cpu().numpy()).as_tuple() == (64, 0, 0, 0, 8, 8, 0, 0)   # (a canvas of k: nothing to hold)
        assert bool((d == 0).all()) and bool((b == 0).all()) and bool((h == 9).all())

    still_works()
    for kwargs, text in (({"fmt": 0}, "RGBA8"), ({"fmt": FMT8, "k": 256}, "INDEX16"), ({"fmt": 3}, "format"), ({"k": 0}, "k = 0"),
                         ({"width": 0}, "zero"), ({"rows": 0}, "zero"), ({"fmt": FMT16, "delta": d.data_ptr() + 1}, "aligned"),
                         ({"rec": info.data_ptr() + 4}, "aligned"), ({"src": s.data_ptr() + 2}, "aligned"),
                         ({"held": h.data_ptr() + 1}, "aligned")):
        with pytest.raises(kg.KmgError, match=text) as e:
            call(**kwargs)
        assert e.value.status == -1
        still_works()
    L = kg.lib()
    for missing in range(6):
        ptrs = [C.c_void_p(x.data_ptr()) for x in (s, a, b, h, d, info)]
        ptrs[missing] = None
        assert L.kmg_dev_frame_delta_lossy(processor.handle, ptrs[0], ptrs[1], ptrs[2], ptrs[3], 8, 8, 0, FMT8, 5, 100, ptrs[4], ptrs[5],
                                           C.c_void_p(st)) == -1
        assert b"NULL" in L.kmg_last_error()
        still_works()
    ptrs = [C.c_void_p(x.data_ptr()) for x in (s, a, b, h, d, info)]
    assert L.kmg_dev_frame_delta_lossy(None, ptrs[0], ptrs[1], ptrs[2], ptrs[3], 8, 8, 0, FMT8, 5, 100, ptrs[4], ptrs[5], C.c_void_p(st)) == -1
    still_works()


# ---- the sequence layer ----------------------------------------------------------------------------------------------------------
def _noisy(tokyo, n, h, w, amp, seed, block=False, y0=150, x0=300):
    rng = np.random.default_rng(seed)
    base = np.ascontiguousarray(tokyo[y0:y0 + h, x0:x0 + w])
    frames = []
    for t in range(n):
        f = _near(rng, base, amp)
        if block:
            f[4 + 5 * t:20 + 5 * t, 6 + 9 * t:30 + 9 * t, :3] = (250, 20, 30)
        frames.append(f)
    return frames


def _exact_maps(processor, frames, k, mode, fmt, more=()):
    """the frames' own exact maps I_t (and those of `more`, which do not shape the palette): the existing _output_frame on a
    sequence of its own"""
    h, w = frames[0].shape[:2]
    with processor.sequence() as seq:
        for f in frames:
            seq.add(f)
        pal = seq.output(k, mode, fmt, w, h)
        return pal, [seq.frame(f, delta=False)[0] for f in list(frames) + list(more)]


def _drive(seq, frames, tolerances):
    return [seq.frame(f) if tol is None else seq.frame(f, tolerance=tol) for f, tol in zip(frames, tolerances)]


def _same(got, states, k):
    for t, ((m, info, full), s) in enumerate(zip(got, states)):
        assert info.as_tuple() == s["record"], t
        assert full == s["is_full"] and np.array_equal(m, s["map"]), t
    for shown, s in zip(sequence_ref.replay([(m, full) for m, _, full in got], k), states):
        assert np.array_equal(shown, s["canvas"])


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_noise_under_the_tolerance(torch_cuda, processor, oracle, tokyo, mode, fmt):
    import kmeans_gpu_amd as kg
    k, h, w = 24, 96, 128
    frames = _noisy(tokyo, 4, h, w, 2, 21)
    tol = kg.tolerance_of(8.0)
    assert all(int(H.distance(oracle, frames[0], f).max()) <= tol for f in frames[1:])     # the noise stays under the tolerance
    pal, maps = _exact_maps(processor, frames, k, mode, fmt)
    tolerances = [tol] * len(frames)
    states = H.replay(oracle, frames, maps, k, tolerances)
    with processor.sequence() as seq:
        for f in frames:
            seq.add(f)
        assert np.array_equal(seq.output(k, mode, fmt, w, h), pal)
        got = _drive(seq, frames, tolerances)
    assert got[0][0].dtype == _np_dtype(fmt) and isinstance(got[0][1], kg.FrameHold)
    _same(got, states, k)
    check_invariant(oracle, frames, maps, k, tolerances, states)
    assert got[0][1].changed == h * w and np.array_equal(got[0][0], maps[0])              # against a canvas of k the delta IS I_0
    for t in (1, 2, 3):
        assert got[t][1].changed == states[t]["record"][0] == 0 and got[t][1].rect is None
        assert got[t][1].held == int((maps[t] != maps[0]).sum())
        assert int((maps[t] != maps[t - 1]).sum()) > 0, "the exact maps were expected to flicker under the noise"


def test_exact_and_lossy_frames_alternate(torch_cuda, processor, oracle, tokyo):
    k, h, w = 16, 80, 112
    frames = _noisy(tokyo, 8, h, w, 2, 33, block=True)
    _, maps = _exact_maps(processor, frames, k, 1, FMT8)
    tolerances = [None, 9000, None, 9000, 9000, None, None, 9000]     # (an odd and an even number of swaps before a lossy frame)
    states = H.replay(oracle, frames, maps, k, tolerances)
    with processor.sequence() as seq:
        for f in frames:
            seq.add(f)
        seq.output(k, 1, FMT8, w, h)
        got = _drive(seq, frames, tolerances)
        _same(got, states, k)
        # a full exact frame (no KMG_FRAME_DELTA) anchors every pixel as well
        extra = _noisy(tokyo, 2, h, w, 1, 34, block=True)
        m0, _, full = seq.frame(extra[0], delta=False)
        m1, info, full1 = seq.frame(extra[1], tolerance=9000)
    _, emaps = _exact_maps(processor, frames, k, 1, FMT8, more=extra)
    assert full and np.array_equal(m0, emaps[8])
    want = H.hold(oracle, extra[1], emaps[9], emaps[8], extra[0], k, 9000)
    assert not full1 and info.as_tuple() == want[3] and np.array_equal(m1, want[0])
    check_invariant(oracle, frames, maps, k, tolerances, states)
    assert any(s["record"][0] > 0 and s["record"][6] > 0 for s, tol in zip(states, tolerances) if tol is not None)


def test_a_pixel_that_turns_transparent_comes_back_full(torch_cuda, oracle):
    import kmeans_gpu_amd as kg
    a = alpha_ref.sprite(h=96, w=128, seed=5)
    b = np.roll(a, 17, axis=1)
    c = _near(np.random.default_rng(1), b, 1)
    frames, k, tol = [a, b, c], 9, 6000
    with kg.ImageProcessor(alpha_cutoff=128) as p:
        _, maps = _exact_maps(p, frames, k, 0, FMT8)
        states = H.replay(oracle, frames, maps, k, [tol] * 3)
        with p.sequence() as seq:
            for f in frames:
                seq.add(f)
            seq.output(k, 0, FMT8, 128, 96)
            got = _drive(seq, frames, [tol] * 3)
    _same(got, states, k)
    assert not got[0][2] and got[1][2] and got[1][1].cleared > 0 and np.array_equal(got[1][0], maps[1])
    assert not got[2][2] and got[2][1].cleared == 0
    check_invariant(oracle, frames, maps, k, [tol] * 3, states)


def test_begin_frames_end_begin_at_another_size(torch_cuda, oracle, tokyo):
    import kmeans_gpu_amd as kg
    with kg.ImageProcessor() as p, p.sequence() as seq:
        counts = []
        for rnd, (h, w, fmt, mode) in enumerate(((64, 96, FMT8, 1), (33, 57, FMT16, 3)) * 2):
            frames = _noisy(tokyo, 3, h, w, 2, 40 + rnd, block=True)
            seq.clear()
            for f in frames:
                seq.add(f)
            k = 10
            seq.output(k, mode, fmt, w, h)
            maps = [seq.frame(f, delta=False)[0] for f in frames]
            seq.output(k, mode, fmt, w, h)                         # a second begin: a fresh canvas, nothing held
            tolerances = [5000, None, 5000] if rnd % 2 else [5000, 5000, 5000]
            _same(_drive(seq, frames, tolerances), H.replay(oracle, frames, maps, k, tolerances), k)
            if rnd % 2:
                seq.end_output()
                with pytest.raises(kg.KmgError):
                    seq.frame(frames[0], tolerance=5000)
            counts.append(p.debug_block_counts()[0])
        assert counts[2:] == [counts[1]] * 2, counts               # the blocks are handed out again, none is allocated


# ---- Python and the CLI -----------------------------------------------------------------------------------------------------------
def test_python_frame_against_the_c_call(torch_cuda, processor, tokyo):
    import kmeans_gpu_amd as kg
    k, h, w, tol = 12, 48, 64, 7000
    frames = _noisy(tokyo, 3, h, w, 2, 50, block=True)
    L = kg.lib()
    with processor.sequence() as one, processor.sequence() as two:
        for f in frames:
            one.add(f); two.add(f)
        one.output(k, 1, FMT8, w, h); two.output(k, 1, FMT8, w, h)
        for f in frames:
            m, info, full = one.frame(f, tolerance=tol)
            out, rec, is_full = np.zeros((h, w), np.uint8), kg.FrameHold(), C.c_int(-1)
            assert L.kmg_sequence_output_frame_lossy(two._h, f.ctypes.data, kg.FRAME_DELTA, tol, out.ctypes.data_as(C.c_void_p), C.byref(rec),
                                                     C.byref(is_full)) == 0
            assert np.array_equal(m, out) and info.as_tuple() == rec.as_tuple() and full == bool(is_full.value)
        # what the call needs: KMG_FRAME_DELTA, info and is_full, an index format
        f = frames[0]
        for flags, r, fl in ((0, C.byref(rec), C.byref(is_full)), (1, None, C.byref(is_full)), (1, C.byref(rec), None), (3, C.byref(rec), C.byref(is_full))):
            assert L.kmg_sequence_output_frame_lossy(two._h, f.ctypes.data, flags, tol, out.ctypes.data_as(C.c_void_p), r, fl) == -1
        with pytest.raises(kg.KmgError, match="KMG_FRAME_DELTA"):
            one.frame(f, delta=False, tolerance=tol)
        with pytest.raises(kg.KmgError, match="uint32"):
            one.frame(f, tolerance=1 << 32)
        m, info, full = one.frame(frames[-1], tolerance=tol)       # the refusals left the output as it was
        assert info.changed == 0 and (m == k).all()
        one.output(k, 2, 0, w, h)
        with pytest.raises(kg.KmgError, match="RGBA8"):
            one.frame(f, tolerance=tol)
        two.end_output()
        assert L.kmg_sequence_output_frame_lossy(two._h, f.ctypes.data, 1, tol, out.ctypes.data_as(C.c_void_p), C.byref(rec), C.byref(is_full)) == -1
        assert b"no output is open" in L.kmg_last_error()


def test_cli_sequence_lossy(torch_cuda, processor, oracle, tokyo, tmp_path, capsys):
    import kmeans_gpu_amd as kg
    from PIL import Image
    from kmeans_gpu_amd import cli
    frames = _noisy(tokyo, 4, 96, 128, 2, 60, block=True)
    paths = []
    for i, f in enumerate(frames):
        paths.append(str(tmp_path / f"f{i}.png"))
        Image.fromarray(f, "RGBA").save(paths[-1])
    out = str(tmp_path / "anim.png")
    assert cli.main(["sequence", "-i", *paths, "-c", "12", "-m", "dither", "--lossy", "1.5", "--report", "-o", out]) == 0
    text = capsys.readouterr().out
    pal, maps = _exact_maps(processor, frames, 12, 1, FMT8)
    states = H.replay(oracle, frames, maps, 12, [kg.tolerance_of(1.5)] * 4)
    for t, s in enumerate(states):
        assert f"Frame {t}: changed={s['record'][0]} held={s['record'][6]} " in text
    plte, trns, shown = read_apng(open(out, "rb").read())
    assert np.array_equal(plte[:12], pal[:, :3]) and len(shown) == 4
    for got, s in zip(shown, states):
        assert np.array_equal(got, s["canvas"])
    assert 0 < states[1]["record"][0] < int((maps[1] != maps[0]).sum())
