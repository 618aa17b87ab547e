"""Per-frame palettes on the device (include/kmeans_hip.h at kmg_dev_frame_delta_colour and kmg_sequence_output_begin_local; DESIGN.md
4.14), against tests/local_ref.py:
  1. k_frame_local bit for bit -- delta map, shown words, held source and every record field: widths and rows around the 4-pixel
     group and the 1024-pixel tile, both index types at their smallest and largest k, indices above k, a palette with duplicate
     entries and a zero word, every buffer on the vector route and at element offsets 1..3 (the per-pixel route), sentinels around
     every buffer; three uneven bands in reverse order on two streams; a band with several tiles per workgroup; the per-lane (x, y)
     cursor where a workgroup walks several tiles (tests/tile_walk.py, tests/probe_run.py): one-pixel frames, pairs, a clear and
     planted held pixels whose record is known by construction, exact and lossy, in bands of 4200, 4100, 2099, 4102, 4102 and 2049
     tiles of 1024 pixels of the widths 1000 (step_y = 1), 1024 (step_x = 0), 1023, 300 (step_y = 3), 3 and 1 (both formats, all
     six), and as the second of two bands with an odd row0;
  2. the same-palette equivalence with kmg_dev_frame_delta / _lossy on the device, at three tolerances;
  3. a ten-frame random walk, exact and lossy frames alternating, a new palette per frame;
  4. the sequence layer: cold frames against kmg_reduce_indexed, delta frames against the model and the replay, warm frames against
     the oracle, alpha mode, a refused frame, the two kinds of output kept apart, fixed colours, the C++ mirror, the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fixed_ref
import hold_ref
import local_ref as R
import probe_run
import sequence_ref
import tile_walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT8, FMT16 = 1, 2
PAD = 16
WORD = 0xA5C3A5C3
SRC, INDEX, PAL, SHOWN, HELD, DELTA = range(6)
WORDS = (SRC, PAL, SHOWN, HELD)
# elements into the allocations of (source, indices, palette, shown, held source, delta map).  The vector route needs the three
# RGBA8 streams at a multiple of 4 words and the two index buffers at a multiple of 4 elements; the palette is read word by word
VECTOR = [(0, 0, 0, 0, 0, 0), (4, 8, 1, 4, 8, 12)]
PER_PIXEL = [(1, 1, 1, 1, 1, 1), (2, 2, 2, 2, 2, 2), (3, 3, 3, 3, 3, 3), (0, 1, 0, 0, 0, 0), (0, 0, 0, 2, 0, 0), (0, 0, 0, 0, 0, 3)]


def _dtype(fmt):
    return np.uint8 if fmt == FMT8 else np.uint16


def _sentinel(fmt):
    return 0xA5 if fmt == FMT8 else 0xA5C3


class _Dev:
    """the six buffers of a colour-keyed delta call, each `off` elements into a sentinel-filled allocation, and the record"""

    def __init__(self, torch, fmt, n, k, offs):
        self.torch, self.fmt, self.offs = torch, fmt, offs
        self.len = [k if i == PAL else n for i in range(6)]
        self.bufs = []
        for i in range(6):
            if i in WORDS:
                host = np.full(self.len[i] + 2 * PAD, WORD, np.uint32).view(np.int32)
            else:
                host = np.full(n + 2 * PAD, _sentinel(fmt), _dtype(fmt)).view(np.uint8 if fmt == FMT8 else np.int16)
            self.bufs.append(torch.from_numpy(host).cuda())
        self.info = torch.zeros(6, dtype=torch.int64, device="cuda")

    def ptr(self, i, first=0):
        return self.bufs[i].data_ptr() + self.bufs[i].element_size() * (self.offs[i] + first)

    def put(self, i, a):
        a = np.ascontiguousarray(a)
        if i in WORDS:
            flat = (a if a.dtype == np.uint32 else R.words(a)).reshape(-1).view(np.int32)
        else:
            flat = a.reshape(-1).view(np.uint8 if self.fmt == FMT8 else np.int16)
        assert flat.shape[0] == self.len[i]
        self.bufs[i][self.offs[i]:self.offs[i] + self.len[i]] = self.torch.from_numpy(flat.copy()).cuda()

    def get(self, i, shape):
        host = self.bufs[i].cpu().numpy()
        host = host.view(np.uint32) if i in WORDS else host.view(_dtype(self.fmt))
        o, s = self.offs[i], WORD if i in WORDS else _sentinel(self.fmt)
        assert (host[:o] == s).all() and (host[o + self.len[i]:] == s).all(), "written outside the band"
        return host[o:o + self.len[i]].reshape(shape)

    def fresh(self):
        import kmeans_gpu_amd as kg
        self.info.copy_(self.torch.from_numpy(np.frombuffer(kg.FrameHold.fresh_bytes(), np.int64).copy()))

    def record(self, lossy):
        import kmeans_gpu_amd as kg
        rec = kg.FrameHold.from_array(self.info.cpu().numpy()).as_tuple()
        if not lossy:
            assert rec[6:] == (0, 0), "the exact pass touched held / held_sse"
        return rec if lossy else rec[:6]


def _palette(rng, k, special=True):
    """k words with alpha 255; `special`: some entries repeat an earlier one's bytes and one word is zero"""
    rgb = np.zeros(0, np.int64)
    while rgb.shape[0] < k:                                               # k distinct colours
        rgb = np.unique(np.concatenate([rgb, rng.integers(0, 1 << 24, 2 * k + 8)]))
    rgb = rng.permutation(rgb)[:k].astype("<u4")
    pal = np.concatenate([rgb.view(np.uint8).reshape(k, 4)[:, :3], np.full((k, 1), 255, np.uint8)], axis=1)
    if special and k >= 2:
        for j in rng.integers(1, k, max(1, k // 5)):
            pal[j] = pal[rng.integers(0, j)]
        pal[rng.integers(0, k)] = 0
    return np.ascontiguousarray(pal)


def _case(rng, rows, width, k, dtype, top=None):
    """(source, indices, palette, shown, held source): indices up to `top` (default: the type's largest, so above k), shown words
    from this palette, from another one, and zeros; a third of the pixels already show what the frame wants"""
    held = rng.integers(0, 256, (rows, width, 4)).astype(np.uint8)
    kind = rng.random((rows, width))
    near = np.clip(held.astype(np.int64) + rng.integers(-2, 3, held.shape), 0, 255).astype(np.uint8)
    src = np.where((kind < 0.3)[..., None], held, np.where((kind < 0.7)[..., None], near, held ^ np.uint8(0x80))).astype(np.uint8)
    pal = _palette(rng, k)
    top = int(np.iinfo(dtype).max) if top is None else top
    index = rng.integers(0, k + 1, (rows, width)).astype(dtype)
    if top > k:
        hi = rng.random((rows, width)) < 0.05
        index[hi] = rng.integers(k + 1, top + 1, int(hi.sum())).astype(dtype)
    table = np.concatenate([R.words(_palette(rng, k, special=False)), np.zeros(1, np.uint32)])
    was = rng.integers(0, k + 1, (rows, width))
    shown = np.where(rng.random((rows, width)) < 0.5, R.lookup(was, pal, k)[1], table[was]).astype(np.uint32)
    same = rng.random((rows, width)) < 0.33
    shown[same] = R.lookup(index, pal, k)[1][same]
    return src, index, pal, shown, held


def _run(torch, processor, dev, case, k, width, rows, fmt, tol, bands=None):
    """tol None: the exact pass.  bands: [(first row, end row, stream)]"""
    st = torch.cuda.current_stream().cuda_stream
    src, index, pal, shown, held = case
    dtype = _dtype(fmt)
    dev.put(SRC, src); dev.put(INDEX, index.astype(dtype)); dev.put(PAL, pal); dev.put(SHOWN, shown); dev.put(HELD, held)
    dev.put(DELTA, np.full(width * rows, _sentinel(fmt), dtype)); dev.fresh()
    torch.cuda.synchronize()
    for r0, r1, stream in (bands or [(0, rows, st)]):
        if tol is None:
            processor.frame_delta_colour(dev.ptr(INDEX, r0 * width), dev.ptr(PAL), dev.ptr(SHOWN, r0 * width), width, r1 - r0, r0, fmt, k,
                                         dev.ptr(DELTA, r0 * width), dev.info.data_ptr(), stream)
        else:
            processor.frame_delta_colour_lossy(dev.ptr(SRC, r0 * width), dev.ptr(INDEX, r0 * width), dev.ptr(PAL), dev.ptr(SHOWN, r0 * width),
                                               dev.ptr(HELD, r0 * width), width, r1 - r0, r0, fmt, k, tol, dev.ptr(DELTA, r0 * width),
                                               dev.info.data_ptr(), stream)
    torch.cuda.synchronize()


def _want(oracle, case, k, tol):
    src, index, pal, shown, held = case
    if tol is None:
        d, new_shown, rec = R.colour(index, shown, pal, k)
        return d, new_shown, held, rec
    return R.lossy(oracle, src, index, shown, held, pal, k, tol)


def _check(dev, case, want, k, width, rows, fmt, lossy, what):
    dtype = _dtype(fmt)
    assert dev.record(lossy) == want[3], what
    assert np.array_equal(dev.get(DELTA, (rows, width)), want[0].astype(dtype)), what
    assert np.array_equal(dev.get(SHOWN, (rows, width)), want[1]), what
    assert np.array_equal(R.unwords(dev.get(HELD, (rows, width))), want[2]), what
    assert np.array_equal(R.unwords(dev.get(SRC, (rows, width))), case[0]) and np.array_equal(dev.get(INDEX, (rows, width)), case[1].astype(dtype)), what
    assert np.array_equal(R.unwords(dev.get(PAL, (k,))), case[2]), what


KS = {FMT8: (1, 2, 255), FMT16: (1, 256, 3072)}


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
@pytest.mark.parametrize("width", [1, 3, 37, 64, 1027])
def test_pass_against_the_reference(torch_cuda, processor, oracle, fmt, width):
    dtype = _dtype(fmt)
    rng = np.random.default_rng(width * 7 + fmt)
    sent = held_some = 0
    for rows in (1, 2, 7):
        for k in KS[fmt]:
            case = _case(rng, rows, width, k, dtype)
            wants = {tol: _want(oracle, case, k, tol) for tol in (None, 3000)}
            sent += wants[3000][3][0]
            held_some += wants[3000][3][6]
            for offs in VECTOR + PER_PIXEL:
                dev = _Dev(torch_cuda, fmt, width * rows, k, offs)
                for tol, want in wants.items():
                    _run(torch_cuda, processor, dev, case, k, width, rows, fmt, tol)
                    _check(dev, case, want, k, width, rows, fmt, tol is not None, f"rows {rows}, k {k}, tolerance {tol}, offsets {offs}")
    assert sent > 0 and (width < 37 or held_some > 0)


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
def test_three_uneven_bands_in_reverse_order_on_two_streams(torch_cuda, processor, oracle, fmt):
    torch = torch_cuda
    width, rows, k = 1027, 11, 200 if fmt == FMT8 else 900
    case = _case(np.random.default_rng(fmt), rows, width, k, _dtype(fmt))
    st, other = torch.cuda.current_stream().cuda_stream, torch.cuda.Stream()
    bands = [(7, 11, st), (2, 7, other.cuda_stream), (0, 2, st)]
    for offs in (VECTOR[1], PER_PIXEL[0]):
        dev = _Dev(torch, fmt, width * rows, k, offs)
        for tol in (None, 3000):
            want = _want(oracle, case, k, tol)
            _run(torch, processor, dev, case, k, width, rows, fmt, tol)
            _check(dev, case, want, k, width, rows, fmt, tol is not None, f"one call, tolerance {tol}")
            _run(torch, processor, dev, case, k, width, rows, fmt, tol, bands)
            _check(dev, case, want, k, width, rows, fmt, tol is not None, f"three bands, tolerance {tol}, offsets {offs}")


_large = {}


def _large_case(oracle):
    """2101 x 1024: 2101 tiles for at most 2048 workgroups, so tile_run's `per` is 2 -- made once for both formats"""
    if not _large:
        width, rows, k = 2101, 1024, 200
        assert (width * rows + 1023) // 1024 > 2048
        case = _case(np.random.default_rng(99), rows, width, k, np.uint8)
        _large["case"] = case
        _large["want"] = {tol: _want(oracle, case, k, tol) for tol in (None, 3000)}
    return _large["case"], _large["want"]


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
def test_more_tiles_than_workgroups(torch_cuda, processor, oracle, fmt):
    width, rows, k = 2101, 1024, 200
    case, wants = _large_case(oracle)
    dev = _Dev(torch_cuda, fmt, width * rows, k, VECTOR[1])
    for tol, want in wants.items():
        _run(torch_cuda, processor, dev, case, k, width, rows, fmt, tol)
        _check(dev, case, want, k, width, rows, fmt, tol is not None, f"tolerance {tol}")
        assert want[3][0] > 0


PROBE_BANDS = [(name, 0) for name, _, _, _ in tile_walk.shapes(1024)] + [("below", tile_walk.BAND_ROW0)]


@pytest.mark.parametrize("lossy", [False, True])
@pytest.mark.parametrize("fmt", [FMT8, FMT16])
@pytest.mark.parametrize("name,row0", PROBE_BANDS)
def test_local_box_of_single_pixels_over_several_tiles_per_workgroup(torch_cuda, processor, oracle, fmt, name, row0, lossy):
    _, width, rows, per = next(s for s in tile_walk.shapes(1024) if s[0] == name)
    probe_run.drive(probe_run.LocalState(torch_cuda, processor, oracle, fmt, width, rows, lossy), per, row0)


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
def test_same_palette_equals_the_index_passes_on_the_device(torch_cuda, processor, oracle, fmt):
    """one palette of distinct non-zero words, indices <= k: kmg_dev_frame_delta / _lossy and the colour passes write the same delta
    map and record, and shown == P'[canvas] afterwards"""
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    dtype, t_dtype = _dtype(fmt), torch.uint8 if fmt == FMT8 else torch.int16
    rng = np.random.default_rng(31 + fmt)
    width, rows, k = 203, 9, 255 if fmt == FMT8 else 600
    pal = _palette(rng, k, special=False)
    assert len(set(R.words(pal).tolist())) == k and (R.words(pal) != 0).all()
    src, index, _, _, held = _case(rng, rows, width, k, dtype, top=k)
    canvas = np.where(rng.random((rows, width)) < 0.5, index, rng.integers(0, k + 1, (rows, width))).astype(dtype)
    shown = R.lookup(canvas, pal, k)[1]
    st = torch.cuda.current_stream().cuda_stream
    D = hold_ref.distance(oracle, src, held)
    middle = int(np.median(D[D > 0]))
    for tol in (None, 0, middle, 0xFFFFFFFF):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8 if fmt == FMT8 else np.int16).copy()).cuda()
        d_index, d_canvas, d_delta = up(index), up(canvas), torch.zeros(rows * width, dtype=t_dtype, device="cuda")
        d_src, d_held = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(held.copy()).cuda()
        info = torch.from_numpy(np.frombuffer(kg.FrameHold.fresh_bytes(), np.int64).copy()).cuda()
        if tol is None:
            processor.frame_delta(d_index.data_ptr(), d_canvas.data_ptr(), width, rows, 0, fmt, k, d_delta.data_ptr(), info.data_ptr(), st)
        else:
            processor.frame_delta_lossy(d_src.data_ptr(), d_index.data_ptr(), d_canvas.data_ptr(), d_held.data_ptr(), width, rows, 0, fmt, k, tol,
                                        d_delta.data_ptr(), info.data_ptr(), st)
        torch.cuda.synchronize()
        dev = _Dev(torch, fmt, width * rows, k, VECTOR[0])
        _run(torch, processor, dev, (src, index, pal, shown, held), k, width, rows, fmt, tol)
        rec = kg.FrameHold.from_array(info.cpu().numpy()).as_tuple()
        assert dev.record(True) == rec, tol
        assert np.array_equal(dev.get(DELTA, (rows, width)), d_delta.cpu().numpy().view(dtype).reshape(rows, width)), tol
        new_canvas = d_canvas.cpu().numpy().view(dtype).reshape(rows, width)
        assert np.array_equal(dev.get(SHOWN, (rows, width)), R.lookup(new_canvas, pal, k)[1]), tol
        if tol is not None:
            assert np.array_equal(R.unwords(dev.get(HELD, (rows, width))), d_held.cpu().numpy()), tol
        if tol == middle:
            want = hold_ref.hold(oracle, src, index, canvas, held, k, tol)[3]
            assert want == rec and want[0] > 0 and want[6] > 0          # the reference holds some pixels and sends some


def test_ten_frame_random_walk(torch_cuda, processor, oracle):
    """exact and lossy frames alternate over one state, every frame with a new random palette"""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    width, rows, k, fmt = 133, 21, 40, FMT8
    dev = _Dev(torch, fmt, width * rows, k, VECTOR[0])
    shown, held = np.zeros((rows, width), np.uint32), np.zeros((rows, width, 4), np.uint8)
    src = rng.integers(0, 256, (rows, width, 4)).astype(np.uint8)
    index = rng.integers(0, k, (rows, width)).astype(np.uint8)
    pal = _palette(rng, k)
    n_held = n_sent = 0
    for t in range(10):
        if t:
            move = rng.random((rows, width)) < 0.3
            src = np.where(move[..., None], rng.integers(0, 256, src.shape), np.clip(src.astype(np.int64) + rng.integers(-1, 2, src.shape), 0, 255)).astype(np.uint8)
            index = np.where(rng.random((rows, width)) < 0.5, index, rng.integers(0, k + 1, (rows, width))).astype(np.uint8)
            new = _palette(rng, k)
            keep = rng.random(k) < 0.5                                   # half of the entries keep their colour
            pal = np.where(keep[:, None], pal, new)
        tol = None if t % 2 == 0 else 2500
        case = (src, index, pal, shown, held)
        want = _want(oracle, case, k, tol)
        if tol is None:
            want = (want[0], want[1], src, want[3])                      # the caller's part of an exact frame: held source = the frame
        _run(torch, processor, dev, case, k, width, rows, fmt, tol)
        if tol is None:
            dev.put(HELD, src)
        _check(dev, case, want, k, width, rows, fmt, tol is not None, f"frame {t}")
        shown, held = want[1], want[2]
        n_sent += want[3][0]
        n_held += want[3][6] if tol is not None else 0
    assert n_sent > 0 and n_held > 0


def test_refusals(torch_cuda, processor):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    st = torch.cuda.current_stream().cuda_stream
    words = [torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(4)]         # source, palette, shown, held
    idx, d = torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    info = torch.zeros(6, dtype=torch.int64, device="cuda")

    def call(lossy, fmt=FMT8, k=5, width=8, rows=8, pal=None, shown=None, rec=None):
        pal = words[1].data_ptr() if pal is None else pal
        shown = words[2].data_ptr() if shown is None else shown
        rec = info.data_ptr() if rec is None else rec
        if lossy:
            processor.frame_delta_colour_lossy(words[0].data_ptr(), idx.data_ptr(), pal, shown, words[3].data_ptr(), width, rows, 0, fmt, k, 10,
                                               d.data_ptr(), rec, st)
        else:
            processor.frame_delta_colour(idx.data_ptr(), pal, shown, width, rows, 0, fmt, k, d.data_ptr(), rec, st)

    for lossy in (False, True):
        for kwargs, text in (({"fmt": 0}, "RGBA8"), ({"k": 256}, "INDEX16"), ({"fmt": 3}, "format"), ({"k": 0}, "k = 0"), ({"width": 0}, "zero"),
                             ({"rows": 0}, "zero"), ({"fmt": FMT16, "k": 3073}, "k = 3073"), ({"pal": words[1].data_ptr() + 2}, "aligned"),
                             ({"shown": words[2].data_ptr() + 1}, "aligned"), ({"rec": info.data_ptr() + 4}, "aligned"), ({"pal": 0}, "NULL")):
            with pytest.raises(kg.KmgError, match=text) as e:
                call(lossy, **kwargs)
            assert e.value.status == -1
        words[1].fill_(0x01020304); words[2].zero_()
        info.copy_(torch.from_numpy(np.frombuffer(kg.FrameHold.fresh_bytes(), np.int64).copy()))
        call(lossy)
        torch.cuda.synchronize()
        assert kg.FrameHold.from_array(info.cpu().numpy()).as_tuple() == (64, 0, 0, 0, 8, 8, 0, 0)
        assert bool((words[2] == 0x01020304).all()) and bool((d == 0).all())


# ---- the sequence layer ----------------------------------------------------------------------------------------------------------
def _frames(n, h, w, seed, alpha=False):
    """frames of synth's uniform stream laid over a gradient: a scene whose colours drift, with a block that moves"""
    from kmeans_gpu_amd import synth
    noise = synth.uniform_rgba_numpy(seed, h * w).reshape(h, w, 4).astype(np.int64)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for t in range(n):
        f = np.zeros((h, w, 4), np.int64)
        f[..., 0] = (x * 255) // max(w - 1, 1) + 20 * t
        f[..., 1] = (y * 255) // max(h - 1, 1)
        f[..., 2] = 128 + 30 * t
        f[..., :3] += noise[..., :3] // 16
        f[3 + 2 * t:12 + 2 * t, 5 + 3 * t:17 + 3 * t, :3] = (250, 20, 30)
        f[..., 3] = 255
        if alpha:
            f[..., 3] = np.where((x + 5 * t) % w < w // 3, 0, 255)
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


SIZES = [(64, 96, 8), (29, 37, 64)]


@pytest.mark.parametrize("h,w,k", SIZES)
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_cold_frames_are_reduce_indexed_and_replay(torch_cuda, processor, oracle, mode, h, w, k):
    import kmeans_gpu_amd as kg
    frames = _frames(4, h, w, 5)
    own = [processor.reduce_indexed(k, f, kg.Algorithm.Kmeans, mode) for f in frames]
    palettes, maps = [p for p, _ in own], [m for _, m in own]
    with processor.sequence() as seq:
        seq.output_local(k, mode, FMT8, w, h)
        for f, P, I in zip(frames, palettes, maps):
            m, pal, info, full = seq.frame_local(f, delta=False)
            assert full and np.array_equal(m, I) and np.array_equal(pal, P) and info.as_tuple() == R.FRESH8
        # delta frames on a fresh output: exact, lossy, exact, lossy
        tolerances = [None, 6000, None, 6000]
        states = R.encode(oracle, frames, maps, palettes, k, tolerances)
        seq.output_local(k, mode, FMT8, w, h)
        got = [seq.frame_local(f, tolerance=tol) for f, tol in zip(frames, tolerances)]
    for t, ((m, pal, info, full), s) in enumerate(zip(got, states)):
        assert np.array_equal(pal, palettes[t]) and info.as_tuple() == s["record"], t
        assert full == s["is_full"] and np.array_equal(m, s["map"]), t
    shown = R.replay_colour([(m, pal, full) for m, pal, _, full in got], k)
    for t, s in enumerate(states):
        assert np.array_equal(shown[t], s["shown"]), t
        if tolerances[t] is None:
            assert np.array_equal(shown[t], R.lookup(maps[t], palettes[t], k)[1])
    assert got[0][2].changed == h * w and not got[0][3]
    assert 0 < states[1]["record"][0] < h * w


@pytest.mark.parametrize("h,w,k", SIZES)
@pytest.mark.parametrize("mode", [0, 1])
def test_warm_frames_equal_the_oracle_model(torch_cuda, processor, oracle, mode, h, w, k):
    frames = _frames(3, h, w, 9)
    cents, its = [sequence_ref.centroids(oracle, frames[:1], k)], []
    for f in frames[1:]:
        c, it = R.warm_centroids(oracle, f.reshape(-1, 4), cents[-1])
        cents.append(c)
        its.append(it)
    palettes = [fixed_ref.palette_bytes(oracle, c) for c in cents]
    maps = []
    for f, c in zip(frames, cents):
        lab = oracle.rgb_to_lab(f.reshape(-1, 4))
        labels = oracle.assign(lab, c) if mode == 0 else oracle.dither(lab, w, h, c)
        maps.append(labels.reshape(h, w).astype(np.uint8))
    states = R.encode(oracle, frames, maps, palettes, k, [None] * 3)
    with processor.sequence() as seq:
        seq.output_local(k, mode, FMT8, w, h, warm=True)
        got = [seq.frame_local(f) for f in frames]
        cold = processor.reduce_indexed(k, frames[1], reduce_mode=mode)
    for t, ((m, pal, info, full), s) in enumerate(zip(got, states)):
        assert np.array_equal(pal, palettes[t]), t
        assert info.as_tuple() == s["record"] and full == s["is_full"] and np.array_equal(m, s["map"]), t
    print(f"warm Lloyd iterations: {its}; palette of frame 1 warm == cold: {np.array_equal(cold[0], palettes[1])}")


def test_alpha_mode_refusal_and_the_frame_after_it(torch_cuda, oracle):
    import kmeans_gpu_amd as kg
    h, w, k = 64, 96, 8
    frames = _frames(3, h, w, 3, alpha=True)
    nothing = frames[0].copy()
    nothing[..., 3] = 0
    tolerances = [None, 5000, None]

    def drive(seq, last_in_full):
        seq.output_local(k, 1, FMT8, w, h, warm=True)
        got = [seq.frame_local(frames[0])]
        with pytest.raises(kg.KmgError, match="alpha_cutoff") as e:
            seq.frame_local(nothing)
        assert e.value.status == -1
        # shown and held are as they were, and the frame after the failed one starts cold: reduce_indexed's palette
        got.append(seq.frame_local(frames[1], tolerance=5000))
        got.append(seq.frame_local(frames[2], delta=not last_in_full))
        return got

    with kg.ImageProcessor(alpha_cutoff=128) as p:
        own = [p.reduce_indexed(k, f, kg.Algorithm.Kmeans, 1) for f in frames[:2]]
        with p.sequence() as seq:
            got = drive(seq, False)
            # the warm third frame's own map and palette: the same calls again, the last frame asked for in full
            I2, P2, rec2, full2 = drive(seq, True)[2]
    assert full2 and rec2.as_tuple() == R.FRESH8
    palettes, maps = [own[0][0], own[1][0], P2], [own[0][1], own[1][1], I2]
    states = R.encode(oracle, frames, maps, palettes, k, tolerances)
    for t, ((m, pal, info, full), s) in enumerate(zip(got, states)):
        assert np.array_equal(pal, palettes[t]) and info.as_tuple() == s["record"], t
        assert full == s["is_full"] and np.array_equal(m, s["map"]), t
    # a shown pixel turns transparent: the frame comes back in full
    assert not got[0][3] and got[1][3] and got[1][2].cleared > 0 and np.array_equal(got[1][0], maps[1])
    shown = R.replay_colour([(m, pal, full) for m, pal, _, full in got], k)
    for t, s in enumerate(states):
        assert np.array_equal(shown[t], s["shown"]), t
    assert np.array_equal(shown[1], R.lookup(maps[1], palettes[1], k)[1])


def test_the_two_kinds_of_output_stay_apart(torch_cuda, processor):
    import kmeans_gpu_amd as kg
    h, w, k = 29, 37, 8
    frames = _frames(2, h, w, 4)
    L = kg.lib()
    out, pal, cnt = np.zeros((h, w), np.uint8), np.zeros((k, 4), np.uint8), C.c_uint32()
    rec, hold, full = kg.FrameDelta(), kg.FrameHold(), C.c_int()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    with processor.sequence() as seq:
        seq.add(frames[0])
        seq.output_local(k, 0, FMT8, w, h)
        first = seq.frame_local(frames[0])
        assert L.kmg_sequence_output_frame(seq._h, vp(frames[1]), 1, vp(out), C.byref(rec), C.byref(full)) == -1
        assert b"per-frame palettes" in L.kmg_last_error()
        assert L.kmg_sequence_output_frame_lossy(seq._h, vp(frames[1]), 1, 100, vp(out), C.byref(hold), C.byref(full)) == -1
        again = seq.frame_local(frames[0])                               # the output stayed open: nothing changed
        assert again[2].changed == 0 and (again[0] == k).all() and np.array_equal(again[1], first[1])
        for flags, tol in ((2, None), (0, C.byref(C.c_uint32(5)))):
            assert L.kmg_sequence_output_frame_local(seq._h, vp(frames[1]), flags, tol, vp(out), vp(pal), C.byref(cnt), C.byref(hold), C.byref(full)) == -1
        seq.output(k, 0, FMT8, w, h)                                     # a shared begin ends the local output
        assert L.kmg_sequence_output_frame_local(seq._h, vp(frames[1]), 1, None, vp(out), vp(pal), C.byref(cnt), C.byref(hold), C.byref(full)) == -1
        assert b"shared palette" in L.kmg_last_error()
        m, info, is_full = seq.frame(frames[0])                          # ... which stays open
        assert info.changed == h * w
        seq.end_output()
        assert L.kmg_sequence_output_frame_local(seq._h, vp(frames[1]), 1, None, vp(out), vp(pal), C.byref(cnt), C.byref(hold), C.byref(full)) == -1
        assert b"no output is open" in L.kmg_last_error()
        for kwargs, text in (({"format": 0}, "RGBA8"), ({"mode": 2}, "meld"), ({"k": 256}, "INDEX16"), ({"k": 0}, "k must"), ({"width": 0}, "zero")):
            args = {"k": k, "mode": 0, "format": FMT8, "width": w, "height": h}
            args.update(kwargs)
            with pytest.raises(kg.KmgError, match=text):
                seq.output_local(**args)
        assert L.kmg_sequence_output_begin_local(seq._h, k, 0, FMT8, w, h, 2) == -1


def test_fixed_colours(torch_cuda):
    import kmeans_gpu_amd as kg
    h, w, k = 29, 37, 8
    frames = _frames(2, h, w, 6)
    pins = np.array([[0, 0, 0, 255], [255, 255, 255, 255]], np.uint8)
    with kg.ImageProcessor(fixed_colors=pins) as p, p.sequence() as seq:
        want = [p.reduce_indexed(k, f, kg.Algorithm.Kmeans, 1) for f in frames]
        seq.output_local(k, 1, FMT8, w, h)
        for f, (P, I) in zip(frames, want):
            m, pal, _, _ = seq.frame_local(f, delta=False)
            assert np.array_equal(pal, P) and np.array_equal(m, I) and np.array_equal(pal[:2, :3], pins[:, :3])
        seq.output_local(k, 1, FMT8, w, h, warm=True)
        with pytest.raises(kg.KmgError) as e:
            seq.frame_local(frames[0])
        assert e.value.status == -5 and "fixed" in str(e.value)         # KMG_ERR_UNSUPPORTED


def test_cpp_mirror_agrees_with_the_binding(torch_cuda, processor, tmp_path):
    libdir = os.path.join(ROOT, "kmeans-gpu_amd", "lib")
    exe = str(tmp_path / "check_local_api")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "kmeans-gpu_amd", "host"),
                    os.path.join(ROOT, "tests", "native", "check_local_api.cpp"), "-o", exe, "-L", libdir, "-lkmeans_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    import kmeans_gpu_amd as kg
    h, w, k = 29, 37, 8
    frames = _frames(3, h, w, 8)
    raw, out = tmp_path / "frames.rgba", tmp_path / "out.bin"
    np.stack(frames).tofile(raw)
    r = subprocess.run([exe, str(raw), str(w), str(h), str(k), str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok refused 1" in r.stdout, r.stdout + r.stderr
    data, pos = np.fromfile(out, np.uint8), 0
    with processor.sequence() as seq:
        seq.output_local(k, 1, FMT8, w, h, warm=True)
        for t, f in enumerate(frames):
            m, pal, info, full = seq.frame_local(f, tolerance=None if t < 2 else kg.tolerance_of(2.0))
            n = int(data[pos:pos + 4].view(np.uint32)[0]); pos += 4
            assert n == k and np.array_equal(data[pos:pos + 4 * n].reshape(n, 4), pal); pos += 4 * n
            assert np.array_equal(data[pos:pos + h * w].reshape(h, w), m); pos += h * w
            assert kg.FrameHold.from_array(data[pos:pos + 48]).as_tuple() == info.as_tuple(); pos += 48
            assert bool(data[pos]) == full; pos += 1
    assert pos == data.size


def test_cli_sequence_local(torch_cuda, processor, oracle, tmp_path, capsys):
    import kmeans_gpu_amd as kg
    from PIL import Image
    from kmeans_gpu_amd import cli
    h, w, k = 29, 37, 8
    frames = _frames(3, h, w, 12)
    paths = []
    for i, f in enumerate(frames):
        paths.append(str(tmp_path / f"f{i}.png"))
        Image.fromarray(f, "RGBA").save(paths[-1])
    out = str(tmp_path / "anim.gif")
    assert cli.main(["sequence", "-i", *paths, "-c", str(k), "-m", "dither", "--local", "--lossy", "1.5", "--report", "-o", out]) == 0
    text = capsys.readouterr().out
    own = [processor.reduce_indexed(k, f, kg.Algorithm.Kmeans, 1) for f in frames]
    states = R.encode(oracle, frames, [m for _, m in own], [p for p, _ in own], k, [kg.tolerance_of(1.5)] * 3)
    for t, s in enumerate(states):
        assert f"Frame {t}: changed={s['record'][0]} held={s['record'][6]} " in text
    got = R.gif_decode(open(out, "rb").read())
    assert got["global_table"] is None and len(got["frames"]) == 3
    for t, (fr, (P, _)) in enumerate(zip(got["frames"], own)):
        assert np.array_equal(fr["table"][:k], P[:, :3]) and fr["transparent"] == k and fr["disposal"] == 1
    for a, s in zip(R.gif_canvases(got), states):
        assert np.array_equal(a, s["shown"])
    for fr, s in zip(got["frames"], states):                             # delta frames are cropped to the box of their record
        x0, y0, x1, y1 = s["record"][2:6]
        assert not s["is_full"] and s["record"][0] > 0 and (fr["x"], fr["y"], fr["w"], fr["h"]) == (x0, y0, x1 - x0, y1 - y0)


@pytest.mark.parametrize("lossy", [[], ["--lossy", "1.5"]])
def test_cli_sequence_local_alpha_cutoff_writes_full_frames(torch_cuda, tmp_path, capsys, lossy):
    """with --alpha-cutoff every frame is written in full with disposal 2, with or without --lossy (a full frame holds nothing)"""
    import kmeans_gpu_amd as kg
    from PIL import Image
    from kmeans_gpu_amd import cli
    h, w, k = 29, 37, 8
    frames = _frames(3, h, w, 13, alpha=True)
    paths = []
    for i, f in enumerate(frames):
        paths.append(str(tmp_path / f"f{i}.png"))
        Image.fromarray(f, "RGBA").save(paths[-1])
    out = str(tmp_path / "anim.gif")
    assert cli.main(["sequence", "-i", *paths, "-c", str(k), "--local", "--alpha-cutoff", "128", "--report", "-o", out] + lossy) == 0
    text = capsys.readouterr().out
    assert "3 written in full" in text and "held" not in text and "changed pixels" not in text
    with kg.ImageProcessor(alpha_cutoff=128) as p:
        own = [p.reduce_indexed(k, f, kg.Algorithm.Kmeans, 0) for f in frames]
    got = R.gif_decode(open(out, "rb").read())
    assert len(got["frames"]) == 3
    for t, (fr, (P, I)) in enumerate(zip(got["frames"], own)):
        assert f"Frame {t}: changed=0 (written in full)" in text
        assert (fr["x"], fr["y"], fr["w"], fr["h"], fr["disposal"], fr["transparent"]) == (0, 0, w, h, 2, k)
        assert np.array_equal(fr["table"][:k], P[:, :3]) and np.array_equal(fr["indices"], I)
    # disposal 2 clears the canvas before the next frame: each frame shows its own P_t[I_t], transparent where I_t == k
    for a, (P, I) in zip(R.gif_canvases(got), own):
        assert np.array_equal(a, R.lookup(I, P, k)[1]) and (I == k).any() and (I != k).any()
