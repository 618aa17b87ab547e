"""Clip output on the device (include/kmeans_hip.h at kmg_dev_frame_delta_clip and kmg_sequence_output_frames):
  1. kmg_dev_frame_delta_clip byte for byte against the per-frame passes kmg_dev_frame_delta / kmg_dev_frame_delta_lossy run one
     after another on the same device -- every out map, every 48-byte record, d_full, the final canvas and held source and the
     guard bytes around all of them; frames around the 4-pixel group and the tile, clips around KMG_CLIP_FRAMES, both index types,
     aligned pointers and pointers one element off, slot k planted so that clears fall in no frame, the first, a middle one, two in
     a row and the last, with and without KMG_CLIP_FULL_ON_CLEAR; one case against hold_ref.replay; records that combine;
  2. kmg_sequence_output_frames against a twin sequence on a processor of its own that is driven frame by frame;
  3. the refusals, in the header's order."""
import ctypes as C

import numpy as np
import pytest

import hold_ref as H

pytestmark = pytest.mark.gpu

FMT8, FMT16 = 1, 2
SHAPES = [(1, 1), (3, 1), (5, 7), (23, 7), (64, 4), (1025, 1)]
LONG_SHAPE = (23, 7)
PATTERNS = ("none", "first", "middle", "two", "last")
PAD = 16                                # elements of guard on either side; a body at PAD elements allows every vector access


def _np_dtype(fmt):
    return np.uint8 if fmt == FMT8 else np.uint16


class _Buf:
    """n elements of `dtype`, `off` elements past the aligned position of a guard-filled allocation"""

    def __init__(self, torch, dtype, body, off=0):
        self.dtype, self.off = np.dtype(dtype), off
        body = np.ascontiguousarray(body).reshape(-1).view(self.dtype)
        self.n = body.shape[0]
        self.guard = {1: 0xA5, 2: 0xA5C3, 4: 0xA5C3A5C3, 8: 0x0123456789ABCDEF}[self.dtype.itemsize]
        host = np.full(self.n + 2 * PAD + off, self.guard, self.dtype)
        host[PAD + off:PAD + off + self.n] = body
        signed = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[self.dtype.itemsize]
        self.t = torch.from_numpy(host.view(signed)).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + self.dtype.itemsize * (PAD + self.off)

    def get(self):
        host = self.t.cpu().numpy().view(self.dtype)
        a = PAD + self.off
        assert (host[:a] == self.guard).all() and (host[a + self.n:] == self.guard).all(), "written outside the buffer"
        return host[a:a + self.n].copy()


def _near(rng, a, amp):
    out = np.clip(a.astype(np.int64) + rng.integers(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8)
    out[..., 3] = a[..., 3]
    return out


def _clear_frames(pattern, T):
    m = T // 2
    return {"none": [], "first": [0], "middle": [m], "two": [m, min(m + 1, T - 1)], "last": [T - 1]}[pattern]


def _case(seed, width, rows, T, k, dtype, pattern):
    """canvas, held, sources, maps: a caller's canvas with slot k, ordinary indices and indices above k; maps that keep slot k where
    the pixel showed it (no clear) and that turn shown pixels to slot k in the frames of `pattern` only"""
    import kmeans_gpu_amd as kg
    rng = np.random.default_rng(seed)
    n = width * rows
    top = min(k + 40, np.iinfo(dtype).max)
    canvas = rng.integers(0, k, n)
    kind = rng.random(n)
    canvas[kind < 0.25] = k
    canvas[kind > 0.9] = rng.integers(k, top + 1, int((kind > 0.9).sum()))
    canvas = canvas.astype(dtype)
    held = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    clears = _clear_frames(pattern, T)
    srcs, maps, prev, ps = [], [], canvas, held
    for t in range(T):
        I = rng.integers(0, k, n)
        keep = rng.random(n) < 0.4
        I[keep] = prev[keep]                                         # still pixels, and slot k that stays slot k
        I[(prev == k) & ~keep] = rng.integers(0, k, int(((prev == k) & ~keep).sum()))
        above = rng.random(n) < 0.05
        if top > k:
            I[above & (I != k)] = top
        if t in clears:
            shown = np.nonzero(prev != k)[0]
            if shown.size:
                I[rng.choice(shown, max(1, shown.size // 10), replace=False)] = k
        I = I.astype(dtype)
        s = np.where((rng.random(n) < 0.3)[:, None], rng.integers(0, 256, (n, 4)).astype(np.uint8), _near(rng, ps, 2)).astype(np.uint8)
        maps.append(I); srcs.append(s)
        prev, ps = I, s
    tols = [(0, kg.tolerance_of(3.0), H.D_MAX)[(t + seed) % 3] for t in range(T)]
    return canvas, held, srcs, maps, tols


def _fresh48():
    import kmeans_gpu_amd as kg
    return np.frombuffer(kg.FrameHold.fresh_bytes(), np.uint64).copy()


def _reference(torch, processor, case, width, rows, fmt, k, lossy, flag):
    """the per-frame passes one after another, each on the whole frame and a fresh record; with `flag`, the rule of
    kmg_sequence_output_frame_lossy where a frame's own record has cleared > 0"""
    import kmeans_gpu_amd as kg
    canvas, held, srcs, maps, tols = case
    st = torch.cuda.current_stream().cuda_stream
    dtype = _np_dtype(fmt)
    n = width * rows
    d_canvas, d_held = _Buf(torch, dtype, canvas), _Buf(torch, np.uint32, held)
    outs, recs, full = [], [], []
    for t in range(len(maps)):
        d_src, d_index = _Buf(torch, np.uint32, srcs[t]), _Buf(torch, dtype, maps[t])
        d_out, d_info = _Buf(torch, dtype, np.full(n, 0x5A, dtype)), _Buf(torch, np.uint64, _fresh48())
        if lossy:
            processor.frame_delta_lossy(d_src.ptr, d_index.ptr, d_canvas.ptr, d_held.ptr, width, rows, 0, fmt, k, tols[t], d_out.ptr, d_info.ptr, st)
        else:
            processor.frame_delta(d_index.ptr, d_canvas.ptr, width, rows, 0, fmt, k, d_out.ptr, d_info.ptr, st)
        torch.cuda.synchronize()
        rec = d_info.get()
        is_full = bool(flag and rec[1] > 0)
        if is_full:
            d_canvas, d_held = _Buf(torch, dtype, maps[t]), _Buf(torch, np.uint32, srcs[t])
        outs.append(maps[t].copy() if is_full else d_out.get())
        recs.append(rec)
        full.append(1 if is_full else 0)
    final_held = d_held.get() if lossy else np.ascontiguousarray(srcs[-1]).reshape(-1).view(np.uint32)   # (an exact clip: the last frame)
    return outs, recs, full, d_canvas.get(), final_held


def _clip(torch, processor, case, width, rows, fmt, k, lossy, flag, off, records=None):
    import kmeans_gpu_amd as kg
    canvas, held, srcs, maps, tols = case
    st = torch.cuda.current_stream().cuda_stream
    dtype = _np_dtype(fmt)
    n, T = width * rows, len(maps)
    d_canvas, d_held = _Buf(torch, dtype, canvas, off), _Buf(torch, np.uint32, held, off)
    d_src = [_Buf(torch, np.uint32, s, off) for s in srcs]
    d_index = [_Buf(torch, dtype, m, off) for m in maps]
    d_out = [_Buf(torch, dtype, np.full(n, 0x5A, dtype), off) for _ in maps]
    d_info = _Buf(torch, np.uint64, np.tile(_fresh48(), T) if records is None else records)
    d_full = _Buf(torch, np.uint32, np.full(T, 0x77, np.uint32))
    torch.cuda.synchronize()
    processor.frame_delta_clip([b.ptr for b in d_src], [b.ptr for b in d_index], d_canvas.ptr, d_held.ptr, width, rows, fmt, k,
                               tols if lossy else None, [b.ptr for b in d_out], d_info.ptr, d_full.ptr if flag else 0,
                               kg.CLIP_FULL_ON_CLEAR if flag else 0, st)
    torch.cuda.synchronize()
    for b, want in zip(d_src + d_index, srcs + maps):                  # the inputs and their guards are as they were
        assert np.array_equal(b.get(), np.ascontiguousarray(want).reshape(-1).view(b.dtype))
    full = d_full.get()
    return ([b.get() for b in d_out], list(d_info.get().reshape(T, 6)), list(full) if flag else [0] * T, d_canvas.get(), d_held.get(),
            full)


def _compare(got, want, T, flag):
    outs, recs, full, canvas, held, full_words = got
    w_outs, w_recs, w_full, w_canvas, w_held = want
    for t in range(T):
        assert np.array_equal(outs[t], w_outs[t]), ("out", t)
        assert np.array_equal(recs[t], w_recs[t]), ("record", t, recs[t], w_recs[t])
    assert [int(v) for v in full] == w_full
    if not flag:
        assert (full_words == 0x77).all(), "d_full was touched without the flag"
    assert np.array_equal(canvas, w_canvas), "canvas"
    assert np.array_equal(held, w_held), "held source"


def _lengths(width, rows):
    import kmeans_gpu_amd as kg
    F = kg.CLIP_FRAMES
    return [1, 2, 5, F] + ([F + 1, 2 * F + 1] if (width, rows) == LONG_SHAPE else [])


@pytest.mark.parametrize("fmt,k", [(FMT8, 255), (FMT16, 600)])
@pytest.mark.parametrize("width,rows", SHAPES)
def test_clip_against_the_per_frame_passes(torch_cuda, processor, fmt, k, width, rows):
    import kmeans_gpu_amd as kg
    torch, dtype, F = torch_cuda, _np_dtype(fmt), kg.CLIP_FRAMES
    seen_full, i = set(), SHAPES.index((width, rows))
    for T in _lengths(width, rows):
        for lossy in (True, False):
            for flag in (False, True):
                i += 1
                patterns = PATTERNS if (width, rows) == LONG_SHAPE and T == 5 else (PATTERNS[i % 5],)
                if T > 2 * F:                                          # several launches: clears in a later launch and in the last frame
                    patterns = tuple(dict.fromkeys(patterns + ("two", "last")))
                for pattern in patterns:
                    case = _case(1000 + i, width, rows, T, k, dtype, pattern)
                    want = _reference(torch, processor, case, width, rows, fmt, k, lossy, flag)
                    if flag and (width, rows) == LONG_SHAPE and T == 5:
                        assert want[2] == [1 if t in _clear_frames(pattern, T) else 0 for t in range(T)], pattern
                        seen_full.add(pattern)
                    for off in (0, 1):
                        _compare(_clip(torch, processor, case, width, rows, fmt, k, lossy, flag, off), want, T, flag)
    if (width, rows) == LONG_SHAPE:
        assert seen_full == set(PATTERNS)


def test_clip_against_replay(torch_cuda, processor, oracle):
    """from a canvas of k with nothing held: the model every frame-by-frame test of the sequence layer uses"""
    torch, (width, rows), k, T = torch_cuda, (23, 7), 40, 6
    canvas, held, srcs, maps, tols = _case(7, width, rows, T, k, np.uint8, "two")
    maps = [np.minimum(m, k) for m in maps]
    canvas, held = np.full(width * rows, k, np.uint8), np.zeros((width * rows, 4), np.uint8)
    states = H.replay(oracle, [s.reshape(rows, width, 4) for s in srcs], [m.reshape(rows, width) for m in maps], k, tols)
    outs, recs, full, got_canvas, got_held, _ = _clip(torch, processor, (canvas, held, srcs, maps, tols), width, rows, FMT8, k, True, True, 0)
    import kmeans_gpu_amd as kg
    for t, s in enumerate(states):
        assert kg.FrameHold.from_array(recs[t]).as_tuple() == s["record"], t
        assert bool(full[t]) == s["is_full"] and np.array_equal(outs[t].reshape(rows, width), s["map"]), t
    assert sum(int(v) for v in full) >= 1
    assert np.array_equal(got_canvas.reshape(rows, width), states[-1]["canvas"])
    assert np.array_equal(got_held.view(np.uint8).reshape(rows, width, 4), states[-1]["held"])


def test_clip_records_combine(torch_cuda, processor):
    torch, (width, rows), k, T = torch_cuda, (23, 7), 255, 5
    case = _case(11, width, rows, T, k, np.uint8, "middle")
    want = _reference(torch, processor, case, width, rows, FMT8, k, True, False)
    start = (7, 2, 3, 1, 9, 4, 11, 123456789012)                      # changed, cleared, x0, y0, x1, y1, held, held_sse
    one = np.zeros(6, np.uint64)
    one[0], one[1], one[3], one[4], one[5] = start[0], start[1], start[4] | (start[5] << 32), start[6], start[7]
    one[2] = start[2] | (start[3] << 32)
    before = np.tile(one, T)
    got = _clip(torch, processor, case, width, rows, FMT8, k, True, False, 0, records=before)
    import kmeans_gpu_amd as kg
    for t in range(T):
        assert kg.FrameHold.from_array(got[1][t]).as_tuple() == H.combine(start, kg.FrameHold.from_array(want[1][t]).as_tuple()), t


def test_clip_refusals(torch_cuda, processor):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = kg.lib()
    n, T = 64, 2
    s = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(T)]
    a = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(T)]
    d = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(T)]
    b = torch.full((n,), 5, dtype=torch.uint8, device="cuda")
    h = torch.zeros(n, dtype=torch.int32, device="cuda")
    info = torch.zeros(6 * T, dtype=torch.int64, device="cuda")
    full = torch.zeros(T, dtype=torch.int32, device="cuda")
    arr = lambda ts, drop=None: (C.c_void_p * T)(*[None if i == drop else t.data_ptr() for i, t in enumerate(ts)])
    tol = (C.c_uint32 * T)(100, 100)

    def call(p=processor.handle, n_frames=T, src=True, index=True, canvas=b.data_ptr(), held=h.data_ptr(), width=8, height=8, fmt=FMT8, k=5,
             flags=0, out=True, rec=info.data_ptr(), d_full=full.data_ptr()):
        rc = L.kmg_dev_frame_delta_clip(p, n_frames, arr(s) if src is True else src, arr(a) if index is True else index, C.c_void_p(canvas),
                                        C.c_void_p(held), width, height, fmt, k, tol, flags, arr(d) if out is True else out, C.c_void_p(rec),
                                        C.c_void_p(d_full), st)
        return rc, L.kmg_last_error().decode()

    def still_works():
        b.fill_(5); h.fill_(7)
        for x in s:
            x.fill_(9)
        info.copy_(torch.from_numpy(np.tile(_fresh48(), T).view(np.int64)))
        assert call(flags=kg.CLIP_FULL_ON_CLEAR)[0] == 0
        torch.cuda.synchronize()
        recs = info.cpu().numpy().reshape(T, 6)
        assert kg.FrameHold.from_array(recs[0]).as_tuple() == (64, 0, 0, 0, 8, 8, 0, 0)
        assert kg.FrameHold.from_array(recs[1]).as_tuple() == H.FRESH
        assert bool((b == 0).all()) and bool((h == 9).all()) and bool((full == 0).all())

    still_works()
    # one fault at a time, then two at once: the header's order decides which one is named
    for kwargs, text in (({"fmt": 0}, "RGBA8"), ({"fmt": 3}, "format"), ({"k": 0}, "k = 0"), ({"fmt": FMT8, "k": 256}, "INDEX16"),
                         ({"index": None}, "NULL"), ({"width": 0}, "zero"), ({"rec": info.data_ptr() + 4}, "aligned"),
                         ({"n_frames": 0}, "no frames"), ({"out": arr(d, drop=1)}, "frame 1"), ({"flags": 2}, "unknown flags"),
                         ({"flags": 1, "d_full": 0}, "d_full"),
                         ({"fmt": 0, "k": 0}, "RGBA8"), ({"width": 0, "n_frames": 0}, "zero"), ({"n_frames": 0, "flags": 2}, "no frames"),
                         ({"out": arr(d, drop=1), "flags": 2}, "frame 1"), ({"flags": 3, "d_full": 0}, "unknown flags")):
        rc, msg = call(**kwargs)
        assert rc == -1 and text in msg, (kwargs, msg)
        still_works()
    for kwargs in ({"p": None}, {"src": None}, {"out": None}, {"canvas": 0}, {"held": 0}, {"rec": 0}, {"src": arr(s, drop=0)}, {"index": arr(a, drop=1)}):
        rc, msg = call(**kwargs)
        assert rc == -1 and "NULL" in msg, (kwargs, msg)
        still_works()
    for kwargs in ({"fmt": FMT16, "out": (C.c_void_p * T)(d[0].data_ptr(), d[1].data_ptr() + 1)}, {"src": (C.c_void_p * T)(s[0].data_ptr() + 2, s[1].data_ptr())},
                   {"held": h.data_ptr() + 1}):
        rc, msg = call(**kwargs)
        assert rc == -1 and "aligned" in msg, (kwargs, msg)
        still_works()


# ---- the host call against a twin sequence ---------------------------------------------------------------------------------------
H_, W_ = 19, 37
_twins = {}


def _pair(cutoff):
    """two processors with equal options: one takes the clips, its twin the same frames one at a time"""
    import kmeans_gpu_amd as kg
    if cutoff not in _twins:
        _twins[cutoff] = (kg.ImageProcessor(alpha_cutoff=cutoff), kg.ImageProcessor(alpha_cutoff=cutoff))
    return _twins[cutoff]


def _frames(tokyo, n, seed):
    """frames whose alpha lies on both sides of 128, with a transparent block that moves, so that shown pixels turn transparent"""
    rng = np.random.default_rng(seed)
    base = np.ascontiguousarray(tokyo[200:200 + H_, 400:400 + W_])
    frames = []
    for t in range(n):
        f = _near(rng, base, 2)
        f[3:9, (5 * t) % 30:(5 * t) % 30 + 6, :3] = (240, 30, 40)
        alpha = rng.choice(np.array([127, 128, 129, 200, 255], np.uint8), (H_, W_), p=[0.04, 0.04, 0.04, 0.08, 0.8])
        alpha[10:16, (7 * t) % 28:(7 * t) % 28 + 8] = 40
        f[..., 3] = alpha
        frames.append(f)
    return frames


@pytest.fixture(scope="module", autouse=True)
def _close_twins():
    yield
    for pair in _twins.values():
        for proc in pair:
            proc.close()
    _twins.clear()


def _drive_twin(seq, frames, delta, tols):
    return [seq.frame(f, delta=delta, tolerance=None if tols is None else tols[t]) for t, f in enumerate(frames)]


def _same_frames(got, want):
    assert len(got) == len(want)
    for t, ((m, info, full), (wm, winfo, wfull)) in enumerate(zip(got, want)):
        assert type(info) is type(winfo) and info.as_tuple() == winfo.as_tuple(), (t, info, winfo)
        assert full == wfull and m.dtype == wm.dtype and np.array_equal(m, wm), t


@pytest.mark.parametrize("T", [7, 9])
@pytest.mark.parametrize("cutoff", [0, 128])
@pytest.mark.parametrize("fmt", [FMT8, FMT16])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_frames_against_a_twin(torch_cuda, tokyo, mode, fmt, cutoff, T):
    """T = 7 lies below KMG_CLIP_MIN_FRAMES, the measured minimum of the launch chain (profiles/r12_clip_time.txt: two frames were
    up to 1.63 of the per-frame path, eight at most 0.80), so its clips are single-frame calls and its report says so; T = 9 takes
    the chain, cut into 3."""
    import kmeans_gpu_amd as kg
    MIN_CLIP = kg.CLIP_MIN_FRAMES
    assert 7 < MIN_CLIP <= 9
    p, q = _pair(cutoff)
    k = 12
    F = _frames(tokyo, 2 * T + 2, 50 + mode)
    e = 1 if fmt == FMT8 else 2
    cut3 = 3 * H_ * W_ * (4 + 2 * e)                                  # three frames resident: 7 frames in 3 pieces
    kinds = [("exact", fmt, True, False), ("lossy", fmt, True, True), ("no delta", fmt, False, False)] + ([("rgba8", 0, False, False)] if fmt == FMT8 else [])
    fired = False
    for kind, out_fmt, delta, lossy in kinds:
        tols = [(kg.tolerance_of(3.0), 0, H.D_MAX, 9000)[t % 4] for t in range(len(F))] if lossy else None
        part = lambda a, b: None if tols is None else tols[a:b]
        with p.sequence() as seq, q.sequence() as twin:
            for f in F:
                seq.add(f); twin.add(f)
            assert np.array_equal(seq.output(k, mode, out_fmt, W_, H_), twin.output(k, mode, out_fmt, W_, H_))
            # frame, clip, frame, clip on one open output
            got = _drive_twin(seq, F[:1], delta, part(0, 1))
            got += seq.frames(F[1:1 + T], delta=delta, tolerance=part(1, 1 + T))
            r1 = seq.last_clip_report
            got += _drive_twin(seq, F[1 + T:2 + T], delta, part(1 + T, 2 + T))
            got += seq.frames(F[2 + T:], delta=delta, tolerance=part(2 + T, 2 + 2 * T), max_resident_bytes=cut3 if out_fmt else 3 * H_ * W_ * 12)
            r2 = seq.last_clip_report
            want = _drive_twin(twin, F, delta, tols)
            _same_frames(got, want)
            for r, pieces in ((r1, 1), (r2, 3)):
                assert r.batched + r.per_image == T, r
                if T < MIN_CLIP:
                    assert r.as_tuple() == (0, 0, T, 1), r
                    continue
                assert r.sub_clips == pieces, r
                assert mode != 3 or r.batched == 0
                assert r.launches >= (pieces if delta else 0)
            fired |= lossy and any(full for _, _, full in got[1:])
            # the state is equal: one more frame on both sides
            if out_fmt:
                _same_frames([seq.frame(F[0], tolerance=9000)], [twin.frame(F[0], tolerance=9000)])
            # a clip of one frame is a frame
            _same_frames(seq.frames(F[3:4], delta=delta, tolerance=part(3, 4)), _drive_twin(twin, F[3:4], delta, part(3, 4)))
            _same_frames([seq.frame(F[5], delta=False)], [twin.frame(F[5], delta=False)])
    assert fired == (cutoff != 0), "a frame that clears a shown pixel was expected exactly in alpha mode"


def test_frames_refusals(torch_cuda, tokyo):
    import kmeans_gpu_amd as kg
    p, q = _pair(128)
    L = kg.lib()
    k, T = 8, 3
    F = _frames(tokyo, 6, 77)
    src = (C.c_void_p * T)(*[f.ctypes.data for f in F[:T]])
    outs = [np.zeros((H_, W_), np.uint8) for _ in range(T)]
    dst = (C.c_void_p * T)(*[o.ctypes.data for o in outs])
    info, full, tol = (kg.FrameHold * T)(), (C.c_int * T)(), (C.c_uint32 * T)(5000, 5000, 5000)

    def call(seq, n=T, rgba=src, flags=kg.FRAME_DELTA, tols=None, out=dst, rec=info, is_full=full):
        rc = L.kmg_sequence_output_frames(seq._h if seq is not None else None, n, rgba, flags, tols, 0, out, rec, is_full, None)
        return rc, L.kmg_last_error().decode()

    def drop(a, i):
        b = (C.c_void_p * T)(*a)
        b[i] = None
        return b

    with p.sequence() as seq, q.sequence() as twin:
        for f in F:
            seq.add(f); twin.add(f)
        assert call(None)[0] == -1
        rc, msg = call(seq)
        assert rc == -1 and "no output is open" in msg
        seq.output_local(k, 0, FMT8, W_, H_)
        rc, msg = call(seq)
        assert rc == -1 and "per-frame palettes" in msg
        seq.frame_local(F[0])                                          # (the local output still works)
        seq.output(k, 0, FMT8, W_, H_); twin.output(k, 0, FMT8, W_, H_)
        at = 0
        for kwargs, text in (({"rgba": None}, "NULL"), ({"out": None}, "NULL"), ({"flags": 3}, "unknown flags"), ({"flags": 0, "tols": tol}, "KMG_FRAME_DELTA"),
                             ({"rec": None}, "info"), ({"is_full": None}, "info"), ({"n": 0}, "no frames"), ({"rgba": drop(src, 1)}, "frame 1"),
                             ({"out": drop(dst, 2)}, "frame 2")):
            rc, msg = call(seq, **kwargs)
            assert rc == -1 and text in msg, (kwargs, msg)
            _same_frames([seq.frame(F[at % 6], tolerance=4000)], [twin.frame(F[at % 6], tolerance=4000)])   # usable and unchanged
            at += 1
        seq.output(k, 0, 0, W_, H_)                                    # RGBA8 has no delta
        rc, msg = call(seq, out=(C.c_void_p * T)(*[np.zeros((H_, W_, 4), np.uint8).ctypes.data] * T))
        assert rc == -1 and "RGBA8" in msg
        seq.frame(F[0], delta=False)
