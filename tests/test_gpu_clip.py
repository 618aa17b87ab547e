"""Clip output on the device (include/kmeans_hip.h at kmg_dev_frame_delta_clip and kmg_sequence_output_frames):
  1. kmg_dev_frame_delta_clip byte for byte against the per-frame passes kmg_dev_frame_delta / kmg_dev_frame_delta_lossy run one
     after another on the same device -- every out map, every 48-byte record, d_full, the final canvas and held source and the
     guard bytes around all of them; frames around the 4-pixel group and the tile, clips around KMG_CLIP_FRAMES, both index types,
     aligned pointers and pointers one element off, slot k planted so that clears fall in no frame, the first, a middle one, two in
     a row and the last, with and without KMG_CLIP_FULL_ON_CLEAR; one case against hold_ref.replay; records that combine;
  1b. where a workgroup of k_clip_hold walks several tiles (tests/tile_walk.py; a tile is 1024 pixels): clips whose frame t changes
     only probe t, so every out map, record, d_full word, the canvas and the held source are known by construction -- bands of 4200,
     4100, 2099, 4102, 4102 and 2049 tiles of the widths 1000 (step_y = 1), 1024 (step_x = 0), 1023, 300 (step_y = 3), 3 and 1, exact
     and lossy, with and without the flag, both index types, pointers at their base and one element in, one band over
     KMG_CLIP_FRAMES + 1 frames; a dense clip of 1000 x 4300 (4200 tiles) against hold_ref.replay_from and the per-frame passes;
     2048, 2049 and 2050 tiles as one row and as rows of 7 (empty workgroups, a ragged last tile); clips of 4096 and 4099 frames
     (k_clip_cleared's frame stride); two calls queued back to back, and the host arrays overwritten once the call has returned;
  2. kmg_sequence_output_frames against a twin sequence on a processor of its own that is driven frame by frame;
  3. the refusals, in the header's order."""
import ctypes as C

import numpy as np
import pytest

import hold_ref as H
import probe_run as P
import tile_walk as W

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


# ---- several tiles per workgroup: probes in one launch ----------------------------------------------------------------------------
def _room(torch, dtype, n, off, fill):
    whole = torch.full((n + 32,), fill, dtype=dtype, device="cuda")
    return whole, whole[off:off + n]


def _guards_intact(torch, whole, body, fill):
    off = body.storage_offset() - whole.storage_offset()
    return bool((whole[:off] == fill).all()) and bool((whole[off + body.shape[0]:] == fill).all())


def _probe_clip(torch, processor, fmt, width, rows, n_frames=None):
    """Frame t changes only pixel at[t]: the construction of tests/probe_run.py with its two alternating sources, for every
    combination of exact / lossy, flag, and pointer offset"""
    import kmeans_gpu_amd as kg
    k, n, td = P.K[fmt], width * rows, P.torch_dtype(torch, fmt)
    w = W.walk(n, width, 1024)
    assert w.tiles > W.WORKGROUPS
    ps = W.probes(w)
    at = [p.i for p in ps]
    T = n_frames or len(at)
    at = [at[t % len(at)] for t in range(T)]
    clear = next(t for t, p in enumerate(ps) if "last_tile" in p.labels and "wg_mid" in p.labels and "first_tile" not in p.labels)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(width + fmt)
    canvas0 = torch.randint(0, k, (n,), dtype=td, device="cuda", generator=gen)
    A = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int32, device="cuda", generator=gen)
    marks = torch.tensor(sorted(set(at)), dtype=torch.int64, device="cuda")
    cur = dict(zip(sorted(set(at)), canvas0[marks].cpu().tolist()))
    values = []
    for t, g in enumerate(at):
        values.append(k if t == clear else (cur[g] + 1 + g % (k - 1)) % k)
        cur[g] = values[-1]
    st = torch.cuda.current_stream().cuda_stream
    fresh = torch.from_numpy(np.tile(_fresh48(), T).view(np.int64)).cuda()
    for off in (0, 1):
        # sources: two shared buffers, far apart at the probes and equal elsewhere; maps: I_t = I_{t-1} but for probe t
        src = []
        for name in "AB":
            whole, body = _room(torch, torch.int32, n, off, 0x5A5A5A5A)
            body.copy_(A)
            if name == "B":
                body[marks] = body[marks] ^ P.FAR
            src.append((whole, body))
        maps, prev = [], canvas0
        for t, g in enumerate(at):
            m = _room(torch, td, n, off, 0x5A)[1]
            m.copy_(prev)
            m[g] = values[t]
            maps.append(m)
            prev = m
        frame_src = [src[1 - t % 2][1] for t in range(T)]               # B first: every anchor starts as A
        for lossy in (True, False):
            for flag in (False, True):
                what = (fmt, width, off, lossy, flag)
                canvas_w, canvas = _room(torch, td, n, off, 0x5A)
                canvas.copy_(canvas0)
                held_w, held = _room(torch, torch.int32, n, off, 0x5A5A5A5A)
                held.copy_(A)
                outs = [_room(torch, td, n, off, 0x5A) for _ in range(T)]
                info, full = fresh.clone(), torch.full((T,), 0x77, dtype=torch.int32, device="cuda")
                processor.frame_delta_clip([b.data_ptr() for b in frame_src], [m.data_ptr() for m in maps], canvas.data_ptr(), held.data_ptr(),
                                           width, rows, fmt, k, [P.TOL] * T if lossy else None, [b.data_ptr() for _, b in outs], info.data_ptr(),
                                           full.data_ptr() if flag else 0, kg.CLIP_FULL_ON_CLEAR if flag else 0, st)
                torch.cuda.synchronize()
                recs = info.cpu().numpy().reshape(T, 6)
                for t, g in enumerate(at):
                    is_clear = values[t] == k
                    got = kg.FrameHold.from_array(recs[t]).as_tuple()
                    assert got == P.box(width, [g], cleared=int(is_clear)), (what, t, sorted(ps[t % len(ps)].labels), W.locate(w, g), got)
                    out = outs[t][1]
                    if flag and is_clear:
                        assert torch.equal(out, maps[t]), (what, t, "a full frame")
                    else:
                        assert int(torch.count_nonzero(out != k)) == int(not is_clear) and int(out[g]) == values[t], (what, t, "out")
                    assert _guards_intact(torch, outs[t][0], out, 0x5A), (what, t)
                want_full = [int(flag and values[t] == k) if flag else 0x77 for t in range(T)]
                assert full.cpu().tolist() == want_full, what
                assert sum(1 for v in values if v == k) == 1
                assert torch.equal(canvas, maps[-1]) and _guards_intact(torch, canvas_w, canvas, 0x5A), (what, "canvas")
                # lossy: nothing was held, every pixel is anchored at the last frame; exact: the held source is the last frame
                assert torch.equal(held, frame_src[-1]) and _guards_intact(torch, held_w, held, 0x5A5A5A5A), (what, "held source")
        for (whole, body), name in zip(src, "AB"):
            assert _guards_intact(torch, whole, body, 0x5A5A5A5A)
        for t, m in enumerate(maps):                                     # the inputs are as they were
            assert int(m[at[t]]) == values[t]


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
@pytest.mark.parametrize("name,width,rows,per", W.shapes(1024))
def test_clip_probes_over_several_tiles_per_workgroup(torch_cuda, processor, fmt, name, width, rows, per):
    assert W.walk(width * rows, width, 1024).per == per
    _probe_clip(torch_cuda, processor, fmt, width, rows)


def test_clip_probes_over_two_launches(torch_cuda, processor):
    """KMG_CLIP_FRAMES + 1 frames over the same many-tile runs: the state passes through the canvas and the held source"""
    import kmeans_gpu_amd as kg
    _, width, rows, _ = W.shapes(1024)[2]
    _probe_clip(torch_cuda, processor, FMT8, width, rows, n_frames=kg.CLIP_FRAMES + 1)


# ---- a dense clip against the CPU ------------------------------------------------------------------------------------------------------
DENSE = (1000, 4300)
RECT = (50, 100, 950, 4200)             # x0, y0, x1, y1: touches no border
_dense = {}


def _dense_case(oracle):
    """T = 5 frames; about a tenth of the pixels change, all inside RECT, whose four corners change in frames 0 .. 3 (one each); half of the
    changes stay within the tolerance (held); clears in frames 2 and 3 (the pattern "two" of _case).  Made once, with its
    reference, for both formats (indices below 256) and both offsets."""
    import kmeans_gpu_amd as kg
    if _dense:
        return _dense
    (width, rows), T, k = DENSE, 5, 200
    x0, y0, x1, y1 = RECT
    rng = np.random.default_rng(2024)
    n = width * rows
    canvas = rng.integers(0, k, (rows, width))
    kind = rng.random((rows, width))
    canvas[kind < 0.25] = k
    canvas[kind > 0.95] = k + 40
    canvas = canvas.astype(np.uint8)
    held = rng.integers(0, 256, (rows, width, 4)).astype(np.uint8)
    inside = np.zeros((rows, width), bool)                           # the dense changes stay 3 pixels inside RECT: a corner is alone
    inside[y0 + 3:y1 - 3, x0 + 3:x1 - 3] = True
    corners = [(y0, x0), (y0, x1 - 1), (y1 - 1, x0), (y1 - 1, x1 - 1)]
    srcs, maps, prev, ps = [], [], canvas, held
    for t in range(T):
        move = inside & (rng.random((rows, width)) < 0.11)
        for c in corners:
            move[c] = False
        if t < 4:
            move[corners[t]] = True
        I = prev.copy()
        new = rng.integers(0, k - 1, (rows, width)).astype(np.uint8)
        new[new >= prev] += 1                                        # differs from prev, below k or k + 40 ... never slot k by chance
        new[new == k] = 0
        I[move] = new[move]
        far = move & (rng.random((rows, width)) < 0.5)
        if t < 4:
            far[corners[t]] = True
        if t in (2, 3):
            shown = np.nonzero((move & far & (prev != k)).reshape(-1))[0]
            I.reshape(-1)[rng.choice(shown, shown.size // 10, replace=False)] = k
        s = ps.copy()
        s[move] = _near(rng, ps[move], 2)
        s[far] = ps[far] ^ np.uint8(0x80)
        s[..., 3] = ps[..., 3]
        maps.append(I); srcs.append(s)
        prev, ps = I, s
    tols = [kg.tolerance_of(3.0)] * T
    states = H.replay_from(oracle, canvas, held, srcs, maps, k, tols, True, use_table=True)
    for t, s in enumerate(states):                                   # one pixel pins two sides of the box, a different one per frame
        r = s["record"]
        assert r[0] > 1000 and r[6] > 1000
        assert r[2:6] == ((x0, y0, x1 - 3, y1 - 3), (x0 + 3, y0, x1, y1 - 3), (x0, y0 + 3, x1 - 3, y1), (x0 + 3, y0 + 3, x1, y1),
                          (x0 + 3, y0 + 3, x1 - 3, y1 - 3))[t], (t, r)
    assert [s["is_full"] for s in states] == [False, False, True, True, False]
    flat = lambda a: [np.ascontiguousarray(v).reshape(n, *v.shape[2:]) for v in a]
    _dense.update(case=(canvas.reshape(-1), held.reshape(n, 4), flat(srcs), flat(maps), tols), states=states, k=k, per_frame={})
    return _dense


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("fmt", [FMT8, FMT16])
def test_clip_dense_against_replay_from(torch_cuda, processor, oracle, fmt, off):
    import kmeans_gpu_amd as kg
    d = _dense_case(oracle)
    (width, rows), k, T = DENSE, d["k"], 5
    dtype = _np_dtype(fmt)
    canvas, held, srcs, maps, tols = d["case"]
    case = (canvas.astype(dtype), held, srcs, [m.astype(dtype) for m in maps], tols)
    got = _clip(torch_cuda, processor, case, width, rows, fmt, k, True, True, off)
    outs, recs, full, got_canvas, got_held, _ = got
    for t, s in enumerate(d["states"]):
        assert kg.FrameHold.from_array(recs[t]).as_tuple() == s["record"], t
        assert bool(full[t]) == s["is_full"] and np.array_equal(outs[t], s["map"].reshape(-1).astype(dtype)), t
    assert np.array_equal(got_canvas, d["states"][-1]["canvas"].reshape(-1).astype(dtype))
    assert np.array_equal(got_held.view(np.uint8).reshape(-1, 4), d["states"][-1]["held"].reshape(-1, 4))
    if fmt not in d["per_frame"]:                                     # the per-frame passes on the device, once per format
        d["per_frame"][fmt] = _reference(torch_cuda, processor, case, width, rows, fmt, k, True, True)
    _compare(got, d["per_frame"][fmt], T, True)


# ---- uneven partitions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_rows_of_7", [False, True])
@pytest.mark.parametrize("n", [2048 * 1024 - 1, 2048 * 1024 + 1, 2049 * 1024 + 3])
def test_clip_uneven_partitions(torch_cuda, processor, oracle, n, as_rows_of_7):
    """2048 tiles on 2048 workgroups with a ragged last one; 2049 and 2050 tiles, two per workgroup: 1023 workgroups are empty (and
    return early) and the last tile is ragged.  Three lossy frames with the flag, clears in the last frame only."""
    import kmeans_gpu_amd as kg
    width, rows = (7, (n + 6) // 7) if as_rows_of_7 else (n, 1)
    k, T = 255, 3
    w = W.walk(width * rows, width, 1024)
    assert (w.per, w.nonempty) == ((1, 2048) if n < 2048 * 1024 else (2, 1025)) and (width * rows) % 1024 != 0
    case = _case(n % 1000, width, rows, T, k, np.uint8, "last")
    canvas, held, srcs, maps, tols = case
    states = H.replay_from(oracle, canvas.reshape(rows, width), held.reshape(rows, width, 4), [s.reshape(rows, width, 4) for s in srcs],
                           [m.reshape(rows, width) for m in maps], k, tols, True, use_table=True)
    assert [s["is_full"] for s in states] == [False, False, True]
    outs, recs, full, got_canvas, got_held, _ = _clip(torch_cuda, processor, case, width, rows, FMT8, k, True, True, 0)
    for t, s in enumerate(states):
        assert kg.FrameHold.from_array(recs[t]).as_tuple() == s["record"], t
        assert np.array_equal(outs[t], s["map"].reshape(-1)), t
    assert [int(v) for v in full] == [0, 0, 1]
    assert np.array_equal(got_canvas, states[-1]["canvas"].reshape(-1))
    assert np.array_equal(got_held.view(np.uint8).reshape(-1, 4), states[-1]["held"].reshape(-1, 4))


# ---- clips longer than k_clip_cleared's grid ---------------------------------------------------------------------------------------
def _long_case(T, width, rows, k, clears, seed):
    """a canvas with slot k; maps that turn a shown pixel to slot k in the frames of `clears` and in no other"""
    import kmeans_gpu_amd as kg
    rng = np.random.default_rng(seed)
    n = width * rows
    canvas = rng.integers(0, k, n).astype(np.uint8)
    canvas[rng.random(n) < 0.3] = k
    held = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    srcs, maps, prev, ps = [], [], canvas, held
    for t in range(T):
        I = prev.copy()
        move = rng.random(n) < 0.4
        I[move] = rng.integers(0, k, int(move.sum()))
        if t in clears:
            shown = np.nonzero(prev != k)[0]
            I[rng.choice(shown, 2, replace=False)] = k
        s = np.where((rng.random(n) < 0.3)[:, None], rng.integers(0, 256, (n, 4)).astype(np.uint8), _near(rng, ps, 2)).astype(np.uint8)
        maps.append(I); srcs.append(s)
        prev, ps = I, s
    tols = [(0, kg.tolerance_of(3.0), H.D_MAX)[t % 3] for t in range(T)]
    return canvas, held, srcs, maps, tols


@pytest.mark.parametrize("T", [4096, 4096 + 3])
def test_clip_longer_than_the_cleared_grid(torch_cuda, processor, oracle, T):
    """k_clip_cleared launches min(T, 4096) rows of workgroups and strides the frames by that: frames 4096 .. 4098 are a workgroup's
    second turn.  The frame buffers are slices of three allocations, 48 elements apart; every third one lies one element further in,
    where no vector access is allowed."""
    import kmeans_gpu_amd as kg
    torch, (width, rows), k = torch_cuda, (5, 7), 40
    n = width * rows
    clears = [t for t in (0, 4095, 4096, 4098) if t < T]
    canvas, held, srcs, maps, tols = _long_case(T, width, rows, k, clears, T)
    states = H.replay_from(oracle, canvas.reshape(rows, width), held.reshape(rows, width, 4), [s.reshape(rows, width, 4) for s in srcs],
                           [m.reshape(rows, width) for m in maps], k, tols, True)
    assert [t for t, s in enumerate(states) if s["is_full"]] == clears
    at = [48 * t + 16 + (1 if t % 3 == 0 else 0) for t in range(T)]
    h_src, h_map = np.full((48 * T + 64, 4), 0xA5, np.uint8), np.full(48 * T + 64, 0xA5, np.uint8)
    for t in range(T):
        h_src[at[t]:at[t] + n] = srcs[t]
        h_map[at[t]:at[t] + n] = maps[t]
    d_src, d_map = torch.from_numpy(h_src).cuda(), torch.from_numpy(h_map).cuda()
    d_out = torch.full((48 * T + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    d_canvas, d_held = torch.from_numpy(canvas).cuda(), torch.from_numpy(held).cuda()
    info = torch.from_numpy(np.tile(_fresh48(), T).view(np.int64)).cuda()
    full = torch.full((T,), 0x77, dtype=torch.int32, device="cuda")
    processor.frame_delta_clip([d_src.data_ptr() + 4 * a for a in at], [d_map.data_ptr() + a for a in at], d_canvas.data_ptr(), d_held.data_ptr(),
                               width, rows, FMT8, k, tols, [d_out.data_ptr() + a for a in at], info.data_ptr(), full.data_ptr(),
                               kg.CLIP_FULL_ON_CLEAR, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert full.cpu().tolist() == [1 if t in clears else 0 for t in range(T)]
    recs, out = info.cpu().numpy().reshape(T, 6), d_out.cpu().numpy()
    want_out = np.full(48 * T + 64, 0xA5, np.uint8)
    for t, s in enumerate(states):
        assert kg.FrameHold.from_array(recs[t]).as_tuple() == s["record"], t
        want_out[at[t]:at[t] + n] = s["map"].reshape(-1)
    assert np.array_equal(out, want_out), "an out map, or a byte between two of them"
    assert np.array_equal(d_canvas.cpu().numpy(), states[-1]["canvas"].reshape(-1))
    assert np.array_equal(d_held.cpu().numpy(), states[-1]["held"].reshape(-1, 4))
    assert np.array_equal(d_src.cpu().numpy(), h_src) and np.array_equal(d_map.cpu().numpy(), h_map)


# ---- call boundaries ---------------------------------------------------------------------------------------------------------------
def _enqueue(torch, processor, bufs, case, width, rows, fmt, k, a, b, stream, garbage=False):
    """frames [a, b) of the clip as one call on `stream`, with no synchronisation; garbage: through ctypes, and the host arrays and
    the tolerances are overwritten as soon as the call has returned"""
    import kmeans_gpu_amd as kg
    d_src, d_index, d_out, d_canvas, d_held, d_info, d_full = bufs
    tols = case[4]
    if not garbage:
        processor.frame_delta_clip([x.ptr for x in d_src[a:b]], [x.ptr for x in d_index[a:b]], d_canvas.ptr, d_held.ptr, width, rows, fmt, k,
                                   tols[a:b], [x.ptr for x in d_out[a:b]], d_info.ptr + 48 * a, d_full.ptr + 4 * a, kg.CLIP_FULL_ON_CLEAR, stream)
        return
    m = b - a
    arrays = [(C.c_void_p * m)(*[x.ptr for x in v[a:b]]) for v in (d_src, d_index, d_out)]
    tol = (C.c_uint32 * m)(*tols[a:b])
    rc = kg.lib().kmg_dev_frame_delta_clip(processor.handle, m, arrays[0], arrays[1], C.c_void_p(d_canvas.ptr), C.c_void_p(d_held.ptr), width, rows,
                                           fmt, k, tol, kg.CLIP_FULL_ON_CLEAR, arrays[2], C.c_void_p(d_info.ptr + 48 * a),
                                           C.c_void_p(d_full.ptr + 4 * a), C.c_void_p(stream))
    for arr in arrays + [tol]:
        C.memset(arr, 0xEE, C.sizeof(arr))
    assert rc == 0, kg.lib().kmg_last_error()


def _clip_buffers(torch, case, fmt, n, T):
    canvas, held, srcs, maps, tols = case
    dtype = _np_dtype(fmt)
    return ([_Buf(torch, np.uint32, s) for s in srcs], [_Buf(torch, dtype, m) for m in maps],
            [_Buf(torch, dtype, np.full(n, 0x5A, dtype)) for _ in maps], _Buf(torch, dtype, canvas), _Buf(torch, np.uint32, held),
            _Buf(torch, np.uint64, np.tile(_fresh48(), T)), _Buf(torch, np.uint32, np.full(T, 0x77, np.uint32)))


def _collect(bufs, T):
    d_src, d_index, d_out, d_canvas, d_held, d_info, d_full = bufs
    full = d_full.get()
    return [b.get() for b in d_out], list(d_info.get().reshape(T, 6)), list(full), d_canvas.get(), d_held.get(), full


@pytest.mark.parametrize("how", ["one stream", "two streams", "arrays overwritten"])
@pytest.mark.parametrize("fmt,k", [(FMT8, 255), (FMT16, 600)])
def test_clip_call_boundaries(torch_cuda, processor, fmt, k, how):
    """two calls queued with no synchronisation between them -- on one stream, and on two streams with an event between them -- leave
    what one clip of all the frames leaves; so does a call whose pointer arrays and tolerances change as soon as it has returned"""
    torch, (width, rows), T, cut = torch_cuda, (1025, 5), 11, 6      # (a clear in either call: frames 5 and 6)
    case = _case(77, width, rows, T, k, _np_dtype(fmt), "two")
    want = _clip(torch, processor, case, width, rows, fmt, k, True, True, 0)
    assert sum(int(v) for v in want[2]) == 2
    bufs = _clip_buffers(torch, case, fmt, width * rows, T)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    if how == "arrays overwritten":
        _enqueue(torch, processor, bufs, case, width, rows, fmt, k, 0, T, st.cuda_stream, garbage=True)
    else:
        _enqueue(torch, processor, bufs, case, width, rows, fmt, k, 0, cut, st.cuda_stream)
        second = st
        if how == "two streams":
            second, event = torch.cuda.Stream(), torch.cuda.Event()
            event.record(st)
            second.wait_event(event)
        _enqueue(torch, processor, bufs, case, width, rows, fmt, k, cut, T, second.cuda_stream)
    torch.cuda.synchronize()
    got = _collect(bufs, T)
    _compare(got, want[:5], T, True)


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
