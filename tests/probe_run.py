"""One-pixel frames for the three per-frame delta passes (test_gpu_sequence.py, test_gpu_hold.py, test_gpu_local.py), over the bands and
probes of tests/tile_walk.py.  A state keeps one resident canvas (and held source, or shown words) of the whole band on the device; a
frame's map equals the canvas except at the pixels a test writes with `set`, so the expected record is known by construction:

    (changed, cleared, x, y, x + 1, y + 1, held, held_sse)   with (y, x) = divmod(i, width)

and so are the maps: the delta map is k everywhere but at the changed pixels, the canvas takes the map, the held source the frame's
source wherever nothing was held.  The lossy states alternate two source buffers A and B that differ strongly (FAR) at every pixel a
test will probe (`mark`) and nowhere else: a probe's source is then far from its anchor whatever frame refreshed it last, and every
other pixel has D = 0.  `drive` runs the whole list for one band."""
import numpy as np

import hold_ref as H
import tile_walk as W

FMT8, FMT16 = 1, 2
K = {FMT8: 200, FMT16: 3000}            # (INDEX16: indices that need their high byte)
FAR = 0x00808080                        # the top bit of R, G and B: far beyond any tolerance below
NEAR = 0x00010101                       # the lowest bit of each: within TOL
TOL = 40000


def torch_dtype(torch, fmt):
    return torch.uint8 if fmt == FMT8 else torch.int16


def palette_words(k):
    """k distinct non-zero RGBA8 words (an odd multiplier permutes the 24-bit values)"""
    j = np.arange(1, k + 1, dtype=np.uint64)
    return (((j * 0x9E3779B1) & 0xFFFFFF) | 0xFF000000).astype(np.uint32)


class _State:
    lossy = False
    kernel = "hold"

    def __init__(self, torch, processor, oracle, fmt, width, rows, offs=0):
        import kmeans_gpu_amd as kg
        self.torch, self.p, self.oracle, self.fmt, self.width, self.rows, self.k = torch, processor, oracle, fmt, width, rows, K[fmt]
        self.n, self.offs, self.frames = width * rows, offs, 0
        self.size = 1 if fmt == FMT8 else 2
        self.gen = torch.Generator(device="cuda")
        self.gen.manual_seed(width * 31 + fmt)
        td = torch_dtype(torch, fmt)
        self.canvas = self._room(td)
        self.canvas.copy_(torch.randint(0, self.k, (self.n,), dtype=td, device="cuda", generator=self.gen))
        self.index = self._room(td)
        self.index.copy_(self.canvas)
        self.delta = self._room(td)
        self.delta.fill_(self.k)
        self.fresh = torch.from_numpy(np.frombuffer(kg.FrameHold.fresh_bytes(), np.int64).copy()).cuda()
        self.info = self.fresh.clone()
        self.st = torch.cuda.current_stream().cuda_stream
        self.dirty = []                 # pixels whose map differs from the canvas in the coming frame

    def _room(self, dtype, n=None):
        n = self.n if n is None else n
        return self.torch.zeros(n + 32, dtype=dtype, device="cuda")[self.offs:self.offs + n]

    def ptr(self, t, first=0):
        return t.data_ptr() + t.element_size() * first

    def shift(self, first):
        """k_frame_delta's: elements between the 16-byte boundary below the band and the band"""
        return 0

    def mark(self, pixels):
        pass

    def other(self, g):
        """an index below k that differs from the one the canvas shows at g"""
        return (int(self.index[g]) + 1 + g % (self.k - 1)) % self.k

    def set(self, g, value):
        self.index[g] = value
        self.dirty.append((g, value))

    def _launch(self, first, rows, row0):
        raise NotImplementedError

    def run(self, bands=None):
        import kmeans_gpu_amd as kg
        self.info.copy_(self.fresh)
        for r0, r1 in (bands or [(0, self.rows)]):
            self._launch(r0 * self.width, r1 - r0, r0)
        self.torch.cuda.synchronize()
        self.frames += 1
        return kg.FrameHold.from_array(self.info.cpu().numpy()).as_tuple()

    def check(self, first=0, held=()):
        """the maps after a frame whose band starts at element `first`; held: pixels that were planted to be held"""
        torch, k = self.torch, self.k
        sent = [(g, v) for g, v in self.dirty if g not in held]
        assert int(torch.count_nonzero(self.delta != k)) == sum(1 for _, v in sent if v != k), "the delta map"
        for g, v in sent:
            assert int(self.delta[g]) == v
        for g in held:
            self.index[g] = self._shown_index(g)
        self._check_state(first, held)
        self.dirty = []

    def _shown_index(self, g):
        return int(self.canvas[g])

    def _check_state(self, first, held):
        assert self.torch.equal(self.canvas, self.index), "the canvas"


class DeltaState(_State):
    """kmg_dev_frame_delta"""
    kernel = "delta"

    def shift(self, first):
        return (self.ptr(self.index, first) % 16) // self.size

    def _launch(self, first, rows, row0):
        assert self.ptr(self.index, first) % 16 == self.ptr(self.canvas, first) % 16 == self.ptr(self.delta, first) % 16
        self.p.frame_delta(self.ptr(self.index, first), self.ptr(self.canvas, first), self.width, rows, row0, self.fmt, self.k,
                           self.ptr(self.delta, first), self.info.data_ptr(), self.st)


class _Lossy(_State):
    lossy = True

    def _sources(self):
        torch = self.torch
        self.A = torch.randint(-2 ** 31, 2 ** 31 - 1, (self.n,), dtype=torch.int32, device="cuda", generator=self.gen)
        self.B = self.A.clone()
        self.held = self.A.clone()

    def mark(self, pixels):
        at = self.torch.tensor(sorted(set(pixels)), dtype=self.torch.int64, device="cuda")
        self.B[at] = self.B[at] ^ FAR

    def src(self):
        return self.A if self.frames % 2 else self.B        # (the first frame takes B: every anchor starts as A)

    def plant_held(self, pixels):
        """the map moves at `pixels` (unmarked ones) and their source stays within TOL of the anchor: (held, held_sse) they add"""
        s, sse = self.src(), 0
        for g in pixels:
            assert int(self.A[g]) == int(self.B[g]) == int(self.held[g])
            _State.set(self, g, self.other(g))
            s[g] = s[g] ^ NEAR
            both = np.array([int(s[g]), int(self.held[g])], np.int32).view(np.uint8).reshape(2, 4)
            D = int(H.distance(self.oracle, both[:1], both[1:])[0])
            assert D <= TOL
            sse += D
        return len(pixels), sse

    def unplant(self, pixels):
        for g in pixels:
            self.A[g] = self.held[g]
            self.B[g] = self.held[g]

    def _check_state(self, first, held):
        torch = self.torch
        last = self.B if self.frames % 2 else self.A        # (frames counts the one that just ran)
        moved = torch.nonzero(self.held[first:] != last[first:]).reshape(-1)
        assert sorted(int(v) + first for v in moved) == sorted(held), "the held source"
        self._check_shown()


class HoldState(_Lossy):
    """kmg_dev_frame_delta_lossy"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._sources()

    def _check_shown(self):
        assert self.torch.equal(self.canvas, self.index), "the canvas"

    def _launch(self, first, rows, row0):
        self.p.frame_delta_lossy(self.ptr(self.src(), first), self.ptr(self.index, first), self.ptr(self.canvas, first), self.ptr(self.held, first),
                                 self.width, rows, row0, self.fmt, self.k, TOL, self.ptr(self.delta, first), self.info.data_ptr(), self.st)


class LocalState(_Lossy):
    """kmg_dev_frame_delta_colour (lossy=False) and kmg_dev_frame_delta_colour_lossy: the canvas is the shown words"""

    def __init__(self, torch, processor, oracle, fmt, width, rows, lossy):
        super().__init__(torch, processor, oracle, fmt, width, rows)
        self.lossy = lossy
        words = np.concatenate([palette_words(self.k), np.zeros(1, np.uint32)])
        self.pal = torch.from_numpy(words.view(np.int32)).cuda()               # (entry k: what slot k shows -- nothing)
        self.shown = self.pal[self.index.long()]
        self.was = self.index.clone()                                            # the index each pixel shows
        del self.canvas
        self._sources()

    def _shown_index(self, g):
        return int(self.was[g])

    def plant_held(self, pixels):
        self.was.copy_(self.index)
        return super().plant_held(pixels)

    def _check_state(self, first, held):
        if self.lossy:
            super()._check_state(first, held)
        else:
            self._check_shown()

    def _check_shown(self):
        assert self.torch.equal(self.shown, self.pal[self.index.long()]), "the shown words"

    def _launch(self, first, rows, row0):
        if self.lossy:
            self.p.frame_delta_colour_lossy(self.ptr(self.src(), first), self.ptr(self.index, first), self.pal.data_ptr(), self.ptr(self.shown, first),
                                            self.ptr(self.held, first), self.width, rows, row0, self.fmt, self.k, TOL, self.ptr(self.delta, first),
                                            self.info.data_ptr(), self.st)
        else:
            self.p.frame_delta_colour(self.ptr(self.index, first), self.pal.data_ptr(), self.ptr(self.shown, first), self.width, rows, row0,
                                      self.fmt, self.k, self.ptr(self.delta, first), self.info.data_ptr(), self.st)


def box(width, pixels, cleared=0, held=(0, 0)):
    ys, xs = zip(*[divmod(g, width) for g in pixels])
    return (len(pixels), cleared, min(xs), min(ys), max(xs) + 1, max(ys) + 1) + tuple(held)


def drive(S, per, row0=0):
    """every probe of the band that starts at row `row0` as a frame of its own, pairs of probes as one frame, one clear, and -- lossy --
    held pixels beside a probe and a probe sent twice in a row; with row0 > 0 also a frame that runs as the two bands [0, row0) and
    [row0, rows) with a probe in each"""
    width, first = S.width, row0 * S.width
    tile = W.tile_elems(S.kernel, S.size)
    w = W.walk(S.n - first, width, tile, S.shift(first))
    assert w.tiles > W.WORKGROUPS and w.per == per
    ps = W.probes(w)
    at = [first + p.i for p in ps]
    above = (row0 // 2) * width + 7 if row0 else None                   # a pixel of the band above
    S.mark(at + ([above] if row0 else []))
    bands = [(row0, S.rows)]
    clear = next(t for t, p in enumerate(ps) if "second_tile" in p.labels and "wg_mid" in p.labels)
    for t, (p, g) in enumerate(zip(ps, at)):
        S.set(g, S.k if t == clear else S.other(g))
        rec = S.run(bands)
        assert rec == box(width, [g], cleared=int(t == clear)), (sorted(p.labels), W.locate(w, p.i), g, rec)
        S.check(first)
    for a, b in W.pairs(ps):
        both = [first + a.i, first + b.i]
        for g in both:
            S.set(g, S.other(g))
        rec = S.run(bands)
        assert rec == box(width, both), (both, rec)
        S.check(first)
    if S.lossy:
        g = at[1]
        taken = set(at)
        plants = [q for q in (at[3] + 1, at[len(at) // 2] - 1, at[-1] - 2) if q not in taken and first <= q < S.n]
        assert len(plants) >= 2
        held = S.plant_held(plants)
        S.set(g, S.other(g))
        rec = S.run(bands)
        assert rec == box(width, [g], held=held), (g, plants, rec)
        S.check(first, held=plants)
        S.unplant(plants)
        for _ in range(2):                                               # the same probe again: its anchor is the frame before
            S.set(g, S.other(g))
            assert S.run(bands) == box(width, [g])
            S.check(first)
    if row0:
        if S.lossy and S.frames % 2:                                     # the band above is anchored at A: its probe needs B
            assert S.run(bands) == H.FRESH
            S.check(first)
        both = [above, at[len(at) // 3]]
        for g in both:
            S.set(g, S.other(g))
        rec = S.run([(0, row0), (row0, S.rows)])
        assert rec == box(width, both), (both, rec)
        S.check(0)
