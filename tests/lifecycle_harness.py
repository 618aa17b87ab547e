"""TEST HARNESS: model-based random call sequences on ONE long-lived processor (tests/test_lifecycle_model.py on the CPU,
tools/fuzz_lifecycle.py and tests/test_gpu_lifecycle.py on the device).

Every operation of the C ABI is a pure function of (pixels, current centroids, a few documented switches), so a stateless
model -- the CPU oracle -- predicts the exact result of every call of any legal sequence and the status of the refused ones.
What a sequence exercises is the STATE the kernels run in: blocks handed from one object to the next, bindings keyed on a
pointer, label tables that are valid or not, the accumulator that must be zero between passes, a cell share, the switches.

  generate(seed, seq)  -> list of plain tuples (deterministic; consults a dry Model so that every op is legal or a listed refusal)
  Runner(env).run(ops) -> executes them on a backend, checks EVERYTHING after every op, raises Mismatch at the first difference
  replay(env, ops)     -> the same for a list printed by a failing run

A backend `env` supplies: mem (alloc / write / read / fill on "device" buffers with a .ptr), streams (two), sync(), processor()
(the surface of kmeans_gpu_amd.ImageProcessor), lloyd(proc, k) (kmeans_gpu_amd.Lloyd), Error (with .status).  KgEnv is the real
binding; the CPU stand-ins live in tests/test_lifecycle_model.py.  No GPU import at module level.

The runner reads everything back after every op, which leaves the device idle between ops -- except after an iterate with
flush = 2: nothing is flushed, synchronised or read, the next op (set_centroids, update, get_centroids, close, a re-creation) is
issued on the same stream while the label pass is still pending on the library's side stream, and the label map it owed is
checked after that op.

What the generator never emits, because include/kmeans_hip.h leaves it open: a pass on a bound buffer whose pixels changed (an
in-place upload is followed at once, per object bound to it, by init_centroids / bind_image / unbind_image, by prepare for a
caller's binding, or by set_centroids + run for a binding the initialisation made); a pass before the centroids were set;
converged_count before an update; labels_from_tables unless one pass or one whole round of shares filled the tables for ONE
centroid table; anything but the listed refusals on a bound image while a cell share is set; under strategy auto, init /
prepare / run on another buffer than the bound one (the object is unbound first: whether they re-bind is the cost model's)."""
import collections
import os

import numpy as np

import oracle_lib as O
import diffuse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_K = 3072
MAX_ITERATIONS, CHECK_PERIOD = 6, 2
CAPS = (1 << 20, 40960, 32768)                     # pixels of the three device pixel buffers
GUARD = 64                                         # guard bytes behind every output
PATTERN = 0xA5
K_CLASSES = ((1, 1), (2, 32), (33, 256), (257, 512), (513, MAX_K))
STRATEGIES = (0, 1, 2, 6)                          # auto, scan, table, table + mask_words
IMAGE_KINDS = ("noise", "few", "blobs", "gradient", "flat", "tokyo", "tiny", "large", "mega")
NI = len(IMAGE_KINDS)                               # image i + NI: the next frame of image i
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
REFUSALS = ("run", "iterate", "assign_update", "labelmap", "partials", "lftu_bigk", "unbound_lft", "unbound_into",
            "unbound_share", "unbound_rebuild", "share_bad")


class Mismatch(AssertionError):
    pass


def k_class(k):
    return next(i for i, (a, b) in enumerate(K_CLASSES) if a <= k <= b)


# ---- images ---------------------------------------------------------------------------------------------------------
_tokyo = None


def _tokyo_image():
    global _tokyo
    if _tokyo is None:
        from PIL import Image
        _tokyo = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "tokyo.png")).convert("RGBA"))
    return _tokyo


_images = {}


def make_images(seed, seq):
    """the host images of one sequence: [(kind, (h, w, 4) uint8)], random alpha on all of them (alpha mode stays off).  "mega" is
    1024 x 1024: at 2^20 pixels the per-pixel scan works four pixels per thread on 1024 partial rows and kmg_lloyd_run leaves the
    one-launch loop of small images for the general one"""
    if (seed, seq) not in _images:
        if len(_images) > 2:
            _images.clear()
        _images[(seed, seq)] = _make_images(seed, seq)
    return _images[(seed, seq)]


def _make_images(seed, seq):
    rng = np.random.default_rng([seed, seq, 77])
    out = []
    for kind in IMAGE_KINDS:
        if kind == "noise":
            w, h = int(rng.integers(150, 220)), int(rng.integers(100, 150))
            a = rng.integers(0, 256, (h * w, 4), dtype=np.uint8)
        elif kind == "few":
            w, h = int(rng.integers(100, 170)), int(rng.integers(60, 100))
            pal = rng.integers(0, 256, (int(rng.integers(2, 13)), 4), dtype=np.uint8)
            a = pal[rng.integers(0, pal.shape[0], h * w)]
        elif kind in ("blobs", "large", "mega"):
            w, h = {"blobs": (int(rng.integers(150, 200)), int(rng.integers(90, 130))), "large": (512, int(rng.integers(300, 500))),
                    "mega": (1024, 1024)}[kind]
            c = rng.integers(0, 256, (int(rng.integers(3, 24)), 3))
            a = np.zeros((h * w, 4), np.uint8)
            a[:, :3] = np.clip(c[rng.integers(0, c.shape[0], h * w)] + rng.normal(0, rng.uniform(3, 25), (h * w, 3)), 0, 255).astype(np.uint8)
        elif kind == "gradient":
            w, h = 256, int(rng.integers(40, 80))
            i = np.arange(w * h)
            a = np.stack([(i % w) * 255 // (w - 1), (i // w) * 255 // (h - 1), (i * 7) % 256, i % 256], 1).astype(np.uint8)
        elif kind == "flat":
            w, h = 64, 48
            a = np.tile(rng.integers(0, 256, (1, 4), dtype=np.uint8), (w * h, 1))
        elif kind == "tokyo":
            t = _tokyo_image()
            w, h = 160, 120
            y, x = int(rng.integers(0, t.shape[0] - h)), int(rng.integers(0, t.shape[1] - w))
            a = np.ascontiguousarray(t[y:y + h, x:x + w]).reshape(-1, 4).copy()
        else:  # tiny: what the top k class runs on
            w, h = int(rng.integers(20, 40)), int(rng.integers(20, 30))
            a = rng.integers(0, 256, (h * w, 4), dtype=np.uint8)
        a[:, 3] = rng.integers(0, 256, h * w, dtype=np.uint8)
        out.append((kind, np.ascontiguousarray(a).reshape(h, w, 4)))
    # image i + NI: the NEXT FRAME of image i -- the same size, other colours (what arrives in a recycled buffer)
    for kind, a in list(out):
        b = a.copy()
        b[..., :3] ^= 0x5A
        out.append((kind, b))
    return out


def make_centroids(kind, seed, k, image=None):
    """the tables set_centroids uploads: oracle init of an image, random Lab, duplicates, far outside the gamut"""
    rng = np.random.default_rng([seed, k, 5])
    if kind == "init":
        h, w = image.shape[:2]
        return O.init_centroids(O.rgb_to_lab(image.reshape(-1, 4)), w, h, k)
    c = np.ones((k, 4), np.float32)
    c[:, 0] = rng.uniform(0, 100, k); c[:, 1] = rng.uniform(-90, 90, k); c[:, 2] = rng.uniform(-90, 90, k)
    if kind == "dup" and k > 1:
        c[rng.integers(0, k, max(k // 2, 1))] = c[int(rng.integers(0, k))]
    if kind == "far":
        far = rng.random(k) < 0.5
        c[far, :3] = rng.uniform(-4000, 4000, (int(far.sum()), 3)).astype(np.float32)
    return c


def gamut_centroids(seed, k):
    pal = np.random.default_rng([seed, k, 9]).integers(0, 256, (k, 4), dtype=np.uint8)
    pal[:, 3] = 255
    return O.centroids4(O.rgb_to_lab(pal)), pal


def cell_of(px):
    """cell of the 32^3 grid a colour lies in (kmg_lloyd_set_cell_share: ranges of this index)"""
    return ((px[:, 0].astype(np.uint32) >> 3) << 10) | ((px[:, 1].astype(np.uint32) >> 3) << 5) | (px[:, 2].astype(np.uint32) >> 3)


# ---- the model ------------------------------------------------------------------------------------------------------
class Slot:
    def __init__(self, k):
        self.k = k
        self.cent = None          # numeric: (k, 4) float32; dry: True once known
        self.nconv = None
        self.bind = None          # (buf, off, n, by, sure): by = "caller" | "init"
        self.share = None         # (part, parts) with parts > 1
        self.tab = None           # centroid bytes the complete label tables describe (dry: True)
        self.acc = None


class Model:
    """legality state of a sequence (dry: what the generator consults) and, numeric, the expected results from the oracle"""

    def __init__(self, images, numeric, cache=None):
        self.images = images
        self.numeric = numeric
        self.slots = [None, None, None]
        self.bufs = [None, None, None]          # image index each pixel buffer holds
        self.strategy = 0
        self.cache = {} if cache is None else cache     # (a caller's dict: the oracle's answers serve several runs of one sequence)

    # -- oracle, cached by (image, band, centroid bytes)
    def px(self, buf, off, n):
        return self.images[self.bufs[buf]][1].reshape(-1, 4)[off:off + n]

    def lab(self, buf, off, n):
        key = ("lab", self.bufs[buf], off, n)
        if key not in self.cache:
            self.cache[key] = O.rgb_to_lab(self.px(buf, off, n))
        return self.cache[key]

    def assign(self, buf, off, n, cent):
        key = ("as", self.bufs[buf], off, n, cent.tobytes())
        if key not in self.cache:
            labels = O.assign(self.lab(buf, off, n), cent)
            self.cache[key] = (labels, O.accumulate(self.lab(buf, off, n), labels, cent.shape[0]))
        return self.cache[key]

    def share_sums(self, buf, off, n, cent, part, parts):
        labels, _ = self.assign(buf, off, n, cent)
        cell = cell_of(self.px(buf, off, n))
        m = (cell >= (32768 * part) // parts) & (cell < (32768 * (part + 1)) // parts)
        return O.accumulate(self.lab(buf, off, n)[m], labels[m], cent.shape[0])

    # -- legality helpers
    def bound_here(self, s, buf, off, n):
        return s.bind is not None and s.bind[:3] == (buf, off, n)

    def sure_here(self, s, buf, off, n):
        return self.bound_here(s, buf, off, n) and s.bind[4]

    def set_bind(self, s, bind):
        s.bind, s.share, s.tab = bind, None, None

    def forced(self):
        return {0: 0, 1: -1, 2: 1, 6: 1}[self.strategy]


# ---- the generator --------------------------------------------------------------------------------------------------
def generate(seed, seq, n_ops=110):
    """one sequence: a list of plain tuples"""
    rng = np.random.default_rng([seed, seq])
    images = make_images(seed, seq)
    m = Model(images, numeric=False)
    ops, pending = [], []

    def emit(op):
        ops.append(op)
        apply_op(m, op)

    def rint(a, b):
        return int(rng.integers(a, b))

    def pick(xs, p=None):
        return xs[int(rng.choice(len(xs), p=p))]

    def pick_k():
        cls = pick([0, 1, 2, 3, 4], [0.1, 0.36, 0.3, 0.16, 0.08])
        lo, hi = K_CLASSES[cls]
        k = rint(lo, hi + 1)
        if rng.random() < 0.3:
            k = pick([lo, hi])
        return k

    def live():
        return [i for i, s in enumerate(m.slots) if s is not None]

    def image_n(buf):
        h, w = images[m.bufs[buf]][1].shape[:2]
        return w * h

    def k_fits(k, n):
        return (k <= 512 or n <= 5000) and (k <= 256 or n <= 70000) and (k <= 32 or n <= 300000)

    def target(L, want_bound=0.6, band=0.3):
        """(buf, off, n) for a pass of slot L: its bound image, a whole image or a band of one, small enough for its k"""
        s = m.slots[L]
        if s.bind is not None and rng.random() < want_bound and k_fits(s.k, s.bind[2]):
            return s.bind[:3]
        for _ in range(20):
            buf = rint(0, 3)
            if m.bufs[buf] is None:
                continue
            n = image_n(buf)
            off = 0
            if rng.random() < band and n > 64:
                off = rint(0, n // 2)
                n = rint(1, n - off + 1) if rng.random() < 0.5 else rint(1, min(n - off, 5000) + 1)
            if not k_fits(s.k, n):
                n = 5000 if s.k > 512 else 70000 if s.k > 256 else 300000
                off = 0
            n = min(n, image_n(buf) - off)
            # a pass on a DIFFERENT range of a buffer the object has bound is a pass on unbound pixels: fine
            return (buf, off, n)
        return None

    def st():
        return rint(0, 2)

    def unbind_first(L, buf, off, n):
        s = m.slots[L]
        if m.forced() == 0 and s.bind is not None and s.bind[:3] != (buf, off, n):
            emit(("unbind", L))

    def recover(buf, force=None):
        """an image was uploaded in place: every object bound to that buffer starts over, as the header asks"""
        n = image_n(buf)
        for L in live():
            s = m.slots[L]
            if s.bind is None or s.bind[0] != buf:
                continue
            by = s.bind[3]
            choices = ["init", "bind", "unbind", "prepare" if by == "caller" else "setrun"]
            if not k_fits(s.k, n) or s.bind[1] != 0:              # (a band further up: prepare / init / run of the new image
                choices = ["unbind"]                              #  work on another pointer and need not drop that binding)
            c = pick(choices, None if len(choices) == 1 else [0.2, 0.2, 0.1, 0.5])
            if force in choices:
                c = force
            if c == "init":
                unbind_first(L, buf, 0, n)
                emit(("init", L, buf, st()))
            elif c == "bind":
                emit(("bind", L, buf, 0, n, st()))
            elif c == "unbind":
                emit(("unbind", L))
            elif c == "prepare":
                unbind_first(L, buf, 0, n)
                emit(("prepare", L, buf, 0, n, rint(0, 2), st()))
            else:
                emit(("set_cent", L, pick(["init", "rand"]), rint(0, 1 << 30), m.bufs[buf]))
                unbind_first(L, buf, 0, n)
                emit(("run", L, buf, 0, n, rint(0, 2), st()))
            if m.slots[L].cent is not None and m.slots[L].share is None and rng.random() < 0.8:
                emit(("assign", L, buf, 0, n, rint(0, 2), 1, st()))

    # every sequence starts with its buffers filled, the larger image in the first one
    emit(("upload", 0, pick([IMAGE_KINDS.index("mega"), IMAGE_KINDS.index("large"), rint(0, 6)], [0.35, 0.4, 0.25])))
    emit(("upload", 1, rint(0, 7)))
    emit(("upload", 2, rint(0, 7)))
    emit(("strategy", pick([2, 2, 0, 6])))
    while len(ops) < n_ops:
        if pending:
            op = pending.pop(0)
            if op is not None and legal(m, op):
                emit(op)
            continue
        r = rng.random()
        Ls = live()
        if not Ls or (len(Ls) < 3 and r < 0.06):
            L = [i for i in range(3) if m.slots[i] is None][0]
            emit(("create", L, pick_k()))
            continue
        L = pick(Ls)
        s = m.slots[L]
        if r < 0.09:                                              # object life
            c = rng.random()
            if c < 0.25:
                emit(("close", L))
            else:
                k = pick_k()
                while k_class(k) == k_class(s.k):
                    k = pick_k()
                emit(("recreate", L, k))
                # the new object works in the old one's blocks: bind and read labels before any pass filled the tables
                t = target(L, 0.0, 0.0)
                if t is not None and k_fits(k, t[2]):
                    emit(("set_cent", L, pick(["rand", "dup"]), rint(0, 1 << 30), 0))
                    emit(("bind", L, t[0], t[1], t[2], st()))
                    emit(("labels", L, t[0], t[1], t[2], st()))
                    if k > 256:
                        emit(("refuse", L, "lftu_bigk", st()))
            continue
        if r < 0.16:                                              # pixels
            bound = [b for b in range(3) if any(x is not None and x.bind is not None and x.bind[0] == b for x in m.slots)]
            buf = pick(bound) if bound and rng.random() < 0.7 else rint(0, 3)
            img = rint(0, NI)
            h, w = images[img][1].shape[:2]
            if w * h > CAPS[buf]:
                img = rint(0, 7)
            if m.bufs[buf] is not None and rng.random() < 0.35:
                img = (m.bufs[buf] + NI) % (2 * NI)                      # the next frame: same size, new pixels
            emit(("upload", buf, img))
            recover(buf)
            continue
        if r < 0.22:                                              # switches
            c = rng.random()
            if c < 0.4:
                emit(("strategy", pick(list(STRATEGIES), [0.2, 0.15, 0.45, 0.2])))
            elif c < 0.75:
                ncu = pick([1, 8, 64, 128])
                emit(("reserve", L, ncu))
                # a label map under the reservation, then back to all CUs
                if s.cent is not None and s.share is None:
                    t = s.bind[:3] if s.bind is not None and s.bind[4] and k_fits(s.k, s.bind[2]) else target(L, 0.0, 0.0)
                    if t is not None:
                        if not m.sure_here(s, *t):
                            emit(("bind", L, t[0], t[1], t[2], st()))
                        emit(("assign", L, t[0], t[1], t[2], 1, rint(0, 2), st()))
                if rng.random() < 0.7:
                    pending.append(("reserve", L, 0))
            elif c < 0.9:
                emit(("profile", L, rint(0, 2)))
            else:
                emit(("profile_read", L))
            continue
        if r < 0.30:                                              # neighbours on the same processor
            c = rng.random()
            if c < 0.7:
                bufs = [b for b in range(3) if m.bufs[b] is not None and image_n(b) <= 40000]
                if bufs:
                    mode = rint(0, 4)
                    fmt = pick([None, None, 1, 2]) if mode != 2 else None
                    k = pick_k() if fmt != 1 else rint(1, 257)
                    if k > 512:
                        k = rint(2, 400)
                    if mode == 3:
                        k = min(k, 300)
                    emit(("apply", pick(bufs), mode, fmt, k, rint(0, 1 << 30), rint(0, 2), st()))
            else:
                emit(("host", pick(["find", "reduce", "palette"]), pick([1, 3, 4, 5, 6]), rint(1, 40), rint(0, 4), rint(0, 1 << 30)))
            continue
        if s.cent is None or r < 0.40:                            # centroids
            c = rng.random()
            if c < 0.45 or s.cent is None and c < 0.7:
                kind = pick(["init", "rand", "dup", "far"], [0.3, 0.4, 0.15, 0.15])
                img = pick([1, 3, 4, 5, 6]) if s.k <= 300 else 6
                emit(("set_cent", L, kind, rint(0, 1 << 30), img))
            elif c < 0.8 or s.cent is None:
                bufs = [b for b in range(3) if m.bufs[b] is not None and k_fits(s.k, image_n(b)) and (s.k <= 256 or image_n(b) <= 5000 or rng.random() < 0.3)]
                if not bufs:
                    continue
                buf = pick(bufs)
                if s.share is not None and s.bind[0] != buf:
                    continue
                unbind_first(L, buf, 0, image_n(buf))
                emit(("init", L, buf, st()))
                if m.slots[L].bind is not None and m.slots[L].bind[3] == "init" and rng.random() < 0.4:
                    # the next frame arrives in the same buffer before any pass ran: the initialisation's binding is of the old one
                    emit(("upload", buf, (m.bufs[buf] + NI) % (2 * NI)))
                    recover(buf, "setrun")
                    continue
            else:
                emit(("get", L, st()))
            if s is m.slots[L] and s.cent is not None and s.bind is not None and s.bind[4] and s.share is None and rng.random() < 0.7 \
                    and k_fits(s.k, s.bind[2]):
                emit(("labels", L, s.bind[0], s.bind[1], s.bind[2], st()))
            continue
        # ---- from here on the object has centroids
        if s.share is not None:                                   # a cell share is set: refusals, another round, or a reset
            buf, off, n = s.bind[:3]
            c = rng.random()
            if c < 0.45:
                kinds = ["run", "iterate", "assign_update", "labelmap", "partials"]
                for i in rng.permutation(5):                      # (refused before anything is launched: cheap, so all five)
                    emit(("refuse", L, kinds[int(i)], st()))
                emit(("share_round", L, 1, 0, 0, min(n, rint(1, n + 1)), 0, st()))
            elif c < 0.6:
                emit(("share_round", L, pick([1, 2, 3, 4, 8]), int(s.k <= 256 and rng.random() < 0.5), 0, n, rint(0, 2), st()))
            elif c < 0.8:
                emit(("bind", L, buf, off, n, st()))
                emit(("assign", L, buf, off, n, rint(0, 2), 1, st()))
            else:
                if off == 0 and n == image_n(buf):
                    emit(("init", L, buf, st()))
                else:
                    emit(("bind", L, buf, off, n, st()))
                emit(("assign", L, buf, off, n, rint(0, 2), 1, st()))
            continue
        if r < 0.50:                                              # binding
            t = target(L, 0.3)
            if t is None:
                continue
            c = rng.random()
            if c < 0.4:
                emit(("bind", L, *t, st()))
            elif c < 0.7:
                unbind_first(L, *t)
                emit(("prepare", L, *t, rint(0, 2), st()))
            elif c < 0.8:
                emit(("unbind", L))
            elif s.bind is not None and s.bind[4]:
                emit(("rebuild", L, st()))
                emit(("assign", L, *s.bind[:3], rint(0, 2), 1, st()))
            continue
        if r < 0.62 and s.bind is not None and s.bind[4] and k_fits(s.k, s.bind[2]):     # cell shares
            n = s.bind[2]
            fused = int(s.k <= 256 and rng.random() < 0.5)
            b_off = rint(0, n) if rng.random() < 0.4 else 0
            b_n = rint(1, n - b_off + 1) if b_off or rng.random() < 0.3 else n
            emit(("share_round", L, pick([1, 2, 3, 4, 8]), fused, b_off, b_n, int(rng.random() < 0.5), st()))
            continue
        if r < 0.68:                                              # refusals that need no share
            c = rng.random()
            if c < 0.3:
                emit(("refuse", L, "share_bad", st()))
            elif s.bind is None:
                emit(("refuse", L, pick(["unbound_lft", "unbound_into", "unbound_share", "unbound_rebuild"]), st()))
            elif s.k > 256 and s.bind[4]:
                emit(("refuse", L, "lftu_bigk", st()))
            continue
        t = target(L)
        if t is None:
            continue
        c = rng.random()                                          # passes
        after_update = False
        if c < 0.18:
            lab, sums = pick([(1, 1), (1, 0), (0, 1)])
            emit(("assign", L, *t, lab, sums, st()))
        elif c < 0.28:
            emit(("labels", L, *t, st()))
        elif c < 0.40:
            emit(("partials", L, *t, rint(0, 2), st()))
            if t[2] >= 8192:                                      # then a smaller pass: fewer partial rows than the last one left
                pending.append(("partials", L, t[0], t[1], rint(1, 4097), rint(0, 2), st()))
        elif c < 0.48:
            emit(("update", L, st()))
            after_update = True
        elif c < 0.60:
            emit(("assign_update", L, *t, rint(0, 2), rint(0, 2), st()))
            after_update = True
        elif c < 0.78:
            if m.sure_here(s, *t) and rng.random() < 0.3:
                # left in flight (flush = 2: no flush, no device synchronisation, nothing read back): the next call on the object
                # meets the label pass still pending on the library's side stream, on the caller's stream 0
                emit(("iterate", L, *t, 1, rint(2, 5), int(rng.random() < 0.85), 2, 0))
                c2 = rng.random()
                if c2 < 0.35:
                    emit(("set_cent", L, pick(["rand", "dup"]), rint(0, 1 << 30), 0))
                    emit(("labels", L, *t, 0))
                elif c2 < 0.55:
                    emit(("update", L, 0))
                elif c2 < 0.7:
                    emit(("get", L, 0))
                elif c2 < 0.85:
                    emit(("close", L))
                else:
                    emit(("recreate", L, pick_k()))
                continue
            if m.sure_here(s, *t):                                # the overlapped path: two sets of label tables
                emit(("iterate", L, *t, 1, rint(2, 5), int(rng.random() < 0.85), int(rng.random() < 0.4), st()))
            else:
                emit(("iterate", L, *t, int(rng.random() < 0.8), rint(1, 5), int(rng.random() < 0.8), rint(0, 2), st()))
        elif c < 0.84:
            if s.nconv is not None:
                emit(("conv", L, st()))
        elif c < 0.94:
            unbind_first(L, *t)
            emit(("run", L, *t, rint(0, 2), st()))
        elif s.tab is not None:
            n = s.bind[2]
            b_off = rint(0, n)
            emit(("lft", L, b_off, rint(1, n - b_off + 1), st()))
        if after_update and s.bind is not None and s.bind[4] and k_fits(s.k, s.bind[2]) and rng.random() < 0.6:
            emit(("labels", L, *s.bind[:3], st()))                # the tables describe the centroids of before the update
        if rng.random() < 0.25 and m.slots[L] is s and s.cent is not None:
            emit(("get", L, st()))
    for L in live():
        emit(("close", L))
    return ops


def legal(m, op):
    """a queued op is dropped if what happened since made it illegal.  Only the kinds the generator queues are known here
    (partials, assign, reserve); any other kind is refused"""
    s = m.slots[op[1]] if isinstance(op[1], int) and op[0] not in ("upload", "apply", "strategy", "host") else None
    if op[0] in ("partials", "assign"):
        return s is not None and s.cent is not None and s.share is None and m.bufs[op[2]] is not None and \
            op[3] + op[4] <= m.images[m.bufs[op[2]]][1].shape[0] * m.images[m.bufs[op[2]]][1].shape[1]
    if op[0] == "reserve":
        return s is not None
    return False


# ---- one op on the model: legality transitions always, expectations when numeric -------------------------------------
def apply_op(m, op):
    """advances the model by `op`; returns what the runner compares (numeric model) or None"""
    name, num = op[0], m.numeric
    exp = {}
    if name == "upload":
        m.bufs[op[1]] = op[2]
        return exp
    if name == "strategy":
        m.strategy = op[1]
        return exp
    if name in ("apply", "host"):
        return exp
    L = op[1]
    if name == "create":
        assert m.slots[L] is None
        m.slots[L] = Slot(op[2])
        if num:
            m.slots[L].acc = np.zeros((op[2], 4), np.int64)
        return exp
    if name == "recreate":
        m.slots[L] = Slot(op[2])
        if num:
            m.slots[L].acc = np.zeros((op[2], 4), np.int64)
        return exp
    s = m.slots[L]
    assert s is not None, op
    if name == "close":
        m.slots[L] = None
        return exp
    if name in ("reserve", "profile", "profile_read"):
        return exp
    if name == "set_cent":
        s.tab = None
        s.cent = make_centroids(op[2], op[3], s.k, m.images[op[4]][1]) if num else True
        return exp
    if name == "get":
        assert s.cent is not None
        exp["cent"] = s.cent
        return exp
    if name == "unbind":
        m.set_bind(s, None)
        return exp
    if name == "bind":
        m.set_bind(s, (op[2], op[3], op[4], "caller", True))
        return exp
    if name == "rebuild":
        assert s.bind is not None and s.bind[4] and s.share is None
        s.tab = None
        return exp
    if name == "init":
        buf = op[2]
        h, w = m.images[m.bufs[buf]][1].shape[:2]
        n = w * h
        f = m.forced()
        same = s.bind is not None and s.bind[0] == buf and s.bind[1] == 0
        if s.k == 1 or f < 0:
            if same:                      # "they drop any earlier binding of the buffer"
                m.set_bind(s, None)
        elif f > 0:
            m.set_bind(s, (buf, 0, n, "init", True))
        else:
            assert s.bind is None or same, op
            m.set_bind(s, (buf, 0, n, "init", False))
        s.tab, s.nconv = None, None
        s.cent = O.init_centroids(m.lab(buf, 0, n), w, h, s.k) if num else True
        exp["cent"] = s.cent
        return exp
    if name == "prepare":
        buf, off, n = op[2:5]
        f = m.forced()
        same = s.bind is not None and s.bind[0] == buf and s.bind[1] == off
        if f > 0:
            m.set_bind(s, (buf, off, n, "caller", True))
            exp["strategy"] = "table"
        elif f < 0:
            if same:
                m.set_bind(s, None)
            exp["strategy"] = "scan"
        else:
            assert s.bind is None or s.bind[:3] == (buf, off, n), op
            m.set_bind(s, (buf, off, n, "caller", False))
        return exp
    assert s.cent is not None, op
    if name == "update":
        s.tab = None
        if num:
            s.cent, s.nconv = O.finalize(s.acc, s.cent)
            exp["cent"] = s.cent
        else:
            s.nconv = True
        return exp
    if name == "conv":
        assert s.nconv is not None
        exp["nconv"] = s.nconv
        return exp
    if name == "lft":
        assert s.bind is not None and s.bind[4] and s.tab is not None
        if num:
            tab = np.frombuffer(s.tab, np.float32).reshape(-1, 4)
            exp["labels"] = m.assign(s.bind[0], s.bind[1], s.bind[2], tab)[0][op[2]:op[2] + op[3]]
        return exp
    if name == "refuse":
        what = op[2]
        exp["status"] = ERR_UNSUPPORTED if what == "lftu_bigk" else ERR_INVALID
        if what in ("run", "iterate", "assign_update", "labelmap", "partials"):
            assert s.share is not None
        elif what == "lftu_bigk":
            assert s.k > 256 and s.bind is not None and s.bind[4]
        elif what != "share_bad":
            assert s.bind is None
        exp["cent"] = s.cent
        return exp
    if name == "share_round":
        parts, fused, b_off, b_n, leave = op[2:7]
        assert s.bind is not None and s.bind[4] and (not fused or s.k <= 256)
        buf, off, n = s.bind[:3]
        if num:
            labels, sums = m.assign(buf, off, n, s.cent)
            exp["part_sums"] = [m.share_sums(buf, off, n, s.cent, p, parts) for p in range(parts)]
            assert np.array_equal(sum(exp["part_sums"]), sums)
            exp["labels"] = labels[b_off:b_off + b_n]
            if fused:
                s.cent, s.nconv = O.finalize(sums, s.cent)
                s.acc = np.zeros_like(s.acc)
                s.tab = None
            else:
                s.acc = exp["part_sums"][-1]
                s.tab = s.cent.tobytes()
            exp["cent"] = s.cent
        else:
            s.tab = None if fused else True
            if fused:
                s.nconv = True
        s.share = (parts - 1, parts) if leave and parts > 1 else None
        return exp
    if name == "run":
        buf, off, n, want = op[2:6]
        assert s.share is None or not m.bound_here(s, buf, off, n)
        if num:
            s.cent, labels, it = O.lloyd(m.lab(buf, off, n), s.cent, MAX_ITERATIONS, CHECK_PERIOD)
            exp.update(cent=s.cent, iterations=it)
            if want:
                exp["labels"] = labels
        s.nconv = None
        f = m.forced()
        if m.bound_here(s, buf, off, n) and s.bind[3] == "caller":
            s.tab = None
        elif f > 0 or (s.bind is not None and s.bind[0] == buf and s.bind[1] == off):
            m.set_bind(s, None)
        else:
            assert f < 0 or s.bind is None, op
        return exp
    # the passes on (buf, off, n)
    buf, off, n = op[2:5]
    here = m.sure_here(s, buf, off, n)
    assert s.share is None or not m.bound_here(s, buf, off, n), op
    if name == "labels":
        if num:
            exp["labels"] = m.assign(buf, off, n, s.cent)[0]
        return exp
    if name == "assign":
        want_l, want_s = op[5:7]
        if num:
            labels, sums = m.assign(buf, off, n, s.cent)
            if want_l:
                exp["labels"] = labels
            if want_s:
                s.acc = sums
        s.tab = (s.cent.tobytes() if num else True) if here else s.tab
        if not here and m.bound_here(s, buf, off, n):
            s.tab = None
        return exp
    if name == "partials":
        if num:
            labels, sums = m.assign(buf, off, n, s.cent)
            if op[5]:
                exp["labels"] = labels
            s.acc = sums
        s.tab = (s.cent.tobytes() if num else True) if here else (None if m.bound_here(s, buf, off, n) else s.tab)
        return exp
    if name == "assign_update":
        want_l, do_update = op[5:7]
        old = s.cent
        if num:
            labels, sums = m.assign(buf, off, n, s.cent)
            if want_l:
                exp["labels"] = labels
            s.acc = sums
            if do_update:
                s.cent, s.nconv = O.finalize(sums, s.cent)
            exp["cent"] = s.cent
        elif do_update:
            s.nconv = True
        s.tab = (old.tobytes() if num else True) if here else (None if m.bound_here(s, buf, off, n) or do_update else s.tab)
        return exp
    if name == "iterate":
        want_l, reps, update_first, flush = op[5:9]
        for _ in range(reps):
            if num:
                if update_first:
                    s.cent, s.nconv = O.finalize(s.acc, s.cent)
                labels, sums = m.assign(buf, off, n, s.cent)
                s.acc = sums
            elif update_first:
                s.nconv = True
        if num:
            exp["labels"] = labels
            exp["cent"] = s.cent
        s.tab = (s.cent.tobytes() if num else True) if here else (None if m.bound_here(s, buf, off, n) or update_first else s.tab)
        return exp
    raise ValueError(op)


# ---- the runner -----------------------------------------------------------------------------------------------------
def _bits(c):
    return np.ascontiguousarray(c, np.float32).view(np.uint32)


class Runner:
    """executes ops on a backend and compares with the numeric model after every op"""

    def __init__(self, env, seed, seq, counters=None, proc=None, cache=None):
        self.env, self.mem = env, env.mem
        self.images = make_images(seed, seq)
        self.model = Model(self.images, numeric=True, cache=cache)
        self.counters = counters if counters is not None else collections.Counter()
        self.own_proc = proc is None
        self.proc = env.processor() if proc is None else proc         # (a caller's processor outlives the sequence)
        self.pix = [self.mem.alloc(4 * c) for c in CAPS]
        self.lab = self.mem.alloc(4 * CAPS[0] + GUARD)
        self.lab2 = self.mem.alloc(4 * CAPS[0] + GUARD)     # the label map of an iterate left in flight
        self.pending = None                                 # (n, expected labels) of it, checked after the NEXT op
        self.out = self.mem.alloc(4 * 40960 + GUARD)
        self.acc = [None, None, None]
        self.obj = [None, None, None]
        self.n_ops = 0

    def close(self):
        for o in self.obj:
            if o is not None:
                o.close()
        self.obj = [None, None, None]
        if self.own_proc:
            self.proc.close()

    def fail(self, what, got=None, want=None):
        detail = ""
        if got is not None and want is not None:
            got, want = np.asarray(got), np.asarray(want)
            if got.shape == want.shape:
                bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
                detail = f": {bad.size} of {got.size} differ, first at {bad[:4].tolist()}: got {got.reshape(-1)[bad[:4]].tolist()} want {want.reshape(-1)[bad[:4]].tolist()}"
            else:
                detail = f": shape {got.shape} against {want.shape}"
        raise Mismatch(what + detail)

    # -- buffers with a pattern in front and guard bytes behind
    def arm(self, buf, nbytes):
        self.mem.fill(buf, 0, nbytes + GUARD, PATTERN)

    def collect(self, buf, nbytes, dtype, what):
        raw = self.mem.read(buf, 0, nbytes + GUARD)
        if not (raw[nbytes:] == PATTERN).all():
            self.fail(f"{what}: written past the end")
        return raw[:nbytes].view(dtype)

    def labels_ptr(self, n):
        self.arm(self.lab, 4 * n)
        return self.lab.ptr

    def check_labels(self, n, want, what="labels"):
        got = self.collect(self.lab, 4 * n, np.uint32, what)
        if not np.array_equal(got, want):
            self.fail(what, got, want)

    def new_acc(self, L, k):
        self.acc[L] = self.mem.alloc(32 * k + GUARD)
        self.mem.fill(self.acc[L], 32 * k, GUARD, PATTERN)
        self.mem.write(self.acc[L], 0, np.zeros(32 * k, np.uint8))

    def check_slot(self, L, exp, stream):
        """after every op on an object: its accumulators (and their guard), and the centroid bits when the model gives them"""
        s = self.model.slots[L]
        if s is None:
            return
        got = self.collect(self.acc[L], 32 * s.k, np.int64, "accumulators").reshape(s.k, 4)
        if not np.array_equal(got, s.acc):
            self.fail("accumulators", got, s.acc)
        if "cent" in exp and exp["cent"] is not None:
            got = self.obj[L].get_centroids(stream)
            if not np.array_equal(_bits(got), _bits(exp["cent"])):
                self.fail("centroid bits", _bits(got), _bits(exp["cent"]))

    def expect_status(self, status, fn, *args):
        try:
            fn(*args)
        except self.env.Error as e:
            if e.status != status:
                self.fail(f"refused with status {e.status}, the header names {status}")
            return
        self.fail(f"a call the header refuses with status {status} was accepted")

    def run(self, ops):
        for i, op in enumerate(ops):
            try:
                self.step(op)
            except Mismatch as e:
                raise Mismatch(f"op {i} {op!r}: {e}") from None
            except self.env.Error as e:
                raise Mismatch(f"op {i} {op!r}: a legal call was refused: {e}") from None
            self.n_ops += 1

    def ptr(self, buf, off):
        return self.pix[buf].ptr + 4 * off

    def step(self, op):
        """one op; if the op before it was left in flight, this one is issued without any device synchronisation in between, and
        the label map that one owes is read once this one is through (a device synchronisation completes it, like a flush)"""
        pend, self.pending = self.pending, None
        self.in_flight = pend is not None
        self.step_inner(op)
        if pend is not None:
            self.env.sync()
            got = self.collect(self.lab2, 4 * pend[0], np.uint32, "labels of the iterate left in flight")
            if not np.array_equal(got, pend[1]):
                self.fail("labels of the iterate left in flight before this op", got, pend[1])

    def quiesce(self):
        if not self.in_flight:
            self.env.sync()

    def step_inner(self, op):
        env, m, name = self.env, self.model, op[0]
        C = self.counters
        C["op:" + name] += 1
        if name == "upload":
            kind, img = self.images[op[2]]
            C["image:" + kind] += 1
            apply_op(m, op)
            env.sync()
            self.mem.write(self.pix[op[1]], 0, img.reshape(-1))
            return
        if name == "strategy":
            C[f"strategy:{op[1]}"] += 1
            apply_op(m, op)
            self.proc.set_strategy(op[1])
            return
        if name == "apply":
            return self.step_apply(op)
        if name == "host":
            return self.step_host(op)
        L = op[1]
        st = env.streams[op[-1]] if name not in ("create", "recreate", "close", "unbind", "reserve", "profile", "profile_read", "set_cent") \
            else env.streams[0]
        o = self.obj[L]
        old = m.slots[L]
        if name in ("create", "recreate"):
            if name == "recreate":
                C["reuse_across_k_class"] += int(k_class(old.k) != k_class(op[2]))
                self.quiesce()
                o.close()
            C[f"kclass:{k_class(op[2])}"] += 1
            apply_op(m, op)
            self.obj[L] = env.lloyd(self.proc, op[2])
            self.new_acc(L, op[2])
            return
        if name == "close":
            apply_op(m, op)
            self.quiesce()
            o.close()
            self.obj[L] = None
            return
        exp = apply_op(m, op)
        s = m.slots[L]
        acc = self.acc[L].ptr
        if name == "set_cent":
            C["centroids:" + op[2]] += 1
            o.set_centroids(s.cent, st)
        elif name == "get":
            pass
        elif name == "reserve":
            o.reserve_cus(op[2])
        elif name == "profile":
            o.profile(bool(op[2]))
        elif name == "profile_read":
            env.sync()
            o.profile_read()
        elif name == "unbind":
            o.unbind_image()
        elif name == "bind":
            o.bind_image(self.ptr(op[2], op[3]), op[4], st)
        elif name == "rebuild":
            o.rebuild_from_histogram(s.bind[2], st)
        elif name == "init":
            h, w = self.images[m.bufs[op[2]]][1].shape[:2]
            o.init_centroids(self.ptr(op[2], 0), w, h, st)
        elif name == "prepare":
            got = o.prepare(self.ptr(op[2], op[3]), op[4], bool(op[5]), st)
            if got not in ("scan", "table") or ("strategy" in exp and got != exp["strategy"]):
                self.fail(f"prepare chose {got!r} under strategy {m.strategy}")
        elif name == "update":
            o.update(acc, st)
        elif name == "conv":
            got = o.converged_count(st)
            if got != exp["nconv"]:
                self.fail(f"converged_count {got}, expected {exp['nconv']}")
        elif name == "labels":
            o.labels(self.ptr(op[2], op[3]), op[4], self.labels_ptr(op[4]), st)
            env.sync()
            self.check_labels(op[4], exp["labels"])
        elif name == "lft":
            b = s.bind
            o.labels_from_tables(self.ptr(b[0], b[1] + op[2]), op[3], self.labels_ptr(op[3]), st)
            env.sync()
            self.check_labels(op[3], exp["labels"], "labels_from_tables")
        elif name == "assign":
            n = op[4]
            o.assign_accumulate(self.ptr(op[2], op[3]), n, self.labels_ptr(n) if op[5] else 0, acc if op[6] else 0, st)
            env.sync()
            if op[5]:
                self.check_labels(n, exp["labels"])
        elif name == "partials":
            n = op[4]
            o.assign_partials(self.ptr(op[2], op[3]), n, self.labels_ptr(n) if op[5] else 0, st)
            o.reduce_partials(n, acc, st)
            env.sync()
            if op[5]:
                self.check_labels(n, exp["labels"])
        elif name == "assign_update":
            n = op[4]
            o.assign_update(self.ptr(op[2], op[3]), n, self.labels_ptr(n) if op[5] else 0, acc, bool(op[6]), st)
            env.sync()
            if op[5]:
                self.check_labels(n, exp["labels"])
        elif name == "iterate":
            n, want_l, reps, update_first, flush = op[4:9]
            p = self.ptr(op[2], op[3])
            if flush == 2:
                C["iterate_left_in_flight"] += 1
                self.arm(self.lab2, 4 * n)
                for _ in range(reps):
                    o.iterate(p, n, self.lab2.ptr, acc, bool(update_first), st)
                self.pending = (n, exp["labels"])
                return                               # nothing is read, nothing waits: the next op finds the device busy
            lp = self.labels_ptr(n)
            for _ in range(reps):
                o.iterate(p, n, lp if want_l else 0, acc, bool(update_first), st)
            if flush:
                o.flush(st)
            else:                                # the tables the LAST iteration wrote, gathered by a label pass of its own
                o.labels(p, n, lp, st)
            env.sync()
            if want_l or not flush:
                self.check_labels(n, exp["labels"], "labels after iterate")
        elif name == "run":
            n = op[4]
            it = o.run(self.ptr(op[2], op[3]), n, self.labels_ptr(n) if op[5] else 0, st)
            if it != exp["iterations"]:
                self.fail(f"run stopped at iteration {it}, the oracle at {exp['iterations']}")
            if op[5]:
                self.check_labels(n, exp["labels"], "labels of run")
        elif name == "share_round":
            parts, fused, b_off, b_n, leave = op[2:7]
            buf, off, n = s.bind[:3]
            C[f"share_parts:{parts}"] += 1
            C["share_fused" if fused else "share_plain"] += 1
            p = self.ptr(buf, off)
            k = s.k
            if fused:
                self.mem.write(self.acc[L], 0, np.zeros(32 * k, np.uint8))
            total = np.zeros((k, 4), np.int64)
            for part in range(parts):
                o.set_cell_share(part, parts, st)
                (o.accumulate_into if fused else o.assign_accumulate)(*((p, n, acc, st) if fused else (p, n, 0, acc, st)))
                env.sync()
                got = self.collect(self.acc[L], 32 * k, np.int64, "share sums").reshape(k, 4)
                want = total + exp["part_sums"][part] if fused else exp["part_sums"][part]
                if not np.array_equal(got, want):
                    self.fail(f"sums of share {part} of {parts}", got, want)
                total = total + exp["part_sums"][part]
            pb = self.ptr(buf, off + b_off)
            if fused:
                o.labels_from_tables_update(pb, b_n, self.labels_ptr(b_n), acc, st)
            else:
                o.labels_from_tables(pb, b_n, self.labels_ptr(b_n), st)
            env.sync()
            self.check_labels(b_n, exp["labels"], "labels from the shares' tables")
            if not (leave and parts > 1):
                o.set_cell_share(0, 1, st)
        elif name == "refuse":
            what = op[2]
            C["refusal:" + what] += 1
            n = s.bind[2] if s.bind is not None else 1000
            p = self.ptr(*s.bind[:2]) if s.bind is not None else self.ptr(0, 0)
            lp = self.labels_ptr(n)
            call = {"run": (o.run, p, n, lp, st), "iterate": (o.iterate, p, n, lp, acc, True, st),
                    "assign_update": (o.assign_update, p, n, 0, acc, True, st), "labelmap": (o.assign_accumulate, p, n, lp, acc, st),
                    "partials": (o.assign_partials, p, n, 0, st), "lftu_bigk": (o.labels_from_tables_update, p, n, lp, acc, st),
                    "unbound_lft": (o.labels_from_tables, p, n, lp, st), "unbound_into": (o.accumulate_into, p, n, acc, st),
                    "unbound_share": (o.set_cell_share, 0, 2, st), "unbound_rebuild": (o.rebuild_from_histogram, n, st),
                    "share_bad": (o.set_cell_share, *pick_bad(op), st)}[what]
            self.expect_status(exp["status"], *call)
            env.sync()
            got = self.collect(self.lab, 4 * n, np.uint8, "refused call")
            if not (got == PATTERN).all():
                self.fail("a refused call wrote labels")
        else:
            raise ValueError(op)
        env.sync()
        self.check_slot(L, exp, st)

    # -- neighbours on the same processor: they trade blocks with the Lloyd objects
    def expected_apply(self, img, cent, mode):
        key = ("apply", img.tobytes(), cent.tobytes(), mode)
        c = self.model.cache
        if key not in c:
            c[key] = diffuse_ref.diffuse(img, diffuse_ref.oracle_apply_replace(O, cent)) if mode == 3 else O.apply(img, cent, mode)
        return c[key]

    def step_apply(self, op):
        _, buf, mode, fmt, k, seed, plan, st = op
        env, m = self.env, self.model
        C = self.counters
        C[f"apply_mode:{mode}"] += 1
        C[f"apply_format:{fmt}"] += 1
        C["apply_plan" if plan else "apply_whole"] += 1
        img = self.images[m.bufs[buf]][1]
        h, w = img.shape[:2]
        cent, _ = gamut_centroids(seed, k)
        size = {None: 4, 1: 1, 2: 2}[fmt]
        self.arm(self.out, size * w * h)
        p = self.ptr(buf, 0)
        if plan and h > 1:
            r = 1 + seed % (h - 1)
            pl = self.proc.apply_plan(cent, mode, w * h, env.streams[st], format=fmt)
            try:
                pl.run(p, w, r, 0, self.out.ptr, env.streams[st])
                pl.run(p + 4 * r * w, w, h - r, r, self.out.ptr + size * r * w, env.streams[1 - st])
                env.sync()
                pl.status()
            finally:
                pl.close()
        else:
            self.proc.apply(p, w, h, 0, cent, mode, self.out.ptr, env.streams[st], format=fmt)
        env.sync()
        want = self.expected_apply(img, cent, mode)
        if fmt is None:
            got = self.collect(self.out, 4 * w * h, np.uint8, "apply").reshape(h, w, 4)
            if not np.array_equal(got, want):
                self.fail(f"output bytes of mode {mode}", got, want)
            return
        idx = self.collect(self.out, size * w * h, np.uint8 if fmt == 1 else np.uint16, "indexed apply").astype(np.int64)
        if idx.max() >= k:
            self.fail(f"index {int(idx.max())} >= k = {k}")
        P = O.lab_to_rgba8(cent[:, :3])
        if not np.array_equal(P[idx].reshape(h, w, 4)[..., :3], want[..., :3]):
            self.fail(f"P[index] of mode {mode}", P[idx].reshape(h, w, 4)[..., :3], want[..., :3])
        if mode == 0 and not np.array_equal(idx, O.assign(O.rgb_to_lab(img.reshape(-1, 4)), cent)):
            self.fail("replace indices are not the oracle's labels")

    def step_host(self, op):
        _, kind, img_i, k, mode, seed = op
        self.counters["host:" + kind] += 1
        img = self.images[img_i][1]
        h, w = img.shape[:2]
        c = self.model.cache
        if kind == "find":
            _, pal = gamut_centroids(seed, k)
            got = self.proc.find(img, pal, mode)
            if op not in c:
                c[op] = diffuse_ref.diffuse(img, diffuse_ref.oracle_find_replace(O, pal)) if mode == 3 else O.find(img, pal, mode)
            want = c[op]
        else:
            if ("kmeans", img_i, k) not in c:
                lab = O.rgb_to_lab(img.reshape(-1, 4))
                c[("kmeans", img_i, k)] = O.lloyd(lab, O.init_centroids(lab, w, h, k), MAX_ITERATIONS, CHECK_PERIOD)[0]
            cent = c[("kmeans", img_i, k)]
            if kind == "reduce":
                got = self.proc.reduce(k, img, 0, mode)
                want = self.expected_apply(img, cent, mode)
            else:
                got = np.asarray(self.proc.palette(k, img, 0)).reshape(-1, 4)
                want = sorted_palette(cent)
        if not np.array_equal(np.asarray(got).reshape(want.shape), want):
            self.fail(f"host {kind} (k = {k}, mode {mode})", np.asarray(got).reshape(want.shape), want)


def sorted_palette(cent):
    """kmg_palette's result for a centroid table (lib.rs:255-286): the palette crate's sRGB8 of every centroid, sorted -- stably --
    by the L of THAT colour converted back to Lab"""
    rgb = [O.palette_lab_to_srgb8(c[:3]) for c in cent]
    L = np.array([O.palette_srgb8_to_lab(c)[0] for c in rgb], np.float32)
    return np.array([list(rgb[i]) + [255] for i in np.argsort(L, kind="stable")], np.uint8)


def pick_bad(op):
    """(part, parts) of a refused set_cell_share: part >= parts, or no parts at all"""
    return (3, 3) if op[-1] else (0, 0)


def run_sequence(env, seed, seq, ops=None, counters=None, proc=None, cache=None):
    """one sequence on a fresh processor (or the caller's): (ops run, blocks allocated, blocks re-used); raises Mismatch with the
    replay text"""
    ops = generate(seed, seq) if ops is None else ops
    r = Runner(env, seed, seq, counters, proc, cache)
    try:
        r.run(ops)
        blocks = r.proc.debug_block_counts()
    except Mismatch as e:
        raise Mismatch(f"seed {seed} sequence {seq}: {e}\nreplay(env, {seed}, {seq}, {ops[:r.n_ops + 1]!r})") from None
    finally:
        r.close()
    return r.n_ops, blocks[0], blocks[1]


def replay(env, seed, seq, ops, proc=None):
    """runs a printed op list again: the images are those of (seed, seq)"""
    return run_sequence(env, seed, seq, ops, proc=proc)


# ---- the real binding -----------------------------------------------------------------------------------------------
class _TorchMem:
    def __init__(self, torch):
        self.torch = torch

    def alloc(self, nbytes):
        t = self.torch.zeros(int(nbytes), dtype=self.torch.uint8, device="cuda")
        t.ptr = t.data_ptr()
        return t

    def write(self, buf, off, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf[off:off + a.size].copy_(self.torch.from_numpy(a))
        self.torch.cuda.synchronize()

    def fill(self, buf, off, nbytes, byte):
        buf[off:off + nbytes].fill_(byte)
        self.torch.cuda.synchronize()

    def read(self, buf, off, nbytes):
        self.torch.cuda.synchronize()
        return buf[off:off + nbytes].cpu().numpy()


class KgEnv:
    """kmeans_gpu_amd on cuda:0: two streams, torch tensors for device memory"""

    def __init__(self):
        import torch
        import kmeans_gpu_amd as kg
        self.torch, self.kg = torch, kg
        self.Error = kg.KmgError
        self.mem = _TorchMem(torch)
        self._streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        self.streams = [s.cuda_stream for s in self._streams]

    def sync(self):
        self.torch.cuda.synchronize()

    def processor(self):
        return self.kg.ImageProcessor(shrink_max_dim=0, max_iterations=MAX_ITERATIONS, check_period=CHECK_PERIOD, strategy="auto")

    def lloyd(self, proc, k):
        return self.kg.Lloyd(proc, k)
