"""TEST HARNESS: model-based random call sequences on the multi-device layer (kmg_group_*, kmg_group_lloyd_*), in the style of
tests/lifecycle_harness.py, whose images, centroid tables and oracle helpers it uses (tests/test_group_model.py on the CPU,
tools/fuzz_group_lifecycle.py and tests/test_gpu_group_lifecycle.py on the device).

Every call of the group layer is a pure function of (the WHOLE image, the current centroids, the flags of the binding and whether
the world has collectives): the bands, their owners, the number of ranks and the strategy never show in a result.  So a stateless
model over tests/oracle_lib.py -- never the single-device library -- predicts every label map, every rank's centroid table, every
iteration count and every host output of any legal sequence, and the status of the refused calls.  What a sequence exercises is
the STATE: one kmg_group_lloyd bound again and again (other images, other bands, other flags), ranks without rows, two objects and
the host calls sharing each rank's processor, block pool and stream, a batch whose images stop at different checks.

  generate(seed, seq)      -> list of plain tuples; the first one names the world (sequence seq runs in world seq % 5)
  GRunner(env).run(ops)    -> executes them, checks EVERYTHING after every op, raises Mismatch at the first difference
  replay(env, seed, seq, ops), scenarios() (the hand-written op lists), coverage(ops) (what the CPU test counts)

Worlds, all in one process on device 0: "rccl1" one rank with KMG_GROUP_FORCE_COLLECTIVES (real RCCL), "solo" one rank without
collectives (the fused_update path), "lb2" / "lb3" / "lb5" ranks sharing the device through KMG_GROUP_LOOPBACK.  A world's group
is created once (env.group) and reused by every sequence and scenario of the process.

An image of a binding is a WINDOW (buffer, first pixel, width, height) of a device pixel buffer -- any readable pixels make an
image -- so widths are mostly odd and bands start off 16-byte alignment.  A band's label map has GUARD bytes behind it and the
whole label buffer is filled with PATTERN before every call that writes one; a band bound without a label map must stay PATTERN.

The (flags, world) table of KMG_GROUP_FUSED_UPDATE in include/kmeans_hip.h is fused_form() below.

What the generator never emits, because include/kmeans_hip.h leaves it open: _step without a _prime / _step since the last
_bind, _init, _run or _run_batch (the sums of a batch image that stopped early are not defined); any call but _bind / _destroy on
an object whose bound pixels were overwritten; a pass before every image has centroids; bands that overlap or leave rows out;
multi-process worlds and the BROKEN state (nothing here may make a rank fail)."""
import collections

import numpy as np

import oracle_lib as O
import lifecycle_harness as H
from lifecycle_harness import Mismatch, GUARD, PATTERN, MAX_ITERATIONS, CHECK_PERIOD, NI, IMAGE_KINDS, K_CLASSES, ERR_INVALID, k_class

FORCE, LOOPBACK = 1, 2                                    # kmg_group_options.flags
CELLS, OVERLAP, FUSED = 1, 2, 4                           # kmg_group_lloyd_bind flags
World = collections.namedtuple("World", "name ranks flags shrink")
WORLDS = (World("rccl1", 1, FORCE, 0), World("solo", 1, 0, 256), World("lb2", 2, LOOPBACK, 0), World("lb3", 3, LOOPBACK, 0),
          World("lb5", 5, LOOPBACK, 256))
WORLD = {w.name: w for w in WORLDS}
CAPS = (1 << 20, 300000)                                  # pixels of the two device pixel buffers
LABEL_BYTES = 4 * (1 << 20) + 4 * 4 * 100000 + 64 * GUARD  # one label buffer per object: every band's map + its guard
BATCH_PIXELS = 100000                                     # largest image of a batch
REFUSALS = ("run_fused", "run_on_batch", "run_batch_fused", "cells_batch", "unbound", "band_leaves", "rows_no_pixels", "k0", "diffuse",
            "alpha", "index", "fused_cells_rowless", "fused_cells_nolabels", "fused_cells_onelabel", "fused_cells_bigk")
MEGA, LARGE, FEW, FLAT, TOKYO, NOISE, BLOBS = (IMAGE_KINDS.index(k) for k in ("mega", "large", "few", "flat", "tokyo", "noise", "blobs"))


def collectives(world):
    return world.ranks > 1 or bool(world.flags & FORCE)


def fused_form(world, flags, k):
    """True: _prime + n x _step = n + 1 updates and the label maps describe the assignment BEFORE the last update; False: the
    plain loop, n updates, label maps of the assignment AFTER the last update.  (FUSED | CELLS with collectives and k > 256 is
    refused by _bind; FUSED alone with collectives is ignored; CELLS needs collectives and k <= 256, else it is ignored)"""
    if not flags & FUSED:
        return False
    if not collectives(world):
        return True
    return bool(flags & CELLS) and k <= 256


def cells_form(world, flags, k):
    return bool(flags & CELLS) and k <= 256 and collectives(world)


def pixel_limit(k):
    return 5000 if k > 512 else 70000 if k > 256 else 300000 if k > 32 else 1 << 20


# ---- the model ------------------------------------------------------------------------------------------------------
class GSlot:
    def __init__(self, k, n_images):
        self.k, self.n_images = k, n_images
        self.bound = None                  # (problems, layouts, labels, flags)
        self.stale = False                 # pixels of a bound buffer were overwritten: bind again
        self.cent = [None] * n_images      # numeric: (k, 4) float32; dry: True
        self.acc = [None] * n_images       # the image's sums of the last assignment
        self.primed = False
        self.prepared, self.strategy_seen = False, 0      # the strategy in force when the bands were last prepared


class GModel:
    def __init__(self, images, numeric, cache=None):
        self.images, self.numeric = images, numeric
        self.world = None
        self.slots = [None, None]
        self.bufs = [None, None]
        self.strategy = 0
        self.cache = {} if cache is None else cache

    def n_buf(self, buf):
        h, w = self.images[self.bufs[buf]][1].shape[:2]
        return w * h

    def px(self, prob):
        buf, off, w, h = prob
        return self.images[self.bufs[buf]][1].reshape(-1, 4)[off:off + w * h]

    def lab(self, prob):
        key = ("lab", self.bufs[prob[0]]) + tuple(prob[1:])
        if key not in self.cache:
            self.cache[key] = O.rgb_to_lab(self.px(prob))
        return self.cache[key]

    def assign(self, prob, cent):
        key = ("as", self.bufs[prob[0]]) + tuple(prob[1:]) + (cent.tobytes(),)
        if key not in self.cache:
            labels = O.assign(self.lab(prob), cent)
            self.cache[key] = (labels, O.accumulate(self.lab(prob), labels, cent.shape[0]))
        return self.cache[key]

    def ready(self, s):
        return s is not None and s.bound is not None and not s.stale and all(c is not None for c in s.cent)


def host_centroids(m, img_i, k):
    """the k-means of a host call on image img_i: shrunk to the world's shrink_max_dim first (0: full resolution, sharded or not)"""
    key = ("kmeans", img_i, k, m.world.shrink)
    if key not in m.cache:
        img = m.images[img_i][1]
        h, w = img.shape[:2]
        s = m.world.shrink
        if s and (w > s or h > s):
            img = O.resize(img, *O.resized_dims(w, h, s))
            h, w = img.shape[:2]
        lab = O.rgb_to_lab(img.reshape(-1, 4))
        m.cache[key] = O.lloyd(lab, O.init_centroids(lab, w, h, k), MAX_ITERATIONS, CHECK_PERIOD)[0]
    return m.cache[key]


def host_expected(m, kind, img_i, k, mode, algo, seed):
    key = ("host", kind, img_i, k, mode, algo, seed, m.world.shrink)
    if key not in m.cache:
        img = m.images[img_i][1]
        if kind == "find":
            want = O.find(img, H.gamut_centroids(seed, k)[1], mode)
        elif algo == 1:
            want = O.reduce_octree(img, k, mode) if kind == "reduce" else O.palette_octree(img, k)
        elif kind == "reduce":
            want = O.apply(img, host_centroids(m, img_i, k), mode)
        else:
            want = H.sorted_palette(host_centroids(m, img_i, k))
        m.cache[key] = want
    return m.cache[key]


def apply_op(m, op):
    """advances the model by `op` (legality always, numbers when numeric); returns what the runner compares"""
    name, num, exp = op[0], m.numeric, {}
    if name == "world":
        m.world = WORLD[op[1]]
        return exp
    if name == "upload":
        m.bufs[op[1]] = op[2]
        for s in m.slots:
            if s is not None and s.bound is not None and any(p[0] == op[1] for p in s.bound[0]):
                s.stale, s.primed = True, False
        return exp
    if name == "strategy":
        m.strategy = op[1]
        return exp
    if name == "host":
        if num:
            exp["out"] = host_expected(m, *op[1:])
        return exp
    if name == "reduce_batch":
        if num:
            exp["outs"] = [host_expected(m, "reduce", i, op[2], op[3], op[4], 0) for i in op[1]]
        return exp
    if name == "single":
        _, rank, buf, off, n, k, seed = op
        if num:
            cent = H.make_centroids("rand", seed, k)
            exp["cent"] = cent
            exp["labels"], exp["sums"] = m.assign((buf, off, n, 1), cent)
        return exp
    if name == "refuse":
        exp["status"] = ERR_INVALID
        what, L = op[1], op[2]
        s = m.slots[L] if L is not None else None
        if what in ("run_fused", "run_batch_fused"):
            assert s.bound is not None and s.bound[3] & FUSED and (s.n_images == 1) == (what == "run_fused")
        elif what in ("run_on_batch", "cells_batch"):
            assert s.n_images > 1 and (what == "cells_batch" or s.bound is not None)
        elif what.startswith("fused_cells"):
            assert s.n_images == 1 and collectives(m.world) and (s.k > 256) == (what == "fused_cells_bigk")
            assert what != "fused_cells_rowless" or m.world.ranks > 1
        elif what in ("band_leaves", "rows_no_pixels", "index"):
            assert s is not None
        return exp
    L = op[1]
    if name == "create":
        assert m.slots[L] is None
        m.slots[L] = GSlot(op[2], op[3])
        return exp
    s = m.slots[L]
    assert s is not None, op
    if name == "destroy":
        m.slots[L] = None
        return exp
    if name == "bind":
        problems, layouts, labels, flags = op[2:6]
        assert len(problems) == s.n_images and not (flags & CELLS and s.n_images > 1)
        for (buf, off, w, h), lay in zip(problems, layouts):
            assert off + w * h <= m.n_buf(buf) and len(lay) == m.world.ranks
            rows = sorted((r0, r) for r0, r in lay if r)
            assert sum(r for _, r in rows) == h and all(a + b == c for (a, b), (c, _) in zip(rows, rows[1:] + [(h, 0)])) and rows[0][0] == 0
        if flags & FUSED and flags & CELLS and collectives(m.world):
            assert s.k <= 256 and labels is not None and all(r and l for (_, r), l in zip(layouts[0], labels[0])), op
        s.bound, s.stale, s.primed, s.prepared = (problems, layouts, labels, flags), False, False, False
        return exp
    assert s.bound is not None and not s.stale, op
    problems, layouts, labels, flags = s.bound
    fused = fused_form(m.world, flags, s.k)
    if name == "init":
        for im, (buf, off, w, h) in enumerate(problems):
            s.cent[im] = O.init_centroids(m.lab(problems[im]), w, h, s.k) if num else True
        s.primed = s.prepared = False
        return exp
    if name == "set_cent":
        _, _, im, kind, seed, img_i = op
        s.cent[im or 0] = H.make_centroids(kind, seed, s.k, m.images[img_i][1]) if num else True
        return exp
    if name in ("get", "sync"):
        return exp
    if name == "member":
        assert s.primed
        r0_rows = layouts[0][0][1]
        if cells_form(m.world, flags, s.k):
            exp["strategy"] = "table"
        elif not r0_rows:
            exp["strategy"] = "scan"
        elif s.strategy_seen in (1, 2):
            exp["strategy"] = "scan" if s.strategy_seen == 1 else "table"
        return exp
    assert m.ready(s), op
    if not s.prepared:
        s.prepared, s.strategy_seen = True, m.strategy

    def one_pass(update_first, update_after):
        out = []
        for im in range(s.n_images):
            if num:
                if update_first:
                    s.cent[im] = O.finalize(s.acc[im], s.cent[im])[0]
                lab_map, s.acc[im] = m.assign(problems[im], s.cent[im])
                if update_after:
                    s.cent[im] = O.finalize(s.acc[im], s.cent[im])[0]
                out.append(lab_map)
        return out

    if name == "prime":
        exp["labels"] = one_pass(False, fused)
        s.primed = True
        return exp
    if name == "step":
        assert s.primed
        for _ in range(op[2]):
            exp["labels"] = one_pass(not fused, fused)
        return exp
    if name in ("run", "run_batch"):
        assert not flags & FUSED and (name == "run_batch" or s.n_images == 1)
        if num:
            exp["labels"], exp["iterations"] = [], []
            for im in range(s.n_images):
                s.cent[im], lab_map, it = O.lloyd(m.lab(problems[im]), s.cent[im], MAX_ITERATIONS, CHECK_PERIOD)
                exp["labels"].append(lab_map)
                exp["iterations"].append(it)
        s.primed = False
        return exp
    raise ValueError(op)


# ---- the generator --------------------------------------------------------------------------------------------------
def make_layout(rng, ranks, h, kind=None, permute=None):
    """one band (row0, rows) per rank: the bands tile rows [0, h) in any owner order; a rank may have none"""
    kind = kind or ("even", "cuts", "rowless", "one_row", "last_all")[int(rng.choice(5, p=[0.25, 0.3, 0.2, 0.15, 0.1]))]
    if ranks == 1:
        return ((0, h),)
    if kind == "even":
        sizes = [(i + 1) * h // ranks - i * h // ranks for i in range(ranks)]
    elif kind == "cuts":
        cuts = [0] + sorted(int(c) for c in rng.integers(0, h + 1, ranks - 1)) + [h]
        sizes = [b - a for a, b in zip(cuts, cuts[1:])]
    elif kind == "rowless":
        nz = int(rng.integers(1, min(ranks - 1, h) + 1))
        cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, h), nz - 1, replace=False)) + [h] if nz > 1 else [0, h]
        sizes = [b - a for a, b in zip(cuts, cuts[1:])] + [0] * (ranks - nz)
        sizes = [sizes[i] for i in rng.permutation(ranks)]
    elif kind == "one_row" and h >= ranks:
        sizes = [1] * (ranks - 1) + [h - (ranks - 1)]
        sizes = [sizes[i] for i in rng.permutation(ranks)]
    else:
        sizes = [0] * (ranks - 1) + [h]
    owners = list(range(ranks))
    if permute if permute is not None else rng.random() < 0.4:
        owners = [int(i) for i in rng.permutation(ranks)]
    lay, row = [None] * ranks, 0
    for seg, size in enumerate(sizes):
        lay[owners[seg]] = (row, size)
        row += size
    return tuple(lay)


def is_permuted(lay):
    r0 = [a for a, r in lay if r]
    return r0 != sorted(r0)


def generate(seed, seq, n_ops=64):
    rng = np.random.default_rng([seed, seq, 31])
    world = WORLDS[seq % len(WORLDS)]
    images = H.make_images(seed, seq)
    m = GModel(images, numeric=False)
    ops, pending = [], []
    n_refused = [0]

    def emit(op):
        ops.append(op)
        apply_op(m, op)

    def rint(a, b):
        return int(rng.integers(a, b))

    def pick(xs, p=None):
        return xs[int(rng.choice(len(xs), p=p))]

    def pick_k():
        lo, hi = K_CLASSES[pick([0, 1, 2, 3, 4], [0.1, 0.4, 0.3, 0.12, 0.08])]
        return pick([lo, hi]) if rng.random() < 0.3 else rint(lo, hi + 1)

    def window(k, cap):
        """(buf, off, w, h): a whole image or a window of a buffer's pixels with at most min(cap, pixel_limit(k)) pixels"""
        cap = min(cap, pixel_limit(k))
        buf = rint(0, 2)
        n = m.n_buf(buf)
        h, w = images[m.bufs[buf]][1].shape[:2]
        if w * h <= cap and rng.random() < 0.45:
            return (buf, 0, w, h)
        c = rng.random()
        if c < 0.12:                                            # fewer rows than ranks
            hh = rint(1, 4)
            ww = rint(17, min(900, cap // hh, n // hh) + 1)
        else:
            ww = rint(17, 700) | 1
            ww = min(ww, n)
            hh = rint(1, max(min(cap, n) // ww, 1) + 1)
            if c < 0.5:
                hh = min(hh, rint(4, 200))
        off = rint(0, n - ww * hh + 1)
        return (buf, off, ww, hh)

    def flags_for(s, layouts, labels):
        if s.n_images > 1:
            return pick([0, OVERLAP, FUSED, OVERLAP | FUSED], [0.45, 0.2, 0.25, 0.1])
        fl = pick([0, CELLS, OVERLAP, FUSED, CELLS | FUSED, CELLS | OVERLAP, OVERLAP | FUSED, 7], [0.2, 0.25, 0.1, 0.12, 0.18, 0.05, 0.05, 0.05])
        if s.bound is not None and rng.random() < 0.5:            # a flag change on the live object, in either direction
            fl = (s.bound[3] ^ CELLS) & ~FUSED | (fl & FUSED)
        if fl & FUSED and fl & CELLS and collectives(world):
            ok = s.k <= 256 and labels is not None and all(r and l for (_, r), l in zip(layouts[0], labels[0]))
            if not ok:
                fl &= ~FUSED
        return fl

    def bind(L, same_problems=False):
        s = m.slots[L]
        cap = BATCH_PIXELS if s.n_images > 1 else 1 << 20
        problems = s.bound[0] if same_problems else tuple(window(s.k, cap) for _ in range(s.n_images))
        want_fused_cells = s.n_images == 1 and s.k <= 256 and collectives(world) and rng.random() < 0.2
        layouts, labels = [], []
        for p in problems:
            if want_fused_cells and p[3] >= world.ranks:
                layouts.append(make_layout(rng, world.ranks, p[3], pick(["even", "cuts", "one_row"])))
                if any(r == 0 for _, r in layouts[-1]):
                    layouts[-1] = make_layout(rng, world.ranks, p[3], "even")
            else:
                layouts.append(make_layout(rng, world.ranks, p[3]))
        c = rng.random()
        if want_fused_cells or c < 0.6:
            labels = tuple(tuple(1 for _ in lay) for lay in layouts)
        elif c < 0.8:
            labels = None
        else:
            labels = tuple(tuple(int(rng.random() < 0.6) for _ in lay) for lay in layouts)
        layouts = tuple(layouts)
        emit(("bind", L, problems, layouts, labels, flags_for(s, layouts, labels)))
        if rng.random() < 0.6:                                    # the new binding is used: a pass, and an update from its sums
            pending.extend([("prime", L), ("step", L, rint(1, 3))])

    def centroids(L):
        s = m.slots[L]
        if rng.random() < 0.5:
            emit(("init", L))
        else:
            for im in range(s.n_images):
                emit(("set_cent", L, im if s.n_images > 1 else None, pick(["init", "rand", "dup", "far"], [0.3, 0.4, 0.15, 0.15]), rint(0, 1 << 30),
                      pick([1, 3, 4, 5, 6]) if s.k <= 300 else 6))

    def probe(L=None):
        """the correct pass after a refusal, on the same group (and the same object where it can run one)"""
        s = m.slots[L] if L is not None else None
        if m.ready(s):
            emit(("prime", L))
        else:
            emit(("host", "find", pick([1, 4, 6]), rint(1, 17), rint(0, 3), 0, rint(0, 1 << 30)))

    def refusal():
        live = [i for i, s in enumerate(m.slots) if s is not None]
        cands = [("k0", None), ("diffuse", None), ("alpha", None), ("unbound", None)]
        for L in live:
            s = m.slots[L]
            cands += [("band_leaves", L), ("rows_no_pixels", L), ("index", L)]
            if s.n_images > 1:
                cands += [("cells_batch", L)] * 2
                if s.bound is not None:
                    cands += [("run_on_batch", L)] * 2
                    if s.bound[3] & FUSED:
                        cands += [("run_batch_fused", L)] * 3
            else:
                if s.bound is not None and s.bound[3] & FUSED:
                    cands += [("run_fused", L)] * 3
                if collectives(world):
                    if s.k > 256:
                        cands += [("fused_cells_bigk", L)] * 3
                    else:
                        cands += [("fused_cells_nolabels", L), ("fused_cells_onelabel", L)] * 2
                        if world.ranks > 1:
                            cands += [("fused_cells_rowless", L)] * 3
        what, L = pick(cands)
        emit(("refuse", what, L, rint(0, 1 << 16)))
        n_refused[0] += 1
        probe(L)

    emit(("world", world.name))
    emit(("upload", 0, pick([MEGA, LARGE, rint(0, 6)], [0.3, 0.4, 0.3])))
    emit(("upload", 1, pick([LARGE, rint(0, 7)], [0.3, 0.7])))
    emit(("strategy", pick([2, 2, 0, 1])))
    while len(ops) < n_ops:
        if pending:
            op = pending.pop(0)
            s = m.slots[op[1]]
            if s is not None and m.ready(s) and (op[0] != "step" or s.primed) and (op[0] != "run_batch" or not s.bound[3] & FUSED):
                emit(op)
            continue
        r = rng.random()
        live = [i for i, s in enumerate(m.slots) if s is not None]
        if not live or (len(live) < 2 and r < 0.12):
            L = [i for i in range(2) if m.slots[i] is None][0]
            k = pick_k()
            emit(("create", L, k, 1 if rng.random() < 0.55 or k > 512 else rint(2, 5)))
            bind(L)
            centroids(L)
            continue
        L = pick(live)
        s = m.slots[L]
        if r < 0.05:
            emit(("destroy", L))
            continue
        if r < 0.12:                                              # pixels: another image, or the next frame into the same buffer
            buf = rint(0, 2)
            nxt = rng.random() < 0.5
            img = (m.bufs[buf] + NI) % (2 * NI) if nxt else pick([MEGA, LARGE, rint(0, 7)]) if buf == 0 else rint(0, 7)
            emit(("upload", buf, img))
            for i in live:
                if m.slots[i].stale:
                    bind(i, same_problems=nxt and rng.random() < 0.7)
                    if rng.random() < 0.4:
                        emit(("init", i))
            continue
        if r < 0.16:
            emit(("strategy", pick([0, 1, 2], [0.25, 0.25, 0.5])))
            continue
        if r < 0.28:                                              # neighbours on the same group
            c = rng.random()
            if c < 0.6:
                kind = pick(["find", "reduce", "palette"])
                img = pick([0, 1, 3, 4, 5, 6, MEGA], [0.15, 0.15, 0.15, 0.1, 0.15, 0.15, 0.15])
                k = rint(1, 9) if img == MEGA else rint(1, 40)
                emit(("host", kind, img, k, rint(0, 3), int(rng.random() < 0.3), rint(0, 1 << 30)))
            elif c < 0.8:
                emit(("reduce_batch", tuple(pick([0, 1, 3, 4, 5, 6]) for _ in range(rint(1, 5))), rint(1, 24), rint(0, 3), int(rng.random() < 0.25)))
            else:
                k = rint(1, 65)
                buf = rint(0, 2)
                n = rint(1, min(m.n_buf(buf), 60000) + 1)
                emit(("single", rint(0, world.ranks), buf, rint(0, m.n_buf(buf) - n + 1), n, k, rint(0, 1 << 30)))
            continue
        if r < 0.38 and 4 * (n_refused[0] + 1) <= len(ops) // 2:   # (a refusal and its probe: at most a quarter of the ops refuse)
            refusal()
            continue
        if not m.ready(s):
            centroids(L)
            continue
        c = rng.random()
        flags = s.bound[3]
        if c < 0.16:
            bind(L, same_problems=rng.random() < 0.5)
        elif c < 0.22:
            emit(("init", L))
        elif c < 0.30:
            emit(("set_cent", L, rint(0, s.n_images) if s.n_images > 1 else None, pick(["rand", "dup", "far", "init"]), rint(0, 1 << 30),
                  pick([1, 3, 4, 5, 6]) if s.k <= 300 else 6))
        elif c < 0.34:
            emit(("get", L, rint(0, s.n_images)))
        elif c < 0.50 or (c < 0.7 and not s.primed):
            emit(("prime", L))
        elif c < 0.70:
            emit(("step", L, rint(1, 4)))
        elif c < 0.73:
            emit(("sync", L))
        elif c < 0.77 and s.primed:
            emit(("member", L))
        elif not flags & FUSED:
            if s.n_images > 1 or rng.random() < 0.15:
                emit(("run_batch", L))
                if s.n_images > 1 and rng.random() < 0.7:         # the loop again on the same object: `active` must be all-ones
                    im = rint(0, s.n_images)
                    pending.extend([("set_cent", L, im, "rand", rint(0, 1 << 30), 1), ("prime", L), ("step", L, rint(1, 3)), ("run_batch", L)])
            else:
                emit(("run", L))
        else:
            emit(("step", L, 1) if s.primed else ("prime", L))
    for L in range(2):
        if m.slots[L] is not None:
            emit(("destroy", L))
    return ops


def coverage(ops):
    """what the seed set must have produced (tests/test_group_model.py asserts on the sum over its sequences)"""
    C = collections.Counter()
    world, slots = None, {}
    for op in ops:
        C["ops"] += 1
        if op[0] == "world":
            world = WORLD[op[1]]
            C["world:" + op[1]] += 1
        elif op[0] == "create":
            C[f"kclass:{k_class(op[2])}"] += 1
            slots[op[1]] = [op[2], None, 0]
        elif op[0] == "destroy":
            slots.pop(op[1], None)
        elif op[0] == "refuse":
            C["refusals"] += 1
            C["refusal:" + op[1]] += 1
        elif op[0] == "bind":
            k, before, _ = slots[op[1]]
            layouts, labels, flags = op[3:6]
            cells = cells_form(world, flags, k)
            C["cells_rowless"] += cells and any(r == 0 for _, r in layouts[0])
            C["rowless"] += any(r == 0 for lay in layouts for _, r in lay)
            C["permuted"] += any(is_permuted(lay) for lay in layouts)
            C["labels_null"] += labels is None
            C["labels_some_null"] += labels is not None and any(not l for per in labels for l in per)
            C["odd_width"] += any(p[2] % 4 for p in op[2])
            C["one_row_band"] += any(r == 1 for lay in layouts for _, r in lay)
            C["fused_form"] += fused_form(world, flags, k)
            C[f"flags:{flags}"] += 1
            if before is not None:
                C["rebind"] += 1
                C["flags_to_cells"] += bool(flags & CELLS) and not before & CELLS
                C["flags_from_cells"] += bool(before & CELLS) and not flags & CELLS
            slots[op[1]][1] = flags
        elif op[0] == "run_batch":
            slots[op[1]][2] += 1
            C["batch_rerun"] += slots[op[1]][2] > 1
        C["op:" + op[0]] += 1
    return C


# ---- the runner -----------------------------------------------------------------------------------------------------
def _bits(c):
    return np.ascontiguousarray(c, np.float32).view(np.uint32)


class GRunner:
    """executes ops on a backend and compares with the numeric model after every op.  The backend `env` supplies mem, sync(),
    Error, group(world) (the surface of kmeans_gpu_amd.Group, one per world, kept), group_lloyd(group, k, n_images)
    (kmeans_gpu_amd.GroupLloyd), lloyd(proc, k) and bad_group(world) (a Group(...) call with alpha_cutoff = 7)"""

    def __init__(self, env, seed, seq, counters=None, cache=None):
        self.env, self.mem = env, env.mem
        self.images = H.make_images(seed, seq)
        self.model = GModel(self.images, numeric=True, cache=cache)
        self.counters = counters if counters is not None else collections.Counter()
        self.pix = [self.mem.alloc(4 * c) for c in CAPS]
        self.lab = [self.mem.alloc(LABEL_BYTES) for _ in range(2)]
        self.lab_used = [0, 0]
        self.bands = [None, None]              # per object: [(image, rank, byte offset, bytes, wanted)]
        self.scratch = self.mem.alloc(4 * 60000 + GUARD)
        self.acc = self.mem.alloc(32 * 64 + GUARD)
        self.obj = [None, None]
        self.group = None
        self.n_ops = 0

    def close(self):
        for o in self.obj:
            if o is not None:
                o.close()
        self.obj = [None, None]
        if self.group is not None:
            self.group.set_strategy(0)

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

    def run(self, ops):
        for i, op in enumerate(ops):
            try:
                self.step(op)
            except Mismatch as e:
                raise Mismatch(f"op {i} {op!r}: {e}") from None
            except self.env.Error as e:
                raise Mismatch(f"op {i} {op!r}: a legal call was refused: {e}") from None
            self.n_ops += 1

    def expect_status(self, status, fn, *args, **kw):
        try:
            fn(*args, **kw)
        except self.env.Error as e:
            if e.status != status:
                self.fail(f"refused with status {e.status}, the header names {status}")
            return
        self.fail(f"a call the header refuses with status {status} was accepted")

    # -- bands: pointers, label maps with a pattern in front and guard bytes behind
    def bind_args(self, L, problems, layouts, labels):
        px, row0, rows, lab, bands, off_b = [], [], [], [], [], 0
        for im, ((buf, off, w, h), lay) in enumerate(zip(problems, layouts)):
            px.append([]); row0.append([]); rows.append([]); lab.append([])
            for rank, (r0, r) in enumerate(lay):
                want = labels is not None and bool(labels[im][rank])
                px[-1].append(self.pix[buf].ptr + 4 * (off + r0 * w) if r or rank % 2 else 0)
                row0[-1].append(r0); rows[-1].append(r)
                lab[-1].append(self.lab[L].ptr + off_b if want else 0)
                bands.append((im, rank, off_b, 4 * r * w, want, r0 * w))
                off_b += 4 * r * w + GUARD
        assert off_b <= LABEL_BYTES, off_b
        return px, row0, rows, (lab if labels is not None else None), bands, off_b

    def arm(self, L):
        self.mem.fill(self.lab[L], 0, self.lab_used[L], PATTERN)

    def check_labels(self, L, want, what):
        """every band's label map against its rows of the image's, its guard, and the maps nobody asked for"""
        raw = self.mem.read(self.lab[L], 0, self.lab_used[L])
        for im, rank, off_b, nbytes, wanted, first in self.bands[L]:
            if not (raw[off_b + nbytes:off_b + nbytes + GUARD] == PATTERN).all():
                self.fail(f"{what}: image {im} rank {rank}: written past the end of the band's label map")
            got = raw[off_b:off_b + nbytes]
            if not wanted:
                if not (got == PATTERN).all():
                    self.fail(f"{what}: image {im} rank {rank}: a label map nobody bound was written")
                continue
            got = got.view(np.uint32)
            if not np.array_equal(got, want[im][first:first + nbytes // 4]):
                self.fail(f"{what}: label map of image {im}, rank {rank} (pixels from {first})", got, want[im][first:first + nbytes // 4])

    def check_centroids(self):
        """after every op: every image's table through the group call, and EVERY rank's table of image 0 through member(i)"""
        for L, s in enumerate(self.model.slots):
            if s is None:
                continue
            o = self.obj[L]
            for im in range(s.n_images):
                if s.cent[im] is None:
                    continue
                got = o.get_centroids(im if s.n_images > 1 else None)
                if not np.array_equal(_bits(got), _bits(s.cent[im])):
                    self.fail(f"centroid bits of object {L}, image {im}", _bits(got), _bits(s.cent[im]))
            if s.cent[0] is not None:
                for rank in range(self.model.world.ranks):
                    member, _ = o.member(rank)
                    got = member.get_centroids(self.group.stream(rank))
                    if not np.array_equal(_bits(got), _bits(s.cent[0])):
                        self.fail(f"centroid bits of object {L} on rank {rank} (kmg_group_lloyd_member)", _bits(got), _bits(s.cent[0]))

    def step(self, op):
        env, m, name, C = self.env, self.model, op[0], self.counters
        C["op:" + name] += 1
        if name == "world":
            apply_op(m, op)
            self.group = env.group(m.world)
            C["world:" + op[1]] += 1
            return
        if name == "upload":
            apply_op(m, op)
            env.sync()
            self.mem.write(self.pix[op[1]], 0, self.images[op[2]][1].reshape(-1))
            return
        if name == "strategy":
            apply_op(m, op)
            self.group.set_strategy(op[1])
            return
        if name == "host":
            exp = apply_op(m, op)
            _, kind, img_i, k, mode, algo, seed = op
            img = self.images[img_i][1]
            if kind == "find":
                got = self.group.find(img, H.gamut_centroids(seed, k)[1], mode)
            elif kind == "reduce":
                got = self.group.reduce(k, img, algo, mode)
            else:
                got = np.asarray(self.group.palette(k, img, algo)).reshape(-1, 4)
            if np.asarray(got).shape != exp["out"].shape or not np.array_equal(got, exp["out"]):
                self.fail(f"group {kind} (k = {k}, mode {mode}, algorithm {algo})", got, exp["out"])
            return self.check_centroids()
        if name == "reduce_batch":
            exp = apply_op(m, op)
            outs = self.group.reduce_batch(op[2], [self.images[i][1] for i in op[1]], op[4], op[3])
            for i, (got, want) in enumerate(zip(outs, exp["outs"])):
                if not np.array_equal(got, want):
                    self.fail(f"image {i} of reduce_batch", got, want)
            return self.check_centroids()
        if name == "single":
            exp = apply_op(m, op)
            _, rank, buf, off, n, k, seed = op
            proc, st = self.group.processor(rank), self.group.stream(rank)
            o = env.lloyd(proc, k)
            try:
                self.mem.fill(self.scratch, 0, 4 * n + GUARD, PATTERN)
                self.mem.fill(self.acc, 0, 32 * k + GUARD, PATTERN)
                o.set_centroids(exp["cent"], st)
                o.assign_accumulate(self.pix[buf].ptr + 4 * off, n, self.scratch.ptr, self.acc.ptr, st)
                env.sync()
            finally:
                o.close()
            raw = self.mem.read(self.scratch, 0, 4 * n + GUARD)
            acc = self.mem.read(self.acc, 0, 32 * k + GUARD)
            if not (raw[4 * n:] == PATTERN).all() or not (acc[32 * k:] == PATTERN).all():
                self.fail("single-device pass on a member processor: written past the end")
            if not np.array_equal(raw[:4 * n].view(np.uint32), exp["labels"]):
                self.fail("labels of a single-device pass on a member processor", raw[:4 * n].view(np.uint32), exp["labels"])
            if not np.array_equal(acc[:32 * k].view(np.int64).reshape(k, 4), exp["sums"]):
                self.fail("sums of a single-device pass on a member processor", acc[:32 * k].view(np.int64).reshape(k, 4), exp["sums"])
            return self.check_centroids()
        if name == "refuse":
            exp = apply_op(m, op)
            C["refusal:" + op[1]] += 1
            self.refuse(op, exp["status"])
            env.sync()
            return self.check_centroids()
        L = op[1]
        if name == "create":
            apply_op(m, op)
            C[f"kclass:{k_class(op[2])}"] += 1
            self.obj[L] = env.group_lloyd(self.group, op[2], op[3])
            return
        o = self.obj[L]
        if name == "destroy":
            apply_op(m, op)
            env.sync()
            o.close()
            self.obj[L] = None
            return
        exp = apply_op(m, op)
        s = m.slots[L]
        if name == "bind":
            problems, layouts, labels, flags = op[2:6]
            px, row0, rows, lab, self.bands[L], self.lab_used[L] = self.bind_args(L, problems, layouts, labels)
            C[f"flags:{flags}"] += 1
            if s.n_images == 1:
                o.bind(px[0], row0[0], rows[0], problems[0][2], problems[0][3], lab[0] if lab is not None else None, flags)
            else:
                o.bind_batch(px, row0, rows, [p[2] for p in problems], [p[3] for p in problems], lab, flags)
        elif name == "init":
            o.init()
        elif name == "set_cent":
            o.set_centroids(s.cent[op[2] or 0], op[2])
        elif name == "get":
            pass
        elif name == "sync":
            o.sync()
        elif name == "member":
            _, got = o.member(0)
            if got not in ("scan", "table") or ("strategy" in exp and got != exp["strategy"]):
                self.fail(f"member(0) reports {got!r} under strategy {m.strategy}, flags {s.bound[3]}")
        elif name in ("prime", "step", "run", "run_batch"):
            self.arm(L)
            if name == "prime":
                o.prime()
            elif name == "step":
                for _ in range(op[2]):
                    o.step()
            elif name == "run":
                it = [o.run()]
            else:
                it = list(o.run_batch())
            o.sync()
            env.sync()
            if name in ("run", "run_batch") and it != exp["iterations"]:
                self.fail(f"{name} stopped at iterations {it}, the oracle at {exp['iterations']}")
            self.check_labels(L, exp["labels"], name)
        else:
            raise ValueError(op)
        env.sync()
        self.check_centroids()

    def refuse(self, op, status):
        _, what, L, arg = op
        env, m, g = self.env, self.model, self.group
        s = m.slots[L] if L is not None else None
        o = self.obj[L] if L is not None else None
        ranks = m.world.ranks
        base = self.pix[0].ptr
        if what in ("run_fused", "run_on_batch"):
            self.expect_status(status, o.run)
        elif what == "run_batch_fused":
            self.expect_status(status, o.run_batch)
        elif what == "k0":
            self.expect_status(status, env.group_lloyd, g, 0, 1 + arg % 2)
        elif what == "alpha":
            self.expect_status(status, env.bad_group, m.world)
        elif what == "diffuse":
            img = self.images[FLAT][1]
            call = [(g.find, img, H.gamut_centroids(arg, 4)[1], 3), (g.reduce, 4, img, 0, 3), (g.reduce_batch, 4, [img, img], 0, 3)][arg % 3]
            self.expect_status(status, *call)
        elif what == "unbound":
            t = env.group_lloyd(g, 4, 1 + arg % 2)
            try:
                self.expect_status(status, [t.prime, t.step, t.init, t.sync, t.run_batch][arg % 5])
            finally:
                t.close()
        elif what == "index":
            if arg % 2:
                self.expect_status(status, o.get_centroids, s.n_images)
            else:
                self.expect_status(status, o.set_centroids, np.ones((s.k, 4), np.float32), s.n_images + arg % 3)
        else:
            # refused binds: the earlier binding of the object stays as it is
            w, h = 33, 2 * ranks + 1
            lay = [(i * 2, 2) for i in range(ranks - 1)] + [(2 * ranks - 2, 3)]
            px = [base + 4 * r0 * w for r0, _ in lay]
            lab = [self.lab[L].ptr + LABEL_BYTES - 4 * w * h + 4 * r0 * w for r0, _ in lay]     # (the end of the buffer: never written)
            flags = 0
            if what == "band_leaves":
                lay[-1] = (lay[-1][0], 4)
            elif what == "rows_no_pixels":
                px[arg % ranks] = 0
            elif what == "cells_batch":
                flags = CELLS
            else:
                flags = CELLS | FUSED
                if what == "fused_cells_rowless":
                    gone, row = arg % ranks, 0
                    owners = [i for i in range(ranks) if i != gone]
                    lay = [(0, 0)] * ranks
                    for j, i in enumerate(owners):
                        lay[i] = (row, 2 if j < len(owners) - 1 else h - row)
                        row += lay[i][1]
                    px = [base + 4 * r0 * w for r0, _ in lay]
                elif what == "fused_cells_nolabels":
                    lab = None
                elif what == "fused_cells_onelabel":
                    lab[arg % ranks] = 0
            r0s, rs = [a for a, _ in lay], [b for _, b in lay]
            if s.n_images == 1:
                self.expect_status(status, o.bind, px, r0s, rs, w, h, lab, flags)
            else:
                n = s.n_images
                self.expect_status(status, o.bind_batch, [px] * n, [r0s] * n, [rs] * n, [w] * n, [h] * n, [lab] * n if lab is not None else None, flags)


def run_sequence(env, seed, seq, ops=None, counters=None, cache=None):
    """one sequence on the world's long-lived group: (ops run, blocks allocated, blocks re-used) over its member processors"""
    ops = generate(seed, seq) if ops is None else ops
    r = GRunner(env, seed, seq, counters, cache)
    try:
        r.run(ops)
        blocks = [r.group.processor(i).debug_block_counts() for i in range(r.model.world.ranks)]
    except Mismatch as e:
        raise Mismatch(f"seed {seed} sequence {seq}: {e}\nreplay(env, {seed}, {seq}, {ops[:r.n_ops + 1]!r})") from None
    finally:
        r.close()
    return r.n_ops, sum(b[0] for b in blocks), max(b[1] for b in blocks)


def replay(env, seed, seq, ops):
    return run_sequence(env, seed, seq, ops)


# ---- the hand-written scenarios: (images of make_images(SCENARIO_SEED, 0)) ------------------------------------------
SCENARIO_SEED = 7


def scenarios():
    """name -> op list.  They run one after the other on the groups of one process, so each works in what the others left"""
    images = H.make_images(SCENARIO_SEED, 0)
    dims = lambda i: images[i][1].shape[1::-1]
    all_l = lambda lay: (tuple(1 for _ in lay),)
    S = {}
    w, h = dims(TOKYO)
    P = ((1, 0, w, h),)
    head = lambda world: [("world", world), ("upload", 0, MEGA), ("upload", 1, TOKYO), ("strategy", 2)]
    # CELLS with the middle rank of three rowless, then all rows on the last rank
    lay = ((0, 50), (0, 0), (50, h - 50))
    last = ((0, 0), (0, 0), (0, h))
    S["cells_middle_rank_rowless_then_all_rows_on_the_last"] = head("lb3") + [
        ("create", 0, 24, 1), ("bind", 0, P, (lay,), ((1, 0, 1),), CELLS), ("init", 0), ("prime", 0), ("step", 0, 2), ("member", 0), ("run", 0),
        ("bind", 0, P, (last,), all_l(last), CELLS), ("prime", 0), ("step", 0, 2), ("init", 0), ("run", 0),
        ("bind", 0, P, (last,), None, CELLS), ("set_cent", 0, None, "rand", 3, 0), ("prime", 0), ("step", 0, 1), ("destroy", 0)]
    # CELLS -> 0 -> CELLS | FUSED -> OVERLAP on one object and one buffer, without _init in between
    for world in ("rccl1", "lb2"):
        n = WORLD[world].ranks
        lay = tuple((i * h // n, (i + 1) * h // n - i * h // n) for i in range(n))
        ops = head(world) + [("create", 0, 40, 1), ("bind", 0, P, (lay,), all_l(lay), CELLS), ("set_cent", 0, None, "init", 1, TOKYO)]
        for fl in (CELLS, 0, CELLS | FUSED, OVERLAP, CELLS, FUSED, CELLS | OVERLAP):
            ops += [("bind", 0, P, (lay,), all_l(lay), fl), ("prime", 0), ("step", 0, 2), ("member", 0)]
            if not fl & FUSED:
                ops += [("run", 0), ("prime", 0), ("step", 0, 1)]
            else:
                ops += [("refuse", "run_fused", 0, 0), ("step", 0, 1)]
        S["flags_changed_on_one_object_" + world] = ops + [("destroy", 0)]
    # h < ranks for _init + _run
    Ph = ((1, 5, 301, 3),)
    lay5 = ((2, 1), (0, 0), (0, 1), (3, 0), (1, 1))
    S["fewer_rows_than_ranks"] = head("lb5") + [("create", 0, 9, 1)] + [x for fl in (0, CELLS) for x in (
        ("bind", 0, Ph, (lay5,), all_l(lay5), fl), ("init", 0), ("run", 0), ("init", 0), ("prime", 0), ("step", 0, 2))] + [("destroy", 0)]
    # bands in reverse owner order on a few-colour image: many ties of the initialisation
    fw, fh = dims(FEW)
    Pf = ((1, 0, fw, fh),)
    rev = tuple(reversed([(i * fh // 3, (i + 1) * fh // 3 - i * fh // 3) for i in range(3)]))
    S["reverse_owner_order_on_a_few_colour_image"] = [("world", "lb3"), ("upload", 1, FEW), ("strategy", 0)] + [x for k in (7, 40) for x in (
        ("create", 0, k, 1), ("bind", 0, Pf, (rev,), all_l(rev), 0), ("init", 0), ("run", 0), ("bind", 0, Pf, (rev,), all_l(rev), CELLS),
        ("init", 0), ("prime", 0), ("step", 0, 2), ("destroy", 0))]
    # a batch of three whose images stop at different checks, then set_centroids_image + prime + steps, then the loop again
    bw, bh = dims(FLAT)
    Pb = ((1, 40, 77, 7), (1, 0, w, h), (1, 100, 51, 20))       # (with k = 6 the oracle stops them at checks 2, never, 4)
    lays = tuple(make_layout(np.random.default_rng(i), 3, p[3], "cuts", False) for i, p in enumerate(Pb))
    S["batch_of_three_stopping_at_different_checks"] = [("world", "lb3"), ("upload", 0, FLAT), ("upload", 1, TOKYO), ("strategy", 2),
        ("create", 1, 6, 3), ("bind", 1, Pb, lays, tuple(tuple(1 for _ in l) for l in lays), 0), ("init", 1), ("run_batch", 1),
        ("set_cent", 1, 1, "rand", 5, 0), ("prime", 1), ("step", 1, 2), ("run_batch", 1), ("set_cent", 1, 0, "far", 6, 0), ("run_batch", 1),
        ("bind", 1, Pb, lays, None, FUSED | OVERLAP), ("prime", 1), ("step", 1, 1), ("refuse", "run_batch_fused", 1, 0), ("step", 1, 1), ("destroy", 1)]
    # two objects, one single and one batch, interleaved with the library's own sharded k-means (shrink 0, 2^20 pixels)
    mw, mh = dims(MEGA)
    Pm = ((0, 0, mw, mh),)
    laym = ((mh - 1, 1), (0, mh - 1))
    Pb2 = ((1, 3, 151, 90), (1, 1000, 99, 60))
    layb = (((0, 45), (45, 45)), ((60, 0), (0, 60)))
    S["two_objects_and_the_sharded_reduce"] = head("lb2") + [
        ("create", 0, 12, 1), ("create", 1, 5, 2), ("bind", 0, Pm, (laym,), all_l(laym), CELLS | FUSED), ("bind", 1, Pb2, layb, ((1, 1), (0, 1)), 0),
        ("init", 0), ("init", 1), ("prime", 0), ("prime", 1), ("host", "reduce", MEGA, 4, 1, 0, 0), ("step", 0, 1), ("step", 1, 1),
        ("host", "palette", MEGA, 3, 0, 0, 0), ("strategy", 0), ("step", 1, 1), ("step", 0, 1), ("single", 1, 0, 11, 50000, 20, 1),
        ("reduce_batch", (TOKYO, FLAT, FEW), 5, 2, 0), ("step", 0, 1), ("run_batch", 1), ("strategy", 1), ("step", 0, 1), ("prime", 1),
        ("destroy", 0), ("destroy", 1)]
    # k = 256 (the limit of the cell-sharded pass) and k = 257 (the plain loop) with the CELLS flag; the refusals of FUSED | CELLS
    lay = ((0, 1), (1, h - 1))
    ops = head("lb2")
    for k in (256, 257, 1, 2):
        ops += [("create", 0, k, 1), ("bind", 0, P, (lay,), all_l(lay), CELLS), ("init", 0), ("prime", 0), ("step", 0, 1), ("run", 0)]
        for what in ("fused_cells_bigk",) if k > 256 else ("fused_cells_rowless", "fused_cells_nolabels", "fused_cells_onelabel"):
            ops += [("refuse", what, 0, 1), ("prime", 0), ("step", 0, 1)]
        ops += [("destroy", 0)]
    S["k_256_and_257_with_the_cells_flag"] = ops
    return S


# ---- the real binding -----------------------------------------------------------------------------------------------
class KgGroupEnv(H.KgEnv):
    """kmeans_gpu_amd on cuda:0: one Group per world, created on first use and kept until close()"""

    def __init__(self):
        super().__init__()
        self.groups = {}

    def group(self, world):
        if world.name not in self.groups:
            self.groups[world.name] = self.kg.Group(devices=[0] * world.ranks, flags=world.flags, shrink_max_dim=world.shrink,
                                                    max_iterations=MAX_ITERATIONS, check_period=CHECK_PERIOD, strategy="auto")
        return self.groups[world.name]

    def bad_group(self, world):
        self.kg.Group(devices=[0] * world.ranks, flags=world.flags, alpha_cutoff=7).close()

    def group_lloyd(self, group, k, n_images):
        return self.kg.GroupLloyd(group, k, n_images)

    def close(self):
        for g in self.groups.values():
            g.close()
        self.groups = {}
