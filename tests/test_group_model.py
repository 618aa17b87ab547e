"""tests/group_harness.py shown to be SOUND and SHARP on the CPU, before the device sees it (tests/test_gpu_group_lifecycle.py runs
the same seeds and scenarios; the generator is deterministic, so what is covered here is covered there).

Sound: a stand-in for kmeans_gpu_amd.Group / GroupLloyd over the oracle that works BAND BY BAND -- every rank labels the pixels
its band pointer names and writes that band's label map, the sums are added over the ranks, every rank keeps a centroid table of
its own -- with the header's refusals, passes every generated sequence of the committed seeds and every hand-written scenario.
Sharp: eight faulty variants of it, one plausible mistake of the group layer each, are each caught by the committed seeds.
Coverage: what the issue of this harness lists (a rank without rows under KMG_GROUP_CELLS, permuted owners, d_labels == NULL, a
flag change on a live object in both directions, a batch run again, every k class, every world) is counted over the generated
lists and asserted.

Wall time of this file: 122 s (118 s of it the campaign: 10 sequences on nine stand-ins sharing the oracle's answers)."""
import collections
import time

import numpy as np
import pytest

import group_harness as G
import lifecycle_harness as H
import oracle_lib as O
from test_lifecycle_model import FakeError, FakeLloyd, FakeProcessor, HostMem, _assign, _view

SEEDS = (201, 202)                    # the seeds tests/test_gpu_group_lifecycle.py runs
SEQUENCES = 5                         # ... and its sequences per seed: one per world

FAULTS = ("init_rank_order", "dummy_pixel_counts", "stale_flags", "active_not_restored", "stale_rank1", "short_last_band",
          "fused_off_by_one", "broken_after_refusal")
ERR_HIP = -3


def _kmeans(img, k, shrink):
    h, w = img.shape[:2]
    if shrink and (w > shrink or h > shrink):
        img = O.resize(img, *O.resized_dims(w, h, shrink))
        h, w = img.shape[:2]
    lab = O.rgb_to_lab(img.reshape(-1, 4))
    return O.lloyd(lab, O.init_centroids(lab, w, h, k), H.MAX_ITERATIONS, H.CHECK_PERIOD)[0]


_host_cache = {}


def _cached(key, fn):
    if key not in _host_cache:
        _host_cache[key] = fn()
    return _host_cache[key]


class FakeGroup:
    def __init__(self, world, fault=None):
        self.world, self.fault = world, fault
        self.n_local = world.ranks
        self.procs = [FakeProcessor(None) for _ in range(world.ranks)]
        self.strategy = 0
        self.broken = False

    def enter(self):
        if self.broken:
            raise FakeError(ERR_HIP, "the group is broken")

    def refuse(self, message):
        if self.fault == "broken_after_refusal":
            self.broken = True
        raise FakeError(H.ERR_INVALID, message)

    def set_strategy(self, v):
        self.strategy = int(v)

    def processor(self, i=0):
        return self.procs[i]

    def stream(self, i=0):
        return i + 1

    def close(self):
        pass

    def _cent(self, img, k):
        return _cached(("km", img.tobytes(), k, self.world.shrink), lambda: _kmeans(img, k, self.world.shrink))

    def find(self, image, colors, reduce_mode=0, out=None):
        self.enter()
        if not 0 <= reduce_mode <= 2:
            self.refuse("unknown mode")
        return _cached(("find", image.tobytes(), colors.tobytes(), reduce_mode), lambda: O.find(image, colors, reduce_mode))

    def reduce(self, color_count, image, algo=0, reduce_mode=0, out=None):
        self.enter()
        if not 0 <= reduce_mode <= 2:
            self.refuse("unknown mode")
        if algo == 1:
            return _cached(("ro", image.tobytes(), color_count, reduce_mode), lambda: O.reduce_octree(image, color_count, reduce_mode))
        return _cached(("rk", image.tobytes(), color_count, reduce_mode, self.world.shrink), lambda: O.apply(image, self._cent(image, color_count), reduce_mode))

    def palette(self, color_count, image, algo=0):
        self.enter()
        if algo == 1:
            return O.palette_octree(image, color_count)
        return H.sorted_palette(self._cent(image, color_count))

    def reduce_batch(self, color_count, images, algo=0, reduce_mode=0):
        self.enter()
        if not 0 <= reduce_mode <= 2:
            self.refuse("unknown mode")
        return [self.reduce(color_count, im, algo, reduce_mode) for im in images]


class FakeGroupLloyd:
    def __init__(self, group, k, n_images=1):
        group.enter()
        if k == 0:
            group.refuse("k must be an integer higher than 0")
        self.g, self.k, self.n_images, self.fault = group, int(k), int(n_images), group.fault
        self.bound = None                                  # (bands[image][rank] = (ptr, row0, rows, label ptr), widths, heights, flags)
        self.cent = [[None] * n_images for _ in range(group.n_local)]        # [rank][image]
        self.shown = [None] * group.n_local                # what member(i) shows: the fault "stale_rank1" lets rank 1 lag
        self.acc = [None] * n_images
        self.active = [True] * n_images
        self.prepared, self.strategy_seen = False, 0

    def close(self):
        pass

    # -- binding
    def bind(self, d_rgba, row0, rows, width, height, d_labels=None, flags=0):
        if self.n_images != 1:
            self.g.refuse("a batch is bound with bind_batch")
        self._bind([d_rgba], [row0], [rows], [width], [height], None if d_labels is None else [d_labels], flags)

    def bind_batch(self, d_rgba, row0, rows, widths, heights, d_labels=None, flags=0):
        self._bind(d_rgba, row0, rows, widths, heights, d_labels, flags)

    def _bind(self, d_rgba, row0, rows, widths, heights, d_labels, flags):
        g = self.g
        g.enter()
        if flags & G.CELLS and self.n_images > 1:
            g.refuse("KMG_GROUP_CELLS: not for a batch")
        for im in range(self.n_images):
            for i in range(g.n_local):
                if rows[im][i] and not d_rgba[im][i]:
                    g.refuse("rows without pixels")
                if row0[im][i] + rows[im][i] > heights[im]:
                    g.refuse("a band leaves the image")
        if flags & G.FUSED and flags & G.CELLS and G.collectives(g.world):
            if self.k > 256 or d_labels is None or any(not r or not l for r, l in zip(rows[0], d_labels[0])):
                g.refuse("FUSED_UPDATE with CELLS: k <= 256, every rank rows and a label map")
        if self.fault == "stale_flags" and self.bound is not None:
            flags = self.bound[3]
        bands = [[(d_rgba[im][i], row0[im][i], rows[im][i], d_labels[im][i] if d_labels is not None else 0) for i in range(g.n_local)]
                 for im in range(self.n_images)]
        self.bound = (bands, list(widths), list(heights), flags)
        self.active = [True] * self.n_images
        self.prepared = False

    # -- centroids
    def _set_all(self, im, cent):
        for rank in range(self.g.n_local):
            self.cent[rank][im] = cent

    def _show(self):
        for rank in range(self.g.n_local):
            self.shown[rank] = self.cent[rank][0]

    def set_centroids(self, centroids4, image=None):
        self.g.enter()
        if (image or 0) >= self.n_images:
            self.g.refuse("image out of range")
        lag = self.cent[1][0] if self.g.n_local > 1 else None
        self._set_all(image or 0, np.array(centroids4, np.float32).reshape(self.k, 4))
        self._after(lag)

    def _after(self, lag):
        self._show()
        if self.fault == "stale_rank1" and self.g.n_local > 1 and lag is not None:
            self.shown[1] = lag

    def get_centroids(self, image=None):
        self.g.enter()
        if (image or 0) >= self.n_images:
            self.g.refuse("image out of range")
        return self.cent[0][image or 0].copy()

    def member(self, i=0):
        obj = self

        class Member:
            def get_centroids(self, stream=0):
                return obj.shown[i].copy()
        bands, _, _, flags = self.bound if self.bound is not None else ([[(0, 0, 0, 0)]], 0, 0, 0)
        table = G.cells_form(self.g.world, flags, self.k) or (bands[0][0][2] and self.strategy_seen == 2)
        return Member(), "table" if table else "scan"

    # -- the passes, band by band
    def _need_bound(self):
        self.g.enter()
        if self.bound is None:
            self.g.refuse("no bands")

    def _pixels(self, im, rank):
        ptr, _, rows, _ = self.bound[0][im][rank]
        return _view(ptr, 4 * rows * self.bound[1][im], np.uint8).reshape(-1, 4)

    def _whole(self, im, by_rank=False):
        ranks = [r for r in range(self.g.n_local) if self.bound[0][im][r][2]]
        if not by_rank:
            ranks.sort(key=lambda r: self.bound[0][im][r][1])
        return np.concatenate([self._pixels(im, r) for r in ranks])

    def _prepare(self):
        if not self.prepared:
            self.prepared, self.strategy_seen = True, self.g.strategy

    def _pass(self):
        """labels + sums of every (active) image under each rank's own table; the sums added over the ranks"""
        self._prepare()
        bands, widths, _, flags = self.bound
        cells = G.cells_form(self.g.world, flags, self.k)
        last = self.g.n_local - 1
        for im in range(self.n_images):
            if not self.active[im]:
                continue
            total = np.zeros((self.k, 4), np.int64)
            for rank in range(self.g.n_local):
                ptr, _, rows, lab_ptr = bands[im][rank]
                cent = self.cent[rank][im]
                if not rows:
                    if cells and self.fault == "dummy_pixel_counts":
                        total = total + _assign(np.zeros((1, 4), np.uint8), cent)[1]
                    continue
                labels, sums, _ = _assign(self._pixels(im, rank), cent)
                total = total + sums
                if lab_ptr:
                    n = rows * widths[im]
                    if self.fault == "short_last_band" and rank == last and self.g.n_local > 1:
                        n -= widths[im]
                    _view(lab_ptr, n, np.uint32)[:] = labels[:n]
            self.acc[im] = total

    def _update(self):
        for im in range(self.n_images):
            if self.active[im]:
                for rank in range(self.g.n_local):
                    self.cent[rank][im] = O.finalize(self.acc[im], self.cent[rank][im])[0]

    def _fused(self):
        return G.fused_form(self.g.world, self.bound[3], self.k)

    def init(self):
        self._need_bound()
        lag = self.cent[1][0] if self.g.n_local > 1 else None
        for im in range(self.n_images):
            px = self._whole(im, by_rank=self.fault == "init_rank_order")
            self._set_all(im, O.init_centroids(O.rgb_to_lab(px), self.bound[1][im], self.bound[2][im], self.k))
        self.prepared = False
        self._after(lag)

    def prime(self):
        self._need_bound()
        lag = self.cent[1][0] if self.g.n_local > 1 else None
        self._pass()
        if self._fused() and self.fault != "fused_off_by_one":
            self._update()
        self._after(lag)

    def step(self):
        self._need_bound()
        lag = self.cent[1][0] if self.g.n_local > 1 else None
        if self._fused():
            self._pass()
            self._update()
        else:
            self._update()
            self._pass()
        self._after(lag)

    def sync(self):
        self._need_bound()

    def run(self):
        if self.n_images != 1:
            self.g.enter()
            self.g.refuse("a batch runs with run_batch")
        return self.run_batch()[0]

    def run_batch(self):
        self._need_bound()
        if self.bound[3] & G.FUSED:
            self.g.refuse("FUSED_UPDATE is for prime / step")
        lag = self.cent[1][0] if self.g.n_local > 1 else None
        self._prepare()
        its = []
        for im in range(self.n_images):
            cent, _, it = O.lloyd(O.rgb_to_lab(self._whole(im)), self.cent[0][im], H.MAX_ITERATIONS, H.CHECK_PERIOD)
            self._set_all(im, cent)
            its.append(it)
        self.active = [True] * self.n_images
        self._pass()                                             # the bands' label maps of the final tables
        if self.fault == "active_not_restored" and self.n_images > 1:
            self.active = [it >= H.MAX_ITERATIONS - 1 for it in its]
        self._after(lag)
        return its


class FakeGroupEnv:
    def __init__(self, fault=None):
        self.fault = fault
        self.mem = HostMem()
        self.Error = FakeError
        self.groups = {}

    def sync(self):
        pass

    def group(self, world):
        if world.name not in self.groups:
            self.groups[world.name] = FakeGroup(world, self.fault)
        return self.groups[world.name]

    def bad_group(self, world):
        g = self.groups.get(world.name)
        if g is not None and self.fault == "broken_after_refusal":
            g.broken = True
        raise FakeError(H.ERR_INVALID, "the kmg_group_* calls have no alpha mode")

    def group_lloyd(self, group, k, n_images):
        return FakeGroupLloyd(group, k, n_images)

    def lloyd(self, proc, k):
        return FakeLloyd(proc, k)


@pytest.fixture(scope="module")
def campaign():
    """every generated sequence on the faithful stand-in and on the faulty ones (the oracle's answers are shared)"""
    t0 = time.time()
    lists, caught, passed = {}, collections.defaultdict(list), []
    envs = {f: FakeGroupEnv(f) for f in (None,) + FAULTS}
    for seed in SEEDS:
        for seq in range(SEQUENCES):
            ops = lists[(seed, seq)] = G.generate(seed, seq)
            cache = {}
            for fault, env in envs.items():
                try:
                    G.run_sequence(env, seed, seq, ops, cache=cache)
                    if fault is None:
                        passed.append((seed, seq))
                except H.Mismatch as e:
                    caught[fault].append((seed, seq, str(e)))
                    if fault is not None:
                        envs[fault] = FakeGroupEnv(fault)          # (a broken group is replaced: the next sequence starts clean)
    print(f"group model campaign: {time.time() - t0:.1f} s")
    return lists, caught, passed


def test_generator_is_deterministic_and_names_its_world():
    a, b = G.generate(SEEDS[0], 3), G.generate(SEEDS[0], 3)
    assert a == b and a[0] == ("world", G.WORLDS[3].name)
    assert G.generate(SEEDS[0], 1) != G.generate(SEEDS[1], 1)


def test_faithful_stand_in_passes_every_sequence(campaign):
    lists, caught, passed = campaign
    assert not caught[None], caught[None][0][2][:3000]
    assert len(passed) == len(SEEDS) * SEQUENCES


@pytest.mark.parametrize("fault", FAULTS)
def test_the_seeds_catch_the_faulty_stand_in(campaign, fault):
    assert campaign[1][fault], f"no sequence of seeds {SEEDS} notices the fault {fault!r}"


def test_faithful_stand_in_passes_every_scenario():
    env = FakeGroupEnv()
    for name, ops in G.scenarios().items():
        try:
            done = G.run_sequence(env, G.SCENARIO_SEED, 0, ops)[0]
        except H.Mismatch as e:
            raise AssertionError(f"scenario {name}: {str(e)[:3000]}") from None
        assert done == len(ops)


def test_the_batch_scenario_stops_its_images_at_different_checks():
    ops = G.scenarios()["batch_of_three_stopping_at_different_checks"]
    m = G.GModel(H.make_images(G.SCENARIO_SEED, 0), numeric=True)
    for op in ops:
        exp = G.apply_op(m, op)
        if op[0] == "run_batch":
            its = exp["iterations"]
            assert its[0] != its[2] and max(its[0], its[2]) < H.MAX_ITERATIONS - 1, its     # both converge, at different checks
            return


def test_a_mismatch_prints_a_list_that_replays(campaign):
    seed, seq, text = campaign[1]["short_last_band"][0]
    assert f"replay(env, {seed}, {seq}, [" in text
    ops = eval(text[text.index("replay(env,"):].split(", ", 3)[3].rsplit(")", 1)[0])          # the printed list, as a person would paste it
    with pytest.raises(H.Mismatch):
        G.replay(FakeGroupEnv("short_last_band"), seed, seq, ops)
    G.replay(FakeGroupEnv(), seed, seq, ops)


def test_coverage_of_the_committed_seeds(campaign):
    C = collections.Counter()
    for ops in campaign[0].values():
        C += G.coverage(ops)
    for key in ("cells_rowless", "permuted", "labels_null", "labels_some_null", "flags_to_cells", "flags_from_cells", "batch_rerun",
                "odd_width", "one_row_band", "fused_form", "op:single", "op:reduce_batch", "op:host", "op:member", "op:upload"):
        assert C[key] > 0, (key, sorted(C.items()))
    for i in range(len(H.K_CLASSES)):
        assert C[f"kclass:{i}"] > 0, (i, sorted(C.items()))
    for w in G.WORLDS:
        assert C["world:" + w.name] > 0, w.name
    assert 4 * C["refusals"] <= C["ops"], (C["refusals"], C["ops"])
    assert sum(C["refusal:" + r] > 0 for r in G.REFUSALS) >= len(G.REFUSALS) - 3, sorted(C.items())
