"""tests/lifecycle_harness.py shown to be SOUND and SHARP on the CPU, before the device sees it (tests/test_gpu_lifecycle.py runs the
same seeds; the generator is deterministic, so what is covered here is covered there).

Sound: a stand-in over the oracle that implements the documented semantics of kmeans_gpu_amd.Lloyd / ImageProcessor -- bindings
keyed on (pointer, n) over a snapshot of the pixels (the histogram), label tables with their validity, the internal accumulator,
partial rows, cell shares, refusals with the header's statuses, blocks handed from closed objects to new ones -- passes every
sequence of every committed seed.  Sharp: eight faulty variants of it, one plausible flag mistake each, are each caught by
every committed seed within its sequence budget.  Coverage: every op kind, k class, strategy value, refusal, image kind and
block re-use across k classes occurs; the minimum counts below are what the committed seeds give.

Wall time of this file: 23 s with 8 oracle threads (2 min 11 s of CPU time; the answers of the oracle are shared by the nine
stand-ins of a sequence); the whole non-GPU suite with it: 141 tests in 130 s."""
import collections
import ctypes

import numpy as np
import pytest

import lifecycle_harness as H
import oracle_lib as O
import diffuse_ref

SEEDS = (101, 102)          # the seeds tests/test_gpu_lifecycle.py runs
SEQUENCES = 6                         # ... and its sequences per seed

FAULTS = ("stale_init_binding", "tables_not_invalidated", "dirty_accumulator", "share_survives", "inherits_tables",
          "stale_partial_rows", "iterate_wrong_set", "reserve_changes_result")


class FakeError(RuntimeError):
    def __init__(self, status, message=""):
        super().__init__(f"stand-in error {status}: {message}")
        self.status = status


def _view(ptr, n, dtype):
    nbytes = int(n) * np.dtype(dtype).itemsize
    return np.frombuffer((ctypes.c_uint8 * nbytes).from_address(ptr), dtype=dtype)


class HostMem:
    class Buf:
        def __init__(self, nbytes):
            self.a = np.zeros(int(nbytes), np.uint8)
            self.ptr = self.a.ctypes.data

    def alloc(self, nbytes):
        return HostMem.Buf(nbytes)

    def write(self, buf, off, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf.a[off:off + a.size] = a

    def fill(self, buf, off, nbytes, byte):
        buf.a[off:off + nbytes] = byte

    def read(self, buf, off, nbytes):
        return buf.a[off:off + nbytes].copy()


_oracle_cache = {}


def _assign(px, cent):
    """(labels, sums, lab) of pixels under a centroid table, remembered across the stand-ins of one sequence"""
    key = (px.tobytes(), cent.tobytes())
    if key not in _oracle_cache:
        lab = O.rgb_to_lab(px)
        labels = O.assign(lab, cent)
        _oracle_cache[key] = (labels, O.accumulate(lab, labels, cent.shape[0]), lab)
    return _oracle_cache[key]


class FakeProcessor:
    def __init__(self, fault):
        self.fault = fault
        self.strategy = 0
        self.idle = []                 # blocks of closed objects: what their last owner left in them
        self.allocated = self.reused = 0

    def take(self):
        if self.idle:
            self.reused += 1
            return self.idle.pop()
        self.allocated += 1
        return {}

    def set_strategy(self, v):
        self.strategy = int(v)

    def forced(self):
        return {0: 0, 1: -1, 2: 1}[self.strategy & 3]

    def close(self):
        pass

    def debug_block_counts(self):
        return self.allocated, self.reused

    def _out(self, img, cent, mode):
        if mode == 3:
            return diffuse_ref.diffuse(img, diffuse_ref.oracle_apply_replace(O, cent))
        return O.apply(img, cent, mode)

    def _index(self, img, cent, mode, want):
        if mode == 0:
            return O.assign(O.rgb_to_lab(img.reshape(-1, 4)), cent)
        if mode == 1:
            h, w = img.shape[:2]
            return O.dither(O.rgb_to_lab(img.reshape(-1, 4)), w, h, cent)
        P = O.lab_to_rgba8(cent[:, :3])[:, :3].astype(np.int64)
        code = (P[:, 0] << 16) | (P[:, 1] << 8) | P[:, 2]
        first = {int(c): i for i, c in reversed(list(enumerate(code)))}
        wc = want.reshape(-1, 4)[:, :3].astype(np.int64)
        return np.array([first[int(c)] for c in (wc[:, 0] << 16) | (wc[:, 1] << 8) | wc[:, 2]], np.uint32)

    def apply(self, d_rgba, width, rows, row0, cent, mode, d_out, stream=0, format=None, _whole=None):
        self.idle.append(self.take())                                  # scratch from the idle blocks, and back
        img = _view(d_rgba, 4 * width * rows, np.uint8).reshape(rows, width, 4) if _whole is None else _whole
        cent = np.ascontiguousarray(cent, np.float32).reshape(-1, 4)
        want = self._out(img, cent, mode)
        if _whole is not None:
            want = want[row0:row0 + rows]
        if format is None:
            _view(d_out, 4 * width * rows, np.uint8)[:] = want.reshape(-1)
            return
        idx = self._index(img, cent, mode, self._out(img, cent, mode)).reshape(img.shape[0], width)
        if _whole is not None:
            idx = idx[row0:row0 + rows]
        _view(d_out, width * rows, np.uint8 if format == 1 else np.uint16)[:] = idx.reshape(-1)

    def apply_plan(self, cent, mode, n_pixels_hint, stream=0, format=None):
        proc = self

        class Plan:
            def __init__(self):
                self.bands = []

            def run(self, d_rgba, width, rows, row0, d_out, stream=0):
                # (the bands of a sequence tile one image from row 0: the diffusion continues across them)
                band = _view(d_rgba, 4 * width * rows, np.uint8).reshape(rows, width, 4).copy()
                self.bands.append(band)
                proc.apply(d_rgba, width, rows, row0, cent, mode, d_out, stream, format, _whole=np.concatenate(self.bands))

            def status(self):
                pass

            def close(self):
                pass
        return Plan()

    def find(self, image, colors, reduce_mode=0):
        pal = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        if reduce_mode == 3:
            return diffuse_ref.diffuse(image, diffuse_ref.oracle_find_replace(O, pal))
        return O.find(image, pal, reduce_mode)

    def _kmeans(self, k, image):
        h, w = image.shape[:2]
        lab = O.rgb_to_lab(image.reshape(-1, 4))
        return O.lloyd(lab, O.init_centroids(lab, w, h, k), H.MAX_ITERATIONS, H.CHECK_PERIOD)[0]

    def reduce(self, k, image, algo=0, reduce_mode=0):
        self.idle.append(self.take())
        return self._out(image, self._kmeans(k, image), reduce_mode)

    def palette(self, k, image, algo=0):
        return H.sorted_palette(self._kmeans(k, image))


MERGE_ROWS = 8


class FakeLloyd:
    """the documented semantics of kmg_lloyd_*, with the library's kept state spelled out so that a flag mistake can be made"""

    def __init__(self, proc, k, fault=None):
        self.p, self.k, self.fault = proc, int(k), fault
        self.cent = np.zeros((self.k, 4), np.float32)
        self.nconv = 0
        self.bound = None                  # dict(ptr, n, snap, by_caller, by_init)
        self.share = None
        self.block = proc.take()           # what the previous owner left: its tables
        self.tab = {"valid": False, "cent": None}
        self.alt = {"valid": False, "cent": None}
        self.acc_int = np.zeros((self.k, 4), np.int64)
        self.rows = {}
        self.last_rows = 0
        self.reserve = 0

    def close(self):
        self.block = {"cent": self.tab["cent"]}
        self.p.idle.append(self.block)

    # -- helpers
    def _px(self, ptr, n):
        return _view(ptr, 4 * n, np.uint8).reshape(n, 4)

    def _here(self, ptr, n):
        return self.bound is not None and self.bound["ptr"] == ptr and self.bound["n"] == n

    def _bind(self, ptr, n, by_caller=False, by_init=False):
        keep_tab = self.fault == "inherits_tables" and self.block.get("cent") is not None
        if keep_tab:                       # the flag that came with the block: the last owner's tables pass for this object's
            self.tab = {"valid": True, "cent": self.block.pop("cent"), "narrow": True}
        self.bound = {"ptr": ptr, "n": n, "snap": self._px(ptr, n).copy(), "by_caller": by_caller, "by_init": by_init}
        if self.fault != "share_survives":
            self.share = None
        if not keep_tab:
            self.tab = {"valid": False, "cent": None}
        self.alt = {"valid": False, "cent": None}

    def _share_mask(self, px):
        if self.share is None:
            return np.ones(px.shape[0], bool)
        part, parts = self.share
        cell = H.cell_of(px)
        return (cell >= (32768 * part) // parts) & (cell < (32768 * (part + 1)) // parts)

    def _gather(self, px, tab):
        labels = _assign(px, tab["cent"])[0]
        return labels & 0xFF if tab.get("narrow") else labels

    def _write_labels(self, d_labels, labels, table_pass):
        n = labels.size
        if table_pass and self.fault == "reserve_changes_result" and self.reserve:
            n -= -(-n * self.reserve // 256)
        _view(d_labels, labels.size, np.uint32)[:n] = labels[:n]

    def _table_sums(self):
        """the cube pass over the bound image's histogram: the sums of the share's colours, the tables (re)written for them"""
        snap = self.bound["snap"]
        labels, sums, lab = _assign(snap, self.cent)
        if self.share is not None:
            m = self._share_mask(snap)
            sums = O.accumulate(lab[m], labels[m], self.k)
        self.tab = {"valid": self.share is None, "cent": self.cent.copy()}
        self.bound["by_init"] = False
        return sums

    def _refuse_shared(self, want_labels, update, rows):
        if self.share is not None and (want_labels or update or rows):
            if self.fault == "dirty_accumulator":
                self.acc_int += 12345                  # the pass got as far as dirtying the accumulator
            raise FakeError(-1, "a cell share is set")

    def _table_pass(self, ptr, n, d_labels, d_acc, update=False, rows=False):
        self._refuse_shared(bool(d_labels), update, rows)
        sums = self._table_sums() + self.acc_int           # (zero between passes)
        self.acc_int[:] = 0
        if d_acc:
            _view(d_acc, 4 * self.k, np.int64)[:] = sums.reshape(-1)
        if d_labels:
            self._write_labels(d_labels, self._gather(self._px(ptr, n), self.tab), True)
        if update:
            self.cent, self.nconv = O.finalize(sums, self.cent)
            self.tab["valid"] = False
        return sums

    def _scan(self, ptr, n, d_labels):
        labels, sums, _ = _assign(self._px(ptr, n), self.cent)
        if d_labels:
            self._write_labels(d_labels, labels, False)
        return sums

    # -- centroids
    def set_centroids(self, c, stream=0):
        self.cent = np.ascontiguousarray(c, np.float32).reshape(self.k, 4).copy()
        if self.fault != "tables_not_invalidated":
            self.tab["valid"] = False

    def get_centroids(self, stream=0):
        out = self.cent.copy()
        out[:, 3] = 1.0
        return out

    def init_centroids(self, d_rgba, w, h, stream=0):
        n = w * h
        self.tab["valid"] = False
        f = self.p.forced()
        if self.k > 1 and f > 0:
            self._bind(d_rgba, n, by_init=True)
        elif self.bound is not None and self.bound["ptr"] == d_rgba:
            self.bound = None
            if self.fault != "share_survives":
                self.share = None
        self.cent = O.init_centroids(O.rgb_to_lab(self._px(d_rgba, n)), w, h, self.k)

    def update(self, d_acc, stream=0):
        acc = _view(d_acc, 4 * self.k, np.int64).reshape(self.k, 4)
        self.cent, self.nconv = O.finalize(acc, self.cent)
        if self.fault != "tables_not_invalidated":
            self.tab["valid"] = False

    def converged_count(self, stream=0):
        return self.nconv

    # -- binding
    def bind_image(self, d_rgba, n, stream=0):
        self._bind(d_rgba, n, by_caller=True)

    def unbind_image(self):
        self.bound, self.share = None, None
        self.tab = {"valid": False, "cent": None}

    def prepare(self, d_rgba, n, want_labels=True, stream=0):
        fresh = self._here(d_rgba, n) and self.bound["by_init"]
        f = self.p.forced()
        table = f > 0 or (f == 0 and n >= 1 << 21)
        if table:
            if not fresh:
                self._bind(d_rgba, n)
            self.bound["by_caller"], self.bound["by_init"] = True, False
            return "table"
        if self.bound is not None and self.bound["ptr"] == d_rgba:
            self.unbind_image()
        return "scan"

    def rebuild_from_histogram(self, n, stream=0):
        if self.bound is None:
            raise FakeError(-1, "no bound image")
        self.tab["valid"] = False

    def set_cell_share(self, part, parts, stream=0):
        if parts == 0 or part >= parts:
            raise FakeError(-1, "bad set_cell_share arguments")
        if self.bound is None:
            raise FakeError(-1, "no bound image")
        self.share = None if parts == 1 else (part, parts)

    # -- passes
    def assign_accumulate(self, d_rgba, n, d_labels, d_acc, stream=0):
        if self._here(d_rgba, n):
            if d_acc:
                self._table_pass(d_rgba, n, d_labels, d_acc)
            else:
                self.assign_partials(d_rgba, n, d_labels)
            return
        sums = self._scan(d_rgba, n, d_labels)
        self.last_rows = 0
        if d_acc:
            _view(d_acc, 4 * self.k, np.int64)[:] = sums.reshape(-1)

    def assign_partials(self, d_rgba, n, d_labels, stream=0):
        if self._here(d_rgba, n):
            self._refuse_shared(bool(d_labels), False, True)
            rows, sums = MERGE_ROWS, self._table_sums()
            if d_labels:
                self._write_labels(d_labels, self._gather(self._px(d_rgba, n), self.tab), True)
        else:
            rows, sums = max(1, min(64, -(-n // 4096))), self._scan(d_rgba, n, d_labels)
        for r in range(rows):                                 # the pass writes ITS rows, the sums in the last of them
            self.rows[r] = sums if r == rows - 1 else np.zeros_like(sums)
        self.last_rows = max(rows, self.last_rows) if self.fault == "stale_partial_rows" else rows

    def reduce_partials(self, n, d_acc, stream=0):
        if self.last_rows == 0:
            raise FakeError(-1, "reduce_partials without a preceding assign_partials")
        total = sum(self.rows[r] for r in range(self.last_rows) if r in self.rows)
        _view(d_acc, 4 * self.k, np.int64)[:] = np.asarray(total).reshape(-1)

    def labels(self, d_rgba, n, d_labels, stream=0):
        tab = self.tab
        if self.fault == "iterate_wrong_set" and self.alt["cent"] is not None and tab["valid"]:
            tab = self.alt
        if self._here(d_rgba, n) and tab["valid"]:
            self._write_labels(d_labels, self._gather(self._px(d_rgba, n), tab), True)
        else:
            self._scan(d_rgba, n, d_labels)

    def labels_from_tables(self, d_rgba, n, d_labels, stream=0):
        if self.bound is None:
            raise FakeError(-1, "no bound image")
        self._write_labels(d_labels, self._gather(self._px(d_rgba, n), self.tab), True)

    def accumulate_into(self, d_rgba, n, d_acc, stream=0):
        if not self._here(d_rgba, n):
            raise FakeError(-1, "the image is not bound")
        _view(d_acc, 4 * self.k, np.int64)[:] += self._table_sums().reshape(-1)

    def labels_from_tables_update(self, d_rgba, n, d_labels, d_acc, stream=0):
        if self.bound is None:
            raise FakeError(-1, "no bound image")
        if self.k > 256:
            raise FakeError(-5, "k <= 256")
        self._write_labels(d_labels, self._gather(self._px(d_rgba, n), self.tab), True)
        acc = _view(d_acc, 4 * self.k, np.int64)
        self.cent, self.nconv = O.finalize(acc.reshape(self.k, 4).copy(), self.cent)
        acc[:] = 0
        self.tab["valid"] = False

    def assign_update(self, d_rgba, n, d_labels, d_acc, do_update=True, stream=0):
        if self._here(d_rgba, n):
            self._table_pass(d_rgba, n, d_labels, d_acc, update=bool(do_update))
            return
        sums = self._scan(d_rgba, n, d_labels)
        _view(d_acc, 4 * self.k, np.int64)[:] = sums.reshape(-1)
        if do_update:
            self.update(d_acc)

    def iterate(self, d_rgba, n, d_labels, d_acc, update_first=True, stream=0):
        if not self._here(d_rgba, n) or not d_labels:
            if update_first:
                self.update(d_acc)
            return self.assign_accumulate(d_rgba, n, d_labels, d_acc)
        if self.share is not None:
            raise FakeError(-1, "iterate: a cell share is set")
        self.tab, self.alt = self.alt, self.tab                       # the other set of label tables
        if update_first:
            self.cent, self.nconv = O.finalize(_view(d_acc, 4 * self.k, np.int64).reshape(self.k, 4).copy(), self.cent)
        _view(d_acc, 4 * self.k, np.int64)[:] = self._table_sums().reshape(-1)
        self._write_labels(d_labels, self._gather(self._px(d_rgba, n), self.tab), True)

    def flush(self, stream=0):
        pass

    def run(self, d_rgba, n, d_labels=0, stream=0):
        if self.share is not None and self._here(d_rgba, n):
            if self.fault == "dirty_accumulator":
                self.acc_int += 12345
            raise FakeError(-1, "lloyd_run: a cell share is set")
        callers = self._here(d_rgba, n) and self.bound["by_caller"]
        px = self._px(d_rgba, n)
        if callers:
            px = self.bound["snap"]                               # trusted: the caller vouches for the contents
        elif self._here(d_rgba, n) and self.bound["by_init"] and self.fault == "stale_init_binding":
            px = self.bound["snap"]                               # the initialisation's histogram, whatever the buffer holds now
        self.cent, labels, it = O.lloyd(O.rgb_to_lab(px), self.cent, H.MAX_ITERATIONS, H.CHECK_PERIOD)
        if d_labels:
            self._write_labels(d_labels, _assign(self._px(d_rgba, n), self.cent)[0] if callers else labels, callers)
        if not callers and (self.p.forced() > 0 or (self.bound is not None and self.bound["ptr"] == d_rgba)):
            self.unbind_image()
        elif callers:
            self.tab["valid"] = False
        return it

    # -- switches
    def reserve_cus(self, n_cus):
        self.reserve = int(n_cus)

    def profile(self, enable=True):
        pass

    def profile_read(self):
        return {}


class FakeEnv:
    Error = FakeError

    def __init__(self, fault=None):
        self.fault = fault
        self.mem = HostMem()
        self.streams = [0, 0]

    def sync(self):
        pass

    def processor(self):
        return FakeProcessor(self.fault)

    def lloyd(self, proc, k):
        return FakeLloyd(proc, k, self.fault)


@pytest.fixture(scope="module")
def campaign():
    """every committed (seed, sequence) on the faithful stand-in and on each faulty one that seed has not caught yet"""
    O.lib()
    counters = collections.Counter()
    caught = {seed: {} for seed in SEEDS}
    failures, reused, n_ops = [], {}, 0
    for seed in SEEDS:
        reused[seed] = 0
        for seq in range(SEQUENCES):
            _oracle_cache.clear()
            answers = {}                          # the model's oracle answers: the same for every stand-in of this sequence
            ops = H.generate(seed, seq)
            try:
                done, _, again = H.run_sequence(FakeEnv(), seed, seq, ops, counters, cache=answers)
                reused[seed] += again
                n_ops += done
            except H.Mismatch as e:
                failures.append(str(e)[:3000])
            for fault in FAULTS:
                if fault in caught[seed]:
                    continue
                try:
                    H.run_sequence(FakeEnv(fault), seed, seq, ops, cache=answers)
                except H.Mismatch as e:
                    caught[seed][fault] = (seq, str(e).split("\n")[0][:200])
    _oracle_cache.clear()
    return {"counters": counters, "caught": caught, "failures": failures, "reused": reused, "ops": n_ops}


def test_generator_is_deterministic():
    assert H.generate(SEEDS[0], 1) == H.generate(SEEDS[0], 1)
    assert H.generate(SEEDS[0], 1) != H.generate(SEEDS[1], 1)
    ops = H.generate(SEEDS[0], 0)
    assert eval(repr(ops)) == ops                      # a sequence is a list of plain tuples: the printed list replays


def test_faithful_stand_in_passes_every_sequence(campaign):
    assert not campaign["failures"], "\n\n".join(campaign["failures"])
    assert all(n > 0 for n in campaign["reused"].values()), campaign["reused"]


@pytest.mark.parametrize("fault", FAULTS)
def test_every_seed_catches_the_faulty_stand_in(campaign, fault):
    for seed in SEEDS:
        assert fault in campaign["caught"][seed], f"seed {seed} does not catch {fault} in {SEQUENCES} sequences"


def test_a_mismatch_prints_a_list_that_replays(campaign):
    seq, _ = campaign["caught"][SEEDS[0]]["tables_not_invalidated"]
    with pytest.raises(H.Mismatch) as e:
        H.run_sequence(FakeEnv("tables_not_invalidated"), SEEDS[0], seq)
    text = str(e.value)
    assert f"seed {SEEDS[0]} sequence {seq}: op " in text
    ops = eval(text[text.index("replay(env, "):].split(", ", 3)[3][:-1])
    with pytest.raises(H.Mismatch):
        H.replay(FakeEnv("tables_not_invalidated"), SEEDS[0], seq, ops)
    assert H.replay(FakeEnv(), SEEDS[0], seq, ops)[0] == len(ops)


# what the committed seeds give (SEEDS x SEQUENCES), exactly: the generator is deterministic.  None may be zero.
MINIMUM = {
    'apply_format:1': 9, 'apply_format:2': 4, 'apply_format:None': 33, 'apply_mode:0': 11, 'apply_mode:1': 17,
    'apply_mode:2': 7, 'apply_mode:3': 11, 'apply_plan': 28, 'apply_whole': 18, 'centroids:dup': 25, 'centroids:far': 8,
    'centroids:init': 29, 'centroids:rand': 58, 'host:find': 7, 'host:palette': 11, 'host:reduce': 4, 'image:blobs': 8,
    'image:few': 18, 'image:flat': 11, 'image:gradient': 15, 'image:large': 6, 'image:mega': 9, 'image:noise': 17,
    'image:tiny': 22, 'image:tokyo': 7, 'iterate_left_in_flight': 2, 'kclass:0': 11, 'kclass:1': 24, 'kclass:2': 24,
    'kclass:3': 15, 'kclass:4': 8, 'op:apply': 46, 'op:assign': 109, 'op:assign_update': 25, 'op:bind': 92, 'op:close': 41,
    'op:conv': 9, 'op:create': 41, 'op:get': 84, 'op:host': 22, 'op:init': 59, 'op:iterate': 50, 'op:labels': 94, 'op:lft': 3,
    'op:partials': 59, 'op:prepare': 38, 'op:profile': 10, 'op:profile_read': 3, 'op:rebuild': 3, 'op:recreate': 41,
    'op:refuse': 97, 'op:reserve': 34, 'op:run': 44, 'op:set_cent': 120, 'op:share_round': 39, 'op:strategy': 31,
    'op:unbind': 36, 'op:update': 23, 'op:upload': 113, 'refusal:assign_update': 3, 'refusal:iterate': 3, 'refusal:labelmap': 3,
    'refusal:lftu_bigk': 13, 'refusal:partials': 3, 'refusal:run': 3, 'refusal:share_bad': 26, 'refusal:unbound_into': 14,
    'refusal:unbound_lft': 9, 'refusal:unbound_rebuild': 8, 'refusal:unbound_share': 12, 'reuse_across_k_class': 41,
    'share_fused': 13, 'share_parts:1': 7, 'share_parts:2': 8, 'share_parts:3': 7, 'share_parts:4': 9, 'share_parts:8': 8,
    'share_plain': 26, 'strategy:0': 11, 'strategy:1': 3, 'strategy:2': 9, 'strategy:6': 8,
}


def test_coverage_of_the_committed_seeds(campaign):
    c = campaign["counters"]
    print(dict(sorted(c.items())), campaign["ops"])
    need = [f"kclass:{i}" for i in range(5)] + [f"strategy:{v}" for v in H.STRATEGIES] + ["refusal:" + r for r in H.REFUSALS] + \
           ["image:" + k for k in H.IMAGE_KINDS] + ["reuse_across_k_class", "iterate_left_in_flight"] + \
           ["op:" + o for o in ("create", "close", "recreate", "upload", "set_cent", "init", "get", "assign", "labels", "partials", "update",
                                "assign_update", "iterate", "conv", "run", "bind", "prepare", "unbind", "rebuild", "share_round", "lft",
                                "strategy", "reserve", "profile", "profile_read", "apply", "host", "refuse")] + \
           [f"share_parts:{p}" for p in (1, 2, 3, 4, 8)] + ["share_fused", "share_plain"] + \
           [f"apply_mode:{m}" for m in range(4)] + [f"apply_format:{f}" for f in (None, 1, 2)] + ["apply_plan", "apply_whole"] + \
           ["host:find", "host:reduce", "host:palette"] + ["centroids:" + k for k in ("init", "rand", "dup", "far")]
    assert set(need) == set(MINIMUM), sorted(set(need) ^ set(MINIMUM))
    low = {name: (c[name], MINIMUM[name]) for name in need if c[name] < MINIMUM[name] or MINIMUM[name] < 1}
    assert not low, low
