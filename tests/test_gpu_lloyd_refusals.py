"""Which refusal wins: the device-pointer calls of one Lloyd problem (kmg_lloyd_*, kmg_debug_* of csrc/kmg_lloyd.hip), each with one
fault and with every pair of faults.

Built like tests/test_gpu_refusals.py.  Per call the module holds an ORDERED list of faults -- the order in which the library's code
checks them -- with the status and the full message of each.  A call with one fault must return that fault's status and message; a
call with two must return those of the fault that stands earlier in the list.  A fault is a set of argument or object-state values;
two faults make a pair when they do not set one key to two values, which is decided when the cases are made: nothing is skipped at
run time.  (A weighted object has neither a caller's binding nor a cell share, and a cell share needs a binding: the faults say so
in their keys.)  The faults: the object NULL, each pointer NULL, n = 0, zero width and height, both outputs NULL, k = 0 and
KMG_MAX_K + 1 at create, more seeds than k and a seed that is not finite, an unknown weighting, set_weighting under a caller's
binding, n_fixed > k, set_fixed with a share set, j = 0 and j >= k, 129 reserved CUs, part >= parts and parts = 0, a weighted
object, no bound image, no current colour table, k = 257 where the call takes k <= 256, rebuild_from_histogram with 0 and 2^32
pixels, reduce_partials without a preceding assign_partials, and a cell share for the passes, the loop and the statistics that
need the whole cube -- wherever the call refuses them.

Only refusals that come BEFORE the call enqueues anything are listed: whichever of two faults wins, a refused call never reaches a
launch with a bad pointer.

Left out on purpose, and pinned by reading:
  * images of more than 2^32-1 pixels: with a wrong order the call would read far past the small buffer used here.  The refusal is
    one function, check_pixel_count in csrc/kmg_checks.h, called before the first launch of bind_image, init_centroids(_seeded)
    and init_step.
  * weighted passes over more than 2^28 pixels, for the same reason: one function in csrc/kmg_lloyd.hip, called by kmg_lloyd_run
    and the per-pixel assign pass before their first launch; tests/test_gpu_weight.py refuses 2^28 + 1 pixels on a real buffer.
  * kmg_lloyd_init_step's "the band changed since step j = 1" and "never started (j = 1)": they come after enqueued work.

Inputs: a 32 x 32 image of a seeded 300-colour palette on the device; one object with k = 4 and one with k = 257 on one processor,
a second k = 4 object that is weighted and a third that never ran a pass; the binding is kmg_lloyd_bind_image on the 1 024 pixels
(the plain-histogram route), followed by one pass for sums so that the colour table is current.  The object's state is made anew
before every call."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INV, UNS = -1, -5                       # KMG_ERR_INVALID_ARGUMENT, KMG_ERR_UNSUPPORTED
MAX_K = 3072
W = H = 32
N = W * H
K = 4


def F(name, sets, status, msg):
    return (name, sets, status, msg)


def bad(call, *keys, **values):
    """the faults a call answers with "bad <call> arguments": the object NULL, the pointers `keys` NULL, the `values`"""
    msg = f"bad {call} arguments"
    return [F("object NULL", {"obj": None}, INV, msg), *[F(f"{key} NULL", {key: False}, INV, msg) for key in keys],
            *[F(f"{key} = {v}", {key: v}, INV, msg) for key, v in values.items()]]


UNBOUND = {"bound": False, "share": False}
SHARE = {"bound": True, "share": True}


def weighted(call):
    return F("weighted object", {"obj": "weighted", **UNBOUND}, INV,
             f"{call}: the object's sums are weighted (kmg_lloyd_set_weighting): the colour table counts pixels")


def unbound(msg, status=INV):
    return F("no bound image", UNBOUND, status, msg)


K257 = {"obj": "k257"}
NO_TABLE = "no current colour table"
WHOLE_CUBE = F("cell share set", SHARE, INV, "statistics / checks of a bound image need the whole cube: a cell share is set")
ONE_SHARE = F("cell share set", SHARE, INV, "a cell share is set: this pass returns one share's sums only -- no label map, no update, no "
              "partial rows (all-reduce the sums, all-gather the tables, then kmg_lloyd_labels_from_tables)")
REBUILD = "bad rebuild_from_histogram arguments"

BASE = {"obj": "k4", "bound": True, "share": False, "partials": False, "p": True, "out": True, "k": K, "rgba": True, "n": N, "w": W, "h": H,
        "labels": True, "acc": True, "c4": True, "seeds": "finite", "n_seeds": 2, "weighting": 0, "n_fixed": 0, "j": 1, "key": True,
        "colour": True, "n_cus": 0, "part": 0, "parts": 2, "n_pixels": N, "count": True, "ms": True, "launches": True}

# call -> (base values that differ from BASE, the faults in the order the call checks them)
CALLS = {
    "kmg_lloyd_create": ({}, [F("processor NULL", {"p": False}, INV, "bad lloyd_create arguments"),
                              F("out NULL", {"out": False}, INV, "bad lloyd_create arguments"),
                              F("k = 0", {"k": 0}, INV, "k must be an integer higher than 0"),
                              F("k = KMG_MAX_K + 1", {"k": MAX_K + 1}, UNS, "k = 3073 exceeds KMG_MAX_K = 3072")]),
    "kmg_lloyd_set_centroids": ({}, bad("set_centroids", "c4")),
    "kmg_lloyd_get_centroids": ({}, bad("get_centroids", "c4")),
    # (the weighted object is refused before the NULL image)
    "kmg_lloyd_bind_image": (UNBOUND, [weighted("bind_image"), *bad("bind_image", "rgba", n=0)]),
    "kmg_lloyd_prepare": (UNBOUND, bad("prepare", "rgba", n=0)),
    "kmg_debug_bound_image": ({}, [*bad("bound_image", "out"), unbound("no image is bound")]),
    "kmg_lloyd_unbind_image": ({}, bad("unbind_image")),
    "kmg_debug_check_table": (UNBOUND, bad("check_table", "out")),
    "kmg_debug_table_stats": ({}, [*bad("table_stats", "out"), unbound(NO_TABLE), WHOLE_CUBE]),
    "kmg_debug_check_pairs": ({}, [*bad("check_pairs", "out"), unbound(NO_TABLE),
                                   F("k = 257", K257, INV, "pair entries exist for k <= 256 only"), WHOLE_CUBE]),
    "kmg_lloyd_init_centroids": (UNBOUND, bad("init_centroids", "rgba", w=0, h=0)),
    "kmg_lloyd_init_centroids_seeded": (UNBOUND, [
        *bad("init_centroids_seeded", "rgba", "seeds", w=0, h=0),
        F("more seeds than k", {"n_seeds": K + 1}, INV, "init_centroids_seeded: 5 seeds for k = 4"),
        F("seed not finite", {"seeds": "not finite"}, INV, "init_centroids_seeded: seed 1 is not finite")]),
    "kmg_lloyd_set_weighting": (UNBOUND, [
        F("object NULL", {"obj": None}, INV, "lloyd object is NULL"), F("unknown weighting", {"weighting": 7}, INV, "unknown weighting 7"),
        F("caller's binding", {"bound": True}, INV,
          "set_weighting: an image is bound (kmg_lloyd_unbind_image first): the colour table counts pixels")]),
    "kmg_lloyd_set_fixed": ({}, [*bad("set_fixed", n_fixed=K + 1),
                                 F("cell share set", SHARE, INV, "set_fixed: a cell share is set (kmg_lloyd_set_cell_share)")]),
    "kmg_lloyd_init_step": (UNBOUND, [*bad("init_step", "key", "rgba", j=0), F("j = k", {"j": K}, INV, "bad init_step arguments")]),
    "kmg_lloyd_init_pick_band": (UNBOUND, bad("init_pick_band", "key", "colour", "rgba")),
    "kmg_lloyd_set_centroid_rgba": ({}, bad("set_centroid_rgba", "colour", j=K)),
    "kmg_lloyd_assign_accumulate": ({}, [*bad("assign_accumulate", "rgba", n=0),
                                         F("both outputs NULL", {"labels": False, "acc": False}, INV, "bad assign_accumulate arguments"),
                                         ONE_SHARE]),
    "kmg_lloyd_accumulate_into": ({}, [*bad("accumulate_into", "rgba", "acc", n=0), weighted("accumulate_into"),
                                       unbound("accumulate_into: the image is not bound (kmg_lloyd_bind_image / _prepare)")]),
    "kmg_lloyd_assign_partials": ({}, [*bad("assign_partials", "rgba", n=0), ONE_SHARE]),
    "kmg_lloyd_reserve_cus": ({}, bad("reserve_cus", n_cus=129)),
    "kmg_lloyd_labels": ({}, bad("labels", "rgba", "labels", n=0)),
    "kmg_lloyd_set_cell_share": ({}, [*bad("set_cell_share", parts=0), F("part >= parts", {"part": 2}, INV, "bad set_cell_share arguments"),
                                      weighted("set_cell_share"), unbound("set_cell_share: no bound image")]),
    "kmg_lloyd_labels_from_tables": ({}, [*bad("labels_from_tables", "rgba", "labels", n=0), unbound("labels_from_tables: no bound image")]),
    "kmg_lloyd_labels_from_tables_update": ({}, [
        *bad("labels_from_tables_update", "rgba", "labels", "acc", n=0), weighted("labels_from_tables_update"),
        unbound("labels_from_tables_update: no bound image"),
        F("k = 257", K257, UNS, "labels_from_tables_update: k <= 256 (the label pass that carries a tail)")]),
    # (a NULL object, too, is answered with "no bound image")
    "kmg_lloyd_histogram_buffer": ({}, [F("object NULL", {"obj": None}, INV, "histogram_buffer: no bound image"),
                                        unbound("histogram_buffer: no bound image")]),
    "kmg_lloyd_rebuild_from_histogram": ({}, [F("object NULL", {"obj": None}, INV, REBUILD), unbound(REBUILD),
                                              F("0 pixels", {"n_pixels": 0}, INV, REBUILD), F("2^32 pixels", {"n_pixels": 1 << 32}, INV, REBUILD)]),
    "kmg_lloyd_table_buffers": ({}, [F("object NULL", {"obj": None}, INV, "table_buffers: no bound image"),
                                     unbound("table_buffers: no bound image")]),
    "kmg_lloyd_reduce_partials": ({**UNBOUND, "partials": True}, [
        *bad("reduce_partials", "acc", n=0),
        F("no assign_partials before", {"obj": "fresh", "partials": False}, INV, "reduce_partials without a preceding assign_partials")]),
    "kmg_lloyd_profile": ({}, bad("profile")),
    "kmg_lloyd_profile_read": ({}, bad("profile_read", "ms", "launches")),
    "kmg_lloyd_update": ({}, bad("update", "acc")),
    "kmg_lloyd_assign_update": ({}, [*bad("assign_update", "rgba", "acc", n=0), ONE_SHARE]),
    "kmg_lloyd_iterate": ({}, [*bad("iterate", "rgba", "acc", n=0),
                               F("cell share set", SHARE, INV, "iterate: a cell share is set (kmg_lloyd_set_cell_share)")]),
    "kmg_lloyd_flush": ({}, bad("flush")),
    "kmg_lloyd_converged_count": ({}, bad("converged_count", "count")),
    "kmg_lloyd_run": ({}, [*bad("lloyd_run", "rgba", n=0),
                           F("cell share set", SHARE, INV,
                             "lloyd_run: a cell share is set (kmg_lloyd_set_cell_share): the loop would update from one share's sums")]),
}


def compatible(f, g):
    return all(g[1].get(key, v) == v for key, v in f[1].items())


SINGLES = [(call, i) for call, (_, faults) in CALLS.items() for i in range(len(faults))]
PAIRS = [(call, i, j) for call, (_, faults) in CALLS.items() for i, j in itertools.combinations(range(len(faults)), 2)
         if compatible(faults[i], faults[j])]


class Env:
    """the processor, the four objects and the device buffers every case uses"""

    def __init__(self, kg, torch):
        self.kg, self.L, self.torch = kg, kg.lib(), torch
        rng = np.random.default_rng(20240608)
        palette = rng.integers(0, 256, (300, 4), dtype=np.uint8)
        palette[:, 3] = 255
        self.img = torch.from_numpy(np.ascontiguousarray(palette[rng.integers(0, 300, N)])).cuda()
        self.labels = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.acc = torch.zeros((257, 4), dtype=torch.int64, device="cuda")
        self.key = torch.tensor([int(self.L.kmg_init_first_key(W, H))], dtype=torch.int64, device="cuda")   # (names a pixel of the image)
        self.colour = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.c4 = np.zeros((257, 4), np.float32)
        self.c4[:, 0] = rng.uniform(0.0, 100.0, 257)
        self.c4[:, 1:3] = rng.uniform(-60.0, 60.0, (257, 2))
        self.seeds = {"finite": self.c4[:K + 1].copy(), "not finite": self.c4[:K + 1].copy()}
        self.seeds["not finite"][1, 2] = np.inf
        self.out = (C.c_uint64 * 14)()
        self.count, self.strategy, self.iterations = C.c_uint32(), C.c_int(), C.c_uint32()
        self.ms, self.launches = (C.c_double * 8)(), (C.c_uint32 * 8)()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.proc = kg.ImageProcessor(device=0)
        self.obj = {None: None}
        for name, k in (("k4", K), ("k257", 257), ("weighted", K), ("fresh", K)):
            h = C.c_void_p()
            self.ok(self.L.kmg_lloyd_create(self.proc._h, k, C.byref(h)))
            self.ok(self.L.kmg_lloyd_set_centroids(h, self.c4.ctypes.data, self.stream))
            self.obj[name] = h
        self.ok(self.L.kmg_lloyd_set_weighting(self.obj["weighted"], 1))
        torch.cuda.synchronize()

    def close(self):
        self.torch.cuda.synchronize()
        for h in self.obj.values():
            if h is not None:
                self.L.kmg_lloyd_destroy(h)
        self.proc.close()

    def ok(self, rc):
        assert rc == 0, self.L.kmg_last_error().decode()

    def establish(self, a):
        """the object's state before the call: bound by the caller with a current colour table (and a cell share), or unbound.  The
        weighted object and the one that never ran a pass stay as they were made: only refused calls meet them."""
        L, s, img, st = self.L, self.obj[a["obj"]], self.img.data_ptr(), self.stream
        if a["obj"] not in ("k4", "k257"):
            return
        if a["bound"]:
            self.ok(L.kmg_lloyd_bind_image(s, img, N, st))
            self.ok(L.kmg_lloyd_assign_accumulate(s, img, N, None, self.acc.data_ptr(), st))
            if a["share"]:
                self.ok(L.kmg_lloyd_set_cell_share(s, 0, 2, st))
        else:
            self.ok(L.kmg_lloyd_unbind_image(s))
        if a["partials"]:
            self.ok(L.kmg_lloyd_assign_partials(s, img, N, None, st))

    def call(self, name, a):
        """the call with the values of `a`: (status, message)"""
        self.establish(a)
        L, st, s = self.L, self.stream, self.obj[a["obj"]]
        rgba = self.img.data_ptr() if a["rgba"] else None
        labels = self.labels.data_ptr() if a["labels"] else None
        acc = self.acc.data_ptr() if a["acc"] else None
        key = self.key.data_ptr() if a["key"] else None
        colour = self.colour.data_ptr() if a["colour"] else None
        out = self.out if a["out"] else None
        c4 = self.c4.ctypes.data if a["c4"] else None
        seeds = self.seeds[a["seeds"]].ctypes.data if a["seeds"] else None
        n, w, h = a["n"], a["w"], a["h"]
        made = C.c_void_p()
        rc = {
            "kmg_lloyd_create": lambda: L.kmg_lloyd_create(self.proc._h if a["p"] else None, a["k"], C.byref(made) if a["out"] else None),
            "kmg_lloyd_set_centroids": lambda: L.kmg_lloyd_set_centroids(s, c4, st),
            "kmg_lloyd_get_centroids": lambda: L.kmg_lloyd_get_centroids(s, c4, st),
            "kmg_lloyd_bind_image": lambda: L.kmg_lloyd_bind_image(s, rgba, n, st),
            "kmg_lloyd_prepare": lambda: L.kmg_lloyd_prepare(s, rgba, n, 1, C.byref(self.strategy), st),
            "kmg_debug_bound_image": lambda: L.kmg_debug_bound_image(s, out),
            "kmg_lloyd_unbind_image": lambda: L.kmg_lloyd_unbind_image(s),
            "kmg_debug_check_table": lambda: L.kmg_debug_check_table(s, out, st),
            "kmg_debug_table_stats": lambda: L.kmg_debug_table_stats(s, out, st),
            "kmg_debug_check_pairs": lambda: L.kmg_debug_check_pairs(s, out, st),
            "kmg_lloyd_init_centroids": lambda: L.kmg_lloyd_init_centroids(s, rgba, w, h, st),
            "kmg_lloyd_init_centroids_seeded": lambda: L.kmg_lloyd_init_centroids_seeded(s, rgba, w, h, seeds, a["n_seeds"], st),
            "kmg_lloyd_set_weighting": lambda: L.kmg_lloyd_set_weighting(s, a["weighting"]),
            "kmg_lloyd_set_fixed": lambda: L.kmg_lloyd_set_fixed(s, a["n_fixed"]),
            "kmg_lloyd_init_step": lambda: L.kmg_lloyd_init_step(s, rgba, n, 0, a["j"], key, st),
            "kmg_lloyd_init_pick_band": lambda: L.kmg_lloyd_init_pick_band(s, rgba, n, 0, key, colour, st),
            "kmg_lloyd_set_centroid_rgba": lambda: L.kmg_lloyd_set_centroid_rgba(s, a["j"], colour, st),
            "kmg_lloyd_assign_accumulate": lambda: L.kmg_lloyd_assign_accumulate(s, rgba, n, labels, acc, st),
            "kmg_lloyd_accumulate_into": lambda: L.kmg_lloyd_accumulate_into(s, rgba, n, acc, st),
            "kmg_lloyd_assign_partials": lambda: L.kmg_lloyd_assign_partials(s, rgba, n, labels, st),
            "kmg_lloyd_reserve_cus": lambda: L.kmg_lloyd_reserve_cus(s, a["n_cus"]),
            "kmg_lloyd_labels": lambda: L.kmg_lloyd_labels(s, rgba, n, labels, st),
            "kmg_lloyd_set_cell_share": lambda: L.kmg_lloyd_set_cell_share(s, a["part"], a["parts"], st),
            "kmg_lloyd_labels_from_tables": lambda: L.kmg_lloyd_labels_from_tables(s, rgba, n, labels, st),
            "kmg_lloyd_labels_from_tables_update": lambda: L.kmg_lloyd_labels_from_tables_update(s, rgba, n, labels, acc, st),
            "kmg_lloyd_histogram_buffer": lambda: L.kmg_lloyd_histogram_buffer(s, None, None),
            "kmg_lloyd_rebuild_from_histogram": lambda: L.kmg_lloyd_rebuild_from_histogram(s, a["n_pixels"], st),
            "kmg_lloyd_table_buffers": lambda: L.kmg_lloyd_table_buffers(s, None, None, None, None),
            "kmg_lloyd_reduce_partials": lambda: L.kmg_lloyd_reduce_partials(s, n, acc, st),
            "kmg_lloyd_profile": lambda: L.kmg_lloyd_profile(s, 0),
            "kmg_lloyd_profile_read": lambda: L.kmg_lloyd_profile_read(s, self.ms if a["ms"] else None, self.launches if a["launches"] else None),
            "kmg_lloyd_update": lambda: L.kmg_lloyd_update(s, acc, st),
            "kmg_lloyd_assign_update": lambda: L.kmg_lloyd_assign_update(s, rgba, n, labels, acc, 1, st),
            "kmg_lloyd_iterate": lambda: L.kmg_lloyd_iterate(s, rgba, n, labels, acc, 0, st),
            "kmg_lloyd_flush": lambda: L.kmg_lloyd_flush(s, st),
            "kmg_lloyd_converged_count": lambda: L.kmg_lloyd_converged_count(s, C.byref(self.count) if a["count"] else None, st),
            "kmg_lloyd_run": lambda: L.kmg_lloyd_run(s, rgba, n, labels, C.byref(self.iterations), st),
        }[name]()
        msg = L.kmg_last_error().decode() if rc else ""
        if made:
            L.kmg_lloyd_destroy(made)
        return rc, msg


@pytest.fixture(scope="module")
def env(torch_cuda):
    import kmeans_gpu_amd as kg
    e = Env(kg, torch_cuda)
    yield e
    e.close()


def run(env, call, picked):
    base, faults = CALLS[call]
    a = {**BASE, **base}
    for i in picked:
        a.update(faults[i][1])
    _, _, status, msg = faults[picked[0]]
    got = env.call(call, a)
    print(call, [faults[i][0] for i in picked], "->", got)
    assert got == (status, msg)


def test_every_call_and_fault_is_covered():
    assert len(CALLS) == 37 and len(SINGLES) == sum(len(f) for _, f in CALLS.values())
    # every fault of a call with more than one meets at least one other: none stands in the list without its place being tested
    for call, (_, faults) in CALLS.items():
        met = {i for c, i, j in PAIRS if c == call} | {j for c, i, j in PAIRS if c == call}
        assert met == set(range(len(faults))) or len(faults) == 1, call
    # a weighted object has no binding and no share; a share needs a binding
    for _, (base, faults) in CALLS.items():
        for i, j in itertools.combinations(range(len(faults)), 2):
            a = {**BASE, **base, **faults[i][1], **faults[j][1]}
            if compatible(faults[i], faults[j]):
                assert not (a["share"] and not a["bound"]) and not (a["obj"] == "weighted" and a["bound"])


@pytest.mark.parametrize("call", list(CALLS))
def test_the_unfaulted_call_succeeds(env, call):
    assert env.call(call, {**BASE, **CALLS[call][0]}) == (0, "")


@pytest.mark.parametrize("call,i", SINGLES, ids=[f"{c}-{CALLS[c][1][i][0]}" for c, i in SINGLES])
def test_one_fault(env, call, i):
    run(env, call, (i,))


@pytest.mark.parametrize("call,i,j", PAIRS, ids=[f"{c}-{CALLS[c][1][i][0]}+{CALLS[c][1][j][0]}" for c, i, j in PAIRS])
def test_the_earlier_of_two_faults_wins(env, call, i, j):
    run(env, call, (i, j))
