"""Which refusal wins: the host-buffer calls of the C ABI (kmg_find .. kmg_compare), the sequence calls and the host calls of a
group of one device, each with one fault and with every pair of faults.

Per call the module holds an ORDERED list of faults -- the order in which the library's code checks them -- with the status and
the full message of each.  A call with one fault must return that fault's status and message; a call with two must return those
of the fault that stands earlier in the list.  A fault is a set of argument or processor-state values; two faults make a pair
when they do not set one key to two values, which is decided when the cases are made: nothing is skipped at run time.  The
faults: each pointer NULL, zero width and height, k = 0 and KMG_MAX_K + 1, algorithm -1 and 2, mode -1 and one past the call's
last, format -1 and 3, meld with an index format, INDEX8 with 257 colours, INDEX8 with 256 colours and alpha_cutoff = 1, k below
the processor's fixed-colour count, the octree with fixed colours and with weighting on, and an image with no pixel at the
cutoff -- wherever the call refuses them.

Left out on purpose: the refusal of an image of more than 2^32-1 pixels.  With a wrong order the call would read far past the
small buffers used here.  It is pinned by reading: the image triple (pointer, zero side, 2^32-1) is one function,
check_image_buffer in csrc/kmg_checks.h, and it is the first thing every call does with the image.

Inputs: a 32 x 32 image of a seeded 300-colour palette; the largest k that reaches the device is 257."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INV, UNS = -1, -5                       # KMG_ERR_INVALID_ARGUMENT, KMG_ERR_UNSUPPORTED
MAX_K = 3072
W = H = 32
KMEANS, OCTREE = 0, 1
REPLACE, MELD_MODE, DIFFUSE = 0, 2, 3
RGBA8, INDEX8, INDEX16 = 0, 1, 2
FRAME_DELTA = 1
N_FIXED = 3


def F(name, sets, status, msg):
    return (name, sets, status, msg)


ZERO = "image has zero width or height"
OUT_NULL = "output pointer is NULL"
PROC = F("processor NULL", {"p": False}, INV, "processor is NULL")
IMG = [F("image NULL", {"rgba": False}, INV, "image pointer is NULL"), F("zero width", {"w": 0}, INV, ZERO),
       F("zero height", {"h": 0}, INV, ZERO)]
K0 = F("k = 0", {"k": 0}, INV, "k must be an integer higher than 0")
KMAX = F("k = KMG_MAX_K + 1", {"k": MAX_K + 1, "algo": KMEANS}, UNS, "k = 3073 exceeds KMG_MAX_K = 3072")
ALGOS = [F(f"algorithm {v}", {"algo": v}, INV, f"unknown algorithm {v}") for v in (-1, 2)]
FORMATS = [F(f"format {v}", {"format": v}, INV, f"unknown output format {v}") for v in (-1, 3)]
OCT_W = F("octree, weighting on", {"algo": OCTREE, "weighting": 1}, INV, "the octree has no alpha weighting (it is on for the processor)")
OCT_F = F("octree, fixed colours", {"algo": OCTREE, "fixed": N_FIXED}, INV, "the octree has no fixed colours (3 are set on the processor)")
K_FIX = F("k below the fixed colours", {"k": 2, "fixed": N_FIXED}, INV, "k = 2 is below the 3 fixed colours of the processor")
NOPIX = F("no pixel at the cutoff", {"cutoff": 1, "img": "transparent"}, INV, "no pixel reaches alpha_cutoff = 1")
MELD = F("meld, index format", {"mode": MELD_MODE, "format": INDEX8}, INV, "meld blends two colours: it has no index output")
EMPTY = F("no pixel at the cutoff", {"seq": "empty"}, INV, "no pixel reaches alpha_cutoff (the working sequence is empty)")


def modes(last):
    return [F(f"mode {v}", {"mode": v}, INV, f"unknown mode {v}") for v in (-1, last + 1)]


def nulls(keys, msg):
    return [F(f"{key} NULL", {key: False}, INV, msg) for key in keys]


def index8(label, key, slot_always=False):
    """INDEX8 with 257 colours, INDEX8 with 256 colours and alpha_cutoff = 1 (the k-means algorithm: an octree may return fewer)"""
    def full(a):
        slot = " plus the transparent slot" if slot_always or a["cutoff"] else ""
        return f"INDEX8 holds 256 indices; {label} = {a[key]}{slot} needs INDEX16"
    return [F("INDEX8, 257 colours", {"format": INDEX8, key: 257, "algo": KMEANS}, INV, full),
            F("INDEX8, 256 colours, cutoff 1", {"format": INDEX8, key: 256, "cutoff": 1, "algo": KMEANS}, INV, full)]


def quality_range(a):
    return f"colour counts [{a['k_min']}, {a['k_max']}]: 1 <= k_min <= k_max <= 3072"


PAL_EMPTY = [F("palette NULL", {"pal": False}, INV, "palette is empty"), F("no colours", {"k": 0}, INV, "palette is empty")]
COMPARE_PAL = "an index format needs a palette of 1 .. 3072 colours"
GROUP_FIXED = "the processor of rank 0 has fixed colours set: the kmg_group_* calls have no pinned entries"
GROUP_WEIGHT = "the processor of rank 0 has alpha weighting on: the kmg_group_* calls have no weighted sums"
GROUP_STATE = [F("k below the fixed colours", {"k": 2, "fixed": N_FIXED}, INV, GROUP_FIXED),
               F("octree, fixed colours", {"algo": OCTREE, "fixed": N_FIXED}, INV, GROUP_FIXED),
               F("octree, weighting on", {"algo": OCTREE, "weighting": 1}, INV, GROUP_WEIGHT)]
# (a NULL group has no processor whose state could be refused first)
GROUP_NULL = F("group NULL", {"g": False, "fixed": 0, "weighting": 0}, INV, "group is NULL")
SEQ_NULL = F("sequence NULL", {"s": False}, INV, "sequence is NULL")

BASE = {"p": True, "g": True, "s": True, "seq": "main", "rgba": True, "img": "opaque", "w": W, "h": H, "k": 4, "k_min": 4, "k_max": 6,
        "algo": KMEANS, "mode": REPLACE, "format": RGBA8, "pal": True, "out": True, "out_pal": True, "out_count": True, "stats": True,
        "info": True, "is_full": True, "cutoff": 0, "fixed": 0, "weighting": 0}

# call -> (base values that differ from BASE, the faults in the order the call checks them)
CALLS = {
    "kmg_find": ({}, [PROC, *IMG, *PAL_EMPTY, F("out NULL", {"out": False}, INV, OUT_NULL), KMAX, *modes(DIFFUSE)]),
    "kmg_find_indexed": ({}, [PROC, *IMG, *PAL_EMPTY, F("out NULL", {"out": False}, INV, OUT_NULL), *FORMATS, KMAX, *modes(DIFFUSE), MELD,
                              *index8("k", "k")]),
    "kmg_reduce": ({}, [PROC, *IMG, K0, F("out NULL", {"out": False}, INV, OUT_NULL), *ALGOS, *modes(DIFFUSE), KMAX, OCT_W, OCT_F, K_FIX,
                        NOPIX]),
    "kmg_reduce_indexed": ({}, [PROC, *IMG, K0, *nulls(("out", "out_pal", "out_count"), OUT_NULL), *ALGOS, *modes(DIFFUSE), *FORMATS, KMAX,
                                OCT_W, OCT_F, K_FIX, NOPIX, MELD, *index8("k", "k")]),
    "kmg_palette": ({}, [PROC, *IMG, K0, *nulls(("out", "out_count"), OUT_NULL), *ALGOS, KMAX, OCT_W, OCT_F, K_FIX, NOPIX]),
    "kmg_reduce_quality": ({}, [F("k = 0", {"k_min": 0}, INV, quality_range), F("k = KMG_MAX_K + 1", {"k_max": MAX_K + 1}, INV, quality_range),
                                *modes(DIFFUSE), *FORMATS, MELD,
                                F("INDEX8, 257 colours", {"format": INDEX8, "k_max": 257}, INV, "INDEX8 holds 256 indices; k_max = 257 needs INDEX16"),
                                PROC, *IMG, *nulls(("out", "out_pal", "out_count"), OUT_NULL),
                                F("k below the fixed colours", {"k_min": 2, "fixed": N_FIXED}, INV, K_FIX[3]),
                                index8("k_max", "k_max")[1], NOPIX]),
    "kmg_compare": ({"format": INDEX16, "k": 8}, [
        *FORMATS, F("palette NULL", {"pal": False}, INV, COMPARE_PAL), F("k = 0", {"k": 0}, INV, COMPARE_PAL),
        F("k = KMG_MAX_K + 1", {"k": MAX_K + 1}, INV, COMPARE_PAL),
        F("INDEX8, 257 colours", {"format": INDEX8, "k": 257}, INV, "INDEX8 holds 256 indices; k = 257 needs INDEX16"),
        PROC, *IMG, *nulls(("out", "stats"), "output or statistics pointer is NULL"), index8("k", "k")[1]]),
    "kmg_sequence_add": ({}, [SEQ_NULL, *IMG]),
    "kmg_sequence_palette": ({}, [*nulls(("s", "out", "out_count"), "sequence_palette: a pointer is NULL"), K0, KMAX, EMPTY, K_FIX]),
    "kmg_sequence_output_begin": ({}, [*nulls(("s", "out_pal", "out_count"), "sequence_output_begin: a pointer is NULL"), *IMG[1:],
                                       *modes(DIFFUSE), *FORMATS, MELD, *index8("k", "k", slot_always=True), K0, KMAX, EMPTY, K_FIX]),
    "kmg_sequence_output_begin_local": ({"format": INDEX16}, [
        SEQ_NULL, *IMG[1:], K0, KMAX, *modes(DIFFUSE), *FORMATS, F("meld, index format", {"mode": MELD_MODE}, INV, MELD[3]),
        *index8("k", "k", slot_always=True)]),
    "kmg_sequence_output_frame": ({"seq": "shared"}, [
        SEQ_NULL, *nulls(("rgba", "out"), "sequence_output_frame: a pointer is NULL"),
        *nulls(("info", "is_full"), "KMG_FRAME_DELTA needs info and is_full")]),
    "kmg_sequence_output_frame_lossy": ({"seq": "shared"}, [
        SEQ_NULL, *nulls(("rgba", "out"), "sequence_output_frame_lossy: a pointer is NULL"),
        *nulls(("info", "is_full"), "KMG_FRAME_DELTA needs info and is_full")]),
    # (the open output has k = 2 colours)
    "kmg_sequence_output_frame_local": ({"seq": "local"}, [
        SEQ_NULL, *nulls(("rgba", "out", "out_pal", "out_count", "info", "is_full"), "sequence_output_frame_local: a pointer is NULL"),
        F("k below the fixed colours", {"fixed": N_FIXED}, INV, K_FIX[3]), NOPIX]),
    "kmg_group_palette": ({}, [*GROUP_STATE, K0, *nulls(("out", "out_count"), OUT_NULL), *ALGOS, KMAX, GROUP_NULL, *IMG]),
    "kmg_group_find": ({}, [*PAL_EMPTY, F("out NULL", {"out": False}, INV, OUT_NULL), *modes(MELD_MODE), KMAX, GROUP_NULL, *IMG]),
    "kmg_group_reduce": ({}, [*GROUP_STATE, K0, F("out NULL", {"out": False}, INV, OUT_NULL), *ALGOS, *modes(MELD_MODE), KMAX, GROUP_NULL,
                              *IMG]),
}


def compatible(f, g):
    return all(g[1].get(key, v) == v for key, v in f[1].items())


SINGLES = [(call, i) for call, (_, faults) in CALLS.items() for i in range(len(faults))]
PAIRS = [(call, i, j) for call, (_, faults) in CALLS.items() for i, j in itertools.combinations(range(len(faults)), 2)
         if compatible(faults[i], faults[j])]


class Env:
    """the processor, the group of one device, the sequences and the buffers every case uses"""

    def __init__(self, kg):
        self.kg, self.L = kg, kg.lib()
        rng = np.random.default_rng(20240607)
        palette = rng.integers(0, 256, (300, 4), dtype=np.uint8)
        palette[:, 3] = 255
        self.img = {"opaque": np.ascontiguousarray(palette[rng.integers(0, 300, W * H)])}
        self.img["transparent"] = self.img["opaque"].copy()
        self.img["transparent"][:, 3] = 0
        self.pal = rng.integers(0, 256, (MAX_K + 1, 4), dtype=np.uint8)
        self.fixed = np.ascontiguousarray(palette[:N_FIXED])
        self.out = np.zeros(W * H * 4, np.uint8)            # (kmg_compare: a map of index 0)
        self.out_pal = np.zeros((MAX_K + 1) * 4, np.uint8)
        self.out_count, self.is_full, self.reached = C.c_uint32(), C.c_int(), C.c_int()
        self.stats, self.info, self.delta_info = kg.ErrorStats(), kg.FrameHold(), kg.FrameDelta()
        self.tolerance = C.c_uint32(0)
        self.proc = kg.ImageProcessor(device=0)
        self.group = kg.Group(devices=[0])
        self.group_proc = C.c_void_p(self.L.kmg_group_processor(self.group._h, 0))
        self.seq = {}
        for name in ("main", "empty", "shared", "local"):
            h = C.c_void_p()
            self.ok(self.L.kmg_sequence_create(self.proc._h, C.byref(h)))
            self.seq[name] = h
            self.state(self.proc._h, {"cutoff": int(name == "empty"), "fixed": 0, "weighting": 0})
            self.ok(self.L.kmg_sequence_add(h, self.ptr(self.img["transparent" if name == "empty" else "opaque"]), W, H))
        self.state(self.proc._h, BASE)
        self.ok(self.L.kmg_sequence_output_begin(self.seq["shared"], 4, REPLACE, INDEX8, W, H, self.ptr(self.out_pal), C.byref(self.out_count)))
        self.ok(self.L.kmg_sequence_output_begin_local(self.seq["local"], 2, REPLACE, INDEX8, W, H, 0))

    def close(self):
        for h in self.seq.values():
            self.L.kmg_sequence_destroy(h)
        self.group.close()
        self.proc.close()

    def ok(self, rc):
        assert rc == 0, self.L.kmg_last_error().decode()

    @staticmethod
    def ptr(a):
        return a.ctypes.data

    def state(self, proc, a):
        self.ok(self.L.kmg_processor_set_alpha_cutoff(proc, a["cutoff"]))
        self.ok(self.L.kmg_processor_set_fixed_colors(proc, self.ptr(self.fixed) if a["fixed"] else None, a["fixed"]))
        self.ok(self.L.kmg_processor_set_weighting(proc, a["weighting"]))

    def call(self, name, a):
        """the call with the values of `a`: (status, message)"""
        L, on_group = self.L, name.startswith("kmg_group_")
        proc = self.group_proc if on_group else self.proc._h
        self.state(proc, a)
        try:
            p = proc if a["p"] else None
            g = self.group._h if a["g"] else None
            s = self.seq[a["seq"]] if a["s"] else None
            rgba = self.ptr(self.img[a["img"]]) if a["rgba"] else None
            pal = self.ptr(self.pal) if a["pal"] else None
            out = self.ptr(self.out) if a["out"] else None
            out_pal = self.ptr(self.out_pal) if a["out_pal"] else None
            out_count = C.byref(self.out_count) if a["out_count"] else None
            info = C.byref(self.info) if a["info"] else None
            is_full = C.byref(self.is_full) if a["is_full"] else None
            w, h, k, algo, mode, fmt = a["w"], a["h"], a["k"], a["algo"], a["mode"], a["format"]
            rc = {
                "kmg_find": lambda: L.kmg_find(p, rgba, w, h, pal, k, mode, out),
                "kmg_find_indexed": lambda: L.kmg_find_indexed(p, rgba, w, h, pal, k, mode, fmt, out),
                "kmg_reduce": lambda: L.kmg_reduce(p, rgba, w, h, k, algo, mode, out),
                "kmg_reduce_indexed": lambda: L.kmg_reduce_indexed(p, rgba, w, h, k, algo, mode, fmt, out_pal, out_count, out),
                "kmg_palette": lambda: L.kmg_palette(p, rgba, w, h, k, algo, out, out_count),
                "kmg_reduce_quality": lambda: L.kmg_reduce_quality(p, rgba, w, h, a["k_min"], a["k_max"], 0xFFFFFFFF, mode, fmt, out_pal, out_count,
                                                                   out, C.byref(self.stats), C.byref(self.reached)),
                "kmg_compare": lambda: L.kmg_compare(p, rgba, out, w, h, fmt, pal, k, 1, C.byref(self.stats) if a["stats"] else None),
                "kmg_sequence_add": lambda: L.kmg_sequence_add(s, rgba, w, h),
                "kmg_sequence_palette": lambda: L.kmg_sequence_palette(s, k, out, out_count),
                "kmg_sequence_output_begin": lambda: L.kmg_sequence_output_begin(s, k, mode, fmt, w, h, out_pal, out_count),
                "kmg_sequence_output_begin_local": lambda: L.kmg_sequence_output_begin_local(s, k, mode, fmt, w, h, 0),
                "kmg_sequence_output_frame": lambda: L.kmg_sequence_output_frame(s, rgba, FRAME_DELTA, out,
                                                                                 C.byref(self.delta_info) if a["info"] else None, is_full),
                "kmg_sequence_output_frame_lossy": lambda: L.kmg_sequence_output_frame_lossy(s, rgba, FRAME_DELTA, 0, out, info, is_full),
                "kmg_sequence_output_frame_local": lambda: L.kmg_sequence_output_frame_local(s, rgba, FRAME_DELTA, None, out, out_pal, out_count, info,
                                                                                             is_full),
                "kmg_group_palette": lambda: L.kmg_group_palette(g, rgba, w, h, k, algo, out, out_count),
                "kmg_group_find": lambda: L.kmg_group_find(g, rgba, w, h, pal, k, mode, out),
                "kmg_group_reduce": lambda: L.kmg_group_reduce(g, rgba, w, h, k, algo, mode, out),
            }[name]()
            return rc, (L.kmg_last_error().decode() if rc else "")
        finally:
            self.state(proc, BASE)


@pytest.fixture(scope="module")
def env(torch_cuda):
    import kmeans_gpu_amd as kg
    e = Env(kg)
    yield e
    e.close()


def run(env, call, picked):
    base, faults = CALLS[call]
    a = {**BASE, **base}
    for i in picked:
        a.update(faults[i][1])
    _, _, status, msg = faults[picked[0]]
    want = (status, msg(a) if callable(msg) else msg)
    got = env.call(call, a)
    print(call, [faults[i][0] for i in picked], "->", got)
    assert got == want


def test_every_call_and_fault_is_covered():
    assert len(CALLS) == 17 and len(SINGLES) == sum(len(f) for _, f in CALLS.values())
    # every fault of a call meets at least one other: none stands in the list without its place being tested
    for call, (_, faults) in CALLS.items():
        met = {i for c, i, j in PAIRS if c == call} | {j for c, i, j in PAIRS if c == call}
        assert met == set(range(len(faults))), call


@pytest.mark.parametrize("call", list(CALLS))
def test_the_unfaulted_call_succeeds(env, call):
    assert env.call(call, {**BASE, **CALLS[call][0]}) == (0, "")


@pytest.mark.parametrize("call,i", SINGLES, ids=[f"{c}-{CALLS[c][1][i][0]}" for c, i in SINGLES])
def test_one_fault(env, call, i):
    run(env, call, (i,))


@pytest.mark.parametrize("call,i,j", PAIRS, ids=[f"{c}-{CALLS[c][1][i][0]}+{CALLS[c][1][j][0]}" for c, i, j in PAIRS])
def test_the_earlier_of_two_faults_wins(env, call, i, j):
    run(env, call, (i, j))
