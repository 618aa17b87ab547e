"""The refusals an apply plan makes on its own (kmg_apply_plan_*, kmg_dev_apply of csrc/kmg_apply.hip), each with its status and full
message, each beside the nearest call that is accepted; and the plan's scratch block handed back and taken again on every route.

Refusals.  Every one is made on the host before the call enqueues anything, so a refused call never reaches a launch with a bad
pointer.  At create: the processor, the table or the output pointer NULL, k = 0, k above KMG_MAX_K, a mode and a format outside the
enumerations, meld with an index format, INDEX8 without room (k = 257; k = 256 in alpha mode, which needs the transparent slot), a
centroid outside the box of the index formats (one case per bound).  At run: the plan or a buffer NULL, zero width or rows, an
INDEX16 output at an odd address, a diffusion band that does not start at the rows done so far or has another width.
kmg_apply_plan_status on NULL.  kmg_dev_apply with a NULL argument, a zero side or k = 0.  The accepted neighbour of a refusal
differs from it in the faulted value only and sits on the other side of the check: k = KMG_MAX_K, k = 256 (255 in alpha mode), the
centroid on the bound itself, the even address, the band that does continue.

Left out on purpose: a band of more than 2^32-1 pixels (w * rows), for the reason tests/test_gpu_lloyd_refusals.py gives -- were the
check to move behind a launch, the kernel would walk far past the small buffers used here.

Arena hand-back.  For every (strategy, k, mode) of the table in tests/test_gpu_alpha_routes.py, at alpha_cutoff 0, as RGBA8 and --
where the mode has an index output -- as INDEX16 and (k <= 256) INDEX8: create a plan, run it in two bands, synchronise the
stream, destroy the plan with synchronise = 0, create it again on the same processor and run it again.  The second plan takes the
block the first gave back; its bytes must equal the first's and kmg_dev_apply's.

One image of 67 x 33 pixels, bands of 17 and 16 rows: the second band starts 1139 pixels in, so its pointers are not 16-byte
aligned (RGBA8) and odd (INDEX8); 2211 pixels are more than one workgroup of every output kernel."""
import ctypes as C

import numpy as np
import pytest

from conftest import set_strategy
from test_gpu_alpha_routes import ROUTES

pytestmark = pytest.mark.gpu

INV, UNS = -1, -5                       # KMG_ERR_INVALID_ARGUMENT, KMG_ERR_UNSUPPORTED
MAX_K = 3072
W, H, SPLIT = 67, 33, 17
N = W * H
REPLACE, DITHER, MELD, DIFFUSE = 0, 1, 2, 3
RGBA8, INDEX8, INDEX16 = 0, 1, 2
BYTES = {None: 4, RGBA8: 4, INDEX8: 1, INDEX16: 2}

PLAN_ARGS, RUN_ARGS, APPLY_ARGS = "bad apply_plan arguments", "bad apply_plan_run arguments", "bad apply arguments"
BOX = "centroid 2 (%g, %g, %g) is outside L in [-100, 200], a, b in [-300, 300] (index formats)"

# ---- create: values of kmg_apply_plan_create (format None) / kmg_apply_plan_create_format.  "edit": (component, value) of centroid 2
CREATE = {"p": True, "c4": True, "out": True, "k": 4, "mode": REPLACE, "format": None, "alpha": False, "edit": None}


def box(component, outside, on_bound):
    triple = [50.0, 10.0, -10.0]
    triple[component] = outside
    return ({"format": INDEX16, "edit": (component, outside)}, INV, BOX % tuple(triple), {"format": INDEX16, "edit": (component, on_bound)})


# name -> (the refused values, status, message, the accepted neighbour's values)
CREATE_CASES = {
    "processor NULL": ({"p": False}, INV, PLAN_ARGS, {}),
    "processor NULL, with a format": ({"p": False, "format": INDEX8}, INV, PLAN_ARGS, {"format": INDEX8}),
    "table NULL": ({"c4": False}, INV, PLAN_ARGS, {}),
    "out NULL": ({"out": False}, INV, PLAN_ARGS, {}),
    "k = 0": ({"k": 0}, INV, PLAN_ARGS, {"k": 1}),
    "k = KMG_MAX_K + 1": ({"k": MAX_K + 1}, UNS, "k = 3073 exceeds KMG_MAX_K = 3072", {"k": MAX_K}),
    "mode -1": ({"mode": -1}, INV, "unknown mode -1", {"mode": REPLACE}),
    "mode 4": ({"mode": 4}, INV, "unknown mode 4", {"mode": DIFFUSE}),
    "format -1": ({"format": -1}, INV, "unknown output format -1", {"format": RGBA8}),
    "format 3": ({"format": 3}, INV, "unknown output format 3", {"format": INDEX16}),
    "meld, INDEX8": ({"mode": MELD, "format": INDEX8}, INV, "meld blends two colours: it has no index output", {"mode": MELD, "format": RGBA8}),
    "meld, INDEX16": ({"mode": MELD, "format": INDEX16}, INV, "meld blends two colours: it has no index output",
                      {"mode": DITHER, "format": INDEX16}),
    "INDEX8, k = 257": ({"format": INDEX8, "k": 257}, INV, "INDEX8 holds 256 indices; k = 257 needs INDEX16", {"format": INDEX8, "k": 256}),
    "INDEX8, k = 255 + 1 in alpha mode": ({"format": INDEX8, "k": 256, "alpha": True}, INV,
                                          "INDEX8 holds 256 indices; k = 256 plus the transparent slot needs INDEX16",
                                          {"format": INDEX8, "k": 255, "alpha": True}),
    "L below the box": box(0, -100.5, -100.0),
    "L above the box": box(0, 200.5, 200.0),
    "a below the box": box(1, -300.5, -300.0),
    "a above the box": box(1, 300.5, 300.0),
    "b below the box": box(2, -300.5, -300.0),
    "b above the box": box(2, 300.5, 300.0),
}

# ---- run: one fresh plan per case.  "done": rows of a first band run before the call (diffusion); "odd": d_out one byte further
RUN = {"plan": True, "rgba": True, "d_out": True, "w": W, "rows": SPLIT, "row0": 0, "mode": REPLACE, "format": None, "done": 0, "odd": False}
DIFF = {"mode": DIFFUSE}
SECOND = {"mode": DIFFUSE, "done": SPLIT, "row0": SPLIT, "rows": H - SPLIT}

RUN_CASES = {
    "plan NULL": ({"plan": False}, INV, RUN_ARGS, {}),
    "image NULL": ({"rgba": False}, INV, RUN_ARGS, {}),
    "output NULL": ({"d_out": False}, INV, RUN_ARGS, {}),
    "zero width": ({"w": 0}, INV, RUN_ARGS, {"w": 1}),
    "zero rows": ({"rows": 0}, INV, RUN_ARGS, {"rows": 1}),
    "zero width, diffusion": ({**DIFF, "w": 0}, INV, RUN_ARGS, {**DIFF, "w": 1}),
    "zero rows, INDEX8": ({"format": INDEX8, "rows": 0}, INV, RUN_ARGS, {"format": INDEX8, "rows": 1}),
    "INDEX16 at an odd address": ({"format": INDEX16, "odd": True}, INV, "INDEX16 output must be 2-byte aligned", {"format": INDEX16}),
    "INDEX16 at an odd address, diffusion": ({**DIFF, "format": INDEX16, "odd": True}, INV, "INDEX16 output must be 2-byte aligned",
                                             {**DIFF, "format": INDEX16}),
    "INDEX8 at an odd address is fine": (None, 0, "", {"format": INDEX8, "odd": True}),
    "first diffusion band not at row 0": ({**DIFF, "row0": 1}, INV, "diffusion band starts at row 1, the plan has done 0 rows", DIFF),
    "diffusion band one row early": ({**SECOND, "row0": SPLIT - 1}, INV, "diffusion band starts at row 16, the plan has done 17 rows", SECOND),
    "diffusion band one row late": ({**SECOND, "row0": SPLIT + 1, "rows": H - SPLIT - 1}, INV,
                                    "diffusion band starts at row 18, the plan has done 17 rows", SECOND),
    "diffusion band of another width": ({**SECOND, "w": W - 1}, INV, "diffusion band has width 66, the image has 67", SECOND),
    "other rows and width do not matter without diffusion": (None, 0, "", {"row0": SPLIT + 1, "rows": H - SPLIT - 1, "w": W - 1}),
}

# ---- kmg_dev_apply
APPLY = {"p": True, "rgba": True, "d_out": True, "c4": True, "w": W, "rows": H, "k": 4}
APPLY_CASES = {
    "processor NULL": ({"p": False}, {}), "image NULL": ({"rgba": False}, {}), "output NULL": ({"d_out": False}, {}),
    "table NULL": ({"c4": False}, {}), "zero width": ({"w": 0}, {"w": 1}), "zero rows": ({"rows": 0}, {"rows": 1}), "k = 0": ({"k": 0}, {"k": 1}),
}


class Env:
    """two processors (alpha ignored, alpha mode), the image and the output buffers on the device"""

    def __init__(self, kg, torch):
        self.kg, self.L, self.torch = kg, kg.lib(), torch
        rng = np.random.default_rng(6733)
        self.image = rng.integers(0, 256, (N, 4), dtype=np.uint8)
        self.d_in = torch.from_numpy(self.image).cuda()
        self.d_out = torch.zeros(4 * N + 16, dtype=torch.uint8, device="cuda")
        assert self.d_in.data_ptr() % 16 == 0 and self.d_out.data_ptr() % 16 == 0
        self.c4 = np.zeros((MAX_K + 1, 4), np.float32)
        self.c4[:, 0] = rng.uniform(0.0, 100.0, MAX_K + 1)
        self.c4[:, 1:3] = rng.uniform(-60.0, 60.0, (MAX_K + 1, 2))
        self.c4[2, :3] = (50.0, 10.0, -10.0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.procs = {False: kg.ImageProcessor(device=0), True: kg.ImageProcessor(device=0, alpha_cutoff=1)}

    def close(self):
        self.torch.cuda.synchronize()
        for p in self.procs.values():
            p.close()

    def message(self, rc):
        return self.L.kmg_last_error().decode() if rc else ""

    def create(self, a):
        """(status, message) of kmg_apply_plan_create[_format]; a plan that was made is destroyed again"""
        L = self.L
        c4 = self.c4.copy()
        if a["edit"]:
            c4[2, a["edit"][0]] = a["edit"][1]
        p = self.procs[a["alpha"]]._h if a["p"] else None
        table = c4.ctypes.data if a["c4"] else None
        made = C.c_void_p()
        out = C.byref(made) if a["out"] else None
        if a["format"] is None:
            rc = L.kmg_apply_plan_create(p, table, a["k"], a["mode"], N, self.stream, out)
        else:
            rc = L.kmg_apply_plan_create_format(p, table, a["k"], a["mode"], a["format"], N, self.stream, out)
        got = rc, self.message(rc)
        assert bool(made) == (rc == 0)
        if made:
            L.kmg_apply_plan_destroy(made, 1)
        return got

    def plan(self, k, mode, fmt, proc=None):
        made = C.c_void_p()
        p = (proc or self.procs[False])._h
        if fmt is None:
            rc = self.L.kmg_apply_plan_create(p, self.c4.ctypes.data, k, mode, N, self.stream, C.byref(made))
        else:
            rc = self.L.kmg_apply_plan_create_format(p, self.c4.ctypes.data, k, mode, fmt, N, self.stream, C.byref(made))
        assert rc == 0, self.message(rc)
        return made

    def run(self, a):
        """(status, message) of kmg_apply_plan_run on a fresh plan"""
        L, st = self.L, self.stream
        pl = self.plan(4, a["mode"], a["format"])
        try:
            if a["done"]:
                rc = L.kmg_apply_plan_run(pl, self.d_in.data_ptr(), W, a["done"], 0, self.d_out.data_ptr(), st)
                assert rc == 0, self.message(rc)
            first = 4 * W * a["row0"]                                   # (of the image; the output starts at the buffer's first byte)
            rc = L.kmg_apply_plan_run(pl if a["plan"] else None, self.d_in.data_ptr() + first if a["rgba"] else None, a["w"], a["rows"],
                                      a["row0"], self.d_out.data_ptr() + (1 if a["odd"] else 0) if a["d_out"] else None, st)
            got = rc, self.message(rc)
            if rc == 0:
                rc = L.kmg_apply_plan_status(pl)
                assert rc == 0, self.message(rc)
            return got
        finally:
            L.kmg_apply_plan_destroy(pl, 1)

    def apply(self, a):
        rc = self.L.kmg_dev_apply(self.procs[False]._h if a["p"] else None, self.d_in.data_ptr() if a["rgba"] else None, a["w"], a["rows"], 0,
                                  self.c4.ctypes.data if a["c4"] else None, a["k"], REPLACE, self.d_out.data_ptr() if a["d_out"] else None,
                                  self.stream)
        return rc, self.message(rc)


@pytest.fixture(scope="module")
def env(torch_cuda):
    import kmeans_gpu_amd as kg
    e = Env(kg, torch_cuda)
    yield e
    e.close()


@pytest.mark.parametrize("name", list(CREATE_CASES))
def test_create_refuses_and_accepts_the_neighbour(env, name):
    refused, status, msg, accepted = CREATE_CASES[name]
    got = env.create({**CREATE, **refused})
    print(name, "->", got)
    assert got == (status, msg)
    assert env.create({**CREATE, **accepted}) == (0, "")


@pytest.mark.parametrize("name", list(RUN_CASES))
def test_run_refuses_and_accepts_the_neighbour(env, name):
    refused, status, msg, accepted = RUN_CASES[name]
    if refused is not None:
        got = env.run({**RUN, **refused})
        print(name, "->", got)
        assert got == (status, msg)
    assert env.run({**RUN, **accepted}) == (0, "")


def test_status_refuses_null(env):
    rc = env.L.kmg_apply_plan_status(None)
    assert (rc, env.message(rc)) == (INV, "bad apply_plan_status arguments")
    for mode in (REPLACE, DIFFUSE):                                     # a plan that never ran answers KMG_OK
        pl = env.plan(4, mode, None)
        assert env.L.kmg_apply_plan_status(pl) == 0
        env.L.kmg_apply_plan_destroy(pl, 1)
    env.L.kmg_apply_plan_destroy(None, 1)                               # (and destroying nothing is allowed)


@pytest.mark.parametrize("name", list(APPLY_CASES))
def test_dev_apply_refuses_and_accepts_the_neighbour(env, name):
    refused, accepted = APPLY_CASES[name]
    assert env.apply({**APPLY, **refused}) == (INV, APPLY_ARGS)
    assert env.apply({**APPLY, **accepted}) == (0, "")


# ---- the arena hand-back path, route by route
def formats_of(k, mode):
    return [RGBA8] + ([] if mode == MELD else ([INDEX8] if k <= 256 else []) + [INDEX16])


HAND_BACK = [(s, k, m, f) for s, k, m in ROUTES for f in formats_of(k, m)]
_palettes = {}


def _centroids(kg, k):
    if k not in _palettes:
        rng = np.random.default_rng(k)
        rgb = rng.choice(1 << 24, k, replace=False).astype(np.uint32) | np.uint32(0xFF000000)
        _palettes[k] = kg.palette_to_centroids(rgb.view(np.uint8).reshape(k, 4))
    return _palettes[k]


def _in_two_bands(env, cent, mode, fmt):
    L, st, px = env.L, env.stream, BYTES[fmt]
    env.d_out.fill_(0x5A)
    made = C.c_void_p()
    rc = L.kmg_apply_plan_create_format(env.procs[False]._h, cent.ctypes.data, cent.shape[0], mode, fmt, N, st, C.byref(made))
    assert rc == 0, env.message(rc)
    for r0, r1 in ((0, SPLIT), (SPLIT, H)):
        rc = L.kmg_apply_plan_run(made, env.d_in.data_ptr() + 4 * W * r0, W, r1 - r0, r0, env.d_out.data_ptr() + px * W * r0, st)
        assert rc == 0, env.message(rc)
    env.torch.cuda.current_stream().synchronize()
    rc = L.kmg_apply_plan_status(made)
    assert rc == 0, env.message(rc)
    L.kmg_apply_plan_destroy(made, 0)
    return env.d_out[:px * N].cpu().numpy().copy()


@pytest.mark.parametrize("strategy,k,mode,fmt", HAND_BACK)
def test_a_second_plan_on_the_block_the_first_gave_back(env, strategy, k, mode, fmt):
    set_strategy(strategy)
    cent = _centroids(env.kg, k)
    first = _in_two_bands(env, cent, mode, fmt)
    second = _in_two_bands(env, cent, mode, fmt)
    env.d_out.fill_(0x5A)
    rc = env.L.kmg_dev_apply_format(env.procs[False]._h, env.d_in.data_ptr(), W, H, 0, cent.ctypes.data, k, mode, fmt, env.d_out.data_ptr(),
                                    env.stream)
    assert rc == 0, env.message(rc)
    whole = env.d_out[:BYTES[fmt] * N].cpu().numpy()
    assert np.array_equal(second, first), "the second plan's bytes differ from the first's"
    assert np.array_equal(second, whole), "the plans' bytes differ from kmg_dev_apply's"
    if fmt != RGBA8:
        assert int(whole.view(np.uint8 if fmt == INDEX8 else np.uint16).max()) < k
