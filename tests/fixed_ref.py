"""Test-side model of fixed palette colours (kmg_processor_set_fixed_colors, kmg_lloyd_init_centroids_seeded, kmg_lloyd_set_fixed;
the contract is in include/kmeans_hip.h), built only from the oracle's wrappers (tests/oracle_lib.py: rgb_to_lab, cie94 per pair,
assign, accumulate, finalize) and numpy.

Seeded initialisation: the loop of orc_init_centroids with the picks of the first f centroids replaced by the seeds.  Pinned Lloyd
loop: orc_lloyd with `pick` applied to the free rows [f:] only; the pinned rows count as converged."""
import ctypes as C

import numpy as np


def pins_lab(oracle, colours):
    """P_j: the palette-crate Lab of each pinned colour -- the conversion of a `find` palette -- as (f, 4) float32 (L, a, b, 1)"""
    colours = np.asarray(colours, np.uint8) if len(colours) else np.zeros((0, 4), np.uint8)
    out = np.ones((colours.shape[0], 4), np.float32)
    for j in range(colours.shape[0]):
        out[j, :3] = oracle.palette_srgb8_to_lab(colours[j, :3])
    return out


def _distances(oracle, lab, c):
    """cie94(pixel_i, c) for every pixel, one orc_cie94 call per pair (pixel first: CIE94 is asymmetric)"""
    fn = oracle.lib().orc_cie94
    fp = C.POINTER(C.c_float)
    c = np.ascontiguousarray(c[:3], np.float32)
    pc = c.ctypes.data_as(fp)
    base = lab.ctypes.data
    out = np.empty(lab.shape[0], np.float32)
    for i in range(lab.shape[0]):
        out[i] = fn(C.cast(base + 12 * i, fp), pc)
    return out


def _argmax(dist):
    """the reference's arg-max: inside each block of 16 consecutive pixels the earliest maximum, folded from Candidate(0, 0.0);
    across blocks the last block that attains the largest block value"""
    n = dist.shape[0]
    best_i, best_d = 0, np.float32(0.0)
    for s0 in range(0, n, 16):
        l_i, l_d = 0, np.float32(0.0)
        for i in range(s0, min(s0 + 16, n)):
            if l_d < dist[i]:
                l_d, l_i = dist[i], i
        if not l_d < best_d:
            best_d, best_i = l_d, l_i
    return best_i


def _argmax_fast(dist):
    """_argmax with numpy (the same rule): per block np.argmax is the earliest maximum, a block of zeros names pixel 0"""
    n = dist.shape[0]
    pad = (-n) % 16
    d = np.concatenate([dist, np.full(pad, -1.0, np.float32)]).reshape(-1, 16)
    l_i = d.argmax(1) + 16 * np.arange(d.shape[0])
    l_d = d.max(1)
    l_i = np.where(l_d > 0, l_i, 0)
    l_d = np.maximum(l_d, np.float32(0.0))
    b = d.shape[0] - 1 - int(np.argmax(l_d[::-1]))              # the last block that attains the largest value
    return int(l_i[b])


def init_centroids(oracle, lab, w, h, k, seeds4):
    """(k, 4) float32: seeds in rows [0, f), farthest-point picks after them.  f = 0: c_0 is the reference's pixel pick."""
    lab = np.ascontiguousarray(lab, np.float32).reshape(-1, 3)
    seeds4 = np.asarray(seeds4, np.float32).reshape(-1, 4)
    f = seeds4.shape[0]
    assert f <= k and lab.shape[0] == w * h
    cent = np.ones((k, 4), np.float32)
    cent[:f, :3] = seeds4[:, :3]
    if f == 0:
        x0 = int(np.float32(w) * np.float32(0.5625))
        y0 = int(np.float32(h) * np.float32(0.93359375))
        cent[0, :3] = lab[y0 * w + x0]
    dist = np.full(lab.shape[0], 1000000.0, np.float32)
    for j in range(1, k):
        dist = np.fmin(dist, _distances(oracle, lab, cent[j - 1]))
        if j >= f:
            cent[j, :3] = lab[_argmax_fast(dist)]
    return cent


def step(oracle, acc, cent4, f, convergence=1.0):
    """one update from the sums `acc`: (new centroids, convergence count) -- `pick` on the free rows, f added to its count"""
    cent = np.array(cent4, np.float32).reshape(-1, 4).copy()
    k = cent.shape[0]
    n = 0
    if f < k:
        free, n = oracle.finalize(np.ascontiguousarray(acc[f:]), cent[f:], convergence)
        cent[f:] = free
    return cent, f + n


def lloyd(oracle, lab, cent4, f, max_iterations=128, check_period=8, convergence=1.0):
    """orc_lloyd with rows [0, f) pinned: (centroids, labels, iterations)"""
    lab = np.ascontiguousarray(lab, np.float32).reshape(-1, 3)
    cent = np.array(cent4, np.float32).reshape(-1, 4).copy()
    k = cent.shape[0]
    labels = oracle.assign(lab, cent)
    it = 0
    while it < max_iterations:
        acc = oracle.accumulate(lab, labels, k)
        cent, conv = step(oracle, acc, cent, f, convergence)
        labels = oracle.assign(lab, cent)
        if it > 0 and it % check_period == 0 and conv >= k:
            break
        it += 1
    return cent, labels, it if it < max_iterations else max_iterations - 1


def palette_centroids(oracle, px, w, h, k, colours, **loop):
    """the palette step on a working image of w x h pixels (RGBA8 rows of `px`) with the pinned colours: (centroids, iterations)"""
    lab = oracle.rgb_to_lab(px)
    pins = pins_lab(oracle, colours)
    cent = init_centroids(oracle, lab, w, h, k, pins)
    cent, _, it = lloyd(oracle, lab, cent, pins.shape[0], **loop)
    return cent, it


def palette_bytes(oracle, cent4):
    """the palette of the output pass in index order: lab_to_rgb.wgsl of every centroid"""
    return oracle.lab_to_rgba8(np.ascontiguousarray(np.asarray(cent4, np.float32)[:, :3]))
