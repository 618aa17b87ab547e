"""Test-side model of alpha-weighted k-means (kmg_processor_set_weighting, kmg_lloyd_set_weighting; the contract is in
include/kmeans_hip.h), built only from the oracle's wrappers (tests/oracle_lib.py) and numpy.

A pixel of the working image weighs its alpha byte a; it is kept iff a >= max(t, 1).  The initialisation is unweighted (alpha
mode's at that cutoff, the fixed colours first).  The Lloyd loop is the reference's with the sums (sum a q, sum a): oracle.assign,
a numpy weighted add of the per-pixel q that oracle.accumulate gives, oracle.finalize on the free rows, under the reference's check
rule.  `lloyd_replicated` is the contract's literal wording instead: oracle.lloyd on the list in which pixel i appears a_i times."""
import numpy as np

import alpha_ref
import fixed_ref


def cutoff(t):
    """the cutoff of the working image under weighting: a pixel of weight 0 is never kept"""
    return max(int(t), 1)


def pixel_q(oracle, lab):
    """(n, 3) int64: q = rint(Lab 2^20) of every pixel, as oracle.accumulate sums it (every pixel a cluster of its own)"""
    lab = np.ascontiguousarray(lab, np.float32).reshape(-1, 3)
    n = lab.shape[0]
    acc = oracle.accumulate(lab, np.arange(n, dtype=np.uint32), n)
    assert np.all(acc[:, 3] == 1)
    return np.ascontiguousarray(acc[:, :3])


def accumulate(q, a, labels, k):
    """(k, 4) int64: (sum a qL, sum a qa, sum a qb, sum a) per cluster"""
    a = np.asarray(a).astype(np.int64).reshape(-1)
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    acc = np.zeros((k, 4), np.int64)
    np.add.at(acc[:, :3], labels, q * a[:, None])
    np.add.at(acc[:, 3], labels, a)
    return acc


def lloyd(oracle, lab, a, cent4, f=0, max_iterations=128, check_period=8, convergence=1.0):
    """the weighted loop with rows [0, f) pinned: (centroids, labels, iterations)"""
    lab = np.ascontiguousarray(lab, np.float32).reshape(-1, 3)
    cent = np.array(cent4, np.float32).reshape(-1, 4).copy()
    k = cent.shape[0]
    q = pixel_q(oracle, lab)
    labels = oracle.assign(lab, cent)
    it = 0
    while it < max_iterations:
        cent, conv = fixed_ref.step(oracle, accumulate(q, a, labels, k), cent, f, convergence)
        labels = oracle.assign(lab, cent)
        if it > 0 and it % check_period == 0 and conv >= k:
            break
        it += 1
    return cent, labels, it if it < max_iterations else max_iterations - 1


def lloyd_replicated(oracle, lab, a, cent4, **loop):
    """the contract's wording: the default loop on the pixel list in which pixel i appears a_i times: (centroids, iterations)"""
    lab = np.ascontiguousarray(lab, np.float32).reshape(-1, 3)
    rep = np.repeat(lab, np.asarray(a).astype(np.int64).reshape(-1), axis=0)
    cent, _, it = oracle.lloyd(rep, cent4, **loop)
    return cent, it


def working_pixels(oracle, rgba, t, shrink_max_dim=256):
    """(pixels, width, height) of the working image of one frame -- alpha mode's at max(t, 1) -- or None when no pixel is kept"""
    return alpha_ref.kept_pixels(alpha_ref.shrink(oracle, rgba, shrink_max_dim), cutoff(t))


def centroids_of_working(oracle, px, w, h, k, colours=(), warm4=None, **loop):
    """the palette step on a working image (RGBA8 rows of `px`, weights in their alpha bytes): (centroids, labels, iterations).
    warm4: the loop starts from those k centroids instead of the initialisation (a warm per-frame palette)"""
    px = np.ascontiguousarray(px, np.uint8).reshape(-1, 4)
    lab = oracle.rgb_to_lab(px)
    pins = fixed_ref.pins_lab(oracle, colours)
    if warm4 is not None:
        cent, f = np.array(warm4, np.float32).reshape(-1, 4), 0
    elif pins.shape[0]:
        cent, f = fixed_ref.init_centroids(oracle, lab, w, h, k, pins), pins.shape[0]
    else:
        cent, f = oracle.init_centroids(lab, w, h, k), 0
    return lloyd(oracle, lab, px[:, 3], cent, f, **loop)


def kmeans_centroids(oracle, rgba, k, t, colours=(), warm4=None, shrink_max_dim=256, **loop):
    """the k x 4 centroid table of the weighted palette step of one image; None: no pixel is kept"""
    got = working_pixels(oracle, rgba, t, shrink_max_dim)
    if got is None:
        return None
    return centroids_of_working(oracle, got[0], got[1], got[2], k, colours, warm4, **loop)[0]


def sequence_centroids(oracle, frames, cutoffs, k, colours=(), shrink_max_dim=256, **loop):
    """the shared palette of a sequence: W = the working pixels of every frame, each cut at the cutoff in force at its add
    (`cutoffs`: the values alpha mode's compaction ran with; 0 = the whole frame), then the weighted loop on W"""
    parts, dims = [], []
    for f, c in zip(frames, cutoffs):
        s = alpha_ref.shrink(oracle, f, shrink_max_dim)
        kept = alpha_ref.compact(s, c)
        parts.append(kept)
        dims.append((s.shape[1], s.shape[0], kept.shape[0] == s.shape[0] * s.shape[1]))
    px = np.concatenate(parts)
    if px.shape[0] == 0:
        return None
    as_image = len(frames) == 1 and dims[0][2]
    w, h = (dims[0][0], dims[0][1]) if as_image else (px.shape[0], 1)
    return centroids_of_working(oracle, px, w, h, k, colours, **loop)[0]


def weighted_sprite(seed=11):
    """alpha_ref.sprite() with its opaque pixels given random alpha in 1 .. 255 (the half-transparent edges keep 128)"""
    img = alpha_ref.sprite()
    rng = np.random.default_rng(seed)
    opaque = img[..., 3] == 255
    img[opaque, 3] = rng.integers(1, 256, int(opaque.sum()), dtype=np.uint8)
    return img
