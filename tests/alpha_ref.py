"""Test-side reference of alpha mode (kmg_options.alpha_cutoff; the contract is in include/kmeans_hip.h at kmg_options), built only
from the oracle's wrappers (tests/oracle_lib.py) and numpy.

A pixel is kept when its alpha byte is >= t.  The palette step shrinks as the default call does, keeps the kept pixels of the
shrunk image in raster order and runs the default pipeline on them as an image of n_kept x 1 pixels (the shrunk image itself when
every pixel is kept).  The outputs are the default mode's bytes with the input's alpha; KMG_MODE_DIFFUSE leaves excluded pixels
out of the diffusion (`diffuse`, restated from tests/diffuse_ref.py with the exclusion rule; `diffuse_serial` is the literal
raster loop)."""
import numpy as np

import diffuse_ref

MODE_DIFFUSE = 3


def shrink(oracle, rgba, max_dim):
    h, w = rgba.shape[:2]
    if max_dim and (w > max_dim or h > max_dim):
        nw, nh = oracle.resized_dims(w, h, max_dim)
        return oracle.resize(rgba, nw, nh)
    return np.ascontiguousarray(rgba)


def kept_pixels(rgba, t):
    """(pixels, width, height) of the image the pipeline sees: the kept pixels in raster order as n_kept x 1, or the image itself
    when every pixel is kept; None when none is"""
    h, w = rgba.shape[:2]
    keep = rgba[..., 3] >= t
    n_kept = int(keep.sum())
    if n_kept == 0:
        return None
    if n_kept == w * h:
        return rgba.reshape(-1, 4), w, h
    return np.ascontiguousarray(rgba[keep]), n_kept, 1


def kmeans_centroids(oracle, rgba, k, t, shrink_max_dim=256):
    """the k x 4 centroid table of the k-means palette step; None: no pixel is kept"""
    got = kept_pixels(shrink(oracle, rgba, shrink_max_dim), t)
    if got is None:
        return None
    px, w, h = got
    lab = oracle.rgb_to_lab(px)
    cent = oracle.init_centroids(lab, w, h, k)
    cent, _, _ = oracle.lloyd(lab, cent)
    return cent


def sorted_by_L(oracle, colours):
    """lib.rs:255-286: ascending palette-crate Lab L of the 8-bit colour, stable"""
    L = [float(oracle.palette_srgb8_to_lab(c[:3])[0]) for c in colours]
    order = sorted(range(len(colours)), key=lambda i: L[i])
    return np.ascontiguousarray(colours[order], np.uint8).reshape(-1, 4)


def palette_kmeans(oracle, rgba, k, t, shrink_max_dim=256):
    cent = kmeans_centroids(oracle, rgba, k, t, shrink_max_dim)
    if cent is None:
        return None
    pal = np.full((k, 4), 255, np.uint8)
    for j in range(k):
        pal[j, :3] = oracle.palette_lab_to_srgb8(cent[j, :3])
    return sorted_by_L(oracle, pal)


def palette_octree(oracle, rgba, k, t):
    got = kept_pixels(shrink(oracle, rgba, 128), t)
    if got is None:
        return None
    return sorted_by_L(oracle, oracle.octree_palette(got[0], k))


def with_alpha(out, rgba):
    out = np.array(out, np.uint8)
    out[..., 3] = rgba[..., 3]
    return out


def diffuse(rgba, replace, t, nearest=None):
    """KMG_MODE_DIFFUSE in alpha mode, by anti-diagonals as diffuse_ref.diffuse: an excluded pixel has S = 0 and e = 0"""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    near = nearest if nearest is not None else diffuse_ref.Nearest(replace)
    src = rgba[..., :3].astype(np.int32)
    kept = rgba[..., 3] >= t
    err = np.zeros((h + 1, w + 2, 3), np.int32)
    out = np.empty((h, w, 4), np.uint8)
    out[..., 3] = rgba[..., 3]
    for d in range(w + 2 * (h - 1)):
        y = np.arange(max(0, (d - w + 2) // 2), min(h - 1, d // 2) + 1)
        x = d - 2 * y
        ok = (x >= 0) & (x < w)
        y, x = y[ok], x[ok]
        if y.size == 0:
            continue
        kp = kept[y, x][:, None]
        S = np.where(kp, 7 * err[y + 1, x] + 3 * err[y, x + 2] + 5 * err[y, x + 1] + err[y, x], 0)
        v = 16 * src[y, x] + ((S + 8) >> 4)
        tq = np.clip(v, 0, 4080)
        c = (tq + 8) >> 4
        o = near(c[:, 0].astype(np.int64) | (c[:, 1].astype(np.int64) << 8) | (c[:, 2].astype(np.int64) << 16))
        ob = np.stack([o & 255, (o >> 8) & 255, (o >> 16) & 255], axis=1).astype(np.int32)
        out[y, x, :3] = ob
        err[y + 1, x + 1] = np.where(kp, tq - 16 * ob, 0)
    return out


def diffuse_serial(rgba, replace, t):
    """the exclusion rule as written: raster order, one pixel and one channel at a time"""
    rgba = np.asarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    near = diffuse_ref.Nearest(replace)
    e = [[(0, 0, 0)] * w for _ in range(h)]

    def E(x, y, ch):
        return e[y][x][ch] if 0 <= x < w and 0 <= y < h else 0

    out = np.empty((h, w, 4), np.uint8)
    for y in range(h):
        for x in range(w):
            keep = int(rgba[y, x, 3]) >= t
            ts = []
            for ch in range(3):
                S = 7 * E(x - 1, y, ch) + 3 * E(x + 1, y - 1, ch) + 5 * E(x, y - 1, ch) + 1 * E(x - 1, y - 1, ch) if keep else 0
                v = 16 * int(rgba[y, x, ch]) + ((S + 8) >> 4)
                ts.append(min(max(v, 0), 4080))
            c = [(tq + 8) >> 4 for tq in ts]
            o = int(near(np.array([c[0] | (c[1] << 8) | (c[2] << 16)], np.int64))[0])
            ob = (o & 255, (o >> 8) & 255, (o >> 16) & 255)
            out[y, x] = (ob[0], ob[1], ob[2], rgba[y, x, 3])
            e[y][x] = tuple(ts[ch] - 16 * ob[ch] for ch in range(3)) if keep else (0, 0, 0)
    return out


def apply(oracle, rgba, cent4, mode, t):
    """kmg_dev_apply / the output step of kmg_reduce for a centroid table"""
    if mode == MODE_DIFFUSE:
        return diffuse(rgba, diffuse_ref.oracle_apply_replace(oracle, cent4), t)
    return with_alpha(oracle.apply(rgba, cent4, mode), rgba)


def find(oracle, rgba, palette_rgba, mode, t):
    if mode == MODE_DIFFUSE:
        return diffuse(rgba, diffuse_ref.oracle_find_replace(oracle, palette_rgba), t)
    return with_alpha(oracle.find(rgba, palette_rgba, mode), rgba)


def reduce_kmeans(oracle, rgba, k, mode, t):
    cent = kmeans_centroids(oracle, rgba, k, t)
    return None if cent is None else apply(oracle, rgba, cent, mode, t)


def reduce_octree(oracle, rgba, k, mode, t):
    pal = palette_octree(oracle, rgba, k, t)
    return None if pal is None else find(oracle, rgba, pal, mode, t)


def compact(rgba, t):
    """kmg_dev_alpha_compact: the kept pixels in order"""
    px = np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)
    return px[px[:, 3] >= t]


# ---- test images ---------------------------------------------------------------------------------------------------------------
def soft_disc(rgba, soft=12.0):
    """rgba with alpha = a disc in the middle (opaque inside, a linear edge `soft` pixels wide, transparent outside)"""
    h, w = rgba.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    r = np.hypot(x - (w - 1) / 2.0, y - (h - 1) / 2.0)
    R = 0.4 * min(w, h)
    a = np.clip((R + soft / 2 - r) / soft, 0.0, 1.0)
    out = np.array(rgba, np.uint8)
    out[..., 3] = np.rint(255.0 * a).astype(np.uint8)
    return out


def sprite(h=72, w=96, seed=5):
    """a sprite-like image on a (0, 0, 0, 0) background: a few opaque shapes in flat and shaded colours, half-transparent edges"""
    rng = np.random.default_rng(seed)
    out = np.zeros((h, w, 4), np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    for _ in range(6):
        cy, cx = rng.integers(8, h - 8), rng.integers(8, w - 8)
        ry, rx = rng.integers(4, 14), rng.integers(4, 18)
        d = ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2
        col = rng.integers(0, 256, 3)
        inside = d <= 1.0
        shade = np.clip(1.0 - 0.4 * d, 0.0, 1.0)[..., None]
        out[inside, :3] = np.clip(col * shade[inside] + rng.integers(-6, 7, (int(inside.sum()), 3)), 0, 255).astype(np.uint8)
        out[inside, 3] = 255
        edge = (d > 1.0) & (d <= 1.3) & (out[..., 3] == 0)
        out[edge, :3] = col.astype(np.uint8)
        out[edge, 3] = 128
    return out
