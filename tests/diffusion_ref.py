"""Test-side reference of KMG_MODE_DIFFUSE for any filter of kmg_diffusion (the contract in include/kmeans_hip.h).

`diffuse(rgba, replace, weights, divisor)` evaluates the contract by anti-diagonals d = x + 3 y: a pixel's predecessors are
(x - dx, y - dy) with dy = 0, dx = 1, 2 (d - 1, d - 2), dy = 1, dx = -2 .. 2 (d - 1 .. d - 5) and dy = 2 (d - 4 .. d - 8), all on
earlier diagonals, so every diagonal is one numpy step.  `diffuse_serial` is the literal raster loop.  `keep` (h, w) bool is alpha
mode's mask: a pixel that is not kept has S = 0 and e = 0 (its output is the replace bytes of its own colour).  The nearest colours
come from diffuse_ref.Nearest, i.e. from whatever replace pass the caller hands over (the oracle's).  `weights` is
kmg_diffusion_weights' array: [0..1] row 0 (dx = +1, +2), [2..6] row 1, [7..11] row 2 (dx = -2 .. +2).

TABLE repeats the table of the header for the tests that check what the library returns; everything else takes the weights from
the library."""
import numpy as np

from diffuse_ref import Nearest

NAMES = ["floyd-steinberg", "sierra-lite", "atkinson", "burkes", "sierra2", "sierra3", "jarvis", "stucki"]
TABLE = [
    (16, [7, 0], [0, 3, 5, 1, 0], [0, 0, 0, 0, 0]),
    (4, [2, 0], [0, 1, 1, 0, 0], [0, 0, 0, 0, 0]),
    (8, [1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]),
    (32, [8, 4], [2, 4, 8, 4, 2], [0, 0, 0, 0, 0]),
    (16, [4, 3], [1, 2, 3, 2, 1], [0, 0, 0, 0, 0]),
    (32, [5, 3], [2, 4, 5, 4, 2], [0, 2, 3, 2, 0]),
    (48, [7, 5], [3, 5, 7, 5, 3], [1, 3, 5, 3, 1]),
    (42, [8, 4], [2, 4, 8, 4, 2], [1, 2, 4, 2, 1]),
]


def table_weights(filter):
    d, r0, r1, r2 = TABLE[filter]
    return np.array(r0 + r1 + r2, np.int32), d


def taps(weights):
    """[(dx, dy, weight)] of the non-zero entries"""
    w = [int(v) for v in weights]
    out = [(1, 0, w[0]), (2, 0, w[1])]
    out += [(dx, 1, w[4 + dx]) for dx in range(-2, 3)] + [(dx, 2, w[9 + dx]) for dx in range(-2, 3)]
    return [t for t in out if t[2]]


def diffuse(rgba, replace, weights, divisor, keep=None, nearest=None):
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    near = nearest if nearest is not None else Nearest(replace)
    tp, D = taps(weights), int(divisor)
    assert D % 2 == 0
    dxs = np.array([t[0] for t in tp], np.int64)[:, None]
    dys = np.array([t[1] for t in tp], np.int64)[:, None]
    wts = np.array([t[2] for t in tp], np.int64)[:, None, None]
    src = rgba[..., :3].astype(np.int64)
    err = np.zeros((h + 2, w + 4, 3), np.int64)             # e(x, y) at [y + 2, x + 2]; the border stays 0
    out = np.empty((h, w, 4), np.uint8)
    out[..., 3] = 255
    for d in range(w + 3 * (h - 1)):
        y_lo, y_hi = max(0, -(-(d - w + 1) // 3)), min(h - 1, d // 3)
        if y_lo > y_hi:
            continue
        y = np.arange(y_lo, y_hi + 1)
        x = d - 3 * y
        ok = (x >= 0) & (x < w)
        y, x = y[ok], x[ok]
        if y.size == 0:
            continue
        S = (wts * err[y + 2 - dys, x + 2 - dxs]).sum(0)     # (taps, pixels, 3) -> (pixels, 3)
        k = np.ones(y.size, bool) if keep is None else keep[y, x]
        S[~k] = 0
        v = 16 * src[y, x] + (S + D // 2) // D              # numpy's // on integers is the mathematical floor
        t = np.clip(v, 0, 4080)
        c = (t + 8) >> 4
        o = near(c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16))
        ob = np.stack([o & 255, (o >> 8) & 255, (o >> 16) & 255], axis=1)
        out[y, x, :3] = ob
        e = t - 16 * ob
        e[~k] = 0
        err[y + 2, x + 2] = e
    return out


def diffuse_serial(rgba, replace, weights, divisor, keep=None, nearest=None):
    """the contract as written: raster order, one pixel and one channel at a time"""
    rgba = np.asarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    near = nearest if nearest is not None else Nearest(replace)
    tp, D = taps(weights), int(divisor)
    e = [[(0, 0, 0)] * w for _ in range(h)]

    def E(x, y, ch):
        return e[y][x][ch] if 0 <= x < w and 0 <= y < h else 0

    out = np.empty((h, w, 4), np.uint8)
    for y in range(h):
        for x in range(w):
            kept = keep is None or bool(keep[y, x])
            ts = []
            for ch in range(3):
                S = sum(wt * E(x - dx, y - dy, ch) for dx, dy, wt in tp) if kept else 0
                v = 16 * int(rgba[y, x, ch]) + (S + D // 2) // D          # Python's // is the mathematical floor
                ts.append(min(max(v, 0), 4080))
            c = [(t + 8) >> 4 for t in ts]
            o = int(near(np.array([c[0] | (c[1] << 8) | (c[2] << 16)], np.int64))[0])
            ob = (o & 255, (o >> 8) & 255, (o >> 16) & 255)
            out[y, x] = (ob[0], ob[1], ob[2], 255)
            e[y][x] = tuple(ts[ch] - 16 * ob[ch] for ch in range(3)) if kept else (0, 0, 0)
    return out
