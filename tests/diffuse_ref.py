"""Test-side reference of KMG_MODE_DIFFUSE (the contract in include/kmeans_hip.h at kmg_reduce_mode).

`diffuse(rgba, replace)` evaluates the contract by anti-diagonals d = x + 2 y: the four predecessors of a pixel lie on d - 1 (left,
above-right), d - 2 (above) and d - 3 (above-left), so every diagonal is one numpy step.  `replace(colours)` maps an (m, 4) array
of opaque colours to the bytes the replace mode writes for them; `Nearest` wraps one, asks it only for colours not seen before
(in batches) and remembers the answers in a 2^24 table.  `diffuse_serial` is the literal raster loop in plain Python."""
import numpy as np


class Nearest:
    def __init__(self, replace):
        self.replace = replace
        self.table = np.full(1 << 24, -1, np.int64)

    def __call__(self, codes):
        """codes: int array of r | g << 8 | b << 16 -> uint32 output words (alpha 255)"""
        got = self.table[codes]
        miss = got < 0
        if miss.any():
            new = np.unique(codes[miss])
            px = np.empty((new.size, 4), np.uint8)
            px[:, 0] = new & 255; px[:, 1] = (new >> 8) & 255; px[:, 2] = (new >> 16) & 255; px[:, 3] = 255
            o = np.ascontiguousarray(self.replace(px)).reshape(-1, 4).astype(np.int64)
            self.table[new] = o[:, 0] | (o[:, 1] << 8) | (o[:, 2] << 16) | (255 << 24)
            got = self.table[codes]
        return got


def oracle_find_replace(oracle, palette_rgba):
    """replace(colours) of kmg_find: the oracle's own replace pass with the palette"""
    return lambda px: oracle.find(px.reshape(1, -1, 4), palette_rgba, oracle.MODE_REPLACE)


def oracle_apply_replace(oracle, cent4):
    """replace(colours) for a centroid table (kmg_reduce: the palette the k-means or octree pass found)"""
    return lambda px: oracle.apply(px.reshape(1, -1, 4), cent4, oracle.MODE_REPLACE)


def diffuse(rgba, replace, nearest=None):
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    near = nearest if nearest is not None else Nearest(replace)
    src = rgba[..., :3].astype(np.int32)
    err = np.zeros((h + 1, w + 2, 3), np.int32)             # e(x, y) at [y + 1, x + 1]; the border stays 0
    out = np.empty((h, w, 4), np.uint8)
    out[..., 3] = 255
    for d in range(w + 2 * (h - 1)):
        y = np.arange(max(0, (d - w + 2) // 2), min(h - 1, d // 2) + 1)
        x = d - 2 * y
        keep = (x >= 0) & (x < w)
        y, x = y[keep], x[keep]
        if y.size == 0:
            continue
        S = 7 * err[y + 1, x] + 3 * err[y, x + 2] + 5 * err[y, x + 1] + err[y, x]
        v = 16 * src[y, x] + ((S + 8) >> 4)
        t = np.clip(v, 0, 4080)
        c = (t + 8) >> 4
        o = near(c[:, 0].astype(np.int64) | (c[:, 1].astype(np.int64) << 8) | (c[:, 2].astype(np.int64) << 16))
        ob = np.stack([o & 255, (o >> 8) & 255, (o >> 16) & 255], axis=1).astype(np.int32)
        out[y, x, :3] = ob
        err[y + 1, x + 1] = t - 16 * ob
    return out


def diffuse_serial(rgba, replace):
    """the contract as written: raster order, one pixel and one channel at a time"""
    rgba = np.asarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    near = Nearest(replace)
    e = [[(0, 0, 0)] * w for _ in range(h)]

    def E(x, y, ch):
        return e[y][x][ch] if 0 <= x < w and 0 <= y < h else 0

    out = np.empty((h, w, 4), np.uint8)
    for y in range(h):
        for x in range(w):
            ts = []
            for ch in range(3):
                S = 7 * E(x - 1, y, ch) + 3 * E(x + 1, y - 1, ch) + 5 * E(x, y - 1, ch) + 1 * E(x - 1, y - 1, ch)
                v = 16 * int(rgba[y, x, ch]) + ((S + 8) >> 4)
                ts.append(min(max(v, 0), 4080))
            c = [(t + 8) >> 4 for t in ts]
            o = int(near(np.array([c[0] | (c[1] << 8) | (c[2] << 16)], np.int64))[0])
            ob = (o & 255, (o >> 8) & 255, (o >> 16) & 255)
            out[y, x] = (ob[0], ob[1], ob[2], 255)
            e[y][x] = tuple(ts[ch] - 16 * ob[ch] for ch in range(3))
    return out
