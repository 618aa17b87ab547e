"""Test-side reference of KMG_MODE_DITHER with a threshold map (include/kmeans_hip.h at kmg_dither_map), built from the oracle's own
pieces: Lab from oracle_lib.rgb_to_lab, the threshold from oracle_lib.dither_threshold, the offsets in np.float32 as the contract
writes them (v = level / n_levels - 0.5, t = threshold * strength, off = t * v: one rounding each), and the labels from
oracle_lib.assign over the table [sentinel (10000, 10000, 10000), c_0 .. c_(k-1)]: label 0 maps to k and label j to j - 1.  The
sentinel stands first, so it keeps ties as the strict `<` of mix_colors.wgsl:73-80 does.  k = 1: all zeros (the mode is replace).

With the reference's matrix, n_levels = 16 and strength 1 this equals oracle_lib.dither label for label
(tests/test_dither_map_contract.py)."""
import numpy as np

BAYER4 = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.uint16)    # mix_colors.wgsl:14-17
SENTINEL = np.array([[10000.0, 10000.0, 10000.0, 1.0]], np.float32)


def bayer(side):
    """the Bayer recursion M2 = [[0, 2], [3, 1]], M2n = [[4M, 4M + 2], [4M + 3, 4M + 1]]"""
    m = np.array([[0, 2], [3, 1]], np.int64)
    while m.shape[0] < side:
        m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
    return m.astype(np.uint16)


def offsets(levels, n_levels, threshold, strength, w, h, row0=0):
    """off of every pixel of a w x h band whose first row is image row row0, float32 (h, w)"""
    levels = np.asarray(levels)
    mh, mw = levels.shape
    v = levels.astype(np.float32) / np.float32(n_levels) - np.float32(0.5)
    t = np.float32(threshold) * np.float32(strength)
    table = (t * v).astype(np.float32)
    ys = (np.arange(h) + row0) % mh
    xs = np.arange(w) % mw
    return table[ys[:, None], xs[None, :]]


def labels(oracle, rgba, cent4, levels, n_levels, strength=1.0, row0=0):
    """the label of every pixel, uint32 (h, w); k where the sentinel stays closest"""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    cent4 = oracle.centroids4(np.asarray(cent4, np.float32))
    k = cent4.shape[0]
    if k == 1:
        return np.zeros((h, w), np.uint32)
    lab = oracle.rgb_to_lab(rgba)
    off = offsets(levels, n_levels, oracle.dither_threshold(cent4), strength, w, h, row0).reshape(-1, 1)
    adjusted = (lab + off).astype(np.float32)
    table = np.concatenate([SENTINEL, cent4]).astype(np.float32)
    lab0 = oracle.assign(adjusted, table)
    return np.where(lab0 == 0, k, lab0 - 1).astype(np.uint32).reshape(h, w)


def palette_bytes(oracle, cent4):
    """the RGBA8 bytes the output pass writes per label: lab_to_rgb.wgsl of the k centroids, then of the sentinel"""
    cent4 = oracle.centroids4(np.asarray(cent4, np.float32))
    return oracle.lab_to_rgba8(np.concatenate([cent4[:, :3], SENTINEL[:, :3]]))


def rgba8(oracle, rgba, cent4, lab, alpha_cutoff=0):
    """the RGBA8 output for a label map: the palette bytes; alpha mode keeps the source's alpha byte"""
    out = palette_bytes(oracle, cent4)[lab]
    if alpha_cutoff:
        out[..., 3] = rgba[..., 3]
    return out


def index_map(rgba, lab, k, alpha_cutoff, dtype):
    """the index output for a label map: the label, k where alpha mode drops the pixel"""
    out = lab.copy()
    if alpha_cutoff:
        out[rgba[..., 3] < alpha_cutoff] = k
    return out.astype(dtype)
