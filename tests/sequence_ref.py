"""Test-side reference of frame sequences (include/kmeans_hip.h at kmg_sequence), built only from the oracle's wrappers
(tests/oracle_lib.py), alpha_ref.shrink / kept_pixels and numpy.

  working_sequence   W = K_0 || K_1 || ... and the image dimensions the pipeline sees it with
  centroids          the default pipeline on W: oracle.rgb_to_lab, init_centroids, lloyd with the processor's loop parameters
  delta / delta_loop the delta rule, vectorised and as the literal per-pixel loop
  combine            two records into one (sums added, minima minned, maxima maxed)
  replay             a compositor: delta maps blended "over" (index k keeps the pixel), full maps as "source"
"""
import numpy as np

import alpha_ref

FRESH = (0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0)


def working_sequence(oracle, frames, t=0, shrink_max_dim=256):
    """(pixels (n, 4), width, height), or None when no pixel is kept"""
    parts, first = [], None
    for i, f in enumerate(frames):
        S = alpha_ref.shrink(oracle, np.ascontiguousarray(f, np.uint8), shrink_max_dim)
        got = alpha_ref.kept_pixels(S, t) if t else (S.reshape(-1, 4), S.shape[1], S.shape[0])
        K = np.zeros((0, 4), np.uint8) if got is None else got[0]
        if i == 0:
            first = (S.shape[1], S.shape[0], K.shape[0] == S.shape[0] * S.shape[1])
        parts.append(K)
    W = np.ascontiguousarray(np.concatenate(parts, axis=0)) if parts else np.zeros((0, 4), np.uint8)
    if W.shape[0] == 0:
        return None
    if len(frames) == 1 and first[2]:
        return W, first[0], first[1]
    return W, W.shape[0], 1


def centroids(oracle, frames, k, t=0, shrink_max_dim=256, max_iterations=128, check_period=8, convergence=1.0):
    """the k x 4 centroid table of the sequence, in the Lloyd loop's order; None: no pixel is kept"""
    got = working_sequence(oracle, frames, t, shrink_max_dim)
    if got is None:
        return None
    W, w, h = got
    lab = oracle.rgb_to_lab(W)
    cent = oracle.init_centroids(lab, w, h, k)
    cent, _, _ = oracle.lloyd(lab, cent, max_iterations=max_iterations, check_period=check_period, convergence=convergence)
    return cent


def sorted_palette(oracle, cent):
    """kmg_sequence_palette: the palette crate's bytes of the centroids, sorted as kmg_palette sorts"""
    pal = np.full((cent.shape[0], 4), 255, np.uint8)
    for j in range(cent.shape[0]):
        pal[j, :3] = oracle.palette_lab_to_srgb8(cent[j, :3])
    return alpha_ref.sorted_by_L(oracle, pal)


def delta(index, canvas, k, row0=0):
    """(delta map, new canvas, record) of a band whose first row is image row row0"""
    index, canvas = np.asarray(index), np.asarray(canvas)
    ch = index != canvas
    d = np.where(ch, index, np.asarray(k, index.dtype)).astype(index.dtype)
    n = int(ch.sum())
    if n == 0:
        return d, index.copy(), FRESH
    ys, xs = np.nonzero(ch)
    rec = (n, int((ch & (index == k)).sum()), int(xs.min()), row0 + int(ys.min()), int(xs.max()) + 1, row0 + int(ys.max()) + 1)
    return d, index.copy(), rec


def delta_loop(index, canvas, k, row0=0):
    """the rule as written: one pixel at a time"""
    index, canvas = np.asarray(index), np.array(canvas)
    rows, width = index.shape
    d = np.empty_like(index)
    changed, cleared, x0, y0, x1, y1 = FRESH
    for r in range(rows):
        for x in range(width):
            c, v = int(index[r, x]), int(canvas[r, x])
            if c == v:
                d[r, x] = k
            else:
                d[r, x] = c
                changed += 1
                x0, y0 = min(x0, x), min(y0, row0 + r)
                x1, y1 = max(x1, x + 1), max(y1, row0 + r + 1)
                if c == k:
                    cleared += 1
            canvas[r, x] = c
    return d, canvas, (changed, cleared, x0, y0, x1, y1)


def combine(a, b):
    return (a[0] + b[0], a[1] + b[1], min(a[2], b[2]), min(a[3], b[3]), max(a[4], b[4]), max(a[5], b[5]))


def composite(canvas, frame_map, k, is_full):
    """one frame over the canvas: "source" for a full map, "over" for a delta map (index k is transparent)"""
    frame_map = np.asarray(frame_map)
    return frame_map.copy() if is_full else np.where(frame_map == k, canvas, frame_map).astype(frame_map.dtype)


def replay(coded, k):
    """what a viewer shows after every frame of [(map, is_full), ...], from a canvas of k"""
    shown, canvas = [], None
    for frame_map, is_full in coded:
        if canvas is None:
            canvas = np.full_like(np.asarray(frame_map), k)
        canvas = composite(canvas, frame_map, k, is_full)
        shown.append(canvas)
    return shown


def encode_sequence(full_maps, k, honour_cleared=True):
    """[(map, record, is_full), ...] as kmg_sequence_output_frame with KMG_FRAME_DELTA codes the full maps I_t"""
    out, canvas = [], None
    for I in full_maps:
        I = np.asarray(I)
        if canvas is None:
            canvas = np.full_like(I, k)
        d, canvas, rec = delta(I, canvas, k)
        full = honour_cleared and rec[1] > 0
        out.append((I.copy() if full else d, rec, full))
    return out
