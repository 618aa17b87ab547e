"""Test-side reference of lossy delta frames (include/kmeans_hip.h at kmg_dev_frame_delta_lossy), built only from
error_ref.q_of / q_table (the oracle's Lab on the grid q = rint(64 Lab)) and numpy.

  distance          D(x, y) = dqL^2 + dqa^2 + dqb^2 over the R, G, B bytes of two RGBA8 arrays: exact integers
  hold / hold_loop  the rule, vectorised and as the literal per-pixel loop
  combine           two records into one (sums added, minima minned, maxima maxed)
  replay            an encoder and a viewer at once: exact and lossy frames over one canvas, with -- per pixel -- the number of the
                    frame that wrote it (whose exact index it shows)
  replay_from       the same from a caller's canvas and held source, with the full-on-clear rule as a switch

A record is 8 exact integers: changed, cleared, x0, y0, x1, y1, held, held_sse."""
import numpy as np

import error_ref

FRESH = (0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0, 0)
D_MAX = 347973309                       # the contract's bound on D of two sRGB8 colours


def distance(oracle, a, b, use_table=None):
    """(n,) int64: D of each pixel of a against the same pixel of b (both (..., 4) uint8; the alpha bytes are not looked at)"""
    a = np.ascontiguousarray(a, np.uint8).reshape(-1, 4)[:, :3]
    b = np.ascontiguousarray(b, np.uint8).reshape(-1, 4)[:, :3]
    assert a.shape == b.shape
    out = np.zeros(a.shape[0], np.int64)
    differs = (a != b).any(axis=1)                                   # equal bytes: D = 0 without a conversion
    if differs.any():
        if use_table is None:
            use_table = int(differs.sum()) > (1 << 19)
        dq = error_ref._q(oracle, a[differs], use_table) - error_ref._q(oracle, b[differs], use_table)
        out[differs] = (dq * dq).sum(axis=1)
    return out


def held_mask(oracle, src, index, canvas, held, k, tolerance, use_table=None):
    """(hold, D): which pixels of the band are held, and D(s, h) where it was needed (0 elsewhere)"""
    index, canvas = np.asarray(index), np.asarray(canvas)
    src, held = np.asarray(src, np.uint8), np.asarray(held, np.uint8)
    rows, width = index.shape
    holdable = (canvas != k) & (index != k)
    D = np.zeros(rows * width, np.int64)
    hb = holdable.reshape(-1)
    if hb.any():                                                     # (a pixel that cannot be held needs no D)
        D[hb] = distance(oracle, src.reshape(-1, 4)[hb], held.reshape(-1, 4)[hb], use_table)
    D = D.reshape(rows, width)
    return holdable & (D <= tolerance), D


def hold(oracle, src, index, canvas, held, k, tolerance, row0=0, use_table=None):
    """(delta map, new canvas, new held source, record) of a band whose first row is image row row0.
    src, held: (rows, width, 4) uint8; index, canvas: (rows, width)"""
    index, canvas = np.asarray(index), np.asarray(canvas)
    src, held = np.asarray(src, np.uint8), np.asarray(held, np.uint8)
    h, D = held_mask(oracle, src, index, canvas, held, k, tolerance, use_table)
    differs = index != canvas
    ch = ~h & differs
    d = np.where(ch, index, np.asarray(k, index.dtype)).astype(index.dtype)
    new_canvas = np.where(h, canvas, index).astype(index.dtype)
    new_held = np.where(h[..., None], held, src).astype(np.uint8)
    counted = h & differs
    n_held, sse = int(counted.sum()), int(D[counted].sum())
    n = int(ch.sum())
    if n == 0:
        return d, new_canvas, new_held, FRESH[:6] + (n_held, sse)
    ys, xs = np.nonzero(ch)
    rec = (n, int((ch & (index == k)).sum()), int(xs.min()), row0 + int(ys.min()), int(xs.max()) + 1, row0 + int(ys.max()) + 1, n_held, sse)
    return d, new_canvas, new_held, rec


def hold_loop(oracle, src, index, canvas, held, k, tolerance, row0=0):
    """the rule as written: one pixel at a time"""
    index, canvas, held = np.asarray(index), np.array(canvas), np.array(held, np.uint8)
    src = np.asarray(src, np.uint8)
    rows, width = index.shape
    d = np.empty_like(index)
    changed, cleared, x0, y0, x1, y1, n_held, sse = FRESH
    for r in range(rows):
        for x in range(width):
            c, v = int(index[r, x]), int(canvas[r, x])
            s, h = src[r, x], held[r, x]
            is_held = False
            if v != k and c != k:
                if (s[:3] == h[:3]).all():
                    D = 0
                else:
                    dq = error_ref.q_of(oracle, s[None])[0] - error_ref.q_of(oracle, h[None])[0]
                    D = int((dq * dq).sum())
                is_held = D <= tolerance
            if is_held:
                d[r, x] = k
                if c != v:
                    n_held += 1
                    sse += D
                continue
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
            held[r, x] = s
    return d, canvas, held, (changed, cleared, x0, y0, x1, y1, n_held, sse)


def combine(a, b):
    return (a[0] + b[0], a[1] + b[1], min(a[2], b[2]), min(a[3], b[3]), max(a[4], b[4]), max(a[5], b[5]), a[6] + b[6], a[7] + b[7])


def replay(oracle, frames, maps, k, tolerances, use_table=None):
    """kmg_sequence_output_frame (tolerance None: an exact delta frame) and kmg_sequence_output_frame_lossy over one open output,
    from a canvas of k.  frames: the sources (h, w, 4); maps: their exact index maps I_t.
    Returns one dict per frame: map (what the call writes), record (6 or 8 integers), is_full, canvas (what a viewer shows after
    the frame), held (the held source), origin (per pixel: the number of the frame that wrote it -- whose exact index it shows
    and whose source is its held source; -1: none yet)"""
    if not len(maps):
        return []
    return replay_from(oracle, np.full_like(np.asarray(maps[0]), k), np.zeros_like(np.asarray(frames[0], np.uint8)), frames, maps, k, tolerances,
                       True, use_table)


def replay_from(oracle, canvas, held, frames, maps, k, tolerances, full_on_clear=True, use_table=None):
    """the same rule from a caller's canvas (h, w) and held source (h, w, 4), neither of which is modified; full_on_clear False: no
    frame is sent in full, a frame that clears a pixel leaves what the pass itself leaves (kmg_dev_frame_delta_clip without
    KMG_CLIP_FULL_ON_CLEAR)"""
    import sequence_ref
    canvas, held = np.array(canvas), np.array(held, np.uint8)
    out, origin = [], np.full(canvas.shape, -1, np.int64)
    for t, (f, I, tol) in enumerate(zip(frames, maps, tolerances)):
        f, I = np.asarray(f, np.uint8), np.asarray(I)
        if tol is None:
            d, _, rec = sequence_ref.delta(I, canvas, k)
            sent = np.ones(I.shape, bool)                            # an exact frame leaves the canvas equal to its map everywhere
            canvas, held = I.copy(), f.copy()
        else:
            sent = ~held_mask(oracle, f, I, canvas, held, k, tol, use_table)[0]   # written now: the exact index, anchored at this frame
            d, canvas, held, rec = hold(oracle, f, I, canvas, held, k, tol, use_table=use_table)
        full = bool(full_on_clear) and rec[1] > 0
        if full:                                                     # "over" cannot show a pixel that turns transparent
            canvas, held, sent = I.copy(), f.copy(), np.ones(I.shape, bool)
        origin = np.where(sent, t, origin)
        out.append({"map": I.copy() if full else d, "record": rec, "is_full": full, "canvas": canvas.copy(), "held": held.copy(),
                    "origin": origin.copy()})
    return out
