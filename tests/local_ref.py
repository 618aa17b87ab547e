"""Test-side reference of per-frame palettes (include/kmeans_hip.h at kmg_dev_frame_delta_colour and
kmg_sequence_output_begin_local), built only from hold_ref.distance (the oracle's Lab on the grid q = rint(64 Lab)),
the oracle's wrappers and numpy.

  words / lookup            RGBA8 bytes as little-endian 32-bit words; p = P[c] for c < k, 0 otherwise
  colour / colour_loop      the exact rule, vectorised and as the literal per-pixel loop
  lossy / lossy_loop        the lossy rule, the same two ways
  combine                   two records into one (sums added, minima minned, maxima maxed)
  replay_colour             a compositor that decodes every coded frame through its own palette
  encode                    kmg_sequence_output_frame_local over one open output, from the frames' maps and palettes
  warm_centroids            the warm start: oracle.lloyd on the frame's working image from all k of C_{t-1}
  gif_decode                a minimal GIF89a reader with its own LZW decoder

The shown canvas is a (rows, width) uint32 array; a record is 6 (exact) or 8 (lossy) exact integers."""
import struct

import numpy as np

import hold_ref

FRESH6 = (0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0)
FRESH8 = FRESH6 + (0, 0)


def words(rgba):
    """(..., 4) uint8 -> (...) uint32, byte 0 in the low bits"""
    a = np.ascontiguousarray(rgba, np.uint8)
    return a.view("<u4").reshape(a.shape[:-1]).astype(np.uint32)


def unwords(w):
    """(...) uint32 -> (..., 4) uint8"""
    w = np.ascontiguousarray(w, "<u4")
    return w.view(np.uint8).reshape(w.shape + (4,))


def lookup(index, palette, k):
    """(c, p): the index with everything above k treated as k, and the word it shows (0 for c == k)"""
    table = np.concatenate([words(np.asarray(palette, np.uint8).reshape(-1, 4))[:k], np.zeros(1, np.uint32)])
    assert table.shape[0] == k + 1
    c = np.minimum(np.asarray(index).astype(np.int64), k)
    return c, table[c]


def _record(ch, p, row0, tail=()):
    n = int(ch.sum())
    if n == 0:
        return FRESH6 + tuple(tail)
    ys, xs = np.nonzero(ch)
    return (n, int((ch & (p == 0)).sum()), int(xs.min()), row0 + int(ys.min()), int(xs.max()) + 1, row0 + int(ys.max()) + 1) + tuple(tail)


def colour(index, shown, palette, k, row0=0):
    """(delta map, new shown, record) of a band whose first row is image row row0"""
    index, shown = np.asarray(index), np.asarray(shown, np.uint32)
    c, p = lookup(index, palette, k)
    ch = p != shown
    d = np.where(ch, c, k).astype(index.dtype)
    return d, p.copy(), _record(ch, p, row0)


def colour_loop(index, shown, palette, k, row0=0):
    """the rule as written: one pixel at a time"""
    index, shown = np.asarray(index), np.array(shown, np.uint32)
    pal = np.asarray(palette, np.uint8).reshape(-1, 4)
    rows, width = index.shape
    d = np.empty_like(index)
    changed, cleared, x0, y0, x1, y1 = FRESH6
    for r in range(rows):
        for x in range(width):
            c, v = int(index[r, x]), int(shown[r, x])
            p = int.from_bytes(bytes(pal[c]), "little") if c < k else 0
            if p == v:
                d[r, x] = k
            else:
                d[r, x] = c if c <= k else k
                changed += 1
                x0, y0 = min(x0, x), min(y0, row0 + r)
                x1, y1 = max(x1, x + 1), max(y1, row0 + r + 1)
                if p == 0:
                    cleared += 1
            shown[r, x] = p
    return d, shown, (changed, cleared, x0, y0, x1, y1)


def held_mask(oracle, src, index, shown, held, palette, k, tolerance, use_table=None):
    """(hold, D): which pixels of the band are held, and D(s, h) where it was needed (0 elsewhere)"""
    shown = np.asarray(shown, np.uint32)
    src, held = np.asarray(src, np.uint8), np.asarray(held, np.uint8)
    rows, width = shown.shape
    _, p = lookup(index, palette, k)
    holdable = (shown != 0) & (p != 0)
    D = np.zeros(rows * width, np.int64)
    hb = holdable.reshape(-1)
    if hb.any():
        D[hb] = hold_ref.distance(oracle, src.reshape(-1, 4)[hb], held.reshape(-1, 4)[hb], use_table)
    D = D.reshape(rows, width)
    return holdable & (D <= tolerance), D


def lossy(oracle, src, index, shown, held, palette, k, tolerance, row0=0, use_table=None):
    """(delta map, new shown, new held source, record)"""
    index, shown = np.asarray(index), np.asarray(shown, np.uint32)
    src, held = np.asarray(src, np.uint8), np.asarray(held, np.uint8)
    h, D = held_mask(oracle, src, index, shown, held, palette, k, tolerance, use_table)
    c, p = lookup(index, palette, k)
    differs = p != shown
    ch = ~h & differs
    d = np.where(ch, c, k).astype(index.dtype)
    new_shown = np.where(h, shown, p).astype(np.uint32)
    new_held = np.where(h[..., None], held, src).astype(np.uint8)
    counted = h & differs
    return d, new_shown, new_held, _record(ch, p, row0, (int(counted.sum()), int(D[counted].sum())))


def lossy_loop(oracle, src, index, shown, held, palette, k, tolerance, row0=0):
    """the rule as written: one pixel at a time"""
    import error_ref
    index, shown, held = np.asarray(index), np.array(shown, np.uint32), np.array(held, np.uint8)
    src = np.asarray(src, np.uint8)
    pal = np.asarray(palette, np.uint8).reshape(-1, 4)
    rows, width = index.shape
    d = np.empty_like(index)
    changed, cleared, x0, y0, x1, y1, n_held, sse = FRESH8
    for r in range(rows):
        for x in range(width):
            c, v = int(index[r, x]), int(shown[r, x])
            p = int.from_bytes(bytes(pal[c]), "little") if c < k else 0
            s, h = src[r, x], held[r, x]
            is_held = False
            if v != 0 and p != 0:
                if (s[:3] == h[:3]).all():
                    D = 0
                else:
                    dq = error_ref.q_of(oracle, s[None])[0] - error_ref.q_of(oracle, h[None])[0]
                    D = int((dq * dq).sum())
                is_held = D <= tolerance
            if is_held:
                d[r, x] = k
                if p != v:
                    n_held += 1
                    sse += D
                continue
            if p == v:
                d[r, x] = k
            else:
                d[r, x] = c if c <= k else k
                changed += 1
                x0, y0 = min(x0, x), min(y0, row0 + r)
                x1, y1 = max(x1, x + 1), max(y1, row0 + r + 1)
                if p == 0:
                    cleared += 1
            shown[r, x] = p
            held[r, x] = s
    return d, shown, held, (changed, cleared, x0, y0, x1, y1, n_held, sse)


def combine(a, b):
    out = (a[0] + b[0], a[1] + b[1], min(a[2], b[2]), min(a[3], b[3]), max(a[4], b[4]), max(a[5], b[5]))
    return out + tuple(x + y for x, y in zip(a[6:], b[6:]))


def replay_colour(coded, k):
    """what a viewer shows after every frame of [(map, palette, is_full), ...], as (h, w) uint32 words, from an empty canvas: each
    map is decoded through its own palette; a delta map goes "over" (index k keeps the pixel), a full map is the "source" """
    out, canvas = [], None
    for frame_map, palette, is_full in coded:
        frame_map = np.asarray(frame_map)
        if canvas is None:
            canvas = np.zeros(frame_map.shape, np.uint32)
        c, p = lookup(frame_map, palette, k)
        canvas = p.copy() if is_full else np.where(c == k, canvas, p).astype(np.uint32)
        out.append(canvas)
    return out


def encode(oracle, frames, maps, palettes, k, tolerances, deltas=None, use_table=None):
    """kmg_sequence_output_frame_local over one open output.  frames: the sources (h, w, 4); maps / palettes: each frame's own I_t
    and P_t; tolerances: None for an exact frame; deltas: False for a frame without KMG_FRAME_DELTA (default: all True).
    One dict per frame: map, record (8 integers), is_full, shown, held."""
    out, shown, held = [], None, None
    for t, (f, I, P, tol) in enumerate(zip(frames, maps, palettes, tolerances)):
        f, I = np.asarray(f, np.uint8), np.asarray(I)
        if shown is None:
            shown, held = np.zeros(I.shape, np.uint32), np.zeros_like(f)
        delta = True if deltas is None else deltas[t]
        if not delta:
            rec, full, d = FRESH8, True, None
            shown, held = lookup(I, P, k)[1], f.copy()
        elif tol is None:
            d, shown, rec = colour(I, shown, P, k)
            rec, held = rec + (0, 0), f.copy()
            full = rec[1] > 0
        else:
            d, shown, held, rec = lossy(oracle, f, I, shown, held, P, k, tol, use_table=use_table)
            full = rec[1] > 0
            if full:
                shown, held = lookup(I, P, k)[1], f.copy()
        out.append({"map": I.copy() if full else d, "record": rec, "is_full": full, "shown": shown.copy(), "held": held.copy()})
    return out


def warm_centroids(oracle, px, prev, max_iterations=128, check_period=8, convergence=1.0):
    """C_t of a warm frame: the Lloyd loop on the working image's pixels px (n, 4) from all k of C_{t-1} -- the seeds as
    fixed_ref.init_centroids places them (L, a, b of the seed, 1 in the fourth column), with no pick left to make"""
    lab = oracle.rgb_to_lab(np.ascontiguousarray(px, np.uint8).reshape(-1, 4))
    cent = np.ones((prev.shape[0], 4), np.float32)
    cent[:, :3] = np.asarray(prev, np.float32)[:, :3]
    cent, _, it = oracle.lloyd(lab, cent, max_iterations=max_iterations, check_period=check_period, convergence=convergence)
    return cent, it


# ---- a minimal GIF89a reader -------------------------------------------------------------------------------------------------------
def _lzw_decode(data, min_code_size, n_pixels):
    clear, end = 1 << min_code_size, (1 << min_code_size) + 1
    out = bytearray()
    table, size, prev = None, min_code_size + 1, None
    acc = nbits = pos = 0
    clears = 0
    while True:
        while nbits < size:
            if pos >= len(data):
                raise ValueError("LZW data ends without an end code")
            acc |= data[pos] << nbits
            nbits += 8
            pos += 1
        code = acc & ((1 << size) - 1)
        acc >>= size
        nbits -= size
        if code == clear:
            table = [bytes([i]) for i in range(clear)] + [b"", b""]
            size, prev = min_code_size + 1, None
            clears += 1
            continue
        if code == end:
            break
        if table is None:
            raise ValueError("LZW data does not start with a clear code")
        if prev is None:
            entry = table[code]
        elif code < len(table):
            entry = table[code]
            if len(table) < 4096:
                table.append(prev + entry[:1])
        elif code == len(table) and len(table) < 4096:
            entry = prev + prev[:1]
            table.append(entry)
        else:
            raise ValueError(f"LZW code {code} is not in the table")
        out += entry
        prev = entry
        if len(table) == (1 << size) and size < 12:
            size += 1
    if len(out) != n_pixels:
        raise ValueError(f"LZW data decodes to {len(out)} pixels, the image has {n_pixels}")
    return bytes(out), clears


def gif_decode(data):
    """{"width", "height", "global_table", "loop", "frames": [...]}; a frame is a dict of x, y, w, h, delay, disposal,
    transparent (index or None), table ((n, 3) uint8), indices ((h, w) uint8), clears (clear codes in its LZW data)"""
    if data[:6] != b"GIF89a":
        raise ValueError("not a GIF89a file")
    width, height, packed, _, _ = struct.unpack("<HHBBB", data[6:13])
    pos = 13
    out = {"width": width, "height": height, "global_table": None, "loop": None, "frames": []}
    if packed & 0x80:
        n = 2 << (packed & 7)
        out["global_table"] = np.frombuffer(data[pos:pos + 3 * n], np.uint8).reshape(n, 3).copy()
        pos += 3 * n
    gce = None

    def sub_blocks(pos):
        chunks = []
        while data[pos]:
            chunks.append(data[pos + 1:pos + 1 + data[pos]])
            pos += 1 + data[pos]
        return b"".join(chunks), pos + 1

    while True:
        kind = data[pos]
        pos += 1
        if kind == 0x3B:
            break
        if kind == 0x21:
            label = data[pos]
            body, pos = sub_blocks(pos + 1)
            if label == 0xF9:
                p, delay, tr = struct.unpack("<BHB", body[:4])
                gce = {"delay": delay, "disposal": (p >> 2) & 7, "transparent": tr if p & 1 else None}
            elif label == 0xFF and body[:11] == b"NETSCAPE2.0":
                out["loop"] = struct.unpack("<H", body[12:14])[0]
            continue
        if kind != 0x2C:
            raise ValueError(f"unknown block {kind:#x}")
        x, y, w, h, p = struct.unpack("<HHHHB", data[pos:pos + 9])
        pos += 9
        if p & 0x40:
            raise ValueError("interlaced images are not supported")
        table = None
        if p & 0x80:
            n = 2 << (p & 7)
            table = np.frombuffer(data[pos:pos + 3 * n], np.uint8).reshape(n, 3).copy()
            pos += 3 * n
        mcs = data[pos]
        body, pos = sub_blocks(pos + 1)
        px, clears = _lzw_decode(body, mcs, w * h)
        frame = {"x": x, "y": y, "w": w, "h": h, "table": table, "indices": np.frombuffer(px, np.uint8).reshape(h, w).copy(), "clears": clears}
        frame.update(gce or {"delay": 0, "disposal": 0, "transparent": None})
        out["frames"].append(frame)
        gce = None
    return out


def gif_canvases(decoded):
    """what a viewer shows after every frame, as (height, width) uint32 RGBA8 words (alpha 255 where something is shown, the word 0
    where nothing is): disposal 1 leaves the frame, disposal 2 clears its rectangle"""
    canvas = np.zeros((decoded["height"], decoded["width"]), np.uint32)
    out = []
    for fr in decoded["frames"]:
        table = fr["table"] if fr["table"] is not None else decoded["global_table"]
        rgba = np.concatenate([table, np.full((table.shape[0], 1), 255, np.uint8)], axis=1)
        p = words(rgba)[fr["indices"]]
        region = canvas[fr["y"]:fr["y"] + fr["h"], fr["x"]:fr["x"] + fr["w"]]
        keep = fr["indices"] == fr["transparent"] if fr["transparent"] is not None else np.zeros(p.shape, bool)
        region[...] = np.where(keep, region, p)
        out.append(canvas.copy())
        if fr["disposal"] == 2:
            region[...] = 0
    return out
