"""A palette-mode APNG writer for the frame output of a Sequence (include/kmeans_hip.h at kmg_sequence_output_frame): zlib and struct
only.

The file is a PNG of colour type 3 whose PLTE holds the k palette colours and one more entry, the transparent slot k (tRNS: 255 for
the colours, 0 for the slot), followed by the animation chunks of the APNG specification: acTL, then per frame one fcTL and the
frame's pixels (IDAT for the first frame, fdAT after it).
  - a delta frame carries the rectangle of its changes only, dispose_op NONE and blend_op OVER: index k keeps what is shown;
  - a full frame carries the whole canvas with blend_op SOURCE (so does the first frame, whose delta against the empty canvas is
    the full map anyway, and which the format wants to cover the canvas);
  - a frame in which nothing changed is a 1 x 1 region at (0, 0) holding the transparent index.
"""
import struct
import zlib

import numpy as np

_SIGNATURE = b"\x89PNG\r\n\x1a\n"
DISPOSE_NONE, BLEND_SOURCE, BLEND_OVER = 0, 0, 1


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _scanlines(region):
    """filter type 0 in front of every row, deflated"""
    h, w = region.shape
    rows = np.zeros((h, w + 1), np.uint8)
    rows[:, 1:] = region
    return zlib.compress(rows.tobytes(), 9)


def encode(palette, width, height, frames, delay_ms=100, loops=0):
    """The bytes of the APNG.  palette: (k, 4) or (k, 3) uint8, k <= 255.  frames: (map, rect, is_full) per frame -- map a
    (height, width) uint8 array of indices (k = transparent), rect = (x0, y0, x1, y1) of the changes or None when nothing changed
    (FrameDelta.rect), is_full true for a map that replaces the canvas."""
    pal = np.ascontiguousarray(palette, np.uint8)
    pal = pal.reshape(-1, pal.shape[-1])[:, :3]
    k = pal.shape[0]
    if not 1 <= k <= 255:
        raise ValueError(f"a palette-mode APNG with a transparent slot holds 1 .. 255 colours, not {k}")
    frames = list(frames)
    if not frames:
        raise ValueError("no frames")
    delay_ms = int(delay_ms)
    if not 0 <= delay_ms <= 0xFFFF:
        raise ValueError("delay_ms must be 0 .. 65535")
    plte = np.zeros((k + 1, 3), np.uint8)
    plte[:k] = pal
    out = [_SIGNATURE,
           _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 3, 0, 0, 0)),
           _chunk(b"PLTE", plte.tobytes()),
           _chunk(b"tRNS", bytes([255] * k + [0])),
           _chunk(b"acTL", struct.pack(">II", len(frames), int(loops)))]
    seq = 0
    for i, (index, rect, is_full) in enumerate(frames):
        index = np.ascontiguousarray(index)
        if index.dtype != np.uint8 or index.shape != (height, width):
            raise ValueError("every frame is a (height, width) uint8 index map")
        if is_full or i == 0:
            x0, y0, x1, y1, blend, region = 0, 0, width, height, BLEND_SOURCE, index
        elif rect is None:
            x0, y0, x1, y1, blend, region = 0, 0, 1, 1, BLEND_OVER, np.full((1, 1), k, np.uint8)
        else:
            x0, y0, x1, y1 = (int(v) for v in rect)
            if not (0 <= x0 < x1 <= width and 0 <= y0 < y1 <= height):
                raise ValueError(f"rectangle {rect} is not inside the {width} x {height} canvas")
            blend, region = BLEND_OVER, index[y0:y1, x0:x1]
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, x1 - x0, y1 - y0, x0, y0, delay_ms, 1000, DISPOSE_NONE, blend)))
        seq += 1
        data = _scanlines(region)
        if i == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    return b"".join(out)


def write(path, palette, width, height, frames, delay_ms=100, loops=0):
    with open(path, "wb") as f:
        f.write(encode(palette, width, height, frames, delay_ms, loops))
