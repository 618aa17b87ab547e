"""A palette-mode PNG writer for optimised index maps (include/kmeans_hip.h at kmg_index_optimize): zlib and struct only.

The file is a PNG of colour type 3 at bit depth 1, 2, 4 or 8.  The rows are taken as kmg_dev_index_remap packs them -- every row
starts on a byte, the leftmost pixel in the high bits, padding bits zero -- which IS a filter-0 scanline without its filter byte:
the writer puts a zero in front of every row and deflates.  PLTE holds the colours; when the map has a transparent slot it is
entry 0 and tRNS is the one byte 0 (every later entry is opaque by default).
"""
import struct
import zlib

import numpy as np

from .apng import _SIGNATURE, _chunk


def encode(palette, width, height, rows, bits, transparent_first=False):
    """The bytes of the PNG.  palette: (n, 4) or (n, 3) uint8 in index order, n <= 2^bits; rows: (height, ceil(width * bits / 8))
    uint8 packed rows; transparent_first: entry 0 is the fully transparent slot."""
    if bits not in (1, 2, 4, 8):
        raise ValueError("a palette-mode PNG has bit depth 1, 2, 4 or 8")
    pal = np.ascontiguousarray(palette, np.uint8)
    pal = pal.reshape(-1, pal.shape[-1])[:, :3]
    if not 1 <= pal.shape[0] <= (1 << bits):
        raise ValueError(f"{pal.shape[0]} palette entries do not fit bit depth {bits}")
    stride = (int(width) * bits + 7) // 8
    rows = np.ascontiguousarray(rows)
    if rows.dtype != np.uint8 or rows.shape != (height, stride):
        raise ValueError(f"the rows of a {width} x {height} map at {bits} bits are a ({height}, {stride}) uint8 array")
    lines = np.zeros((height, stride + 1), np.uint8)            # filter type 0 in front of every row
    lines[:, 1:] = rows
    out = [_SIGNATURE,
           _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, bits, 3, 0, 0, 0)),
           _chunk(b"PLTE", pal.tobytes())]
    if transparent_first:
        out.append(_chunk(b"tRNS", b"\x00"))
    out += [_chunk(b"IDAT", zlib.compress(lines.tobytes(), 9)), _chunk(b"IEND", b"")]
    return b"".join(out)


def write(path, palette, width, height, rows, bits, transparent_first=False):
    with open(path, "wb") as f:
        f.write(encode(palette, width, height, rows, bits, transparent_first))
