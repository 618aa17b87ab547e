"""A small GIF89a writer for index maps with a palette per frame (Sequence.frame_local): no global colour table, and per frame a
graphic control extension (delay, transparent index, disposal) and an image descriptor with a LOCAL colour table.  Only `struct`
and numpy.

A frame is a dict:
  indices      (height, width) uint8 map of the whole canvas; index k (and anything above) is transparent
  palette      (k, 3) or (k, 4) uint8, the frame's own colours in index order (an alpha byte is ignored)
  rect         optional (x0, y0, x1, y1), x1 / y1 exclusive: only this part of the map is written -- a delta frame cropped to the box
               of its record; None: the whole canvas
  delay        hundredths of a second (default 10)
  disposal     1: the frame stays (delta frames), 2: its rectangle is cleared before the next one (default 1)
The local colour table has 2^ceil(log2(k + 1)) entries (at least 2), so index k always exists and is declared transparent.  The
pixel data is real variable-width LZW: codes grow from min_code_size + 1 to 12 bits, and a clear code is sent when the table fills."""
import struct

import numpy as np

MAX_K = 255


def table_bits(k):
    """the local colour table of a frame with k colours has 2^table_bits(k) entries"""
    bits = 1
    while (1 << bits) < k + 1:
        bits += 1
    return bits


def lzw_encode(pixels, min_code_size):
    """bytes of the LZW code stream (before it is cut into sub-blocks) of a sequence of indices < 2^min_code_size"""
    clear, end = 1 << min_code_size, (1 << min_code_size) + 1
    out = bytearray()
    acc = nbits = 0
    size, nxt, table = min_code_size + 1, end + 1, {}

    def emit(code):
        nonlocal acc, nbits
        acc |= code << nbits
        nbits += size
        while nbits >= 8:
            out.append(acc & 255)
            acc >>= 8
            nbits -= 8

    emit(clear)
    it = iter(pixels)
    prefix = next(it)
    for c in it:
        key = (prefix << 8) | c
        code = table.get(key)
        if code is not None:
            prefix = code
            continue
        emit(prefix)
        if nxt < 4096:
            table[key] = nxt
            nxt += 1
            if nxt - 1 == (1 << size):
                size += 1
        else:                                                          # the table is full: start over
            emit(clear)
            size, nxt, table = min_code_size + 1, end + 1, {}
        prefix = c
    emit(prefix)
    emit(end)
    if nbits:
        out.append(acc & 255)
    return bytes(out)


def _sub_blocks(data):
    out = bytearray()
    for i in range(0, len(data), 255):
        chunk = data[i:i + 255]
        out.append(len(chunk))
        out += chunk
    out.append(0)
    return bytes(out)


def encode(width, height, frames, loop=0):
    """the bytes of a GIF89a file; loop: repetitions of the animation (0: for ever, None: no looping extension)"""
    if not (0 < width < 65536 and 0 < height < 65536):
        raise ValueError(f"a GIF canvas is 1 .. 65535 pixels wide and high, not {width} x {height}")
    out = bytearray(b"GIF89a")
    out += struct.pack("<HHBBB", width, height, 0x70, 0, 0)            # no global colour table, 8 bits of colour resolution
    if loop is not None:
        out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    n = 0
    for fr in frames:
        n += 1
        pal = np.asarray(fr["palette"], np.uint8)
        pal = pal.reshape(-1, pal.shape[-1])[:, :3]
        k = pal.shape[0]
        if not 1 <= k <= MAX_K:
            raise ValueError(f"a GIF frame takes 1 .. {MAX_K} colours plus the transparent index, not {k}")
        idx = np.asarray(fr["indices"])
        if idx.shape != (height, width):
            raise ValueError(f"the map is {idx.shape[1]} x {idx.shape[0]}, the canvas {width} x {height}")
        x0, y0, x1, y1 = fr.get("rect") or (0, 0, width, height)
        if not (0 <= x0 < x1 <= width and 0 <= y0 < y1 <= height):
            raise ValueError(f"the rectangle {(x0, y0, x1, y1)} is empty or outside the canvas")
        disposal = int(fr.get("disposal", 1))
        if disposal not in (0, 1, 2, 3):
            raise ValueError(f"unknown disposal {disposal}")
        bits = table_bits(k)
        part = np.minimum(idx[y0:y1, x0:x1].astype(np.int64), k).astype(np.uint8)
        out += struct.pack("<BBBBHBB", 0x21, 0xF9, 4, (disposal << 2) | 1, int(fr.get("delay", 10)), k, 0)
        out += struct.pack("<BHHHHB", 0x2C, x0, y0, x1 - x0, y1 - y0, 0x80 | (bits - 1))
        table = np.zeros((1 << bits, 3), np.uint8)
        table[:k] = pal
        out += table.tobytes()
        mcs = max(2, bits)
        out.append(mcs)
        out += _sub_blocks(lzw_encode(part.tobytes(), mcs))
    if n == 0:
        raise ValueError("a GIF needs at least one frame")
    out.append(0x3B)
    return bytes(out)


def write(path, width, height, frames, loop=0):
    data = encode(width, height, frames, loop)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)
