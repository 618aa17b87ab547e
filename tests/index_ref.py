"""numpy reference of the index-map optimisation (include/kmeans_hip.h at kmg_dev_index_usage / kmg_index_plan / kmg_dev_index_remap;
DESIGN.md 4.13), written as the literal rules of the header: usage by np.bincount, the plan by a Python `sorted` with the tie keys,
remap and pack by a per-pixel loop (np.packbits as a second opinion at one bit)."""
import numpy as np

ORDER_KEEP, ORDER_USAGE, ORDER_LUMA = 0, 1, 2
KEEP_UNUSED, KEEP_TRANSPARENT, TRANSPARENT_FIRST = 4, 8, 16
ALL_FLAGS = 3 | KEEP_UNUSED | KEEP_TRANSPARENT | TRANSPARENT_FIRST
DROPPED = 0xFFFF
MAX_K = 3072


def usage(index, k):
    """the k + 2 counts: [i] pixels with index i, [k] the slot, [k + 1] every index above k"""
    v = np.minimum(np.asarray(index).reshape(-1).astype(np.int64), k + 1)
    return np.bincount(v, minlength=k + 2).astype(np.uint64)


def bits_of(n_slots):
    for b in (1, 2, 4, 8, 16):
        if (1 << b) >= n_slots:
            return b
    raise ValueError(n_slots)


def luma(rgba):
    return 2126 * int(rgba[0]) + 7152 * int(rgba[1]) + 722 * int(rgba[2])


def plan(use, palette, flags):
    """(remap (k + 1,) uint16, palette_out (n_slots, 4) uint8, (n_colors, n_slots, transparent, bits)), or None where the call
    refuses"""
    pal = np.asarray(palette, np.uint8).reshape(-1, 4)
    k = pal.shape[0]
    use = [int(u) for u in use]
    order = flags & 3
    if k == 0 or k > MAX_K or (flags & ~ALL_FLAGS) or order == 3 or use[k + 1] != 0:
        return None
    kept = [i for i in range(k) if use[i] > 0 or (flags & KEEP_UNUSED)]
    if order == ORDER_USAGE:
        kept = sorted(kept, key=lambda i: (-use[i], i))
    elif order == ORDER_LUMA:
        kept = sorted(kept, key=lambda i: (luma(pal[i]), i))
    present = use[k] > 0 or bool(flags & KEEP_TRANSPARENT)
    n_colors = len(kept)
    n_slots = n_colors + (1 if present else 0)
    if n_slots == 0:
        return None
    first = present and bool(flags & TRANSPARENT_FIRST)
    base = 1 if first else 0
    remap = np.full(k + 1, DROPPED, np.uint16)
    out = np.zeros((n_slots, 4), np.uint8)
    for new, old in enumerate(kept):
        remap[old] = base + new
        out[base + new] = pal[old]
    transparent = -1
    if present:
        transparent = 0 if first else n_colors
        remap[k] = transparent
    return remap, out, (n_colors, n_slots, transparent, bits_of(n_slots))


def remap(index, k, table, bits):
    """((height, width) new indices with bad pixels as 0, the number of bad pixels): pixel by pixel"""
    a = np.asarray(index)
    out = np.zeros(a.shape, np.uint16)
    bad = 0
    flat_in, flat_out = a.reshape(-1), out.reshape(-1)
    for i in range(flat_in.shape[0]):
        v = int(flat_in[i])
        m = int(table[v]) if v <= k else DROPPED
        if v > k or m == DROPPED or m >= (1 << bits):
            bad += 1
        else:
            flat_out[i] = m
    return out, bad


def remap_fast(index, k, table, bits):
    """the same with numpy indexing, for the large shapes (checked against remap() on the small ones)"""
    a = np.asarray(index).astype(np.int64)
    t = np.asarray(table).astype(np.int64)
    m = np.where(a <= k, t[np.minimum(a, k)], DROPPED)
    ok = (a <= k) & (m != DROPPED) & (m < (1 << bits))
    return np.where(ok, m, 0).astype(np.uint16), int((~ok).sum())


def pack(index, bits):
    """(height, ceil(width * bits / 8)) uint8: rows start on a byte, leftmost pixel in the high bits, padding bits zero"""
    a = np.asarray(index)
    h, w = a.shape
    if bits == 8:
        return a.astype(np.uint8)
    if bits == 16:
        return a.astype(np.uint16)
    stride = (w * bits + 7) // 8
    out = np.zeros((h, stride), np.uint8)
    per = 8 // bits
    for y in range(h):
        for x in range(w):
            out[y, x // per] |= int(a[y, x]) << (8 - bits * (x % per + 1))
    if bits == 1:
        assert np.array_equal(out, np.packbits(a.astype(np.uint8), axis=1))
    return out


def pack_fast(index, bits):
    """the same without the Python loop, for the large shapes (checked against pack() on the small ones)"""
    a = np.asarray(index)
    if bits >= 8:
        return pack(a, bits)
    h, w = a.shape
    per = 8 // bits
    stride = (w * bits + 7) // 8
    wide = np.zeros((h, stride * per), np.uint8)
    wide[:, :w] = a
    out = np.zeros((h, stride), np.uint8)
    for s in range(per):
        out |= wide[:, s::per] << np.uint8(8 - bits * (s + 1))
    return out
