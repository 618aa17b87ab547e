"""Test-side reference of the quantisation error statistics (kmg_error_stats; the contract is in include/kmeans_hip.h at
kmg_error_stats) and of the quality-targeted colour count (kmg_reduce_quality), built only from the oracle's wrappers
(tests/oracle_lib.py) and numpy.

A record is 14 exact integers: pixels, changed, invalid, sse[3], sad[3], max_abs[3], lab_sse, lab_max.  A pixel is counted when the
source's alpha byte is >= the cutoff (0 counts every pixel); an index >= k on a counted pixel adds 1 to `invalid` and nothing else.
The Lab terms live on the grid q = rint(64 Lab), Lab from the oracle's rgb_to_lab, rint = round half to even."""
import numpy as np

import alpha_ref

RGB, LAB = 1, 2
FIELDS = ("pixels", "changed", "invalid", "sse_r", "sse_g", "sse_b", "sad_r", "sad_g", "sad_b", "max_r", "max_g", "max_b", "lab_sse",
          "lab_max")
MAX_FIELDS = (9, 10, 11, 13)
ZERO = (0,) * 14
_CHUNK = 1 << 22

_q_table = None


def q_of(oracle, rgba):
    """(n, 3) int64: rint(64 L), rint(64 a), rint(64 b) of each pixel's colour"""
    px = np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)
    lab = oracle.rgb_to_lab(px).astype(np.float32)
    return np.rint(lab * np.float32(64.0)).astype(np.int64)


def q_table(oracle):
    """q of all 2^24 colours, index r | g << 8 | b << 16, as int16 (|q| <= 12950); built once"""
    global _q_table
    if _q_table is None:
        tab = np.empty((1 << 24, 3), np.int16)
        for b0 in range(0, 256, 16):
            i = np.arange(b0 << 16, (b0 + 16) << 16, dtype=np.uint32)
            px = np.stack([i & 255, (i >> 8) & 255, (i >> 16) & 255, np.full_like(i, 255)], axis=1).astype(np.uint8)
            q = q_of(oracle, px)
            assert np.abs(q).max() < 32768
            tab[b0 << 16:(b0 + 16) << 16] = q
        _q_table = tab
    return _q_table


def _q(oracle, rgb3, use_table):
    if use_table:
        c = rgb3[:, 0].astype(np.int64) | (rgb3[:, 1].astype(np.int64) << 8) | (rgb3[:, 2].astype(np.int64) << 16)
        return q_table(oracle)[c].astype(np.int64)
    return q_of(oracle, np.concatenate([rgb3, np.zeros((rgb3.shape[0], 1), np.uint8)], axis=1))


def combine(a, b):
    """the combination rule: sums are added, maxima are maxed"""
    return tuple(max(x, y) if i in MAX_FIELDS else x + y for i, (x, y) in enumerate(zip(a, b)))


def _stats_chunk(oracle, s, out, palette, cutoff, what, use_table):
    counted = s[:, 3] >= cutoff
    if palette is None:
        o = out.reshape(-1, 4)[:, :3]
        valid = np.ones(s.shape[0], bool)
    else:
        idx = out.reshape(-1).astype(np.int64)
        valid = idx < palette.shape[0]
        o = palette[np.where(valid, idx, 0)][:, :3]
    use = counted & valid
    s3, o3 = s[use][:, :3], o[use]
    d = np.abs(s3.astype(np.int64) - o3.astype(np.int64))
    differs = d.any(axis=1)
    rec = [int(use.sum()), int(differs.sum()), int((counted & ~valid).sum())] + [0] * 11
    if what & RGB:
        rec[3:6] = [int(v) for v in (d * d).sum(axis=0)]
        rec[6:9] = [int(v) for v in d.sum(axis=0)]
        rec[9:12] = [int(v) for v in (d.max(axis=0) if d.shape[0] else np.zeros(3, np.int64))]
    if what & LAB and differs.any():
        dq = _q(oracle, s3[differs], use_table) - _q(oracle, o3[differs], use_table)
        term = (dq * dq).sum(axis=1)
        rec[12], rec[13] = int(term.sum()), int(term.max())
    return tuple(rec)


def stats(oracle, src, out, palette=None, cutoff=0, what=RGB | LAB, use_table=None):
    """the record of `out` against `src`: src (..., 4) uint8; out the same shape, or -- with palette (k, 4) -- one index per pixel"""
    s = np.ascontiguousarray(src, np.uint8).reshape(-1, 4)
    n = s.shape[0]
    pal = None if palette is None else np.ascontiguousarray(palette, np.uint8).reshape(-1, 4)
    o = np.ascontiguousarray(out).reshape(-1, 4) if pal is None else np.ascontiguousarray(out).reshape(-1)
    assert o.shape[0] == n
    if use_table is None:
        use_table = n > (1 << 20)
    rec = ZERO
    for a in range(0, n, _CHUNK):
        rec = combine(rec, _stats_chunk(oracle, s[a:a + _CHUNK], o[a:a + _CHUNK], pal, cutoff, what, use_table))
    return rec


def expand(palette, index, src):
    """the RGBA8 image an index map stands for: palette[index].rgb with the source's alpha (index >= k: the source pixel itself)"""
    pal = np.ascontiguousarray(palette, np.uint8).reshape(-1, 4)
    idx = np.asarray(index).astype(np.int64)
    out = np.array(src, np.uint8)
    ok = idx < pal.shape[0]
    out[ok, :3] = pal[idx[ok]][:, :3]
    return out


# ---- the quality search --------------------------------------------------------------------------------------------------------
def bisect(accepted, k_min, k_max):
    """the fixed search of kmg_reduce_quality over any predicate accepted(k): (k*, reached, the k evaluated in order)"""
    seen = [k_max]
    if not accepted(k_max):
        return k_max, False, seen
    lo, hi = k_min, k_max
    while lo < hi:
        mid = (lo + hi) // 2
        seen.append(mid)
        if accepted(mid):
            hi = mid
        else:
            lo = mid + 1
    return hi, True, seen


def max_runs(k_min, k_max):
    """1 + ceil(log2(k_max - k_min + 1))"""
    return 1 + int(np.ceil(np.log2(k_max - k_min + 1)))


class Working:
    """W, C_k, E(k) of kmg_reduce_quality from the oracle: the working image of the palette step (the shrink, then the compaction
    in alpha mode), the palette pipeline's centroids at k, and the record of W against P[label]"""

    def __init__(self, oracle, rgba, cutoff=0, shrink_max_dim=256):
        self.oracle = oracle
        got = alpha_ref.kept_pixels(alpha_ref.shrink(oracle, rgba, shrink_max_dim), cutoff)
        assert got is not None
        self.px, self.w, self.h = got
        self.px = np.ascontiguousarray(self.px, np.uint8).reshape(-1, 4)
        self.lab = oracle.rgb_to_lab(self.px)
        self.n = self.px.shape[0]
        self._cache = {}

    def centroids(self, k):
        cent = self.oracle.init_centroids(self.lab, self.w, self.h, k)
        cent, _, _ = self.oracle.lloyd(self.lab, cent)
        return cent

    def record(self, k):
        """(record of W at k, the palette bytes P, the labels)"""
        if k not in self._cache:
            cent = self.centroids(k)
            labels = self.oracle.assign(self.lab, cent)
            pal = self.oracle.lab_to_rgba8(cent[:, :3])
            self._cache[k] = (stats(self.oracle, self.px, labels, palette=pal), pal, labels)
        return self._cache[k]

    def E(self, k):
        return self.record(k)[0][12]

    def search(self, k_min, k_max, target):
        """(k*, reached, record at k*, evaluated k) for a target in units of 1/4096 dE^2"""
        k, reached, seen = bisect(lambda kk: self.E(kk) <= int(target) * self.n, k_min, k_max)
        return k, reached, self.record(k)[0], seen
