"""Index-map optimisation on the device (include/kmeans_hip.h at kmg_dev_index_usage / kmg_dev_index_remap),
against tests/index_ref.py.  Everything is exact:
  1. k_index_usage: shapes around the 4-pixel group, the 1024-pixel tile and the grid cap, both index types, every k at which
     the formats differ, pointers that allow the vector loads and pointers that force the per-element path, five patterns, a
     record that starts at 2^40 per entry between sentinels, a frame in two bands on two streams in both orders;
  2. k_index_remap: every out_bits from each input format, widths around the byte, the dword and the tile, sentinels around the
     output (the byte after the last packed row included), padding bits, in place, the three kinds of bad pixel, misaligned
     pointers;
  3. refusals, after each of which the processor still answers a kmg_find;
  4. reduce_indexed -> optimize_indexed on the photograph, kmg_index_optimize against its three building blocks, and the CLI."""
import ctypes as C
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import index_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

FMT8, FMT16 = 1, 2
FLAT = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099 * 7]
# 2048 workgroups x 1024 pixels per tile round: only a larger band makes a workgroup walk several tiles (the prefetch, the run a
# wave keeps in registers)
MANY_TILES = (4099, 600)
USAGE_K = [(FMT8, 1), (FMT8, 2), (FMT8, 255), (FMT8, 256), (FMT16, 1), (FMT16, 2), (FMT16, 255), (FMT16, 257), (FMT16, 3072)]
PATTERNS = ("constant", "two", "uniform", "above", "runs")
OFFSETS = (0, 4, 1, 2, 3)                 # elements into the allocation: 0 and 4 allow the vector loads, 1, 2, 3 force the per-element path
WIDTHS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 257, 1023, 1025]
ROWS = [1, 2, 5]
BITS = (1, 2, 4, 8, 16)
PAD = 16
BIG = 1 << 40
GUARD = 0x5A5A5A5A5A5A5A5A


def _dtype(fmt):
    return np.uint8 if fmt == FMT8 else np.uint16


def _sentinel(dtype):
    return 0xA5 if dtype == np.uint8 else 0xA5C3


class _Buf:
    """n elements of dtype, `off` elements into a sentinel-filled device allocation"""

    def __init__(self, torch, dtype, n, off, data=None):
        self.torch, self.dtype, self.n, self.off = torch, dtype, n, off
        host = np.full(n + off + PAD, _sentinel(dtype), dtype)
        if data is not None:
            host[off:off + n] = np.asarray(data).reshape(-1)
        self.t = torch.from_numpy(host.view(np.uint8 if dtype == np.uint8 else np.int16)).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + self.off * self.t.element_size()

    def get(self):
        host = self.t.cpu().numpy().view(self.dtype)
        s = _sentinel(self.dtype)
        assert (host[:self.off] == s).all() and (host[self.off + self.n:] == s).all(), "written outside the buffer"
        return host[self.off:self.off + self.n]


def _pattern(rng, name, n, k, dtype):
    top = min(int(np.iinfo(dtype).max), k + 40)                      # the largest value the type can hold, a little above k
    if name == "constant":
        return np.full(n, int(rng.integers(0, min(k, top) + 1)), dtype)
    if name == "two":
        a, b = (int(v) for v in rng.integers(0, min(k, top) + 1, 2))
        out = np.full(n, a, dtype)
        out[1::2] = b
        return out
    if name == "uniform":
        return rng.integers(0, min(k, top) + 1, n).astype(dtype)
    if name == "above":
        return rng.integers(0, top + 1, n).astype(dtype)
    values = rng.integers(0, min(k, top) + 1, n // 100 + 2)
    lengths = rng.integers(1, 301, values.shape[0])
    out = np.repeat(values, lengths)
    while out.shape[0] < n:
        out = np.concatenate([out, out])
    return out[:n].astype(dtype)


class _Record:
    """k + 2 counts in device memory between guard words, every entry starting at `start`"""

    def __init__(self, torch, k, start=BIG):
        self.k, self.start = k, start
        host = np.full(k + 4, GUARD, np.uint64)
        host[1:k + 3] = start
        self.t = torch.from_numpy(host.view(np.int64)).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + 8

    def get(self):
        host = self.t.cpu().numpy().view(np.uint64)
        assert host[0] == GUARD and host[-1] == GUARD, "written outside the record"
        return host[1:-1] - np.uint64(self.start)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


# ---- usage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,k", USAGE_K)
def test_usage_shapes_patterns_offsets(torch_cuda, processor, fmt, k):
    torch, dtype = torch_cuda, _dtype(fmt)
    rng = np.random.default_rng(1000 * fmt + k)
    for n in FLAT:
        for off in OFFSETS:
            for name in PATTERNS if n < 4099 or off in (0, 1) else PATTERNS[:1]:
                a = _pattern(rng, name, n, k, dtype)
                buf, rec = _Buf(torch, dtype, n, off, a), _Record(torch, k)
                processor.index_usage_device(buf.ptr, n, fmt, k, rec.ptr, _stream(torch))
                torch.cuda.synchronize()
                want = R.usage(a, k)
                got = rec.get()
                assert np.array_equal(got, want), (n, off, name, np.nonzero(got != want)[0][:8])
                assert int(got.sum()) == n
                assert np.array_equal(buf.get(), a)


@pytest.mark.parametrize("fmt,k", [(FMT8, 255), (FMT8, 256), (FMT16, 3072)])
def test_usage_many_tiles(torch_cuda, processor, fmt, k):
    torch, dtype = torch_cuda, _dtype(fmt)
    n = MANY_TILES[0] * MANY_TILES[1]
    assert n > 2048 * 1024
    rng = np.random.default_rng(77 + k)
    for name, off in (("constant", 0), ("runs", 0), ("above", 0), ("two", 0), ("runs", 1)):
        a = _pattern(rng, name, n, k, dtype)
        buf, rec = _Buf(torch, dtype, n, off, a), _Record(torch, k)
        processor.index_usage_device(buf.ptr, n, fmt, k, rec.ptr, _stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(rec.get(), R.usage(a, k)), (name, off)


def test_usage_index8_at_256_leaves_the_two_last_entries(torch_cuda, processor):
    torch = torch_cuda
    a = np.arange(5000, dtype=np.uint64).astype(np.uint8)
    buf, rec = _Buf(torch, np.uint8, a.shape[0], 0, a), _Record(torch, 256, start=7)
    processor.index_usage_device(buf.ptr, a.shape[0], FMT8, 256, rec.ptr, _stream(torch))
    torch.cuda.synchronize()
    got = rec.get()
    assert got[256] == 0 and got[257] == 0 and np.array_equal(got, R.usage(a, 256))


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
def test_usage_two_bands_two_streams_either_order(torch_cuda, processor, fmt):
    torch, dtype = torch_cuda, _dtype(fmt)
    width, rows, k = 1025, 37, 200
    rng = np.random.default_rng(5)
    a = _pattern(rng, "runs", width * rows, k, dtype)
    want = R.usage(a, k)
    buf = _Buf(torch, dtype, a.shape[0], 0, a)
    top = 13 * width
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for order in ((0, 1), (1, 0)):
        rec = _Record(torch, k)
        torch.cuda.synchronize()
        bands = [(buf.ptr, top, s1), (buf.ptr + top * buf.t.element_size(), a.shape[0] - top, s2)]
        for i in order:
            ptr, n, s = bands[i]
            processor.index_usage_device(ptr, n, fmt, k, rec.ptr, s.cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(rec.get(), want), order
    # and the host-buffer call combines into the caller's record
    use = processor.index_usage(a.reshape(rows, width), k)
    assert np.array_equal(use, want)
    processor.index_usage(a.reshape(rows, width), k, usage=use)
    assert np.array_equal(use, 2 * want)


# ---- remap -----------------------------------------------------------------------------------------------------------------------
def _table(rng, k, bits, drop=0.0, wide=0.0):
    """k + 1 entries below 2^bits; a share `drop` of them 0xFFFF, a share `wide` of them too large for `bits`"""
    t = rng.integers(0, min(1 << bits, 0xFFFF), k + 1).astype(np.uint16)
    if wide and bits < 16:
        sel = rng.random(k + 1) < wide
        t[sel] = rng.integers(1 << bits, 0xFFFF, int(sel.sum()))
    if drop:
        t[rng.random(k + 1) < drop] = R.DROPPED
    return t


def _out_dtype(bits):
    return np.uint16 if bits == 16 else np.uint8


def _run_remap(torch, processor, a, fmt, k, table, bits, off_in, off_out, bad_start=BIG, in_place=False):
    """(output as (rows, stride or width), bad pixels counted)"""
    rows, width = a.shape
    stride = width if bits >= 8 else (width * bits + 7) // 8
    src = _Buf(torch, _dtype(fmt), a.size, off_in, a)
    dst = src if in_place else _Buf(torch, _out_dtype(bits), rows * stride, off_out)
    bad = torch.from_numpy(np.array([GUARD, bad_start, GUARD], np.uint64).view(np.int64)).cuda()
    processor.index_remap_device(src.ptr, fmt, width, rows, k, table, bits, dst.ptr, bad.data_ptr() + 8, _stream(torch))
    torch.cuda.synchronize()
    b = bad.cpu().numpy().view(np.uint64)
    assert b[0] == GUARD and b[2] == GUARD
    if not in_place:
        assert np.array_equal(src.get(), a.reshape(-1))
    return dst.get().reshape(rows, stride), int(b[1] - np.uint64(bad_start))


def _check_remap(torch, processor, rng, fmt, bits, width, rows, off_in, off_out, drop=0.0, wide=0.0, above=False, k=None):
    dtype = _dtype(fmt)
    if k is None:
        k = int(rng.integers(1, 257 if fmt == FMT8 else 3073))
    top = min(int(np.iinfo(dtype).max), k + (40 if above else 0))
    a = rng.integers(0, top + 1, (rows, width)).astype(dtype)
    table = _table(rng, k, bits, drop, wide)
    got, bad = _run_remap(torch, processor, a, fmt, k, table, bits, off_in, off_out)
    new, want_bad = R.remap_fast(a, k, table, bits)
    want = R.pack_fast(new, bits)
    assert np.array_equal(got, want), (fmt, bits, width, rows, off_in, off_out, k)
    assert bad == want_bad
    if bits < 8 and (width * bits) % 8:
        assert not (got[:, -1] & ((1 << (8 - (width * bits) % 8)) - 1)).any(), "padding bits"
    return bad


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("fmt", [FMT8, FMT16])
def test_remap_shapes_and_offsets(torch_cuda, processor, fmt, bits):
    rng = np.random.default_rng(31 * bits + fmt)
    for width, rows in [(w, r) for w in WIDTHS for r in ROWS] + [(4099, 7)]:
        for off_in, off_out in ((0, 0), (1, 1), (3, 2), (4, 3), (2, 0)):
            _check_remap(torch_cuda, processor, rng, fmt, bits, width, rows, off_in, off_out)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("fmt", [FMT8, FMT16])
def test_remap_bad_pixels_each_kind_and_mixed(torch_cuda, processor, fmt, bits):
    rng = np.random.default_rng(17 * bits + fmt)
    k = 200 if fmt == FMT8 else 700
    seen = []
    for kind in ({"above": True}, {"drop": 0.2}, {"wide": 0.3}, {"above": True, "drop": 0.2, "wide": 0.3}):
        for width, rows, off in ((65, 5, 0), (1025, 2, 1)):
            seen.append(_check_remap(torch_cuda, processor, rng, fmt, bits, width, rows, off, off, k=k, **kind))
    assert min(seen[:4]) > 0 and min(seen[-2:]) > 0                 # (16 bits has no index too wide: that kind counts nothing there)
    assert (min(seen[4:6]) > 0) == (bits < 16)


@pytest.mark.parametrize("fmt", [FMT8, FMT16])
def test_remap_in_place_and_bad_count_combines(torch_cuda, processor, fmt):
    rng = np.random.default_rng(9 + fmt)
    bits, k = (8, 256) if fmt == FMT8 else (16, 3072)
    for width, rows, off in ((1, 1, 0), (33, 5, 1), (4099, 7, 0), (1025, 5, 3)):
        a = rng.integers(0, k + 1 if fmt == FMT16 else 256, (rows, width)).astype(_dtype(fmt))
        table = _table(rng, k, bits, drop=0.1)
        new, want_bad = R.remap_fast(a, k, table, bits)
        for start in (0, BIG, 123):
            got, bad = _run_remap(torch_cuda, processor, a, fmt, k, table, bits, off, off, bad_start=start, in_place=True)
            assert np.array_equal(got, new.astype(_out_dtype(bits))) and bad == want_bad and (want_bad > 0 or a.size == 1)


@pytest.mark.parametrize("bits", [8, 1])
def test_remap_many_tiles(torch_cuda, processor, bits):
    rng = np.random.default_rng(bits)
    width, rows = MANY_TILES
    _check_remap(torch_cuda, processor, rng, FMT8, bits, width, rows, 0, 0, drop=0.01, k=256 if bits == 8 else 1)
    _check_remap(torch_cuda, processor, rng, FMT8, bits, width, rows, 1, 1, k=255 if bits == 8 else 1)


def test_remap_host_call(processor):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 18, (37, 129)).astype(np.uint16)
    table = _table(rng, 16, 4, drop=0.1)
    for bits in BITS:
        got, bad = processor.index_remap(a, 16, table, bits)
        new, want_bad = R.remap_fast(a, 16, table, bits)
        assert np.array_equal(got, R.pack_fast(new, bits)) and bad == want_bad and bad > 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _still_finds(processor):
    img = np.zeros((8, 8, 4), np.uint8)
    img[:, 4:] = 255
    img[..., 3] = 255
    pal = np.array([[0, 0, 0, 255], [255, 255, 255, 255]], np.uint8)
    assert np.array_equal(processor.find(img, pal), img)


def test_usage_refusals(torch_cuda, processor):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    L, st = kg.lib(), C.c_void_p(_stream(torch))
    m = torch.zeros(64, dtype=torch.int16, device="cuda")
    rec = torch.full((3074 + 2,), 5, dtype=torch.int64, device="cuda")

    def call(p=processor.handle, index=m.data_ptr(), n=64, fmt=FMT16, k=9, usage=rec.data_ptr()):
        return L.kmg_dev_index_usage(p, C.c_void_p(index) if index else None, n, fmt, k, C.c_void_p(usage) if usage else None, st)

    assert call() == 0
    torch.cuda.synchronize()
    assert int(rec[0]) == 5 + 64
    rec.fill_(5)
    for kwargs, text in (({"fmt": 0}, "index format"), ({"fmt": 3}, "index format"), ({"k": 0}, "k = 0"), ({"k": 3073}, "3073"),
                         ({"fmt": FMT8, "k": 257}, "INDEX16"), ({"n": 0}, "no pixels"), ({"index": None}, "NULL"), ({"usage": None}, "NULL"),
                         ({"p": None}, "NULL"), ({"index": m.data_ptr() + 1}, "aligned"), ({"usage": rec.data_ptr() + 4}, "aligned")):
        assert call(**kwargs) == -1, kwargs
        assert text in L.kmg_last_error().decode(), (kwargs, L.kmg_last_error())
        torch.cuda.synchronize()
        assert bool((rec == 5).all()), kwargs                       # nothing was enqueued
        _still_finds(processor)
    with pytest.raises(kg.KmgError):
        processor.index_usage(np.zeros((0, 4), np.uint8), 4)
    _still_finds(processor)


def test_remap_refusals(torch_cuda, processor):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    L, st = kg.lib(), C.c_void_p(_stream(torch))
    m = torch.zeros(64, dtype=torch.int16, device="cuda")
    out = torch.full((64,), 77, dtype=torch.int16, device="cuda")
    bad = torch.full((2,), 5, dtype=torch.int64, device="cuda")
    table = np.arange(10, dtype=np.uint16)

    def call(p=processor.handle, src=m.data_ptr(), fmt=FMT16, width=8, rows=8, k=9, remap=table.ctypes.data, bits=16, dst=out.data_ptr(),
             cnt=bad.data_ptr()):
        vp = lambda v: C.c_void_p(v) if v else None
        return L.kmg_dev_index_remap(p, vp(src), fmt, width, rows, k, vp(remap), bits, vp(dst), vp(cnt), st)

    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and int(bad[0]) == 5
    out.fill_(77)
    for kwargs, text in (({"fmt": 0}, "index format"), ({"fmt": 3}, "index format"), ({"k": 0}, "k = 0"), ({"k": 3073}, "3073"),
                         ({"fmt": FMT8, "k": 257}, "INDEX16"), ({"width": 0}, "zero"), ({"rows": 0}, "zero"), ({"bits": 0}, "out_bits"),
                         ({"bits": 3}, "out_bits"), ({"bits": 32}, "out_bits"), ({"src": None}, "NULL"), ({"remap": None}, "NULL"),
                         ({"dst": None}, "NULL"), ({"cnt": None}, "NULL"), ({"p": None}, "NULL"), ({"src": m.data_ptr() + 1}, "aligned"),
                         ({"dst": out.data_ptr() + 1}, "aligned"), ({"cnt": bad.data_ptr() + 4}, "aligned")):
        assert call(**kwargs) == -1, kwargs
        assert text in L.kmg_last_error().decode(), (kwargs, L.kmg_last_error())
        torch.cuda.synchronize()
        assert bool((out == 77).all()) and bool((bad == 5).all()), kwargs
        _still_finds(processor)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def photo(tokyo):
    """a crop of the photograph with a transparent disc (alpha mode drops it, alpha_cutoff = 0 ignores alpha)"""
    img = np.ascontiguousarray(tokyo[100:292, 200:455]).copy()
    yy, xx = np.mgrid[:img.shape[0], :img.shape[1]]
    img[(yy - 90) ** 2 + (xx - 120) ** 2 < 50 ** 2, 3] = 10
    return img


@pytest.fixture(scope="module")
def processors(torch_cuda):
    import kmeans_gpu_amd as kg
    ps = {0: kg.ImageProcessor(), 128: kg.ImageProcessor(alpha_cutoff=128)}
    yield ps
    for p in ps.values():
        p.close()


@pytest.mark.parametrize("cutoff", [0, 128])
@pytest.mark.parametrize("mode", ["Replace", "Dither", "Diffuse"])
@pytest.mark.parametrize("k", [2, 4, 8, 64])
def test_optimize_after_reduce_indexed(processors, photo, k, mode, cutoff):
    import kmeans_gpu_amd as kg
    p = processors[cutoff]
    pal, index = p.reduce_indexed(k, photo, reduce_mode=getattr(kg.ReduceMode, mode))
    n = pal.shape[0]
    flags = kg.INDEX_ORDER_USAGE | kg.INDEX_TRANSPARENT_FIRST
    pal_out, packed, info = p.optimize_indexed(index, pal)
    values = np.unique(index)
    assert info.n_slots == values.shape[0] and info.bits == R.bits_of(info.n_slots)
    assert (info.transparent == 0) == bool((index == n).any()) and info.transparent in (0, -1)
    assert (cutoff == 128) == (info.transparent == 0)
    new = kg.unpack_indices(packed, index.shape[1], info.bits)
    shown = np.concatenate([pal, np.zeros((1, 4), np.uint8)])[index]          # transparent to transparent
    assert np.array_equal(pal_out[new], shown)
    use = p.index_usage(index, n)
    assert np.array_equal(use, R.usage(index, n))
    by_use = kg.index_plan(use, pal, kg.INDEX_ORDER_USAGE)[0]
    assert use[int(np.nonzero(by_use[:n] == 0)[0][0])] == use[:n].max()            # the most used colour comes first
    # the one call equals its three building blocks run by hand, and the reference
    remap, pal_hand, info_hand = kg.index_plan(use, pal, flags)
    map_hand, bad = p.index_remap(index, n, remap, info_hand.bits)
    assert bad == 0 and info_hand.as_tuple() == info.as_tuple()
    assert np.array_equal(pal_hand, pal_out) and np.array_equal(map_hand, packed)
    want_remap, want_pal, want_info = R.plan(use, pal, flags)
    assert np.array_equal(remap, want_remap) and np.array_equal(pal_out, want_pal) and info.as_tuple() == want_info
    assert np.array_equal(packed, R.pack_fast(R.remap_fast(index, n, want_remap, info.bits)[0], info.bits))
    # a wider map on request; a narrower one is refused
    pal8, map8, info8 = p.optimize_indexed(index, pal, bits=8)
    assert np.array_equal(map8, new) and np.array_equal(pal8, pal_out) and info8.as_tuple() == info.as_tuple()
    if info.bits > 1:
        with pytest.raises(kg.KmgError, match="bits"):
            p.optimize_indexed(index, pal, bits=info.bits // 2)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "kmeans-gpu_amd", "python"))
    r = subprocess.run([sys.executable, "-m", "kmeans_gpu_amd.cli", *args], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def _chunks(path):
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(blob):
        n, kind = struct.unpack(">I4s", blob[pos:pos + 8])
        body = blob[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body)
        out.append((kind, body))
        pos += 12 + n
    return out


@pytest.mark.parametrize("k,alpha,depth", [(2, 0, 1), (4, 0, 2), (3, 128, 2), (13, 0, 4), (16, 128, 8), (40, 0, 8)])
def test_cli_reduce_indexed_optimize(tmp_path, photo, k, alpha, depth):
    from PIL import Image
    src, plain, opt = (str(tmp_path / n) for n in ("src.png", "plain.png", "opt.png"))
    Image.fromarray(photo).save(src)
    common = ["-i", src, "-c", str(k), "--indexed"] + (["--alpha-cutoff", str(alpha)] if alpha else [])
    _cli("reduce", *common, "-o", plain)
    _cli("reduce", *common, "--optimize", "-o", opt, "--report")
    a, b = np.array(Image.open(plain).convert("RGBA")), np.array(Image.open(opt).convert("RGBA"))
    visible = a[..., 3] != 0
    assert np.array_equal(a[..., 3], b[..., 3]) and np.array_equal(a[visible], b[visible])
    chunks = dict(_chunks(opt))
    w, h, d, ctype = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    assert (w, h, ctype) == (photo.shape[1], photo.shape[0], 3)
    entries = len(chunks[b"PLTE"]) // 3
    assert d == R.bits_of(entries) and d <= depth, (d, entries)   # (an entry no pixel uses is gone: the depth may be lower)
    if k <= 4:
        assert d == depth
    assert (chunks.get(b"tRNS") == b"\x00") if alpha else (b"tRNS" not in chunks)
    assert entries <= k + (1 if alpha else 0)


def test_cli_sequence_optimize_replays_the_same(tmp_path, photo):
    from PIL import Image
    from test_sequence_contract import read_apng
    frames = []
    for i in range(3):
        f = photo.copy()
        f[20 + 10 * i:60 + 10 * i, 30:90, :3] = (40 * i, 200 - 50 * i, 90)
        path = str(tmp_path / f"f{i}.png")
        Image.fromarray(f).save(path)
        frames.append(path)
    plain, opt = str(tmp_path / "plain.png"), str(tmp_path / "opt.png")
    _cli("sequence", "-i", *frames, "-c", "24", "-o", plain)
    _cli("sequence", "-i", *frames, "-c", "24", "-o", opt, "--optimize")
    def canvases(path):
        """the RGBA canvas shown after each frame, and the number of PLTE entries"""
        plte, trns, shown = read_apng(open(path, "rb").read())
        rgba = np.concatenate([plte, np.full((plte.shape[0], 1), 255, np.uint8)], axis=1)
        rgba[:len(trns), 3] = np.frombuffer(trns, np.uint8)
        rgba[rgba[:, 3] == 0] = 0
        return [rgba[m] for m in shown], plte.shape[0]

    (a, n_plain), (b, n_opt) = canvases(plain), canvases(opt)
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert n_opt <= n_plain
