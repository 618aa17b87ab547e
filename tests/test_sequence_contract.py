"""Frame sequences without a device (include/kmeans_hip.h at kmg_sequence): the test-side reference agrees with
itself and with the existing alpha-mode reference, delta frames replay to the full frames exactly when no shown pixel turns
transparent, the APNG writer round-trips through an independent chunk reader, and the header, the library and the Python package
carry the new surface."""
import ctypes as C
import io
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import alpha_ref
import sequence_ref as R
from conftest import ROOT

NEW = ("kmg_sequence_create", "kmg_sequence_destroy", "kmg_sequence_add", "kmg_sequence_add_device", "kmg_sequence_clear",
       "kmg_sequence_info", "kmg_sequence_centroids", "kmg_sequence_palette", "kmg_dev_frame_delta", "kmg_sequence_output_begin",
       "kmg_sequence_output_frame", "kmg_sequence_output_end")


# ---- an APNG reader of its own: chunks, PLTE / tRNS / acTL / fcTL / IDAT / fdAT, filter type 0 only ------------------------------
def read_apng(data):
    """(palette (n, 3), trns bytes, [index map shown after each frame]) of a palette-mode APNG whose scanlines use filter 0"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1][0] == b"IEND"
    w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, interlace) == (8, 3, 0)
    plte = np.frombuffer(dict(chunks)[b"PLTE"], np.uint8).reshape(-1, 3)
    trns = dict(chunks)[b"tRNS"]
    n_frames, _ = struct.unpack(">II", dict(chunks)[b"acTL"])
    transparent = [i for i, a in enumerate(trns) if a == 0]
    frames, seq, ctl, payload = [], 0, None, b""
    for kind, body in chunks[1:]:
        if kind in (b"fcTL", b"IEND") and ctl is not None:
            frames.append((ctl, payload))
            ctl, payload = None, b""
        if kind == b"fcTL":
            ctl = struct.unpack(">IIIIIHHBB", body)
            assert ctl[0] == seq
            seq += 1
        elif kind == b"IDAT":
            payload += body
        elif kind == b"fdAT":
            assert struct.unpack(">I", body[:4])[0] == seq
            seq += 1
            payload += body[4:]
    assert len(frames) == n_frames
    canvas, shown = np.full((h, w), transparent[0], np.uint8), []
    for (_, fw, fh, x0, y0, _, _, dispose, blend), payload in frames:
        rows = np.frombuffer(zlib.decompress(payload), np.uint8).reshape(fh, fw + 1)
        assert dispose == 0 and (rows[:, 0] == 0).all()
        region = rows[:, 1:]
        under = canvas[y0:y0 + fh, x0:x0 + fw]
        canvas = canvas.copy()
        canvas[y0:y0 + fh, x0:x0 + fw] = region if blend == 0 else np.where(np.isin(region, transparent), under, region)
        shown.append(canvas)
    return plte, trns, shown


# ---- the delta rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k", [(np.uint8, 255), (np.uint8, 5), (np.uint16, 3072), (np.uint16, 300)])
def test_vectorised_delta_is_the_literal_loop(dtype, k):
    rng = np.random.default_rng(k)
    for rows, width in ((1, 1), (3, 15), (5, 17), (2, 64), (7, 9)):
        for p_change in (0.0, 0.1, 1.0):
            canvas = rng.integers(0, k + 1, (rows, width)).astype(dtype)
            index = np.where(rng.random((rows, width)) < p_change, rng.integers(0, k + 1, (rows, width)), canvas).astype(dtype)
            row0 = int(rng.integers(0, 1000))
            d1, c1, r1 = R.delta(index, canvas, k, row0)
            d2, c2, r2 = R.delta_loop(index, canvas, k, row0)
            assert d1.dtype == dtype and np.array_equal(d1, d2) and np.array_equal(c1, c2) and r1 == r2
            assert np.array_equal(c1, index)
            if p_change == 0.0:
                assert r1 == R.FRESH and (d1 == k).all()


def test_bands_combine_to_the_whole_frame():
    rng = np.random.default_rng(3)
    k = 40
    canvas = rng.integers(0, k + 1, (11, 23)).astype(np.uint8)
    index = np.where(rng.random((11, 23)) < 0.2, rng.integers(0, k + 1, (11, 23)), canvas).astype(np.uint8)
    whole = R.delta(index, canvas, k)
    for cut in (1, 5, 10):
        a = R.delta(index[:cut], canvas[:cut], k, 0)
        b = R.delta(index[cut:], canvas[cut:], k, cut)
        assert R.combine(a[2], b[2]) == R.combine(b[2], a[2]) == whole[2]
        assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0])
    assert R.combine(R.FRESH, whole[2]) == whole[2]


def _moving_maps(k, n_frames=5, h=24, w=31, seed=9, with_holes=False):
    """index maps of a block that moves over a static background; with_holes: the block leaves transparent pixels behind"""
    rng = np.random.default_rng(seed)
    back = rng.integers(0, k, (h, w)).astype(np.uint8)
    if with_holes:
        back[:, : w // 2] = k
    maps = []
    for t in range(n_frames):
        m = back.copy()
        m[4 + t:10 + t, 3 + 2 * t:9 + 2 * t] = (t % k)
        maps.append(m)
    return maps


def test_replaying_deltas_reproduces_the_frames_when_nothing_is_cleared():
    k = 17
    maps = _moving_maps(k)
    coded = R.encode_sequence(maps, k)
    assert all(rec[1] == 0 and not full for _, rec, full in coded)
    assert coded[0][1][0] == maps[0].size and np.array_equal(coded[0][0], maps[0])     # against a canvas of k the delta IS I_0
    shown = R.replay([(m, full) for m, _, full in coded], k)
    for got, want in zip(shown, maps):
        assert np.array_equal(got, want)
    # a frame equal to its predecessor: nothing changed, the record stays fresh
    again = R.encode_sequence(maps + [maps[-1]], k)
    assert again[-1][1] == R.FRESH and (again[-1][0] == k).all()


def test_cleared_pixels_need_the_full_frame():
    """the block moves over a transparent area: where it was, the frame's index is k again -- `over` keeps the block there"""
    k = 17
    maps = _moving_maps(k, with_holes=True)
    naive = R.encode_sequence(maps, k, honour_cleared=False)
    assert any(rec[1] > 0 for _, rec, _ in naive)
    shown = R.replay([(m, False) for m, _, _ in naive], k)
    assert not all(np.array_equal(g, w) for g, w in zip(shown, maps)), "deltas alone must fail here"
    coded = R.encode_sequence(maps, k)
    assert any(full for _, _, full in coded)
    for (m, rec, full) in coded:
        assert full == (rec[1] > 0)
    shown = R.replay([(m, full) for m, _, full in coded], k)
    for got, want in zip(shown, maps):
        assert np.array_equal(got, want)


def test_one_frame_reference_is_the_alpha_reference(oracle, tokyo):
    frame = np.ascontiguousarray(tokyo[100:260, 200:420])
    for t in (0, 128):
        img = alpha_ref.soft_disc(frame) if t else frame
        got = R.centroids(oracle, [img], 6, t)
        want = alpha_ref.kmeans_centroids(oracle, img, 6, t)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert R.centroids(oracle, [np.zeros((8, 8, 4), np.uint8)], 3, 1) is None
    W, w, h = R.working_sequence(oracle, [frame, frame[:50, :60]])
    assert (w, h) == (frame.shape[0] * frame.shape[1] + 3000, 1) and np.array_equal(W[-3000:], frame[:50, :60].reshape(-1, 4))


# ---- the APNG writer ----------------------------------------------------------------------------------------------------------------
def _coded_for_apng(maps, k):
    return [(m, None if rec[0] == 0 else rec[2:], full) for m, rec, full in R.encode_sequence(maps, k)]


def test_apng_round_trip(tmp_path):
    from kmeans_gpu_amd import apng
    k = 17
    rng = np.random.default_rng(1)
    palette = rng.integers(0, 256, (k, 4)).astype(np.uint8)
    for holes in (False, True):
        maps = _moving_maps(k, with_holes=holes)
        maps.insert(3, maps[2].copy())                                    # a frame in which nothing changes
        coded = _coded_for_apng(maps, k)
        assert coded[3][1] is None and not coded[3][2]
        h, w = maps[0].shape
        data = apng.encode(palette, w, h, coded, delay_ms=40)
        plte, trns, shown = read_apng(data)
        assert np.array_equal(plte[:k], palette[:, :3]) and plte.shape[0] == k + 1
        assert trns == bytes([255] * k + [0])
        assert len(shown) == len(maps)
        for got, want in zip(shown, maps):
            assert np.array_equal(got, want)
        # delta frames carry their rectangle only
        sizes = [struct.unpack(">II", data[i + 8:i + 16]) for i in (m.start() for m in re.finditer(b"fcTL", data))]
        assert sizes[0] == (w, h) and sizes[3] == (1, 1)
        if not holes:
            assert all(s[0] * s[1] < w * h for s in sizes[1:])
        path = tmp_path / "a.png"
        apng.write(str(path), palette, w, h, coded, delay_ms=40)
        assert path.read_bytes() == data
        try:
            from PIL import Image
        except ImportError:
            continue
        im = Image.open(io.BytesIO(data))
        assert getattr(im, "n_frames", 1) == len(maps)
        rgba = np.concatenate([palette[:, :3], np.full((k, 1), 255, np.uint8)], axis=1)
        rgba = np.concatenate([rgba, np.zeros((1, 4), np.uint8)])
        for i, want in enumerate(maps):
            im.seek(i)
            got = np.array(im.convert("RGBA"))
            vis = want != k
            assert np.array_equal(got[vis], rgba[want][vis]) and (got[~vis][:, 3] == 0).all(), f"PIL, frame {i}"


def test_apng_refuses_what_it_cannot_write():
    from kmeans_gpu_amd import apng
    m = np.zeros((4, 4), np.uint8)
    with pytest.raises(ValueError):
        apng.encode(np.zeros((256, 4), np.uint8), 4, 4, [(m, None, True)])
    with pytest.raises(ValueError):
        apng.encode(np.zeros((3, 4), np.uint8), 4, 4, [])
    with pytest.raises(ValueError):
        apng.encode(np.zeros((3, 4), np.uint8), 4, 4, [(m, None, True), (m, (0, 0, 5, 4), False)])
    with pytest.raises(ValueError):
        apng.encode(np.zeros((3, 4), np.uint8), 5, 4, [(m, None, True)])


# ---- header, library, package --------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import kmeans_gpu_amd as kg
    header = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    L = C.CDLL(kg.library_path())
    for name in NEW:
        assert re.search(r"KMG_API\s+(int|void)\s+" + name + r"\s*\(", header), name
        assert hasattr(L, name), name
        assert name in kg.SYMBOLS
    assert re.search(r"#define\s+KMG_FRAME_DELTA\s+1u", header) and kg.FRAME_DELTA == 1
    assert b"k_frame_delta" in open(kg.library_path(), "rb").read()          # the gfx950 kernel of csrc/kmg_sequence.hip


def test_frame_delta_struct_is_32_bytes(tmp_path):
    import kmeans_gpu_amd as kg
    assert C.sizeof(kg.FrameDelta) == 32
    names = [n for n, _ in kg.FrameDelta._fields_]
    assert names == ["changed", "cleared", "x0", "y0", "x1", "y1"]
    offsets = [getattr(kg.FrameDelta, n).offset for n in names]
    assert offsets == [0, 8, 16, 20, 24, 28]
    header = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    body = re.search(r"typedef struct kmg_frame_delta \{(.*?)\} kmg_frame_delta;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    decls = re.findall(r"(uint64_t|uint32_t)\s+([\w\s,]+);", body)
    fields = [(t, n.strip()) for t, ns in decls for n in ns.split(",")]
    assert fields == [("uint64_t", "changed"), ("uint64_t", "cleared"), ("uint32_t", "x0"), ("uint32_t", "y0"), ("uint32_t", "x1"),
                      ("uint32_t", "y1")]
    # the C compiler's own opinion
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "kmeans_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(kmg_frame_delta), offsetof(kmg_frame_delta, changed), offsetof(kmg_frame_delta, cleared), "
                   "offsetof(kmg_frame_delta, x0), offsetof(kmg_frame_delta, y0), offsetof(kmg_frame_delta, x1), "
                   "offsetof(kmg_frame_delta, y1)); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["32", "0", "8", "16", "20", "24", "28"]
    rec = kg.FrameDelta.from_array(np.array([5, 1, (3 << 32) | 2, (9 << 32) | 7], np.uint64))
    assert rec.as_tuple() == (5, 1, 2, 3, 7, 9) and rec.rect == (2, 3, 7, 9)
    fresh = kg.FrameDelta.from_array(np.frombuffer(kg.FrameDelta.fresh_bytes(), np.uint8))
    assert fresh.as_tuple() == R.FRESH and fresh.rect is None


def test_refusals_that_need_no_device():
    import kmeans_gpu_amd as kg
    L = kg.lib()

    def refused(rc, text):
        assert rc == -1, rc
        assert text in L.kmg_last_error().decode(), L.kmg_last_error().decode()

    one = C.c_void_p(16)                                                   # never dereferenced: every refusal comes first
    refused(L.kmg_dev_frame_delta(None, one, one, 4, 4, 0, 0, 8, one, one, None), "RGBA8")
    refused(L.kmg_dev_frame_delta(None, one, one, 4, 4, 0, 1, 256, one, one, None), "INDEX16")
    refused(L.kmg_dev_frame_delta(None, one, one, 4, 4, 0, 7, 8, one, one, None), "unknown output format")
    refused(L.kmg_dev_frame_delta(None, one, one, 4, 4, 0, 2, 8, one, one, None), "NULL")
    refused(L.kmg_sequence_create(None, None), "NULL")
    refused(L.kmg_sequence_add(None, None, 1, 1), "NULL")
    refused(L.kmg_sequence_output_frame(None, None, 1, None, None, None), "NULL")
    L.kmg_sequence_destroy(None)                                           # (a no-op)


def test_cli_sequence_arguments(tmp_path):
    from kmeans_gpu_amd import cli
    assert cli.sequence_file_path(8, "dither", None, "gfx/a.png") == "gfx/a-sequence-c8-dither.png"
    assert cli.sequence_file_path(8, "dither", "x.png", "gfx/a.png") == "x.png"
    assert cli.validate_delay("100") == 100
    for bad in ("-1", "70000", "x"):
        with pytest.raises(Exception):
            cli.validate_delay(bad)
    for argv in (["sequence", "-i", "a.png", "b.png", "-c", "256"], ["sequence", "-i", "a.png", "-c", "8", "-m", "meld"],
                 ["--devices", "0", "sequence", "-i", "a.png", "-c", "8"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
