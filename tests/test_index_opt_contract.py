"""The host side of the index-map optimisation (include/kmeans_hip.h at kmg_index_plan), no GPU:
  1. kmg_index_plan through ctypes against tests/index_ref.py bit for bit: random records at the colour counts around every bit
     depth, every flag combination, zero-usage patterns, ties, the identity flags, the `bits` boundaries, every refusal with the
     outputs untouched;
  2. what needs no device of the other calls: struct layout, symbols, refusals that come before the device is touched;
  3. the Python helpers (pack / unpack), the reference's fast forms against its per-pixel loops;
  4. the command line's refusals, and the packed PNG writer through PIL."""
import ctypes as C
import io
import itertools
import os
import re

import numpy as np
import pytest

import index_ref as R
from conftest import ROOT

KS = [1, 2, 3, 15, 16, 17, 255, 256, 257, 3072]
FLAGS = [o | u | t | f for o in (0, 1, 2) for u in (0, R.KEEP_UNUSED) for t in (0, R.KEEP_TRANSPARENT) for f in (0, R.TRANSPARENT_FIRST)]
IDENTITY = R.ORDER_KEEP | R.KEEP_UNUSED | R.KEEP_TRANSPARENT
SENT16, SENT8 = 0xBEEF, 0xCD


def _raw_plan(use, pal, k, flags, use_ptr=True, pal_ptr=True, remap_ptr=True, out_ptr=True, info_ptr=True):
    """kmg_index_plan on sentinel-filled outputs: (rc, remap, palette_out, info tuple)"""
    import kmeans_gpu_amd as kg
    L = kg.lib()
    use = np.ascontiguousarray(use, np.uint64)
    pal = np.ascontiguousarray(pal, np.uint8)
    n = max(k, 1) if k <= R.MAX_K else 8
    remap = np.full(n + 1, SENT16, np.uint16)
    out = np.full((n + 1, 4), SENT8, np.uint8)
    info = kg.IndexPlanInfo(0xAAAAAAAA, 0xAAAAAAAA, -77, 0xAAAAAAAA)
    vp = lambda a, on: C.c_void_p(a.ctypes.data) if on else None
    rc = L.kmg_index_plan(vp(use, use_ptr), vp(pal, pal_ptr), k, flags, vp(remap, remap_ptr), vp(out, out_ptr), C.byref(info) if info_ptr else None)
    return rc, remap, out, info.as_tuple()


def _untouched(remap, out, info):
    return (remap == SENT16).all() and (out == SENT8).all() and info == (0xAAAAAAAA, 0xAAAAAAAA, -77, 0xAAAAAAAA)


def _agree(use, pal, flags):
    k = pal.shape[0]
    rc, remap, out, info = _raw_plan(use, pal, k, flags)
    want = R.plan(use, pal, flags)
    if want is None:
        assert rc == -1 and _untouched(remap, out, info), (k, flags)
        return None
    assert rc == 0, (k, flags)
    w_remap, w_pal, w_info = want
    assert info == w_info, (k, flags, info, w_info)
    assert np.array_equal(remap, w_remap), (k, flags)
    assert np.array_equal(out[:w_info[1]], w_pal) and (out[w_info[1]:] == SENT8).all(), (k, flags)
    return want


def _usage_patterns(rng, k):
    """(name, k + 2 counts)"""
    full = rng.integers(1, 1 << 40, k + 2).astype(np.uint64)
    full[k + 1] = 0
    sparse = full.copy()
    sparse[rng.random(k + 2) < 0.5] = 0
    none = np.zeros(k + 2, np.uint64)
    one = none.copy()
    one[int(rng.integers(0, k))] = 3
    slot = none.copy()
    slot[k] = 9
    ties = rng.integers(1, 4, k + 2).astype(np.uint64)               # few distinct counts: many equal-usage ties
    ties[k + 1] = 0
    no_slot = full.copy()
    no_slot[k] = 0
    return [("full", full), ("sparse", sparse), ("none", none), ("one", one), ("slot", slot), ("ties", ties), ("no_slot", no_slot)]


@pytest.mark.parametrize("k", KS)
def test_plan_matches_the_reference(k):
    rng = np.random.default_rng(k)
    pal = rng.integers(0, 256, (k, 4)).astype(np.uint8)
    grey = np.repeat(rng.integers(0, 3, (k, 1)), 4, axis=1).astype(np.uint8)      # three luma values: equal-luma ties
    for name, use in _usage_patterns(rng, k):
        for flags in FLAGS:
            # the one refusal among these: nothing used and nothing kept
            empty = not ((use[:k + 1] > 0).any() or flags & (R.KEEP_UNUSED | R.KEEP_TRANSPARENT))
            for p in (pal, grey) if (flags & 3) == R.ORDER_LUMA else (pal,):
                assert (_agree(use, p, flags) is None) == empty, (name, flags)


def test_plan_properties():
    rng = np.random.default_rng(11)
    k = 40
    pal = rng.integers(0, 256, (k, 4)).astype(np.uint8)
    use = rng.integers(0, 5, k + 2).astype(np.uint64)
    use[k + 1] = 0
    use[k] = 6
    for flags in FLAGS:
        remap, out, (n_colors, n_slots, transparent, bits) = R.plan(use, pal, flags)
        rc, g_remap, g_out, g_info = _raw_plan(use, pal, k, flags)
        assert rc == 0 and np.array_equal(g_remap, remap)
        kept = np.nonzero(remap[:k] != R.DROPPED)[0]
        assert sorted(remap[kept].tolist() + [transparent]) == list(range(n_slots))            # a bijection onto the new indices
        assert all(np.array_equal(out[remap[i]], pal[i]) for i in kept) and not out[transparent].any()
        assert transparent == (0 if flags & R.TRANSPARENT_FIRST else n_colors)
        new_order = kept[np.argsort(remap[kept])]
        if (flags & 3) == R.ORDER_KEEP:
            assert (np.diff(new_order) > 0).all()
        elif (flags & 3) == R.ORDER_USAGE:
            assert all((use[a], -a) > (use[b], -b) for a, b in zip(new_order, new_order[1:]))
        else:
            assert all((R.luma(pal[a]), a) < (R.luma(pal[b]), b) for a, b in zip(new_order, new_order[1:]))
        if not flags & R.KEEP_UNUSED:
            assert (use[:k][remap[:k] == R.DROPPED] == 0).all() and (use[kept] > 0).all()


@pytest.mark.parametrize("k", KS)
def test_identity_flags(k):
    rng = np.random.default_rng(k + 1)
    pal = rng.integers(0, 256, (k, 4)).astype(np.uint8)
    for use in (np.zeros(k + 2, np.uint64), np.concatenate([rng.integers(0, 9, k + 1), [0]]).astype(np.uint64)):
        rc, remap, out, info = _raw_plan(use, pal, k, IDENTITY)
        assert rc == 0 and np.array_equal(remap, np.arange(k + 1)) and np.array_equal(out[:k], pal) and not out[k].any()
        assert info == (k, k + 1, k, R.bits_of(k + 1))


@pytest.mark.parametrize("n_slots,bits", [(1, 1), (2, 1), (3, 2), (4, 2), (5, 4), (16, 4), (17, 8), (256, 8), (257, 16), (3073, 16)])
def test_bits_boundaries(n_slots, bits):
    for with_slot in (False, True):
        k = n_slots - (1 if with_slot else 0)
        if k == 0 or k > R.MAX_K:
            continue
        pal = np.zeros((k, 4), np.uint8)
        use = np.ones(k + 2, np.uint64)
        use[k + 1] = 0
        use[k] = 1 if with_slot else 0
        rc, _, _, info = _raw_plan(use, pal, k, R.ORDER_USAGE)
        assert rc == 0 and info[1] == n_slots and info[3] == bits and R.bits_of(n_slots) == bits


def test_plan_refusals_leave_the_outputs_alone():
    import kmeans_gpu_amd as kg
    L = kg.lib()
    k = 5
    pal = np.arange(20, dtype=np.uint8).reshape(5, 4)
    good = np.array([1, 0, 2, 0, 3, 1, 0], np.uint64)
    assert _raw_plan(good, pal, k, 1)[0] == 0
    above = good.copy()
    above[k + 1] = 1
    cases = [("above k", dict(use=above)), ("nothing to index", dict(use=np.zeros(7, np.uint64))),
             ("unknown flag", dict(flags=32)), ("unknown flag", dict(flags=1 << 31)), ("unknown flag", dict(flags=3)), ("unknown flag", dict(flags=3 | 4 | 8)),
             ("KMG_MAX_K", dict(k=0)), ("KMG_MAX_K", dict(k=R.MAX_K + 1)),
             ("NULL", dict(use_ptr=False)), ("NULL", dict(pal_ptr=False)), ("NULL", dict(remap_ptr=False)), ("NULL", dict(out_ptr=False)),
             ("NULL", dict(info_ptr=False))]
    for text, kw in cases:
        args = dict(use=good, pal=pal, k=k, flags=1)
        args.update(kw)
        if args["k"] > k:                                              # (room for the call to read, were it to)
            args["use"] = np.zeros(args["k"] + 2, np.uint64)
            args["pal"] = np.zeros((args["k"], 4), np.uint8)
        rc, remap, out, info = _raw_plan(**args)
        assert rc == -1, (text, kw)
        assert text in L.kmg_last_error().decode(), (kw, L.kmg_last_error())
        assert _untouched(remap, out, info), kw
    with pytest.raises(kg.KmgError, match="above k"):
        kg.index_plan(above, pal)
    with pytest.raises(ValueError):
        kg.index_plan(good[:-1], pal)


def test_plan_in_place_palette():
    """out_palette_rgba may be the palette itself"""
    import kmeans_gpu_amd as kg
    rng = np.random.default_rng(2)
    k = 50
    pal = rng.integers(0, 256, (k + 1, 4)).astype(np.uint8)
    use = rng.integers(0, 3, k + 2).astype(np.uint64)
    use[k + 1] = 0
    for flags in (1 | 16 | 8, 2, 0, 1 | 4):
        want = R.plan(use, pal[:k], flags)
        buf = pal.copy()
        remap = np.zeros(k + 1, np.uint16)
        info = kg.IndexPlanInfo()
        p = C.c_void_p(buf.ctypes.data)
        assert kg.lib().kmg_index_plan(C.c_void_p(use.ctypes.data), p, k, flags, C.c_void_p(remap.ctypes.data), p, C.byref(info)) == 0
        assert np.array_equal(buf[:info.n_slots], want[1]) and np.array_equal(remap, want[0])


# ---- what needs no device ----------------------------------------------------------------------------------------------------------
NEW = ["kmg_dev_index_usage", "kmg_index_plan", "kmg_dev_index_remap", "kmg_index_usage", "kmg_index_remap", "kmg_index_optimize"]


def test_layout_symbols_constants():
    import kmeans_gpu_amd as kg
    assert C.sizeof(kg.IndexPlanInfo) == 16
    assert [(f[0], getattr(kg.IndexPlanInfo, f[0]).offset) for f in kg.IndexPlanInfo._fields_] == \
        [("n_colors", 0), ("n_slots", 4), ("transparent", 8), ("bits", 12)]
    header = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    L = kg.lib()
    for name in NEW:
        assert name in kg.SYMBOLS and hasattr(L, name) and re.search(r"KMG_API int " + name + r"\(", header), name
    for name, value in (("ORDER_KEEP", 0), ("ORDER_USAGE", 1), ("ORDER_LUMA", 2), ("KEEP_UNUSED", 4), ("KEEP_TRANSPARENT", 8),
                        ("TRANSPARENT_FIRST", 16)):
        assert getattr(kg, "INDEX_" + name) == value == getattr(R, name)
        assert re.search(r"#define KMG_INDEX_" + name + r"\s+" + str(value) + r"u\b", header), name
    assert kg.INDEX_DROPPED == R.DROPPED
    blob = open(kg.library_path(), "rb").read()
    assert b"k_index_usage" in blob and b"k_index_remap" in blob           # the gfx950 kernels of csrc/kmg_usage.hip


def test_host_calls_refuse_before_they_touch_a_device():
    """a NULL processor and every argument refusal come back as KMG_ERR_INVALID_ARGUMENT on a box without a GPU"""
    import kmeans_gpu_amd as kg
    L = kg.lib()
    m = np.zeros((4, 4), np.uint16)
    use = np.full(12, 7, np.uint64)
    table = np.arange(11, dtype=np.uint16)
    out = np.full(64, 0x5A, np.uint8)
    pal = np.zeros((11, 4), np.uint8)
    info = kg.IndexPlanInfo()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    fake = C.c_void_p(8)                                               # never dereferenced: every call below is refused first
    for args in ((None, vp(m), 2, 16, 10, vp(use)), (fake, None, 2, 16, 10, vp(use)), (fake, vp(m), 0, 16, 10, vp(use)),
                 (fake, vp(m), 2, 0, 10, vp(use)), (fake, vp(m), 2, 16, 0, vp(use)), (fake, vp(m), 1, 16, 257, vp(use)),
                 (fake, vp(m), 2, 16, 3073, vp(use)), (fake, vp(m), 2, 16, 10, None), (fake, C.c_void_p(m.ctypes.data + 1), 2, 15, 10, vp(use))):
        assert L.kmg_index_usage(*args) == -1, args
    assert (use == 7).all()
    for args in ((None, vp(m), 2, 4, 4, 10, vp(table), 4, vp(out), None), (fake, None, 2, 4, 4, 10, vp(table), 4, vp(out), None),
                 (fake, vp(m), 0, 4, 4, 10, vp(table), 4, vp(out), None), (fake, vp(m), 2, 0, 4, 10, vp(table), 4, vp(out), None),
                 (fake, vp(m), 2, 4, 0, 10, vp(table), 4, vp(out), None), (fake, vp(m), 2, 4, 4, 0, vp(table), 4, vp(out), None),
                 (fake, vp(m), 2, 4, 4, 10, None, 4, vp(out), None), (fake, vp(m), 2, 4, 4, 10, vp(table), 3, vp(out), None),
                 (fake, vp(m), 2, 4, 4, 10, vp(table), 0, vp(out), None), (fake, vp(m), 2, 4, 4, 10, vp(table), 4, None, None),
                 (fake, vp(m), 2, 4, 4, 10, vp(table), 16, C.c_void_p(out.ctypes.data + 1), None)):
        assert L.kmg_index_remap(*args) == -1, args
    for args in ((None, vp(m), 2, 4, 4, vp(pal), 10, 1, 0, vp(pal), C.byref(info), vp(out)),
                 (fake, None, 2, 4, 4, vp(pal), 10, 1, 0, vp(pal), C.byref(info), vp(out)),
                 (fake, vp(m), 0, 4, 4, vp(pal), 10, 1, 0, vp(pal), C.byref(info), vp(out)),
                 (fake, vp(m), 2, 0, 4, vp(pal), 10, 1, 0, vp(pal), C.byref(info), vp(out)),
                 (fake, vp(m), 2, 4, 4, None, 10, 1, 0, vp(pal), C.byref(info), vp(out)),
                 (fake, vp(m), 2, 4, 4, vp(pal), 0, 1, 0, vp(pal), C.byref(info), vp(out)),
                 (fake, vp(m), 2, 4, 4, vp(pal), 10, 3, 0, vp(pal), C.byref(info), vp(out)),
                 (fake, vp(m), 2, 4, 4, vp(pal), 10, 64, 0, vp(pal), C.byref(info), vp(out)),
                 (fake, vp(m), 2, 4, 4, vp(pal), 10, 1, 5, vp(pal), C.byref(info), vp(out)),
                 (fake, vp(m), 1, 4, 4, vp(pal), 10, 1, 16, vp(pal), C.byref(info), vp(out)),
                 (fake, vp(m), 2, 4, 4, vp(pal), 10, 1, 0, None, C.byref(info), vp(out)),
                 (fake, vp(m), 2, 4, 4, vp(pal), 10, 1, 0, vp(pal), None, vp(out)),
                 (fake, vp(m), 2, 4, 4, vp(pal), 10, 1, 0, vp(pal), C.byref(info), None)):
        assert L.kmg_index_optimize(*args) == -1, args
    assert (out == 0x5A).all()


# ---- the Python helpers and the reference's own forms ----------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 2, 4, 8, 16])
def test_pack_unpack_round_trip(bits):
    import kmeans_gpu_amd as kg
    rng = np.random.default_rng(bits)
    for width in range(1, 18):
        for rows in (1, 3):
            x = rng.integers(0, 1 << bits, (rows, width)).astype(np.uint16 if bits == 16 else np.uint8)
            packed = kg.pack_indices(x, bits)
            assert np.array_equal(packed, R.pack(x, bits)) and np.array_equal(packed, R.pack_fast(x, bits))
            assert packed.shape == (rows, kg.packed_stride(width, bits) if bits < 8 else width)
            assert np.array_equal(kg.unpack_indices(packed, width, bits), x)
            if bits == 1:
                assert np.array_equal(packed, np.packbits(x, axis=1))
    with pytest.raises(ValueError):
        kg.pack_indices(np.full((2, 2), 1 << min(bits, 15), np.uint16), min(bits, 8))
    with pytest.raises(ValueError):
        kg.pack_indices(np.zeros((2, 2), np.uint8), 3)


def test_reference_fast_forms_equal_the_loops():
    rng = np.random.default_rng(4)
    for bits, k in itertools.product((1, 2, 4, 8, 16), (1, 7, 300)):
        a = rng.integers(0, k + 5, (5, 23)).astype(np.uint16)
        table = rng.integers(0, min(2 << bits, 0xFFFF), k + 1).astype(np.uint16)
        table[rng.random(k + 1) < 0.2] = R.DROPPED
        slow, fast = R.remap(a, k, table, bits), R.remap_fast(a, k, table, bits)
        assert np.array_equal(slow[0], fast[0]) and slow[1] == fast[1] and slow[1] > 0
        assert np.array_equal(R.pack(slow[0], bits), R.pack_fast(slow[0], bits))
    a = rng.integers(0, 12, 1000)
    assert R.usage(a, 8).tolist() == [int((a == i).sum()) for i in range(9)] + [int((a > 8).sum())]


# ---- the command line and the writer -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["reduce", "-c", "4", "--optimize"], ["reduce", "-c", "4", "--optimize", "luma"],
                                  ["find", "-p", "#000000,#ffffff", "--optimize"], ["reduce", "-c", "4", "--indexed", "--optimize", "bogus"],
                                  ["palette", "-c", "4", "--optimize"]])
def test_cli_refuses(argv, tmp_path, capsys):
    from PIL import Image
    from kmeans_gpu_amd import cli
    path = str(tmp_path / "a.png")
    Image.fromarray(np.zeros((4, 4, 4), np.uint8), "RGBA").save(path)
    with pytest.raises(SystemExit) as e:
        cli.main(argv[:1] + ["-i", path] + argv[1:])
    assert e.value.code == 2
    assert "--optimize" in capsys.readouterr().err


@pytest.mark.parametrize("transparent", [False, True])
@pytest.mark.parametrize("bits", [1, 2, 4, 8])
def test_packed_png_decodes_through_pil(bits, transparent):
    from PIL import Image
    from kmeans_gpu_amd import png8
    rng = np.random.default_rng(bits)
    n = 1 << bits if bits < 8 else 200
    pal = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    pal[:, 3] = 255
    if transparent:
        pal[0] = 0
    for width, height in ((1, 1), (7, 3), (8, 2), (13, 5), (64, 4), (37, 11)):
        index = rng.integers(0, n, (height, width)).astype(np.uint8)
        rows = R.pack(index, bits)
        blob = png8.encode(pal, width, height, rows, bits, transparent_first=transparent)
        got = np.array(Image.open(io.BytesIO(blob)).convert("RGBA"))
        assert np.array_equal(got, pal[index]), (bits, width, height)
        assert blob[24] == bits and blob[25] == 3                        # IHDR: bit depth, colour type
        assert (b"tRNS" in blob) == transparent
    with pytest.raises(ValueError):
        png8.encode(pal, 4, 4, np.zeros((4, 4), np.uint8), 2 if bits != 2 else 4)
    with pytest.raises(ValueError):
        png8.encode(np.zeros(((1 << bits) + 1, 3), np.uint8), 4, 1, np.zeros((1, (4 * bits + 7) // 8), np.uint8), bits)
