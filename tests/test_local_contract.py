"""The contract of per-frame palettes (include/kmeans_hip.h at kmg_dev_frame_delta_colour) on the CPU, from
tests/local_ref.py: the vectorised rules against the literal loops, the two consequences the header states (same palette,
duplicate entries), a palette change under an unchanged map, bands, replay through per-frame palettes.  Also the pieces that need
no device: the GIF writer against local_ref.gif_decode, the ABI, the CLI's refusals."""
import ctypes as C

import numpy as np
import pytest

import hold_ref
import local_ref as R
import sequence_ref


def _palette(rng, k, duplicates=False):
    """k distinct non-zero words (alpha 255); with `duplicates`, some entries repeat another one's bytes"""
    seen, rows = set(), []
    while len(rows) < k:
        c = tuple(int(x) for x in rng.integers(0, 256, 3))
        if c not in seen:
            seen.add(c)
            rows.append(c + (255,))
    pal = np.array(rows, np.uint8)
    if duplicates and k >= 2:
        for j in rng.integers(1, k, max(1, k // 4)):
            pal[j] = pal[rng.integers(0, j)]
    return pal


def _case(rng, rows, width, k, dtype, above=True):
    """a random band: a held source, a source that equals it / is near it / is far from it, an index map (slot k and, with `above`,
    indices above k included) and a shown canvas made of another palette's words, this palette's words and zeros"""
    held = rng.integers(0, 256, (rows, width, 4)).astype(np.uint8)
    kind = rng.integers(0, 3, (rows, width))
    near = np.clip(held.astype(np.int64) + rng.integers(-3, 4, held.shape), 0, 255).astype(np.uint8)
    far = rng.integers(0, 256, held.shape).astype(np.uint8)
    src = np.where((kind == 0)[..., None], held, np.where((kind == 1)[..., None], near, far)).astype(np.uint8)
    pal = _palette(rng, k, duplicates=True)
    top = np.iinfo(dtype).max
    index = rng.integers(0, k + 1, (rows, width)).astype(dtype)
    if above and k < top:
        hi = rng.random((rows, width)) < 0.05
        index[hi] = rng.integers(k + 1, top + 1, int(hi.sum())).astype(dtype)
    other = R.words(_palette(rng, k))
    was = rng.integers(0, k + 1, (rows, width))
    shown = np.where(rng.random((rows, width)) < 0.5, R.lookup(was, pal, k)[1], np.concatenate([other, np.zeros(1, np.uint32)])[was]).astype(np.uint32)
    same = rng.random((rows, width)) < 0.3
    shown[same] = R.lookup(index, pal, k)[1][same]
    return src, index, shown, held, pal


@pytest.mark.parametrize("dtype,k", [(np.uint8, 255), (np.uint8, 1), (np.uint8, 5), (np.uint16, 3072), (np.uint16, 256)])
def test_vectorised_rules_equal_the_loops(oracle, dtype, k):
    rng = np.random.default_rng(k)
    for rows, width, tol in ((1, 1, 0), (3, 5, 500), (7, 9, 4096), (6, 11, 40000), (4, 4, hold_ref.D_MAX)):
        src, index, shown, held, pal = _case(rng, rows, width, k, dtype)
        a, b = R.colour(index, shown, pal, k, row0=3), R.colour_loop(index, shown, pal, k, row0=3)
        assert a[2] == b[2] and a[0].dtype == b[0].dtype == dtype
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert int(a[0].max()) <= k
        a = R.lossy(oracle, src, index, shown, held, pal, k, tol, row0=3)
        b = R.lossy_loop(oracle, src, index, shown, held, pal, k, tol, row0=3)
        assert a[3] == b[3]
        for x, y in zip(a[:3], b[:3]):
            assert x.dtype == y.dtype and np.array_equal(x, y)


@pytest.mark.parametrize("dtype,k", [(np.uint8, 255), (np.uint8, 2), (np.uint16, 700)])
def test_same_palette_is_the_index_pass(oracle, dtype, k):
    """one palette, distinct non-zero entries, indices <= k: the delta map and record of sequence_ref.delta / hold_ref.hold, and
    shown == P'[canvas] afterwards"""
    rng = np.random.default_rng(k + 7)
    pal = _palette(rng, k)
    assert len(set(R.words(pal).tolist())) == k and (R.words(pal) != 0).all()
    rows, width = 9, 13
    held = rng.integers(0, 256, (rows, width, 4)).astype(np.uint8)
    src = np.where(rng.random((rows, width, 1)) < 0.5, held, rng.integers(0, 256, held.shape)).astype(np.uint8)
    canvas = rng.integers(0, k + 1, (rows, width)).astype(dtype)
    index = np.where(rng.random((rows, width)) < 0.5, canvas, rng.integers(0, k + 1, (rows, width))).astype(dtype)
    index[rng.random((rows, width)) < 0.1] = k
    canvas[0, 0], index[0, 0] = 0, k                                     # (a shown pixel that turns transparent, whatever k)
    shown = R.lookup(canvas, pal, k)[1]
    d, new_canvas, rec = sequence_ref.delta(index, canvas, k, row0=2)
    got = R.colour(index, shown, pal, k, row0=2)
    assert got[2] == rec and np.array_equal(got[0], d) and np.array_equal(got[1], R.lookup(new_canvas, pal, k)[1])
    assert rec[0] > rec[1] > 0
    for tol in (0, 3000, 0xFFFFFFFF):
        d, new_canvas, new_held, rec = hold_ref.hold(oracle, src, index, canvas, held, k, tol, row0=2)
        got = R.lossy(oracle, src, index, shown, held, pal, k, tol, row0=2)
        assert got[3] == rec and np.array_equal(got[0], d) and np.array_equal(got[2], new_held)
        assert np.array_equal(got[1], R.lookup(new_canvas, pal, k)[1])


def test_duplicate_entries_are_not_sent():
    k = 4
    pal = np.array([[10, 20, 30, 255], [200, 100, 50, 255], [10, 20, 30, 255], [1, 2, 3, 255]], np.uint8)   # entry 2 repeats entry 0
    canvas = np.array([[0, 1, 2, 3, 0]], np.uint8)
    index = np.array([[2, 1, 0, 3, 1]], np.uint8)
    shown = R.lookup(canvas, pal, k)[1]
    d, new_shown, rec = R.colour(index, shown, pal, k)
    assert d.tolist() == [[k, k, k, k, 1]] and rec == (1, 0, 4, 0, 5, 1)
    assert np.array_equal(new_shown, R.lookup(index, pal, k)[1])
    assert sequence_ref.delta(index, canvas, k)[2][0] == 3               # the index pass would send the two swaps as well


def test_a_palette_change_under_an_unchanged_map_sends_the_changed_entries():
    rng = np.random.default_rng(5)
    k, rows, width = 16, 12, 17
    pal = _palette(rng, k)
    index = rng.integers(0, k + 1, (rows, width)).astype(np.uint8)
    shown = R.lookup(index, pal, k)[1]
    new = pal.copy()
    moved = [3, 7, 11]
    for j in moved:
        new[j, :3] = new[j, :3] ^ 0x55
    d, new_shown, rec = R.colour(index, shown, new, k)
    want = np.isin(index, moved)
    assert want.any() and np.array_equal(d != k, want) and np.array_equal(d[want], index[want])
    assert rec[0] == int(want.sum()) and rec[1] == 0 and np.array_equal(new_shown, R.lookup(index, new, k)[1])
    assert R.colour(index, shown, pal, k)[2] == R.FRESH6                   # the same palette: nothing to send


def test_bands_combine_to_the_frame(oracle):
    rng = np.random.default_rng(11)
    k = 40
    src, index, shown, held, pal = _case(rng, 9, 13, k, np.uint8)
    whole = R.lossy(oracle, src, index, shown, held, pal, k, 3000)
    exact = R.colour(index, shown, pal, k)
    for cut in (1, 4, 8):
        top = R.lossy(oracle, src[:cut], index[:cut], shown[:cut], held[:cut], pal, k, 3000)
        bottom = R.lossy(oracle, src[cut:], index[cut:], shown[cut:], held[cut:], pal, k, 3000, row0=cut)
        assert R.combine(top[3], bottom[3]) == R.combine(bottom[3], top[3]) == whole[3]
        for i in range(3):
            assert np.array_equal(np.concatenate([top[i], bottom[i]]), whole[i])
        a, b = R.colour(index[:cut], shown[:cut], pal, k), R.colour(index[cut:], shown[cut:], pal, k, row0=cut)
        assert R.combine(a[2], b[2]) == exact[2]
    assert R.combine(R.FRESH8, whole[3]) == whole[3] and R.combine(R.FRESH6, exact[2]) == exact[2]


def test_replay_reproduces_the_maps(oracle):
    """exact frames with a new palette each: the replay shows P_t[I_t]; with lossy frames in between it shows the model's canvas"""
    rng = np.random.default_rng(21)
    k, h, w, n = 12, 10, 14, 7
    frames = [rng.integers(0, 256, (h, w, 4)).astype(np.uint8)]
    for _ in range(n - 1):
        f = np.clip(frames[-1].astype(np.int64) + rng.integers(-1, 2, frames[-1].shape), 0, 255).astype(np.uint8)
        f[rng.random((h, w)) < 0.2] = rng.integers(0, 256, 4)
        frames.append(f)
    maps = [rng.integers(0, k, (h, w)).astype(np.uint8) for _ in range(n)]
    palettes = [_palette(rng, k, duplicates=t % 2 == 1) for t in range(n)]
    states = R.encode(oracle, frames, maps, palettes, k, [None] * n)
    shown = R.replay_colour([(s["map"], P, s["is_full"]) for s, P in zip(states, palettes)], k)
    for t in range(n):
        assert not states[t]["is_full"] and np.array_equal(shown[t], R.lookup(maps[t], palettes[t], k)[1])
        assert np.array_equal(states[t]["held"], frames[t])
    tolerances = [None, 5000, 5000, None, 5000, 0, 0xFFFFFFFF]
    deltas = [True, True, True, False, True, True, True]
    states = R.encode(oracle, frames, maps, palettes, k, tolerances, deltas)
    shown = R.replay_colour([(s["map"], P, s["is_full"]) for s, P in zip(states, palettes)], k)
    for t in range(n):
        assert np.array_equal(shown[t], states[t]["shown"]), t
    assert states[3]["is_full"] and states[3]["record"] == R.FRESH8
    assert states[1]["record"][6] > 0 and states[1]["record"][0] > 0
    assert states[6]["record"][0] == 0                                   # everything shows a colour: everything is held
    # a shown pixel that turns transparent: the frame comes back in full, and every pixel is anchored anew
    maps[2][1, 1] = k
    states = R.encode(oracle, frames, maps, palettes, k, tolerances, deltas)
    assert states[2]["is_full"] and states[2]["record"][1] == 1 and np.array_equal(states[2]["held"], frames[2])
    assert np.array_equal(states[2]["shown"], R.lookup(maps[2], palettes[2], k)[1])


# ---- the GIF writer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 255])
def test_gif_round_trip(oracle, k):
    from kmeans_gpu_amd import gif
    rng = np.random.default_rng(k)
    h, w = 23, 31
    frames, coded = [], []
    shown = np.zeros((h, w), np.uint32)
    ks = [k, max(1, k // 2), k]                                          # local tables of different sizes
    for t, kt in enumerate(ks):
        pal = _palette(rng, kt)
        index = rng.integers(0, kt, (h, w)).astype(np.uint8)
        if t:
            keep = np.ones((h, w), bool)
            keep[3 + t:15 + t, 5:20 + t] = rng.random((12, 15 + t)) < 0.3
            index[keep] = 255                                            # far above kt: written as the transparent index
        d, shown, rec = R.colour(index, shown, pal, kt)
        rect = None if t == 0 else rec[2:6]
        frames.append({"indices": d, "palette": pal, "rect": rect, "delay": 7 + t, "disposal": 1})
        coded.append((d, pal, kt, rect))
    data = gif.encode(w, h, frames, loop=3)
    got = R.gif_decode(data)
    assert (got["width"], got["height"], got["global_table"], got["loop"]) == (w, h, None, 3) and len(got["frames"]) == 3
    for t, (fr, (d, pal, kt, rect)) in enumerate(zip(got["frames"], coded)):
        x0, y0, x1, y1 = rect or (0, 0, w, h)
        assert (fr["x"], fr["y"], fr["w"], fr["h"]) == (x0, y0, x1 - x0, y1 - y0)
        assert fr["delay"] == 7 + t and fr["disposal"] == 1 and fr["transparent"] == kt
        assert fr["table"].shape[0] == 1 << gif.table_bits(kt) >= kt + 1 and fr["table"].shape[0] < 2 * (kt + 1) + 1
        assert np.array_equal(fr["table"][:kt], pal[:, :3])
        assert np.array_equal(fr["indices"], np.minimum(d[y0:y1, x0:x1], kt))
    want = []
    canvas = np.zeros((h, w), np.uint32)
    for d, pal, kt, rect in coded:
        canvas = np.where(np.minimum(d, kt) == kt, canvas, R.lookup(d, pal, kt)[1]).astype(np.uint32)
        want.append(canvas)
    for a, b in zip(R.gif_canvases(got), want):
        assert np.array_equal(a, b)


def test_gif_lzw_fills_the_table_and_sends_a_clear_code():
    from kmeans_gpu_amd import gif
    rng = np.random.default_rng(9)
    h, w, k = 64, 400, 255                                               # 25 600 random bytes: several tables of 4096 codes
    pal = _palette(rng, k)
    index = rng.integers(0, k, (h, w)).astype(np.uint8)
    got = R.gif_decode(gif.encode(w, h, [{"indices": index, "palette": pal, "disposal": 2}], loop=None))
    fr = got["frames"][0]
    assert got["loop"] is None and fr["clears"] >= 3 and fr["disposal"] == 2 and np.array_equal(fr["indices"], index)
    # a flat map: long runs, the code width grows without a clear
    flat = np.zeros((h, w), np.uint8)
    fr = R.gif_decode(gif.encode(w, h, [{"indices": flat, "palette": pal}]))["frames"][0]
    assert fr["clears"] == 1 and np.array_equal(fr["indices"], flat)
    # the smallest image
    fr = R.gif_decode(gif.encode(1, 1, [{"indices": np.zeros((1, 1), np.uint8), "palette": pal[:1]}]))["frames"][0]
    assert fr["indices"].tolist() == [[0]] and fr["table"].shape[0] == 2
    for bad in ({"indices": flat, "palette": np.zeros((256, 4), np.uint8)}, {"indices": flat[:, :5], "palette": pal},
                {"indices": flat, "palette": pal, "rect": (5, 5, 5, 9)}):
        with pytest.raises(ValueError):
            gif.encode(w, h, [bad])
    with pytest.raises(ValueError):
        gif.encode(w, h, [])


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
NEW = ("kmg_dev_frame_delta_colour", "kmg_dev_frame_delta_colour_lossy", "kmg_sequence_output_begin_local", "kmg_sequence_output_frame_local")


def test_new_symbols_are_declared_and_exported():
    import kmeans_gpu_amd as kg
    from test_abi import _declared
    L = C.CDLL(kg.library_path())
    for name in NEW:
        assert name in _declared() and name in kg.SYMBOLS and hasattr(L, name), name
    assert kg.LOCAL_WARM == 1 and "LOCAL_WARM" in kg.__all__
    assert b"k_frame_local" in open(kg.library_path(), "rb").read()


def test_refusals_without_a_device():
    import kmeans_gpu_amd as kg
    L = kg.lib()
    buf = (C.c_uint8 * 64)()
    ptr = C.cast(buf, C.c_void_p)
    # the format and k are checked before anything else, as in kmg_dev_frame_delta
    assert L.kmg_dev_frame_delta_colour(None, ptr, ptr, ptr, 4, 4, 0, 0, 5, ptr, ptr, None) == -1
    assert b"RGBA8" in L.kmg_last_error()
    assert L.kmg_dev_frame_delta_colour(None, ptr, ptr, ptr, 4, 4, 0, 1, 256, ptr, ptr, None) == -1
    assert b"INDEX16" in L.kmg_last_error()
    assert L.kmg_dev_frame_delta_colour(None, ptr, ptr, ptr, 4, 4, 0, 1, 5, ptr, ptr, None) == -1
    assert b"NULL" in L.kmg_last_error()
    assert L.kmg_dev_frame_delta_colour_lossy(None, ptr, ptr, ptr, ptr, ptr, 4, 4, 0, 2, 4000, 10, ptr, ptr, None) == -1
    assert b"k = 4000" in L.kmg_last_error()
    assert L.kmg_dev_frame_delta_colour_lossy(None, ptr, ptr, ptr, ptr, ptr, 4, 4, 0, 2, 40, 10, ptr, ptr, None) == -1
    assert b"NULL" in L.kmg_last_error()
    assert L.kmg_sequence_output_begin_local(None, 8, 0, 1, 4, 4, 0) == -1
    assert b"NULL" in L.kmg_last_error()
    assert L.kmg_sequence_output_frame_local(None, ptr, 1, None, ptr, ptr, None, None, None) == -1
    assert b"NULL" in L.kmg_last_error()


@pytest.mark.parametrize("extra,word", [(["--local", "--optimize"], "--optimize"), (["--local", "--warm", "--fixed", "ff0000"], "--warm"),
                                        (["--warm"], "--local"), (["--local", "-c", "256"], "255")])
def test_cli_refuses(extra, word, tmp_path, capsys):
    from PIL import Image
    from kmeans_gpu_amd import cli
    path = str(tmp_path / "a.png")
    Image.fromarray(np.zeros((4, 4, 4), np.uint8), "RGBA").save(path)
    with pytest.raises(SystemExit) as e:
        cli.main(["sequence", "-i", path, "-c", "2"] + extra)
    assert e.value.code == 2
    assert word in capsys.readouterr().err
