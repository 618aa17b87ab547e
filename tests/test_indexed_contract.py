"""The index formats' sentinel argument and the CLI's palette-PNG writer, without a GPU.

The dither scan starts from the reference's sentinel (10000, 10000, 10000) as label k and takes a centroid only if it is strictly
closer; the index formats promise that the sentinel never wins, for centroids inside the box L in [-100, 200], a, b in [-300, 300].
Here the oracle's orc_assign runs the same first-minimum scan with the sentinel FIRST (so it keeps every tie, as the dither scan
does) over all 2^24 sRGB8 colours shifted by the two extreme Bayer offsets of tables at the corners of the box -- the widest pair
(which gives the largest dither threshold the box allows) and all eight corners -- and must never return the sentinel."""
import itertools

import numpy as np
import pytest

BOX = ((-100.0, 200.0), (-300.0, 300.0), (-300.0, 300.0))
SENTINEL = (10000.0, 10000.0, 10000.0)
CORNERS = np.array(list(itertools.product(*BOX)), np.float32)


def _tables():
    pairs = [np.stack([c, np.array([BOX[i][1] + BOX[i][0] - c[i] for i in range(3)], np.float32)]) for c in CORNERS[:4]]
    return pairs + [CORNERS]


def _all_colours_lab(oracle):
    v = np.arange(1 << 24, dtype=np.uint32)
    rgba = np.empty((1 << 24, 4), np.uint8)
    rgba[:, 0], rgba[:, 1], rgba[:, 2], rgba[:, 3] = v & 255, (v >> 8) & 255, v >> 16, 255
    return oracle.rgb_to_lab(rgba)


def test_box_bounds_the_dither_threshold(oracle):
    """the largest threshold of a table in the box: the widest pair, dAB <= the Euclidean diagonal 900, over sqrt(2)"""
    thr = [oracle.dither_threshold(oracle.centroids4(t)) for t in _tables()]
    assert max(thr) <= 900.0 / np.sqrt(2.0) * (1 + 1e-6)
    assert max(thr) > 200.0                                   # (CIE94 weighs chroma down: 227 for the widest pair)


@pytest.mark.parametrize("table", range(5))
def test_sentinel_never_wins_inside_the_box(oracle, table):
    lab = _all_colours_lab(oracle)
    cent = oracle.centroids4(_tables()[table])
    thr = oracle.dither_threshold(cent)
    with_sentinel = oracle.centroids4(np.vstack([np.array([SENTINEL], np.float32), cent[:, :3]]))
    for m in (0, 15):                                         # the Bayer values of the extreme offsets: -T/2 and +7T/16
        off = np.float32(thr) * (np.float32(m) / np.float32(16.0) - np.float32(0.5))
        shifted = lab + off
        for s in range(0, shifted.shape[0], 1 << 22):
            labels = oracle.assign(shifted[s:s + (1 << 22)], with_sentinel)
            assert (labels != 0).all(), f"table {table}, offset {off}: the sentinel wins for {int((labels == 0).sum())} colours"


def test_sentinel_wins_far_outside_the_box(oracle):
    """(the check can fail: with a centroid far out of the box the sentinel does win)"""
    lab = _all_colours_lab(oracle)[:: 4099]
    far = oracle.centroids4(np.array([SENTINEL, (20000.0, 20000.0, 20000.0)], np.float32))
    assert (oracle.assign(lab, far) == 0).all()


def test_palette_png_round_trip(tmp_path):
    from PIL import Image
    from kmeans_gpu_amd.cli import save_indexed
    rng = np.random.default_rng(5)
    for n, transparent in ((1, False), (7, True), (256, False), (255, True)):
        pal = np.concatenate([rng.integers(0, 256, (n, 3)), np.full((n, 1), 255)], axis=1).astype(np.uint8)
        idx = rng.integers(0, n + (1 if transparent else 0), (13, 29)).astype(np.uint8)
        path = str(tmp_path / f"p{n}.png")
        save_indexed(path, pal, idx, transparent=transparent)
        im = Image.open(path)
        assert im.mode == "P"
        assert np.array_equal(np.array(im), idx)
        plte = np.array(im.getpalette()[:3 * n], np.uint8).reshape(n, 3)
        assert np.array_equal(plte, pal[:, :3])
        rgba = np.array(im.convert("RGBA"))
        if transparent:
            assert "transparency" in im.info
            assert (rgba[idx == n][:, 3] == 0).all() and (rgba[idx < n][:, 3] == 255).all()
        else:
            assert "transparency" not in im.info and (rgba[..., 3] == 255).all()
        assert np.array_equal(rgba[idx < n][:, :3], pal[idx[idx < n]][:, :3])
    with pytest.raises(ValueError):
        save_indexed(str(tmp_path / "x.png"), np.zeros((256, 4), np.uint8), np.zeros((2, 2), np.uint8), transparent=True)


def test_cli_refuses_what_a_palette_png_cannot_hold(tmp_path):
    from PIL import Image
    from kmeans_gpu_amd import cli
    src = str(tmp_path / "in.png")
    Image.fromarray(np.zeros((4, 4, 4), np.uint8), "RGBA").save(src)
    for argv in (["reduce", "-i", src, "-c", "257", "--indexed"],
                 ["reduce", "-i", src, "-c", "256", "--indexed", "--alpha-cutoff", "1"],
                 ["reduce", "-i", src, "-c", "8", "-m", "meld", "--indexed"],
                 ["find", "-i", src, "-p", "#000000,#ffffff", "--indexed", "-o", str(tmp_path / "o.jpg")],
                 ["--devices", "0", "reduce", "-i", src, "-c", "8", "--indexed"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
