"""tests/tile_walk.py on the CPU: for every band the GPU probe tests use (test_gpu_sequence.py, test_gpu_hold.py, test_gpu_local.py,
test_gpu_clip.py) -- more than 2048 tiles, the stated tiles per workgroup, every probe class present, at most 32 probes -- and the
kernels' cursor recurrence, replayed from each probe's run start, lands on divmod(i, width)."""
import pytest

import tile_walk as W

TILES = (1024, 2048, 4096)              # the 4-pixel passes and k_frame_delta INDEX16 / INDEX8
CASES = [(tile, name, width, rows, per, 0) for tile in TILES for name, width, rows, per in W.shapes(tile)]
# k_frame_delta behind a partial first chunk (pointers 3 elements past a 16-byte boundary), and the second of two bands
CASES += [(tile, "below", W.shapes(tile)[0][1], W.shapes(tile)[0][2], 3, 3) for tile in TILES[1:]]
CASES += [(tile, "band", W.shapes(tile)[0][1], W.shapes(tile)[0][2] - W.BAND_ROW0, 3, shift) for tile in TILES
          for shift in ((0,) if tile == 1024 else (0, tile // 512))]


@pytest.mark.parametrize("tile,name,width,rows,per,shift", CASES)
def test_shape_and_probes(tile, name, width, rows, per, shift):
    n = width * rows
    w = W.walk(n, width, tile, shift)
    assert w.tiles > W.WORKGROUPS and w.grid == W.WORKGROUPS and w.per == per
    assert w.step_x == tile % width and w.step_y == tile // width
    assert sum(t1 - t0 for t0, t1 in w.runs) == w.tiles and all(a[1] == b[0] or b[0] == b[1] for a, b in zip(w.runs, w.runs[1:]))
    ps = W.probes(w)
    assert len(ps) <= W.MAX_PROBES and len({p.i for p in ps}) == len(ps)
    seen = set().union(*[p.labels for p in ps])
    assert W.required(w) <= seen, sorted(W.required(w) - seen)
    for p in ps:
        assert 0 <= p.i < n
        assert W.cursor(w, p.i) == divmod(p.i, width)[::-1], (p, W.locate(w, p.i))
    # the classes the band is there for
    if name == "one":
        assert w.tiles == 2049 and w.nonempty == 1025 and w.grid - w.nonempty == 1023
    if name in ("minus1", "three", "one"):
        assert "straddle" in seen
    if name == "equal":
        assert w.step_x == 0 and "wrapped" not in seen
    if name in ("below", "band"):
        assert w.step_y == 1 and "wrapped" in seen
    if name == "mid":
        assert w.step_y == 3
    if name == "three":
        assert w.step_y == tile // 3
    if shift:
        assert "first_chunk" in seen
    assert len(W.pairs(ps)) >= 2
    for a, b in W.pairs(ps):
        assert W.locate(w, a.i)[0] != W.locate(w, b.i)[0]


def test_every_probe_class_is_required_somewhere():
    need = set()
    for tile, _, width, rows, _, shift in CASES:
        need |= W.required(W.walk(width * rows, width, tile, shift))
    assert need == set(W.CLASSES)


@pytest.mark.parametrize("tile", TILES)
def test_cursor_everywhere_on_a_small_band(tile):
    """the recurrence itself, for every element: the model with a grid of 2048 needs a band of millions, so this one shrinks the
    tile count, not the rule -- widths around the group, a prime, the tile and beyond it"""
    for width in (1, 2, 3, 5, tile // 256, tile // 256 + 1, 97, tile - 1, tile, tile + 1):
        for shift in (0, 3):
            n = 3 * tile + 7
            w = W.walk(n, width, tile, shift)
            w = w._replace(per=w.tiles, runs=[(0, w.tiles)], nonempty=1)    # one workgroup walks every tile
            for i in range(0, n, 1 if width > 8 else 3):
                assert W.cursor(w, i) == (i % width, i // width)


@pytest.mark.parametrize("n,per,nonempty", [(2048 * 1024 - 1, 1, 2048), (2048 * 1024 + 1, 2, 1025), (2049 * 1024 + 3, 2, 1025)])
def test_uneven_partitions(n, per, nonempty):
    """the bands of test_gpu_clip.py's uneven partitions, as one row and as rows of 7"""
    for width, m in ((n, n), (7, (n + 6) // 7 * 7)):
        w = W.walk(m, width, 1024)
        assert (w.per, w.nonempty) == (per, nonempty)
        for p in W.probes(w):
            assert W.cursor(w, p.i) == divmod(p.i, width)[::-1]
