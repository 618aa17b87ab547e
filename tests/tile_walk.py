"""Which pixels to probe in a band that makes a workgroup of the delta passes walk several tiles: a test-side mirror of
the grid and the tile runs of k_frame_delta (kmg_sequence.hip), k_frame_hold (kmg_hold.hip), k_frame_local (kmg_local.hip) and
k_clip_hold (kmg_clip.hip), and of the per-lane (x, y) cursor those four kernels carry from tile to tile.  The cursor feeds nothing but
the box of the records, so a test sees it only where ONE known pixel changes: the probes below are those pixels.

  walk(n, width, tile, shift)   the launch: tiles, grid, tiles per workgroup (`per`), the runs [t0, t1), the cursor's step
  probes(w)                     at most MAX_PROBES pixels (flat index, labels) that cover the classes of CLASSES
  required(w)                   the classes this launch must show
  cursor(w, i)                  the kernels' recurrence replayed for pixel i: one division at the run's start, the tile step, the
                                walk inside the lane's group
  shapes(tile)                  the bands the GPU tests use, with the `per` each is chosen for

tests/test_tile_walk.py pins all of it on the CPU."""
from collections import namedtuple

# kmeans-gpu_amd/csrc/kmg_pass.h: kPassMaxGrid (line 23), kPassBlock (line 20), kPassTile = kPassBlock * 4 (line 22), pass_grid
# (line 26), tile_run (lines 29-34); kmeans-gpu_amd/csrc/kmg_sequence.hip: delta_tiles (lines 30-34: a lane takes 16 bytes) and the
# launcher's step (line 178); include/kmeans_hip.h: KMG_CLIP_FRAMES
WORKGROUPS = 2048
LANES = 256
PIXELS_PER_LANE = 4
BYTES_PER_LANE = 16
MAX_PROBES = 32

CLASSES = ("lane0", "lane255", "first_tile", "second_tile", "last_tile", "wg0", "wg1", "wg_mid", "wg_last", "straddle", "wrapped",
           "last_pixel", "ragged", "first_chunk")

Walk = namedtuple("Walk", "n width tile group shift tiles grid per runs nonempty step_x step_y")
Probe = namedtuple("Probe", "i labels")


def tile_elems(kernel, itemsize=1):
    """elements of one tile: "delta" (k_frame_delta: 16 bytes per lane) or "hold" (the other three: 4 pixels per lane)"""
    return LANES * (BYTES_PER_LANE // itemsize if kernel == "delta" else PIXELS_PER_LANE)


def walk(n, width, tile, shift=0):
    """shift: elements between the 16-byte boundary below the pointers and the band (k_frame_delta alone; chunk c of a lane covers
    the flat elements [c group - shift, (c + 1) group - shift))"""
    group = tile // LANES
    tiles = ((n + shift + group - 1) // group + LANES - 1) // LANES
    grid = min(max(tiles, 1), WORKGROUPS)
    per = (tiles + grid - 1) // grid
    runs = []
    for b in range(grid):
        t0 = min(b * per, tiles)
        runs.append((t0, min(t0 + per, tiles)))
    nonempty = sum(1 for t0, t1 in runs if t0 < t1)
    return Walk(n, width, tile, group, shift, tiles, grid, per, runs, nonempty, tile % width, tile // width)


def locate(w, i):
    """(workgroup, tile, lane, position in the lane's group) of flat element i"""
    e = i + w.shift
    t = e // w.tile
    return t // w.per, t, (e % w.tile) // w.group, e % w.group


def _group_start(w, t, lane):
    return t * w.tile + lane * w.group - w.shift


def _straddles(w, lo):
    """the first element of a new row inside the group that starts at lo (not at its first position), or None"""
    r = (max(lo, 0) // w.width + 1) * w.width
    return r if r <= lo + w.group - 1 and r < w.n else None


def _wrapped(w, t0, t, lane):
    """did the tile step take its wrap on the way from tile t0 to tile t?"""
    x = _group_start(w, t0, lane) % w.width
    hit = False
    for _ in range(t - t0):
        x += w.step_x
        if x >= w.width:
            x -= w.width
            hit = True
    return hit


def labels_of(w, i):
    wg, t, lane, j = locate(w, i)
    t0, t1 = w.runs[wg]
    out = set()
    if lane == 0:
        out.add("lane0")
    if lane == LANES - 1:
        out.add("lane255")
    if t == t0:
        out.add("first_tile")
    if t == t0 + 1:
        out.add("second_tile")
    if t == t1 - 1:
        out.add("last_tile")
    for name, b in (("wg0", 0), ("wg1", 1), ("wg_mid", w.nonempty // 2), ("wg_last", w.nonempty - 1)):
        if wg == b:
            out.add(name)
    if t > t0:
        if _straddles(w, i - j) is not None:
            out.add("straddle")
        if _wrapped(w, t0, t, lane):
            out.add("wrapped")
    if i == w.n - 1:
        out.add("last_pixel")
    if t == w.tiles - 1 and (w.n + w.shift) % w.tile != 0:
        out.add("ragged")
    if w.shift and i + w.shift < w.group:
        out.add("first_chunk")
    return frozenset(out)


def required(w):
    """A lane group can straddle a row end only where the width is no multiple of the group (a width of 1000 does not divide the
    tile, yet every row end is a group's end); the tile step can wrap only where step_x != 0."""
    need = set(CLASSES) - {"straddle", "wrapped", "ragged", "first_chunk"}
    if w.width % w.group != 0:
        need.add("straddle")
    if w.step_x != 0:
        need.add("wrapped")
    if (w.n + w.shift) % w.tile != 0:
        need.add("ragged")
    if w.shift:
        need.add("first_chunk")
    return need


def probes(w):
    picked = {}

    def take(i):
        if 0 <= i < w.n and i not in picked:
            picked[i] = None

    mid = w.nonempty // 2
    for a, b in enumerate((0, 1, mid, w.nonempty - 1)):
        t0, t1 = w.runs[b]
        for c, t in enumerate(dict.fromkeys((t0, min(t0 + 1, t1 - 1), t1 - 1))):
            for lane in (0, LANES - 1):
                lo = _group_start(w, t, lane)
                j = (a + 2 * c + lane) % w.group                       # every position of the group gets its turn
                ok = [q for q in range(w.group) if 0 <= lo + q < w.n]
                if ok:
                    take(lo + min(ok, key=lambda q: (abs(q - j), q)))
    # a group that straddles a row end, and a lane whose tile step wrapped, both behind the first tile of a middle run
    t0, t1 = w.runs[mid]
    for t in range(t0 + 1, t1):
        found = [_straddles(w, _group_start(w, t, lane)) for lane in range(LANES)]
        found = [r for r in found if r is not None]
        if found:
            take(found[len(found) // 2])
            break
    for b in range(mid, min(mid + 2 * w.group, w.nonempty)):           # (a width of tile - 1 wraps in one workgroup of group / 2)
        t0, t1 = w.runs[b]
        found = [(t, lane) for t in range(t0 + 1, t1) for lane in range(LANES)
                 if _wrapped(w, t0, t, lane) and 0 <= _group_start(w, t, lane) < w.n - w.group]
        if found:
            t, lane = found[len(found) // 2]
            take(_group_start(w, t, lane) + (lane % w.group))
            break
    take(w.n - 1)
    if (w.n + w.shift) % w.tile != 0:
        first = max((w.tiles - 1) * w.tile - w.shift, 0)
        take(first + (w.n - first) // 2)
    if w.shift:
        take(0)
    out = [Probe(i, labels_of(w, i)) for i in picked]
    assert len(out) <= MAX_PROBES
    return out


def cursor(w, i):
    """(x, y) as the kernels reach it: the division for the lane's group in the first tile of its workgroup's run, the launcher's
    step for every further tile, then the walk inside the group"""
    wg, t, lane, j = locate(w, i)
    t0 = w.runs[wg][0]
    lo = _group_start(w, t0, lane)
    y = lo // w.width if lo >= 0 else -((-lo + w.width - 1) // w.width)
    x = lo - y * w.width
    for _ in range(t - t0):
        xs = x + w.step_x
        y += w.step_y
        if xs >= w.width:
            x, y = xs - w.width, y + 1
        else:
            x = xs
    for _ in range(j):
        x += 1
        if x == w.width:
            x, y = 0, y + 1
    return x, y


def shapes(tile):
    """(name, width, rows, per): the T = 1024 bands, scaled by tile / 1024 where the width or the tile count has to follow the tile"""
    s = tile // 1024
    return [("below", 1000 * s, 4300, 3),                               # step_y = 1, rare wraps
            ("equal", tile, 4100, 3),                                   # step_x = 0
            ("minus1", tile - 1, 2101, 2),
            ("mid", 300 * s, 14000, 3),                                 # step_y = 3
            ("three", 3, 1400000 * s + 1, 3),                           # every group straddles rows
            ("one", 1, 2048 * tile + 5, 2)]                             # 2049 tiles: 1023 trailing workgroups are empty


BAND_ROW0 = 101                         # the two-band runs cut "below" here: the second band alone has more than 2048 tiles


def pairs(ps):
    """a few pairs of probes from different workgroups"""
    by = {}
    for p in ps:
        for name in ("wg0", "wg1", "wg_mid", "wg_last"):
            if name in p.labels:
                by.setdefault(name, []).append(p)
    out = []
    for a, b in (("wg0", "wg_last"), ("wg1", "wg_mid"), ("wg_mid", "wg_last")):
        if a in by and b in by and by[a][-1].i != by[b][0].i:
            out.append((by[a][-1], by[b][0]))
    return out
