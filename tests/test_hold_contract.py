"""The contract of lossy delta frames (include/kmeans_hip.h at kmg_dev_frame_delta_lossy) on the CPU, from
tests/hold_ref.py alone: the vectorised rule against the literal loop, the combination of bands, the anchor (the held source, never
the previous frame), the invariant over replayed sequences, the two ends of the tolerance, slot k, and the full frame after a
cleared pixel.  Also the host-side pieces that need no device: the record's layout, the tolerance of a dE76 distance, the CLI's
refusals."""
import ctypes as C

import numpy as np
import pytest

import hold_ref as H
import sequence_ref


def _case(rng, rows, width, k, dtype):
    """a random band: a held source, a source that equals it / is near it / is far from it, and two index maps with slot k in both"""
    held = rng.integers(0, 256, (rows, width, 4)).astype(np.uint8)
    kind = rng.integers(0, 3, (rows, width))
    near = np.clip(held.astype(np.int64) + rng.integers(-3, 4, held.shape), 0, 255).astype(np.uint8)
    far = rng.integers(0, 256, held.shape).astype(np.uint8)
    src = np.where((kind == 0)[..., None], held, np.where((kind == 1)[..., None], near, far)).astype(np.uint8)
    src[..., 3] = rng.integers(0, 256, (rows, width))                  # (the alpha byte is not part of D)
    canvas = rng.integers(0, k + 1, (rows, width)).astype(dtype)
    index = np.where(rng.random((rows, width)) < 0.5, canvas, rng.integers(0, k + 1, (rows, width))).astype(dtype)
    index[rng.random((rows, width)) < 0.1] = k
    canvas[rng.random((rows, width)) < 0.1] = k
    return src, index, canvas, held


@pytest.mark.parametrize("dtype,k", [(np.uint8, 255), (np.uint8, 5), (np.uint16, 3072)])
def test_vectorised_rule_equals_the_loop(oracle, dtype, k):
    rng = np.random.default_rng(k)
    for rows, width, tol in ((1, 1, 0), (3, 5, 500), (7, 9, 4096), (6, 11, 40000), (4, 4, H.D_MAX)):
        src, index, canvas, held = _case(rng, rows, width, k, dtype)
        a = H.hold(oracle, src, index, canvas, held, k, tol, row0=3)
        b = H.hold_loop(oracle, src, index, canvas, held, k, tol, row0=3)
        assert a[3] == b[3]
        for x, y in zip(a[:3], b[:3]):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def test_two_bands_combine_to_the_frame(oracle):
    rng = np.random.default_rng(11)
    src, index, canvas, held = _case(rng, 9, 13, 40, np.uint8)
    whole = H.hold(oracle, src, index, canvas, held, 40, 3000)
    for cut in (1, 4, 8):
        top = H.hold(oracle, src[:cut], index[:cut], canvas[:cut], held[:cut], 40, 3000)
        bottom = H.hold(oracle, src[cut:], index[cut:], canvas[cut:], held[cut:], 40, 3000, row0=cut)
        assert H.combine(top[3], bottom[3]) == H.combine(bottom[3], top[3]) == whole[3]
        for i in range(3):
            assert np.array_equal(np.concatenate([top[i], bottom[i]]), whole[i])
    assert H.combine(H.FRESH, whole[3]) == whole[3]


def test_the_anchor_is_the_held_source_not_the_previous_frame(oracle):
    """a grey ramp, one level per frame, every frame with an exact index of its own: consecutive frames are 676 apart, frame 0 and
    frame 3 are 6084 apart (the oracle's Lab on the 1/64 grid), the tolerance lies between"""
    tol, k, n = 3000, 40, 12
    grey = [np.full((1, 1, 4), 100 + t, np.uint8) for t in range(n)]
    maps = [np.full((1, 1), t, np.uint8) for t in range(n)]
    for t in range(n - 1):
        assert int(H.distance(oracle, grey[t], grey[t + 1])[0]) <= tol
    first_far = next(t for t in range(n) if int(H.distance(oracle, grey[0], grey[t])[0]) > tol)
    assert first_far == 3
    states = H.replay(oracle, grey, maps, k, [tol] * n)
    sent = [t for t, s in enumerate(states) if s["record"][0] == 1]
    assert sent == [0, 3, 6, 9], "the pixel is sent again whenever it has drifted past the tolerance from its anchor"
    for t, s in enumerate(states):
        anchor = max(a for a in sent if a <= t)
        assert int(s["canvas"][0, 0]) == anchor and int(s["origin"][0, 0]) == anchor and int(s["held"][0, 0, 0]) == 100 + anchor
        assert s["record"][6] == (0 if t in sent else 1)
        assert s["record"][7] == (0 if t in sent else int(H.distance(oracle, grey[t], grey[anchor])[0]))
    # the wrong variant: compare with the previous frame (the held source follows every frame) -- the drift is never seen
    canvas, prev, wrong = np.full((1, 1), k, np.uint8), np.zeros((1, 1, 4), np.uint8), []
    for t in range(n):
        _, canvas, _, rec = H.hold(oracle, grey[t], maps[t], canvas, prev, k, tol)
        prev = grey[t]
        if rec[0]:
            wrong.append(t)
    assert wrong == [0] and int(canvas[0, 0]) == 0


def _noisy_frames(tokyo, n, h, w, amp, seed):
    rng = np.random.default_rng(seed)
    base = np.ascontiguousarray(tokyo[200:200 + h, 300:300 + w])
    frames = []
    for t in range(n):
        f = np.clip(base.astype(np.int64) + rng.integers(-amp, amp + 1, base.shape), 0, 255).astype(np.uint8)
        f[..., 3] = 255
        f[4 + 3 * t:12 + 3 * t, 5 + 4 * t:15 + 4 * t, :3] = (250, 20, 30)  # a block that moves across the noise
        frames.append(f)
    return frames


def check_invariant(oracle, frames, maps, k, tolerances, states):
    """after frame t, a pixel written at frame o <= t shows I_o there, and o < t only when its source is within tolerance_t of
    frame o's; a viewer that composites the maps sees exactly these canvases"""
    for t, s in enumerate(states):
        o = s["origin"]
        assert (o >= 0).all() and (o <= t).all()
        shown = np.choose(o, [np.asarray(m) for m in maps[:t + 1]]) if t else np.asarray(maps[0])
        assert np.array_equal(s["canvas"], shown)
        anchor = np.stack([np.asarray(f) for f in frames[:t + 1]])[o, np.arange(o.shape[0])[:, None], np.arange(o.shape[1])[None, :]]
        assert np.array_equal(s["held"], anchor)
        old = o < t
        if tolerances[t] is None:
            assert not old.any()
        elif old.any():
            D = H.distance(oracle, np.asarray(frames[t])[old], anchor[old])
            assert int(D.max()) <= tolerances[t]
            assert (np.asarray(maps[t])[old] != k).all() and (s["canvas"][old] != k).all()
    viewer = sequence_ref.replay([(s["map"], s["is_full"]) for s in states], k)
    for got, s in zip(viewer, states):
        assert np.array_equal(got, s["canvas"])


@pytest.mark.parametrize("mode", ["replace", "dither"])
def test_invariant_over_a_replayed_sequence(oracle, tokyo, mode):
    k, h, w = 12, 40, 56
    frames = _noisy_frames(tokyo, 7, h, w, 2, 5)
    cent = sequence_ref.centroids(oracle, frames[:2], k)
    maps = []
    for f in frames:
        lab = oracle.rgb_to_lab(f.reshape(-1, 4))
        labels = oracle.assign(lab, cent) if mode == "replace" else oracle.dither(lab, w, h, cent)
        maps.append(labels.reshape(h, w).astype(np.uint8))
    tolerances = [2000, 2000, 0, None, 6000, 300, H.D_MAX]                # (an exact frame in between, both ends of the range)
    states = H.replay(oracle, frames, maps, k, tolerances)
    check_invariant(oracle, frames, maps, k, tolerances, states)
    assert not any(s["is_full"] for s in states)
    exact = [sequence_ref.delta(maps[t], maps[t - 1], k)[2][0] for t in (1, 4)]
    lossy = [states[t]["record"][0] for t in (1, 4)]
    assert all(0 < a < b for a, b in zip(lossy, exact)), (lossy, exact)   # the block is sent, the noise is not
    assert states[1]["record"][6] > 0


def test_the_largest_tolerance_holds_every_holdable_pixel_and_slot_k_is_never_held(oracle):
    rng = np.random.default_rng(3)
    k = 9
    src, index, canvas, held = _case(rng, 24, 31, k, np.uint8)
    assert int(H.distance(oracle, src, held).max()) <= H.D_MAX
    for tol in (H.D_MAX, 0xFFFFFFFF):
        d, new_canvas, new_held, rec = H.hold(oracle, src, index, canvas, held, k, tol)
        holdable = (canvas != k) & (index != k)
        assert holdable.any() and (~holdable).any()
        assert np.array_equal(new_canvas[holdable], canvas[holdable]) and np.array_equal(new_held[holdable], held[holdable])
        assert (d[holdable] == k).all()
        assert rec[6] == int((holdable & (index != canvas)).sum())
        # slot k on either side: the exact rule, the source becomes the held source
        want_d, want_c, want_rec = sequence_ref.delta(np.where(holdable, canvas, index), canvas, k)
        assert np.array_equal(d, want_d) and np.array_equal(new_canvas[~holdable], index[~holdable])
        assert np.array_equal(new_held[~holdable], src[~holdable])
        assert rec[:6] == want_rec
    # ... and a tolerance of 0 holds exactly the pixels whose R, G, B bytes (or whose q) did not move
    d, new_canvas, new_held, rec = H.hold(oracle, src, index, canvas, held, k, 0)
    still = (H.distance(oracle, src, held) == 0).reshape(index.shape) & (canvas != k) & (index != k)
    assert np.array_equal(new_canvas, np.where(still, canvas, index)) and rec[7] == 0


def test_a_cleared_pixel_sends_the_full_frame_and_anchors_every_pixel_anew(oracle):
    rng = np.random.default_rng(8)
    k, h, w = 6, 10, 12
    frames = [rng.integers(0, 256, (h, w, 4)).astype(np.uint8) for _ in range(3)]
    frames[1] = np.clip(frames[0].astype(np.int64) + rng.integers(-1, 2, frames[0].shape), 0, 255).astype(np.uint8)
    frames[2] = np.clip(frames[1].astype(np.int64) + rng.integers(-1, 2, frames[0].shape), 0, 255).astype(np.uint8)
    maps = [rng.integers(0, k, (h, w)).astype(np.uint8) for _ in range(3)]
    maps[1][2, 3] = k                                                  # a shown pixel turns transparent
    states = H.replay(oracle, frames, maps, k, [5000, 5000, 5000])
    assert not states[0]["is_full"] and states[0]["record"][0] == h * w
    s = states[1]
    assert s["is_full"] and s["record"][1] == 1 and s["record"][6] > 0   # (the record as measured: pixels were held in the pass)
    assert np.array_equal(s["map"], maps[1]) and np.array_equal(s["canvas"], maps[1]) and np.array_equal(s["held"], frames[1])
    assert (s["origin"] == 1).all()
    s = states[2]                                                      # the next lossy frame starts from that state
    want = H.hold(oracle, frames[2], maps[2], maps[1], frames[1], k, 5000)
    assert not s["is_full"] and s["record"] == want[3] and np.array_equal(s["map"], want[0])
    assert s["origin"][2, 3] == 2 and s["canvas"][2, 3] == maps[2][2, 3]  # (it showed nothing: never held)
    check_invariant(oracle, frames, maps, k, [5000] * 3, states)


# ---- host-side pieces that need no device ----------------------------------------------------------------------------------------
def test_record_layout_and_tolerance_of_a_distance():
    import kmeans_gpu_amd as kg
    assert C.sizeof(kg.FrameHold) == 48 and C.sizeof(kg.FrameDelta) == 32
    assert [f[0] for f in kg.FrameHold._fields_[:6]] == [f[0] for f in kg.FrameDelta._fields_]
    assert kg.FrameHold.held.offset == 32 and kg.FrameHold.held_sse.offset == 40
    assert kg.FrameHold.FRESH == H.FRESH and len(kg.FrameHold.fresh_bytes()) == 48
    assert kg.FrameHold.fresh_bytes()[:32] == kg.FrameDelta.fresh_bytes()
    rec = kg.FrameHold.from_array(np.array([5, 1, (2 << 32) | 1, (4 << 32) | 3, 7, 7 * 4096 * 9], np.uint64))
    assert rec.as_tuple() == (5, 1, 1, 2, 3, 4, 7, 7 * 4096 * 9) and rec.rect == (1, 2, 3, 4) and rec.held_delta_e_rms == 3.0
    assert kg.MAX_TOLERANCE == H.D_MAX
    assert kg.tolerance_of(0) == 0 and kg.tolerance_of(1.0) == 4096 and kg.tolerance_of(2.5) == 25600
    assert kg.tolerance_of(0.0125) == 1 and kg.tolerance_of(0.011) == 0         # rint(0.64), rint(0.4956)
    for bad in (-0.5, float("nan"), 1024.0, 1e300):
        with pytest.raises(ValueError):
            kg.tolerance_of(bad)
    assert {"kmg_dev_frame_delta_lossy", "kmg_sequence_output_frame_lossy"} <= set(kg.SYMBOLS)


@pytest.mark.parametrize("extra", [["--lossy", "2", "--no-delta"], ["--lossy", "-1"], ["--lossy", "2000"], ["--lossy", "x"]])
def test_cli_refuses(extra, tmp_path, capsys):
    from PIL import Image
    from kmeans_gpu_amd import cli
    path = str(tmp_path / "a.png")
    Image.fromarray(np.zeros((4, 4, 4), np.uint8), "RGBA").save(path)
    with pytest.raises(SystemExit) as e:
        cli.main(["sequence", "-i", path, "-c", "2"] + extra)
    assert e.value.code == 2
    assert "--lossy" in capsys.readouterr().err
