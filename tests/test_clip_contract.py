"""The rule the clip kernels rely on, pinned on the model tests/hold_ref.py::replay -- no device:
  1. after any frame (exact, lossy, or sent in full) the canvas shows slot k exactly where that frame's map does, so frame t >= 1 is
     sent in full exactly when some pixel has I_t == k and I_{t-1} != k (frame 0: the canvas of k never clears);
  2. a clip may be cut at any frame: the state after the first part (canvas, held source) is all the second part needs."""
import numpy as np
import pytest

import hold_ref as H
import sequence_ref


def _clip(rng, T, h, w, k, p_k):
    frames, maps = [], []
    prev_f = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    for t in range(T):
        f = np.where((rng.random((h, w)) < 0.3)[..., None], rng.integers(0, 256, (h, w, 4)).astype(np.uint8),
                     np.clip(prev_f.astype(np.int64) + rng.integers(-2, 3, (h, w, 4)), 0, 255).astype(np.uint8)).astype(np.uint8)
        I = rng.integers(0, k, (h, w))
        I[rng.random((h, w)) < p_k[t]] = k
        frames.append(f); maps.append(I.astype(np.uint8))
        prev_f = f
    return frames, maps


def _full_from_maps(maps, k, canvas=None):
    """the map-only predicate: which frames clear a shown pixel"""
    out, prev = [], np.full_like(maps[0], k) if canvas is None else canvas
    for I in maps:
        out.append(bool(((I == k) & (prev != k)).any()))
        prev = I
    return out


def _replay_from(oracle, frames, maps, k, tolerances, canvas, held):
    """hold_ref.replay from a given state"""
    out = []
    for f, I, tol in zip(frames, maps, tolerances):
        if tol is None:
            d, _, rec = sequence_ref.delta(I, canvas, k)
            rec = tuple(rec)
            canvas, held = I.copy(), f.copy()
        else:
            d, canvas, held, rec = H.hold(oracle, f, I, canvas, held, k, tol)
        full = rec[1] > 0
        if full:
            canvas, held = I.copy(), f.copy()
        out.append({"map": I.copy() if full else d, "record": rec, "is_full": full, "canvas": canvas.copy(), "held": held.copy()})
    return out


def _tolerances(rng, T, mixed):
    import kmeans_gpu_amd as kg
    pool = [0, kg.tolerance_of(1.0), kg.tolerance_of(3.0), 40000, H.D_MAX] + ([None] if mixed else [])
    return [pool[int(i)] for i in rng.integers(0, len(pool), T)]


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("seed", range(6))
def test_is_full_follows_from_the_maps_alone(oracle, seed, mixed):
    rng = np.random.default_rng(seed)
    T, h, w, k = 9, 6, 11, 7
    # frames with much, little and no slot k, so that clears fall in some frames and not in others
    p_k = rng.permutation([0.0, 0.02, 0.3, 0.0, 0.3, 0.3, 0.02, 0.0, 0.3])
    frames, maps = _clip(rng, T, h, w, k, p_k)
    tolerances = _tolerances(rng, T, mixed)
    states = H.replay(oracle, frames, maps, k, tolerances)
    assert [s["is_full"] for s in states] == _full_from_maps(maps, k)
    assert not states[0]["is_full"]
    for s, I in zip(states, maps):                                   # the invariant itself
        assert np.array_equal(s["canvas"] == k, I == k)
    assert any(s["is_full"] for s in states) and not all(s["is_full"] for s in states[1:])


def test_no_slot_k_no_full_frame(oracle):
    rng = np.random.default_rng(3)
    frames, maps = _clip(rng, 6, 5, 9, 12, [0.0] * 6)
    assert not any(s["is_full"] for s in H.replay(oracle, frames, maps, 12, _tolerances(rng, 6, True)))


@pytest.mark.parametrize("mixed", [False, True])
def test_a_clip_may_be_cut_at_any_frame(oracle, mixed):
    rng = np.random.default_rng(17)
    T, h, w, k = 7, 5, 9, 6
    frames, maps = _clip(rng, T, h, w, k, rng.choice([0.0, 0.05, 0.3], T))
    tolerances = _tolerances(rng, T, mixed)
    whole = H.replay(oracle, frames, maps, k, tolerances)
    start = (np.full((h, w), k, np.uint8), np.zeros((h, w, 4), np.uint8))
    for cut in range(T + 1):
        first = _replay_from(oracle, frames[:cut], maps[:cut], k, tolerances[:cut], *start)
        state = (first[-1]["canvas"], first[-1]["held"]) if first else start
        second = _replay_from(oracle, frames[cut:], maps[cut:], k, tolerances[cut:], *state)
        assert [s["is_full"] for s in second] == _full_from_maps(maps[cut:], k, state[0])
        for got, want in zip(first + second, whole):
            assert tuple(got["record"]) == tuple(want["record"]) and got["is_full"] == want["is_full"]
            for key in ("map", "canvas", "held"):
                assert np.array_equal(got[key], want[key]), (cut, key)
