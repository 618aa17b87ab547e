"""The model of fixed palette colours (tests/fixed_ref.py) against the oracle, on the CPU: with no pin it IS the oracle's
initialisation and Lloyd loop, bit for bit; pins survive the loop; k = f returns the pins; a flat image exercises the tie rule."""
import numpy as np
import pytest

import fixed_ref as R


def _image(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h * w, 4), dtype=np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("w,h,k", [(97, 61, 8), (5, 3, 4), (64, 48, 33), (31, 1, 2)])
def test_no_pin_is_the_oracle(oracle, w, h, k):
    lab = oracle.rgb_to_lab(_image(w * h + k, w, h))
    want = oracle.init_centroids(lab, w, h, k)
    got = R.init_centroids(oracle, lab, w, h, k, np.zeros((0, 4), np.float32))
    assert np.array_equal(_bits(got), _bits(want))
    wc, wl, wit = oracle.lloyd(lab, want)
    gc, gl, git = R.lloyd(oracle, lab, got, 0)
    assert np.array_equal(_bits(gc), _bits(wc)) and np.array_equal(gl, wl) and git == wit
    # other loop settings, the early exit of the convergence check included
    wc, wl, wit = oracle.lloyd(lab, want, max_iterations=7, check_period=2, convergence=50.0)
    gc, gl, git = R.lloyd(oracle, lab, got, 0, max_iterations=7, check_period=2, convergence=50.0)
    assert np.array_equal(_bits(gc), _bits(wc)) and np.array_equal(gl, wl) and git == wit


def test_argmax_forms_agree():
    rng = np.random.default_rng(3)
    for n in (1, 15, 16, 17, 100, 257):
        for levels in (1, 2, 5, 1000):
            d = rng.integers(0, levels, n).astype(np.float32)
            assert R._argmax(d) == R._argmax_fast(d), (n, levels)
    assert R._argmax_fast(np.zeros(40, np.float32)) == 0


@pytest.mark.parametrize("f", [1, 3, 5])
def test_pins_survive_the_loop(oracle, f):
    w, h, k = 40, 30, 8
    px = _image(11, w, h)
    colours = np.array([[0, 0, 0, 255], [255, 255, 255, 255], [255, 0, 0, 255], [255, 0, 0, 255], [12, 200, 90, 255]], np.uint8)[:f]
    pins = R.pins_lab(oracle, colours)
    lab = oracle.rgb_to_lab(px)
    c0 = R.init_centroids(oracle, lab, w, h, k, pins)
    assert np.array_equal(_bits(c0[:f]), _bits(pins))
    cent, labels, it = R.lloyd(oracle, lab, c0, f)
    assert np.array_equal(_bits(cent[:f]), _bits(pins))
    assert not np.array_equal(_bits(cent[f:]), _bits(c0[f:]))      # the free ones moved
    assert np.array_equal(labels, oracle.assign(lab, cent))
    # the free centroids were placed knowing the pins: none of the picks is a pixel at distance 0 of a pin
    for j in range(f, k):
        assert min(oracle.cie94(c0[j, :3], pins[q, :3]) for q in range(f)) > 0.0


def test_every_centroid_pinned(oracle):
    w, h = 20, 10
    px = _image(5, w, h)
    colours = np.array([[0, 0, 0, 0], [255, 255, 255, 0], [0, 0, 255, 0]], np.uint8)
    cent, it = R.palette_centroids(oracle, px, w, h, 3, colours)
    assert np.array_equal(_bits(cent), _bits(R.pins_lab(oracle, colours)))
    assert it == 8                                                  # all converged from the start: the first check, it = check_period
    _, it = R.palette_centroids(oracle, px, w, h, 3, colours, check_period=3)
    assert it == 3
    _, it = R.palette_centroids(oracle, px, w, h, 3, colours, max_iterations=5)
    assert it == 4                                                  # no check before max_iterations: the reference's last iteration


def test_flat_image_ties(oracle):
    # every distance ties: the earliest pixel of the LAST block of 16 wins while the distance is positive, pixel 0 once it is 0
    w, h = 11, 3                                                    # 33 pixels: blocks [0, 16), [16, 32), [32, 33)
    px = np.tile(np.array([[90, 120, 30, 255]], np.uint8), (w * h, 1))
    px[32] = (91, 120, 30, 255)                                     # what the arg-max names is visible in the pick
    lab = oracle.rgb_to_lab(px)
    pins = R.pins_lab(oracle, np.array([[200, 10, 10, 255]], np.uint8))
    cent = R.init_centroids(oracle, lab, w, h, 3, pins)
    d = R._distances(oracle, lab, pins[0])
    far = 32 if d[32] >= d[0] else 16                               # a tie among [0, 32) goes to pixel 16; pixel 32 needs >=
    assert np.array_equal(_bits(cent[1, :3]), _bits(lab[far]))
    assert np.array_equal(_bits(cent[2, :3]), _bits(lab[16 if far == 32 else 32]))
    # a pin equal to the only colour: every distance is 0 -> Candidate(0, 0.0) -> pixel 0
    px[:] = (90, 120, 30, 255)
    lab = oracle.rgb_to_lab(px)
    pins = np.ones((1, 4), np.float32)
    pins[0, :3] = lab[0]
    cent = R.init_centroids(oracle, lab, w, h, 2, pins)
    assert np.array_equal(_bits(cent[1, :3]), _bits(lab[0]))
