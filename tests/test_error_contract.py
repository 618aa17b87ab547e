"""The contract of the error statistics (include/kmeans_hip.h at kmg_error_stats) as the model tests/error_ref.py
states it, checked on the CPU against hand-computed values and against itself (combination, index form, cutoff, invalid indices),
the overflow bound DESIGN states, and the fixed search of kmg_reduce_quality driven by the oracle on tokyo.png."""
import numpy as np
import pytest

import error_ref as R

# the range of q = rint(64 Lab) over all 2^24 colours and the bound on the per-pixel Lab term it gives
Q_MIN = (0, -5516, -6903)
Q_MAX = (6400, 6287, 6047)
LAB_TERM_BOUND = 347_973_309


def _img(rng, h, w, alpha=None):
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha is not None:
        a[..., 3] = alpha
    return a


def test_identical_images_give_zeros(oracle):
    rng = np.random.default_rng(1)
    a = _img(rng, 17, 23)
    assert R.stats(oracle, a, a) == (17 * 23,) + (0,) * 13
    b = a.copy()
    b[..., 3] = 255 - a[..., 3]                      # the output's alpha is never read
    assert R.stats(oracle, a, b) == (17 * 23,) + (0,) * 13
    assert R.stats(oracle, a, a, cutoff=128)[0] == int((a[..., 3] >= 128).sum())


def test_hand_computed_values(oracle):
    src = np.array([[[10, 20, 30, 255], [0, 0, 0, 255], [255, 255, 255, 0], [7, 7, 7, 9]]], np.uint8)
    out = np.array([[[13, 16, 30, 0], [0, 0, 0, 1], [250, 255, 255, 255], [7, 8, 7, 9]]], np.uint8)
    rec = R.stats(oracle, src, out, what=R.RGB)
    #            pixels changed invalid  sse r, g, b      sad r, g, b   max r, g, b   lab
    assert rec == (4, 3, 0, 9 + 25, 16 + 1, 0, 3 + 5, 4 + 1, 0, 5, 4, 0, 0, 0)
    # the Lab terms from first principles: q = rint(64 Lab), half to even, per pixel dq^2 summed / maxed
    lab_s = oracle.rgb_to_lab(src.reshape(-1, 4)).astype(np.float64) * 64.0
    lab_o = oracle.rgb_to_lab(out.reshape(-1, 4)).astype(np.float64) * 64.0
    terms = [sum((int(np.rint(a)) - int(np.rint(b))) ** 2 for a, b in zip(ps, po)) for ps, po in zip(lab_s, lab_o)]
    assert terms[1] == 0 and min(terms[0], terms[2], terms[3]) > 0
    both = R.stats(oracle, src, out)
    assert both[:12] == rec[:12] and both[12] == sum(terms) and both[13] == max(terms)
    only_lab = R.stats(oracle, src, out, what=R.LAB)
    assert only_lab == (4, 3, 0) + (0,) * 9 + (sum(terms), max(terms))
    # white: L = 100 exactly, so qL = 6400; black: 0
    assert tuple(R.q_of(oracle, np.array([[255, 255, 255, 255]], np.uint8))[0])[0] == 6400
    assert tuple(R.q_of(oracle, np.array([[0, 0, 0, 255]], np.uint8))[0]) == (0, 0, 0)


def test_rounding_of_q_is_half_to_even(oracle):
    """64 x is exact in binary32, so q rounds at .5 exactly where x = (2 m + 1) / 128: such values round to the even neighbour"""
    x = np.array([0.5 / 64, 1.5 / 64, 2.5 / 64, -0.5 / 64, -1.5 / 64, 100.5 / 64], np.float32)
    q = np.rint(x * np.float32(64.0)).astype(np.int64)
    assert q.tolist() == [0, 2, 2, 0, -2, 100]
    # and the model applies exactly that to the oracle's Lab: a colour whose 64 L has the fraction .5 exists among the greys or
    # not, the rule is the same -- check the model against the rule on every grey
    g = np.arange(256, dtype=np.uint8)
    px = np.stack([g, g, g, np.full_like(g, 255)], axis=1)
    lab = oracle.rgb_to_lab(px)
    want = np.array([[int(np.rint(np.float32(v) * np.float32(64.0))) for v in row] for row in lab])
    assert np.array_equal(R.q_of(oracle, px), want)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bands_combine_to_the_whole_image_in_any_order(oracle, seed):
    rng = np.random.default_rng(seed)
    h, w = 37, 29
    src, out = _img(rng, h, w), _img(rng, h, w)
    same = rng.random((h, w)) < 0.4
    out[same] = src[same]
    for cutoff in (0, 100):
        whole = R.stats(oracle, src, out, cutoff=cutoff)
        s, o = src.reshape(-1, 4), out.reshape(-1, 4)
        bounds = [0] + np.sort(rng.choice(np.arange(1, h * w), 6, replace=False)).tolist() + [h * w]
        parts = [R.stats(oracle, s[a:b], o[a:b], cutoff=cutoff) for a, b in zip(bounds[:-1], bounds[1:])]
        for order in (range(len(parts)), reversed(range(len(parts))), rng.permutation(len(parts))):
            rec = R.ZERO
            for i in order:
                rec = R.combine(rec, parts[i])
            assert rec == whole
        # a part that was not requested leaves its fields alone: RGB-only bands into a record that already holds Lab fields
        rec = (0,) * 12 + (123, 45)
        for a, b in zip(bounds[:-1], bounds[1:]):
            rec = R.combine(rec, R.stats(oracle, s[a:b], o[a:b], cutoff=cutoff, what=R.RGB))
        assert rec[12:] == (123, 45) and rec[:12] == whole[:12]


def test_index_form_equals_rgba8_form_on_the_expanded_image(oracle):
    rng = np.random.default_rng(5)
    h, w = 31, 45
    for k, dtype in ((1, np.uint8), (7, np.uint8), (256, np.uint8), (300, np.uint16)):
        pal = rng.integers(0, 256, (k, 4), dtype=np.uint8)
        src = _img(rng, h, w)
        idx = rng.integers(0, k, (h, w)).astype(dtype)
        hit = rng.random((h, w)) < 0.2                                   # some pixels already have a palette colour
        src[hit, :3] = pal[idx[hit].astype(np.int64)][:, :3]
        for cutoff in (0, 77):
            a = R.stats(oracle, src, idx, palette=pal, cutoff=cutoff)
            b = R.stats(oracle, src, R.expand(pal, idx, src), cutoff=cutoff)
            assert a == b and a[2] == 0 and a[1] > 0


def test_cutoff_and_invalid_rules(oracle):
    rng = np.random.default_rng(6)
    h, w, k = 20, 33, 9
    pal = rng.integers(0, 256, (k, 4), dtype=np.uint8)
    src = _img(rng, h, w)
    idx = rng.integers(0, k, (h, w)).astype(np.uint8)
    base = R.stats(oracle, src, idx, palette=pal, cutoff=0)
    assert base[0] == h * w and base[2] == 0
    for t in (1, 128, 255):
        kept = src[..., 3] >= t
        rec = R.stats(oracle, src, idx, palette=pal, cutoff=t)
        assert rec[0] == int(kept.sum())
        # exactly the record of the kept pixels alone
        assert rec == R.stats(oracle, src[kept].reshape(1, -1, 4), idx[kept].reshape(1, -1), palette=pal, cutoff=0)
        # the transparent slot k on uncounted pixels is legal and adds nothing
        slot = idx.copy()
        slot[~kept] = k
        assert R.stats(oracle, src, slot, palette=pal, cutoff=t) == rec
        # on counted pixels an index >= k goes into `invalid` and adds nothing else
        bad = idx.copy()
        planted = kept & (rng.random((h, w)) < 0.1)
        bad[planted] = rng.integers(k, 256, int(planted.sum())).astype(np.uint8)
        got = R.stats(oracle, src, bad, palette=pal, cutoff=t)
        good = kept & ~planted
        assert got[2] == int(planted.sum()) and got[0] == int(good.sum())
        want = R.stats(oracle, src[good].reshape(1, -1, 4), idx[good].reshape(1, -1), palette=pal, cutoff=0)
        assert got[:2] + got[3:] == want[:2] + want[3:]


def test_overflow_bound_over_all_16m_colours(oracle):
    """every per-pixel Lab term is at most the squared diagonal of the box the q of all 2^24 colours lie in; that is
    below 2^29, so lab_sse stays below 2^61 for 2^32 pixels and the kernel's 32-bit term cannot overflow"""
    q = R.q_table(oracle)
    lo, hi = q.min(axis=0).astype(np.int64), q.max(axis=0).astype(np.int64)
    assert tuple(int(v) for v in lo) == Q_MIN and tuple(int(v) for v in hi) == Q_MAX
    bound = int(((hi - lo) ** 2).sum())
    assert bound == LAB_TERM_BOUND
    assert bound < 2 ** 29 and bound * 2 ** 32 < 2 ** 61
    # the table is the model's own conversion
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, (1000, 4), dtype=np.uint8)
    c = px[:, 0].astype(np.int64) | (px[:, 1].astype(np.int64) << 8) | (px[:, 2].astype(np.int64) << 16)
    assert np.array_equal(q[c].astype(np.int64), R.q_of(oracle, px))
    a, b = _img(rng, 40, 50), _img(rng, 40, 50)
    assert R.stats(oracle, a, b, use_table=True) == R.stats(oracle, a, b, use_table=False)


def test_bisection_model():
    for k_min, k_max in ((2, 64), (1, 1), (1, 2), (5, 300), (1, 3072)):
        for first_ok in list(range(k_min, min(k_max, k_min + 40) + 1)) + [k_max, k_max + 1]:
            k, reached, seen = R.bisect(lambda kk: kk >= first_ok, k_min, k_max)     # a monotone predicate: the smallest accepted k
            assert (k, reached) == ((first_ok, True) if first_ok <= k_max else (k_max, False))
            assert len(seen) <= R.max_runs(k_min, k_max) and len(set(seen)) == len(seen)
    # not monotone: the answer is still an accepted k whose predecessor on the path was refused
    ok = {64, 33, 17, 12, 13, 40}
    k, reached, seen = R.bisect(lambda kk: kk in ok, 2, 64)
    assert reached and k in ok and seen == [64, 33, 17, 9, 13, 11, 12] and k == 12


def tokyo_cases(W):
    """the three targets of the issue, from the oracle's own E at fixed k: E(12), E(64) - 1 and E(2), as mean limits"""
    return [("interior", -(-W.E(12) // W.n)), ("not_reached", (W.E(64) - 1) // W.n), ("k_min", -(-W.E(2) // W.n))]


def test_quality_search_on_tokyo_with_the_oracle(oracle, tokyo):
    W = R.Working(oracle, tokyo)
    assert (W.w, W.h, W.n) == (256, 171, 256 * 171)
    got = {}
    for name, target in tokyo_cases(W):
        assert 0 <= target < 2 ** 32
        k, reached, rec, seen = W.search(2, 64, target)
        got[name] = (k, reached)
        assert len(seen) <= R.max_runs(2, 64) == 7
        assert rec[0] == W.n and rec[2] == 0
        assert (rec[12] <= target * W.n) == reached
    assert 2 < got["interior"][0] < 64 and got["interior"][1]
    assert got["not_reached"] == (64, False)
    assert got["k_min"] == (2, True)
