"""Alpha-weighted k-means (kmg_processor_set_weighting) without a device: the test-side model (tests/weight_ref.py) against the
contract's literal wording -- the default loop on the pixel list in which pixel i appears a_i times --, the kept rule max(t, 1),
`with_weights`, the refusals of the command line's parser, and the declarations of the surface."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import alpha_ref
import weight_ref


@pytest.fixture(scope="module")
def sprite_problem(oracle):
    """the weighted sprite's working image: (pixels, Lab, weights)"""
    px, w, h = weight_ref.working_pixels(oracle, weight_ref.weighted_sprite(), 0)
    assert h == 1 and w == px.shape[0]
    return px, oracle.rgb_to_lab(px), px[:, 3]


@pytest.mark.parametrize("k", [4, 8, 16])
def test_model_is_the_default_loop_on_the_replicated_list(oracle, sprite_problem, k):
    px, lab, a = sprite_problem
    assert a.min() >= 1 and len(np.unique(a)) > 100
    cent0 = oracle.init_centroids(lab, px.shape[0], 1, k)              # unweighted: over the kept pixels, each once
    got, labels, it = weight_ref.lloyd(oracle, lab, a, cent0)
    want, want_it = weight_ref.lloyd_replicated(oracle, lab, a, cent0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and it == want_it
    assert np.array_equal(labels, oracle.assign(lab, got))             # labels do not depend on the weights
    # the weights matter: the unweighted loop ends elsewhere
    plain, _, _ = oracle.lloyd(lab, cent0)
    assert not np.array_equal(got.view(np.uint32), plain.view(np.uint32))


def test_weighted_sums_are_the_sums_of_the_replicated_list(oracle, sprite_problem):
    px, lab, a = sprite_problem
    k = 8
    cent = oracle.init_centroids(lab, px.shape[0], 1, k)
    labels = oracle.assign(lab, cent)
    got = weight_ref.accumulate(weight_ref.pixel_q(oracle, lab), a, labels, k)
    rep = a.astype(np.int64)
    assert np.array_equal(got, oracle.accumulate(np.repeat(lab, rep, axis=0), np.repeat(labels, rep), k))
    assert np.array_equal(got[:, 3], np.bincount(labels, weights=a, minlength=k).astype(np.int64))
    # unit weights: the default sums
    assert np.array_equal(weight_ref.accumulate(weight_ref.pixel_q(oracle, lab), np.ones_like(a), labels, k), oracle.accumulate(lab, labels, k))


def test_a_cluster_of_weightless_members_is_an_empty_cluster(oracle):
    lab = oracle.rgb_to_lab(np.array([[250, 10, 10, 0], [10, 250, 10, 9], [12, 249, 10, 200]], np.uint8))
    cent0 = oracle.centroids4(lab[:2])
    got, labels, _ = weight_ref.lloyd(oracle, lab, np.array([0, 9, 200]), cent0, max_iterations=3)
    assert list(labels) == [0, 1, 1]
    assert np.array_equal(got[0].view(np.uint32), cent0[0].view(np.uint32))          # its members all weigh 0: it stays
    assert not np.array_equal(got[1].view(np.uint32), cent0[1].view(np.uint32))


@pytest.mark.parametrize("t", [0, 1, 2, 128, 255])
def test_kept_rule_is_alpha_modes_compaction_at_max_t_1(oracle, t):
    img = weight_ref.weighted_sprite()
    img[0, :6, 3] = [0, 1, 2, 127, 128, 255]
    px, w, h = weight_ref.working_pixels(oracle, img, t)
    assert np.array_equal(px, alpha_ref.compact(img, max(t, 1))) and (w, h) == (px.shape[0], 1)
    assert px[:, 3].min() >= max(t, 1)
    # every pixel kept: the image itself; none kept: no working image
    full = img.copy()
    full[..., 3] = np.maximum(full[..., 3], max(t, 1))
    px, w, h = weight_ref.working_pixels(oracle, full, t)
    assert (w, h) == (full.shape[1], full.shape[0]) and np.array_equal(px, full.reshape(-1, 4))
    none = img.copy()
    none[..., 3] = max(t, 1) - 1
    assert weight_ref.working_pixels(oracle, none, t) is None


def test_sequence_model_of_one_whole_frame_is_the_image_model(oracle):
    img = weight_ref.weighted_sprite()
    img[..., 3] = np.maximum(img[..., 3], 1)
    a = weight_ref.sequence_centroids(oracle, [img], [1], 5)
    b = weight_ref.kmeans_centroids(oracle, img, 5, 0)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_with_weights():
    import kmeans_gpu_amd as kg
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    w = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    keep = img.copy()
    out = kg.with_weights(img, w)
    assert out is not img and np.array_equal(img, keep)
    assert out.dtype == np.uint8 and out.flags.c_contiguous
    assert np.array_equal(out[..., :3], img[..., :3]) and np.array_equal(out[..., 3], w)
    with pytest.raises(ValueError):
        kg.with_weights(img, w[:, :6])
    with pytest.raises(ValueError):
        kg.with_weights(img, w.astype(np.float32))
    with pytest.raises(ValueError):
        kg.with_weights(img[..., :3], w)


def _files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(9)
    src, good, bad = (str(tmp_path / n) for n in ("src.png", "map.png", "small.png"))
    Image.fromarray(rng.integers(0, 256, (9, 13, 4), dtype=np.uint8), "RGBA").save(src)
    Image.fromarray(rng.integers(0, 256, (9, 13), dtype=np.uint8), "L").save(good)
    Image.fromarray(rng.integers(0, 256, (9, 12), dtype=np.uint8), "L").save(bad)
    return src, good, bad


@pytest.mark.parametrize("command", ["palette", "reduce", "sequence"])
def test_cli_refusals(tmp_path, capsys, command):
    """every refusal ends in the parser, before a processor is made"""
    from kmeans_gpu_amd import cli
    src, good, bad = _files(tmp_path)
    base = [command, "-i", src, "-c", "4"]
    for extra, text in ((["--weights", good, "--alpha-cutoff", "7"], "--alpha-cutoff"),
                        (["--weights", bad], "13x9"),
                        (["--weights", str(tmp_path / "map.gif")], "png or jpg")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err
    if command != "sequence":
        for extra in (["--alpha-weight", "-a", "octree"], ["--weights", good, "-a", "octree"]):
            with pytest.raises(SystemExit) as e:
                cli.main(base + extra)
            assert e.value.code == 2 and "octree" in capsys.readouterr().err
        with pytest.raises(SystemExit) as e:
            cli.main(["--devices", "0,1"] + base + ["--alpha-weight"])
        assert e.value.code == 2 and "--devices" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["find", "-i", src, "-p", "#000000,#ffffff", "--alpha-weight"])     # `find` has no palette step


def test_setters_validate_without_a_device():
    import kmeans_gpu_amd as kg
    L = kg.lib()
    assert L.kmg_processor_set_weighting(None, 1) == -1 and L.kmg_lloyd_set_weighting(None, 1) == -1
    assert kg.WEIGHT_NONE == 0 and kg.WEIGHT_ALPHA == 1
    assert {"kmg_processor_set_weighting", "kmg_lloyd_set_weighting"} <= set(kg.SYMBOLS)


def test_surface_is_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    assert re.search(r"#define KMG_WEIGHT_NONE\s+0\b", header) and re.search(r"#define KMG_WEIGHT_ALPHA\s+1\b", header)
    assert "KMG_API int kmg_processor_set_weighting(kmg_processor *p, int weighting);" in header
    assert "KMG_API int kmg_lloyd_set_weighting(kmg_lloyd *s, int weighting);" in header
    # the options struct did not grow: the sticky setter is the interface
    fields = re.search(r"typedef struct kmg_options \{(.*?)\} kmg_options;", header, flags=re.S).group(1)
    assert "weight" not in fields
    # the clauses a caller must be able to read: no identity with the unweighted result, the bound, the unweighted error measure
    block = header[header.index("/* kmg_processor_set_weighting"):header.index("#define KMG_WEIGHT_NONE")]
    for phrase in ("NO identity", "2^53", "2^28", "KMG_ERR_UNSUPPORTED", "UNWEIGHTED", "max(t, 1)"):
        assert phrase in block, phrase
    assert "kmg_processor_set_weighting" in open(os.path.join(ROOT, "kmeans-gpu_amd", "host", "kmeans_color_gpu.hpp")).read()
    assert "pub fn kmg_processor_set_weighting" in open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    assert "pub fn set_alpha_weight" in open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()


def test_the_problem_of_the_pixel_bound_is_feasible(oracle):
    """the host side of tests/test_gpu_weight.py::test_sums_at_the_pixel_bound needs no device: 2^28 pixels in closed form, runs of
    1 .. 5, and expected sums that reach 2^62 and -2^60 and stay below 2^63"""
    import test_gpu_weight as G
    P = G._bound_problem(oracle)
    G._bound_feasible(P)
    assert sum(P["counts"]) == G.N_BOUND == 1 << 28
    tile = P["tile"]
    runs = np.diff(np.flatnonzero(np.r_[True, tile[1:] != tile[:-1], True]))
    assert runs.min() == 1 and runs.max() == 5 and G.TILE % 4 != 0          # runs straddle the 4-pixel groups
    # the counts of the closed form against a count of the whole pattern, one repetition at a time
    reps, tail = divmod(G.N_BOUND, G.TILE)
    assert list(P["counts"]) == [int(reps * (tile == c).sum() + (tile[:tail] == c).sum()) for c in range(64)]
