#!/usr/bin/env python3
"""Randomised check of alpha mode (kmg_options.alpha_cutoff) and error diffusion (KMG_MODE_DIFFUSE) against the test-side
references: kmg_reduce, kmg_palette and kmg_find (a random palette) of random images (noise / few colours / blobs / gradient /
sprite / soft disc, 1 x 1 ... ~900 x 700, single rows and columns), alpha layouts (random bytes, a binary mask, all kept, exactly one
kept, none kept, the sprite's or disc's own), cutoffs t = 0 and 1..255, k, modes 0..3, k-means and octree, every strategy and
shrink_max_dim 256 or 0 (full resolution, for small enough images).  t > 0 is checked against tests/alpha_ref.py, t = 0 against
the CPU oracle (tests/diffuse_ref.py for mode 3); with no pixel kept, palette and reduce must fail with status -1 and leave `out`
untouched.   usage: fuzz_alpha.py [cases] [seed]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import kmeans_gpu_amd as kg
import oracle_lib as oracle
import alpha_ref
import diffuse_ref

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
procs = {256: kg.ImageProcessor(shrink_max_dim=256), 0: kg.ImageProcessor(shrink_max_dim=0)}
KS = [1, 2, 3, 5, 8, 13, 16, 31, 32, 33, 64, 100, 256, 300, 512, 600]


def image(kind, w, h):
    n = w * h
    if kind == "noise":
        a = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    elif kind == "few":
        pal = rng.integers(0, 256, (int(rng.integers(1, 9)), 4), dtype=np.uint8)
        a = pal[rng.integers(0, pal.shape[0], n)]
    elif kind == "blobs":
        c = rng.integers(0, 256, (int(rng.integers(2, 30)), 3))
        a = np.zeros((n, 4), np.uint8)
        a[:, :3] = np.clip(c[rng.integers(0, c.shape[0], n)] + rng.normal(0, rng.uniform(2, 30), (n, 3)), 0, 255).astype(np.uint8)
    elif kind == "sprite" and w > 16 and h > 16:
        return alpha_ref.sprite(h, w, seed=int(rng.integers(0, 1 << 30)))
    else:  # gradient (and the sprite or the disc's colours)
        i = np.arange(n)
        a = np.stack([(i % w) * 255 // max(w - 1, 1), (i // w) * 255 // max(h - 1, 1), (i * 7) % 256, i % 256], 1).astype(np.uint8)
    img = a.reshape(h, w, 4)
    return alpha_ref.soft_disc(img) if kind == "disc" else img


def set_alpha(img, layout, t):
    """kept = alpha >= t; layouts other than "own" replace the image's alpha"""
    h, w = img.shape[:2]
    n = w * h
    lo, hi = max(t, 1), 256                                 # kept bytes [lo, 255], excluded bytes [0, t)
    a = img[..., 3].reshape(-1)
    if layout == "random":
        a[:] = rng.integers(0, 256, n)
        pick = rng.random(n) < 0.3
        a[pick] = np.array([0, max(t - 1, 0), t if t else 255, 255], np.uint8)[rng.integers(0, 4, int(pick.sum()))]
    elif layout == "binary":
        a[:] = np.where(rng.random(n) < rng.uniform(0.05, 0.95), 255, 0)
    elif layout == "all":
        a[:] = rng.integers(lo, hi, n)
    elif layout in ("one", "none"):
        a[:] = rng.integers(0, max(t, 1), n) if t else 255
        if layout == "one" and t:
            a[int(rng.integers(0, n))] = rng.integers(lo, hi)
    img[..., 3] = a.reshape(h, w)
    return img


def pal_of(cent):
    pal = np.full((cent.shape[0], 4), 255, np.uint8)
    for j in range(cent.shape[0]):
        pal[j, :3] = oracle.palette_lab_to_srgb8(cent[j, :3])
    return alpha_ref.sorted_by_L(oracle, pal)


def references(img, k, mode, algo, t, shrink, pal):
    """(palette, reduce, find) the product must return; None: refused (no pixel kept)"""
    if t:
        fnd = alpha_ref.find(oracle, img, pal, mode, t)
        if algo == kg.Algorithm.Octree:
            p = alpha_ref.palette_octree(oracle, img, k, t)
            return p, (None if p is None else alpha_ref.find(oracle, img, p, mode, t)), fnd
        cent = alpha_ref.kmeans_centroids(oracle, img, k, t, shrink)
        if cent is None:
            return None, None, fnd
        return pal_of(cent), alpha_ref.apply(oracle, img, cent, mode, t), fnd
    if mode == alpha_ref.MODE_DIFFUSE:
        fnd = diffuse_ref.diffuse(img, diffuse_ref.oracle_find_replace(oracle, pal))
    else:
        fnd = oracle.find(img, pal, mode)
    if algo == kg.Algorithm.Octree:
        p = oracle.palette_octree(img, k)
        if mode == alpha_ref.MODE_DIFFUSE:
            return p, diffuse_ref.diffuse(img, diffuse_ref.oracle_find_replace(oracle, p)), fnd
        return p, oracle.reduce_octree(img, k, mode), fnd
    if shrink == 256 and mode != alpha_ref.MODE_DIFFUSE:
        return oracle.palette(img, k), oracle.reduce(img, k, mode), fnd
    cent, _ = oracle.extract_palette_kmeans(img, k, shrink)
    p = oracle.palette(img, k) if shrink == 256 else pal_of(cent)
    if mode == alpha_ref.MODE_DIFFUSE:
        return p, diffuse_ref.diffuse(img, diffuse_ref.oracle_apply_replace(oracle, cent)), fnd
    return p, oracle.apply(img, cent, mode), fnd


def refused(call):
    try:
        call()
    except kg.KmgError as e:
        return e.status == -1
    return False


bad = 0
for case in range(cases):
    kind = ["noise", "few", "blobs", "gradient", "sprite", "disc"][int(rng.integers(0, 6))]
    shape = rng.random()
    w = 1 if shape < 0.08 else int(rng.integers(1, 900))
    h = 1 if 0.08 <= shape < 0.16 else int(rng.integers(1, 700))
    layouts = ["random", "binary", "all", "one", "none"] + (["own"] * 2 if kind in ("sprite", "disc") else [])
    layout = layouts[int(rng.integers(0, len(layouts)))]
    t = 0 if rng.random() < 0.2 else int(rng.integers(1, 256))
    k = int(rng.choice(KS))
    mode = int(rng.integers(0, 4))
    algo = kg.Algorithm.Octree if rng.random() < 0.25 else kg.Algorithm.Kmeans
    strategy = ["auto", "scan", "table", "table+mask_words"][int(rng.integers(0, 4))]
    # full resolution for images up to 300 K pixels (and n k <= 2e7, which keeps the oracle's Lloyd loop quick)
    shrink = 0 if w * h <= 300_000 and w * h * k <= 20_000_000 and rng.random() < 0.4 else 256
    img = image(kind, w, h)
    if layout != "own":
        img = set_alpha(img, layout, t)
    img = np.ascontiguousarray(img)
    pal = rng.integers(0, 256, (int(rng.integers(1, k + 1)), 4), dtype=np.uint8)
    pal[:, 3] = 255
    kg.set_strategy(strategy)
    p = procs[shrink]
    p.set_alpha_cutoff(t)
    want_p, want_r, want_f = references(img, k, mode, algo, t, shrink, pal)
    ok = np.array_equal(p.find(img, pal, mode), want_f)
    if want_p is None:
        out = np.full_like(img, 7)
        ok = ok and refused(lambda: p.palette(k, img, algo))
        ok = ok and refused(lambda: p.reduce(k, img, algo, mode, out=out)) and (out == 7).all()
    else:
        ok = ok and np.array_equal(p.palette(k, img, algo), want_p)
        ok = ok and np.array_equal(p.reduce(k, img, algo, mode), want_r)
    if not ok:
        bad += 1
        print(f"MISMATCH case {case}: {kind} {w}x{h} alpha={layout} t={t} k={k} mode={mode} algo={algo.name} strategy={strategy} "
              f"shrink={shrink} find_palette={pal.shape[0]}", flush=True)
kg.set_strategy("auto")
print(f"{cases} cases, {bad} mismatching")
sys.exit(1 if bad else 0)
