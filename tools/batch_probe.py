#!/usr/bin/env python3
"""Batched palettes against the per-image calls, wall time, for DESIGN.md 4.16 and the crossover constants of kmg_api.hip
(kBatchMinImages).  A batch is N copies of tests/golden/tokyo.png plus N synthetic images of mixed sizes
(2 N images); N in {1, 2, 4, 8, 16, 64, 256}, k in {8, 64, 256}; warm, the minimum of five runs, batch and per-image calls taking turns:
  palette : kmg_palette_batch against the 2 N sequential kmg_palette calls on the same processor
  reduce  : kmg_reduce_batch (replace) against the 2 N sequential kmg_reduce calls, both into result arrays allocated once
  kernels : kmg_dev_palette_batch -- always the batched kernels -- against the per-image kmg_lloyd_init_centroids + kmg_lloyd_run +
            kmg_lloyd_get_centroids on the working images, resident on the device: where the batched chain itself starts to pay;
            `init` = the same batched call with max_iterations = 1, i.e. the k launches of the single-pick initialisation + 2
    python tools/batch_probe.py [largest N] > profiles/r09_batch_time.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import kmeans_gpu_amd as kg
from PIL import Image

largest = int(sys.argv[1]) if len(sys.argv) > 1 else 256
NS = [n for n in (1, 2, 4, 8, 16, 64, 256) if n <= largest]
KS = (8, 64, 256)
RUNS = 5
SIZES = [(64, 64), (256, 171), (96, 200), (512, 384), (300, 200), (33, 257), (128, 128), (640, 360)]

tokyo = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "tokyo.png")).convert("RGBA"))
rng = np.random.default_rng(9)


def synthetic(i):
    """smooth colour fields with noise on top, sizes in rotation: thumbnails, sprites and tiles rather than white noise"""
    w, h = SIZES[i % len(SIZES)]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    f = rng.uniform(0.01, 0.08, 6)
    rgb = np.stack([127 + 120 * np.sin(f[0] * xx + f[1] * yy), 127 + 120 * np.sin(f[2] * xx - f[3] * yy), 127 + 120 * np.cos(f[4] * xx + f[5] * yy)], -1)
    out = np.full((h, w, 4), 255, np.uint8)
    out[..., :3] = np.clip(rgb + rng.normal(0, 6, rgb.shape), 0, 255).astype(np.uint8)
    return out


def best(*fns):
    """minimum wall ms of RUNS runs of each function after one warm run; the functions take turns, so that whatever else the
    machine or the process does at the time meets all of them"""
    for fn in fns:
        fn()                                                         # warm
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(RUNS):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            t[i].append(time.perf_counter() - t0)
    print("   samples ms: " + " | ".join(" ".join(f"{v * 1e3:.2f}" for v in ti) for ti in t), file=sys.stderr)
    return [min(ti) * 1e3 for ti in t]


proc = kg.ImageProcessor()
proc_init = kg.ImageProcessor(max_iterations=1)
st = torch.cuda.current_stream().cuda_stream
rows = [f"tokyo.png {tokyo.shape[1]}x{tokyo.shape[0]} x N + N synthetic images of {len(SIZES)} sizes (2 N images per batch); wall ms, warm, minimum of {RUNS}",
        "batch = one call for all images; sequential = the per-image call image after image on the same processor (the baseline)",
        f"{'':8} {'k':>4} {'N':>4} {'batch':>10} {'sequential':>11} {'batch/seq':>10} {'launches':>9} {'iterations':>10} {'init':>8}"]
worst = {}
for k in KS:
    for n in NS:
        images = [tokyo] * n + [synthetic(i) for i in range(n)]
        t_b, t_s = best(lambda: proc.palette_batch(k, images), lambda: [proc.palette(k, im) for im in images])
        proc.palette_batch(k, images)
        rep = proc.last_batch_report
        rows.append(f"{'palette':8} {k:4d} {n:4d} {t_b:10.3f} {t_s:11.3f} {t_b / t_s:10.3f} {rep.launches:9d} {rep.iterations:10d}")
        worst[("palette", k, n)] = t_b / t_s
        # (results into the same arrays every time, for both: a D2H copy into the untouched pages of a fresh array costs either
        # path 10-30 ms at these sizes, in steps of 10 ms -- nothing of the library's)
        outs = [np.empty_like(im) for im in images]
        t_b, t_s = best(lambda: proc.reduce_batch(k, images, out=outs), lambda: [proc.reduce(k, im, out=o) for im, o in zip(images, outs)])
        rows.append(f"{'reduce':8} {k:4d} {n:4d} {t_b:10.3f} {t_s:11.3f} {t_b / t_s:10.3f} {rep.launches:9d} {rep.iterations:10d}")
        worst[("reduce", k, n)] = t_b / t_s
        # the kernels alone: working images resident on the device
        work = []
        for im in images:
            h, w = im.shape[:2]
            if w > 256 or h > 256:
                sw, sh = kg.resized_dims(w, h)
                d = torch.from_numpy(im).cuda()
                small = torch.empty((sh, sw, 4), dtype=torch.uint8, device="cuda")
                proc.resize(d.data_ptr(), w, h, sw, sh, small.data_ptr(), st)
                work.append((small, sw, sh))
            else:
                work.append((torch.from_numpy(im).cuda(), w, h))
        torch.cuda.synchronize()
        ptrs, ws, hs = [d.data_ptr() for d, _, _ in work], [w for _, w, _ in work], [h for _, _, h in work]

        def per_image():
            for d, w, h in work:
                s = kg.Lloyd(proc, k)
                s.init_centroids(d.data_ptr(), w, h, st)
                s.run(d.data_ptr(), w * h, 0, st)
                s.get_centroids(st)
                s.close()

        t_b, t_s, t_i = best(lambda: proc.palette_batch_device(ptrs, ws, hs, k, st), per_image,
                             lambda: proc_init.palette_batch_device(ptrs, ws, hs, k, st))
        rep = proc.last_batch_report
        rows.append(f"{'kernels':8} {k:4d} {n:4d} {t_b:10.3f} {t_s:11.3f} {t_b / t_s:10.3f} {rep.launches:9d} {rep.iterations:10d} {t_i:8.3f}")
        print(rows[-3] + "\n" + rows[-2] + "\n" + rows[-1], file=sys.stderr, flush=True)
bad = {key: v for key, v in worst.items() if v > 1.10}
rows.append(f"largest batch / sequential over the palette and reduce rows: {max(worst.values()):.3f}" +
            ("" if not bad else "; above 1.10: " + ", ".join(f"{a} k={b} N={c}: {v:.3f}" for (a, b, c), v in sorted(bad.items()))))
print("\n".join(rows))
proc.close()
proc_init.close()
