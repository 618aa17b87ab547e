#!/usr/bin/env python3
"""Batched palettes against the per-image calls, wall time, for DESIGN.md 4.16 and the crossover constants of kmg_api.hip
(kBatchMinImages).  A batch is N copies of tests/golden/tokyo.png plus N synthetic images of mixed sizes
(2 N images); N in {1, 2, 4, 8, 16, 64, 256}, k in {8, 64, 256}; warm, the minimum of five runs, batch and per-image calls taking turns:
  palette : kmg_palette_batch against the 2 N sequential kmg_palette calls on the same processor
  reduce  : kmg_reduce_batch (replace) against the 2 N sequential kmg_reduce calls, both into result arrays allocated once
  kernels : kmg_dev_palette_batch -- always the batched kernels -- against the per-image kmg_lloyd_init_centroids + kmg_lloyd_run +
            kmg_lloyd_get_centroids on the working images, resident on the device: where the batched chain itself starts to pay;
            `init` = the same batched call with max_iterations = 1, i.e. the k launches of the single-pick initialisation + 2
    python tools/batch_probe.py [largest N] > profiles/r09_batch_time.txt

`apply`: the batched output pass (kmg_batch_apply.hip) on the same batches, 2 N in {2, 8, 32, 128, 512}, replace and
dither, the same protocol (warm processor, result arrays allocated once, batch and baseline taking turns, minimum of five):
  bound   : kmg_reduce_indexed_batch(RGBA8) against kmg_reduce_batch -- the same bytes; no point above 1.10
  index8  : kmg_reduce_indexed_batch(INDEX8) against kmg_reduce_batch
  find    : kmg_find_batch(INDEX8) against kmg_find_indexed image after image
  device  : kmg_dev_apply_batch against kmg_dev_apply_format image after image, images and outputs resident on the device
  pruned  : (dither, k = 256, the images a plan of their own sends to the candidate lists) kmg_dev_apply_batch with the strategy
            "scan" -- they join the launch -- against "table" -- they take their own pass inside the call
  ppt     : (tools build only: KMG_LIBRARY=lib/libkmeans_hip_tools.so) kmg_dev_apply_batch with 4 against 8 pixels per thread
    python tools/batch_probe.py apply [largest N] > profiles/r10_batch_apply_time.txt

`quality`: kmg_reduce_quality_batch against kmg_reduce_quality image after image on the same processor, the same
protocol; the first 2, 8 and 128 images of the 128-image set (N = 64), dither, INDEX8 / INDEX16 as reduce_quality chooses;
(k_min, k_max, max dE) = (2, 16, 22.0), (2, 64, 13.0), (2, 256, 8.0) -- targets inside the range of E(k) of these images, so that
the counts chosen spread over the range; the row gives their spread and how many images reached the target
    python tools/batch_probe.py quality [most images] [runs] > profiles/r11_batch_quality_time.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import kmeans_gpu_amd as kg
from PIL import Image

APPLY = len(sys.argv) > 1 and sys.argv[1] == "apply"
QUALITY = len(sys.argv) > 1 and sys.argv[1] == "quality"
args = sys.argv[2:] if APPLY or QUALITY else sys.argv[1:]
largest = int(args[0]) if args else 256
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


def apply_probe():
    import ctypes as C
    L = kg.lib()
    tools = "tools" in os.path.basename(os.environ.get("KMG_LIBRARY", ""))
    proc = kg.ImageProcessor()
    st = torch.cuda.current_stream().cuda_stream
    rows = [f"tokyo.png {tokyo.shape[1]}x{tokyo.shape[0]} x N + N synthetic images of {len(SIZES)} sizes (2 N images per batch); wall ms, warm, minimum of {RUNS}",
            "batch = the new call; base = what it is measured against (tools/batch_probe.py apply)",
            f"{'':8} {'mode':>8} {'k':>4} {'2N':>4} {'batch':>10} {'base':>10} {'batch/base':>10} {'launches':>9} {'batched':>8} {'per_image':>9}"]
    worst = {}

    def row(name, mode, k, n2, t_b, t_s, rep):
        rows.append(f"{name:8} {mode.name.lower():>8} {k:4d} {n2:4d} {t_b:10.3f} {t_s:10.3f} {t_b / t_s:10.3f} {rep.launches:9d} {rep.batched:8d} {rep.per_image:9d}")
        print(rows[-1], file=sys.stderr, flush=True)

    for k in KS:
        pal = rng.integers(0, 256, (k, 4), dtype=np.uint8)
        pal[:, 3] = 255
        c4 = kg.palette_to_centroids(pal)
        for n in [n for n in (1, 4, 16, 64, 256) if n <= largest]:
            images = [tokyo] * n + [synthetic(i) for i in range(n)]
            ws, hs = [im.shape[1] for im in images], [im.shape[0] for im in images]
            rgba = [np.empty_like(im) for im in images]
            rgba2 = [np.empty_like(im) for im in images]
            maps = [np.empty(im.shape[:2], np.uint8) for im in images]
            maps2 = [np.empty(im.shape[:2], np.uint8) for im in images]
            d_imgs = [torch.from_numpy(im).cuda() for im in images]
            d_outs = [torch.empty(im.shape[:2], dtype=torch.uint8, device="cuda") for im in images]
            src, dst = [d.data_ptr() for d in d_imgs], [d.data_ptr() for d in d_outs]

            def find_each():
                for im, o in zip(images, maps2):
                    L.kmg_find_indexed(proc.handle, C.c_void_p(im.ctypes.data), im.shape[1], im.shape[0], C.c_void_p(pal.ctypes.data), k, int(mode),
                                       int(kg.OutputFormat.Index8), C.c_void_p(o.ctypes.data))

            def apply_each():
                for s, w, h, d in zip(src, ws, hs, dst):
                    proc.apply(s, w, h, 0, c4, mode, d, st, format=kg.OutputFormat.Index8)

            for mode in (kg.ReduceMode.Replace, kg.ReduceMode.Dither):
                if tools:
                    def with_ppt(ppt):
                        os.environ["KMG_BATCH_APPLY_PPT"] = str(ppt)
                        proc.apply_batch_device(src, ws, hs, c4, mode, kg.OutputFormat.Index8, dst, st)
                    t_b, t_s = best(lambda: with_ppt(4), lambda: with_ppt(8))
                    row("ppt 4/8", mode, k, 2 * n, t_b, t_s, proc.last_batch_apply_report)
                    worst[(mode.name, k, 2 * n)] = 0.0
                    continue
                t_b, t_s = best(lambda: proc.reduce_indexed_batch(k, images, reduce_mode=mode, format=kg.OutputFormat.RGBA8, out=rgba),
                                lambda: proc.reduce_batch(k, images, reduce_mode=mode, out=rgba2))
                assert all(np.array_equal(a, b) for a, b in zip(rgba, rgba2))
                row("bound", mode, k, 2 * n, t_b, t_s, proc.last_batch_apply_report)
                worst[(mode.name, k, 2 * n)] = t_b / t_s
                t_b, t_s = best(lambda: proc.reduce_indexed_batch(k, images, reduce_mode=mode, format=kg.OutputFormat.Index8, out=maps),
                                lambda: proc.reduce_batch(k, images, reduce_mode=mode, out=rgba2))
                row("index8", mode, k, 2 * n, t_b, t_s, proc.last_batch_apply_report)
                t_b, t_s = best(lambda: proc.find_batch(images, pal, reduce_mode=mode, format=kg.OutputFormat.Index8, out=maps), find_each)
                assert all(np.array_equal(a, b) for a, b in zip(maps, maps2))
                row("find", mode, k, 2 * n, t_b, t_s, proc.last_batch_apply_report)
                t_b, t_s = best(lambda: proc.apply_batch_device(src, ws, hs, c4, mode, kg.OutputFormat.Index8, dst, st), apply_each)
                row("device", mode, k, 2 * n, t_b, t_s, proc.last_batch_apply_report)
                if k == 256 and mode == kg.ReduceMode.Dither:
                    # the images of this batch whose own plan prunes (k >= 128: from 16384 pixels on)
                    big = [i for i in range(len(images)) if ws[i] * hs[i] >= 16384]
                    pick = lambda v: [v[i] for i in big]

                    def under(strategy):
                        proc.set_strategy(strategy)
                        proc.apply_batch_device(pick(src), pick(ws), pick(hs), c4, mode, kg.OutputFormat.Index8, pick(dst), st)
                        proc.set_strategy("auto")
                    t_b, t_s = best(lambda: under("scan"), lambda: under("table"))
                    under("scan")
                    row("pruned", mode, k, len(big), t_b, t_s, proc.last_batch_apply_report)
    bad = {key: v for key, v in worst.items() if v > 1.10}
    rows.append(f"largest batch / base over the bound rows: {max(worst.values()):.3f}" +
                ("" if not bad else "; above 1.10: " + ", ".join(f"{a} k={b} 2N={c}: {v:.3f}" for (a, b, c), v in sorted(bad.items()))))
    print("\n".join(rows))
    proc.close()


def quality_probe():
    global RUNS
    most = int(args[0]) if args else 128
    RUNS = int(args[1]) if len(args) > 1 else RUNS
    proc = kg.ImageProcessor()
    full = []
    for i in range(64):                                              # the 128-image set, tokyo and synthetic images in turn
        full += [tokyo, synthetic(i)]
    rows = [f"tokyo.png {tokyo.shape[1]}x{tokyo.shape[0]} and synthetic images of {len(SIZES)} sizes in turn; wall ms, warm, minimum of {RUNS}",
            "batch = kmg_reduce_quality_batch; sequential = kmg_reduce_quality image after image on the same processor (tools/batch_probe.py quality)",
            f"{'':8} {'k_min':>5} {'k_max':>5} {'dE':>4} {'images':>6} {'batch':>10} {'sequential':>11} {'batch/seq':>10} {'rounds':>6} {'runs':>5} {'launches':>9} "
            f"{'k* min/median/max':>18} {'reached':>7}"]
    for k_min, k_max, de in ((2, 16, 22.0), (2, 64, 13.0), (2, 256, 8.0)):
        for n in [n for n in (2, 8, 128) if n <= most]:
            images = full[:n]
            got, want = [], []

            def batch():
                got[:] = proc.reduce_quality_batch(images, de, k_min, k_max, kg.ReduceMode.Dither, indexed=True)

            def sequential():
                want[:] = [proc.reduce_quality(im, de, k_min, k_max, kg.ReduceMode.Dither, indexed=True) for im in images]

            t_b, t_s = best(batch, sequential)
            assert all(g[0] == w[0] and np.array_equal(g[1], w[1]) and np.array_equal(g[2], w[2]) and g[4] == w[4] for g, w in zip(got, want))
            rep = proc.last_quality_report
            stars = sorted(g[0] for g in got)
            rows.append(f"{'quality':8} {k_min:5d} {k_max:5d} {de:4.1f} {n:6d} {t_b:10.3f} {t_s:11.3f} {t_b / t_s:10.3f} {rep.rounds:6d} {rep.palette_runs:5d} "
                        f"{rep.launches:9d} {f'{stars[0]}/{stars[len(stars) // 2]}/{stars[-1]}':>18} {sum(1 for g in got if g[4]):7d}")
            print(rows[-1], file=sys.stderr, flush=True)
    print("\n".join(rows))
    proc.close()


if APPLY:
    apply_probe()
    sys.exit(0)
if QUALITY:
    quality_probe()
    sys.exit(0)

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
