#!/usr/bin/env python3
"""Index output device times (HIP events), for DESIGN.md 4.7: apply-plan runs (the per-pixel kernel alone) on the tiled photograph
of bench.py at 8192^2, k = 64 and 256, RGBA8 against INDEX8, for replace (the colour-table route), dither (the Lab lists) and
diffuse (the pair table), with the strategy the cost models pick at that size.  Run it under `rocprofv3 --kernel-trace --stats`
for the per-kernel split.
    python tools/indexed_time.py [repeats] > profiles/r09_indexed_time.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python")); sys.path.insert(0, ROOT)
import numpy as np
import torch
import kmeans_gpu_amd as kg
import bench

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
st = torch.cuda.current_stream().cuda_stream
n = 8192 * 8192
img = bench.synthetic_image("photo", n, 0, 64, 0x5EED0B10)
out = torch.empty_like(img)
out8 = torch.empty(n, dtype=torch.uint8, device="cuda")
proc = kg.ImageProcessor(shrink_max_dim=0)


def timed(fn, r):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(r):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / r


host = img[: 1 << 20].cpu().numpy()
rows = [f"8192^2 tiled photograph, apply-plan runs, mean of {reps} (diffuse: {max(1, reps // 10)}) after one warm-up run"]
for k in (64, 256):
    pal = host[np.arange(k, dtype=np.int64) * (host.shape[0] // k)].copy()
    pal[:, 3] = 255
    cent = kg.palette_to_centroids(pal)
    for mode, mname in ((0, "replace"), (1, "dither"), (3, "diffuse")):
        r = reps if mode != 3 else max(1, reps // 10)
        t = []
        for fmt, dst in ((None, out), (kg.OutputFormat.Index8, out8)):
            if mode == 3:
                # diffusion continues across the runs of a plan: every timed run is the first band of a fresh plan (+ its table)
                plans = []

                def run():
                    plans.append(proc.apply_plan(cent, mode, n, st, format=fmt))
                    plans[-1].run(img.data_ptr(), 8192, 8192, 0, dst.data_ptr(), st)
                t.append(timed(run, r))
                for p in plans:
                    p.close()
            else:
                plan = proc.apply_plan(cent, mode, n, st, format=fmt)
                t.append(timed(lambda: plan.run(img.data_ptr(), 8192, 8192, 0, dst.data_ptr(), st), r))
                plan.close()
        saving = 100 * (1 - t[1] / t[0])
        rows.append(f"{mname:>7} k={k:<3}: RGBA8 {t[0]:.3f} ms, INDEX8 {t[1]:.3f} ms ({saving:+.1f} % saved)")
print("\n".join(rows))
proc.close()
