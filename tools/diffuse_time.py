#!/usr/bin/env python3
"""KMG_MODE_DIFFUSE device time (HIP events) of kmg_apply_plan_run -- the diffusion pass alone -- with the plan's table build timed
separately (kmg_apply_plan_create up to its tables' completion), on the tiled photograph of bench.py:
  8192^2 at k = 3, 46 (apollo), 64, 256 and 300 (the k > 256 table); 8192 x 1024 and 1024 x 8192 at k = 64 (the pass follows
  W + 2 H, not W H).
    python tools/diffuse_time.py [repeats]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python")); sys.path.insert(0, ROOT)
import numpy as np, torch
import kmeans_gpu_amd as kg
import bench
from PIL import Image

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
proc = kg.ImageProcessor(shrink_max_dim=0)
st = torch.cuda.current_stream().cuda_stream
px = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "apollo-1x.png")).convert("RGBA")).reshape(-1, 4)
apollo = np.array(sorted(set(map(tuple, px))), np.uint8)
n = 8192 * 8192
photo = bench.synthetic_image("photo", n, 0, 64, 0x5EED0B10)
host = photo[: 1 << 20].cpu().numpy()


def pal_of(k):
    if k == 3:
        return np.array([[5, 5, 5, 255], [255, 255, 255, 255], [255, 0, 0, 255]], np.uint8)
    if k == 46:
        return apollo
    p = host[np.arange(k, dtype=np.int64) * (host.shape[0] // k)].copy(); p[:, 3] = 255
    return p


def ev():
    return torch.cuda.Event(enable_timing=True)


out = torch.empty((n, 4), dtype=torch.uint8, device="cuda")
print(f"{'shape':>12s} {'k':>5s} {'steps W+2H':>10s} {'table ms':>9s} {'pass ms':>9s} {'us/step':>8s}", flush=True)
for (w, h, k) in [(8192, 8192, 3), (8192, 8192, 46), (8192, 8192, 64), (8192, 8192, 256), (8192, 8192, 300), (8192, 1024, 64),
                  (1024, 8192, 64)]:
    cent = kg.palette_to_centroids(pal_of(k))
    img = photo[: w * h]                              # (the tiled rows re-read at width w: still a photograph)
    tb, tp = [], []
    for r in range(reps + 1):
        e0, e1, e2 = ev(), ev(), ev()
        torch.cuda.synchronize()
        e0.record()
        plan = proc.apply_plan(cent, kg.ReduceMode.Diffuse, w * h, st)
        e1.record()
        plan.run(img.data_ptr(), w, h, 0, out.data_ptr(), st)
        e2.record()
        torch.cuda.synchronize()
        plan.close()
        if r:
            tb.append(e0.elapsed_time(e1)); tp.append(e1.elapsed_time(e2))
    steps = w + 2 * (h - 1)
    p = float(np.median(tp))
    print(f"{w:>5d}x{h:<6d} {k:5d} {steps:10d} {np.median(tb):9.3f} {p:9.3f} {p * 1e3 / steps:8.3f}", flush=True)
