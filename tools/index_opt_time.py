#!/usr/bin/env python3
"""Index-map optimisation device times (HIP events), for DESIGN.md 4.13: repeated kmg_dev_index_usage (k = 256) and
kmg_dev_index_remap (8 -> 8 at k = 256, 8 -> 4 at k = 16) launches on 8192^2 INDEX8 maps -- uniform noise, a constant map and the
replace map of the tiled photograph of bench.py -- each beside the floor of its bytes at 6.29 TB/s and beside kmg_dev_compare (RGB
only, INDEX8: 4 + 1 bytes per pixel) on the same map; then the constant / noise and photograph / noise ratios of the usage pass,
which say whether the wave-agreement shortcut does its job.
    python tools/index_opt_time.py [repeats] > profiles/index_opt_time.txt"""
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
W = 8192
n = W * W
COPY_RATE = 6.29e12          # bytes / s: the copy rate the byte floors are computed from
F = kg.OutputFormat
img = bench.synthetic_image("photo", n, 0, 64, 0x5EED0B10)
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


def photo_map(k):
    host = img[: 1 << 20].cpu().numpy()
    pal = host[np.arange(k, dtype=np.int64) * (host.shape[0] // k)].copy()
    pal[:, 3] = 255
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    proc.apply(img.data_ptr(), W, W, 0, kg.palette_to_centroids(pal), 0, out.data_ptr(), st, format=F.Index8)
    torch.cuda.synchronize()
    return out, pal


gen = torch.Generator(device="cuda").manual_seed(5)
rows = [f"8192^2 INDEX8 maps, mean of {reps} launches after one warm-up (the remap with its table's upload); floor = bytes / 6.29 TB/s"]
usage_ms = {}
for k, passes in ((256, ("usage", "remap 8 -> 8")), (16, ("remap 8 -> 4",))):
    photo, pal = photo_map(k)
    maps = (("noise", torch.randint(0, k, (n,), dtype=torch.uint8, device="cuda", generator=gen)),
            ("constant", torch.full((n,), k // 3, dtype=torch.uint8, device="cuda")), ("photograph", photo))
    d_usage = torch.zeros(k + 2, dtype=torch.int64, device="cuda")
    d_stats = torch.zeros(14, dtype=torch.int64, device="cuda")
    d_bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    remap = np.arange(k + 1, dtype=np.uint16)[::-1].copy() % k          # a permutation of the colours; the slot is not in these maps
    for name, m in maps:
        t_cmp = timed(lambda: proc.compare_device(img.data_ptr(), m.data_ptr(), n, d_stats.data_ptr(), F.Index8, pal, 0, kg.ERROR_RGB, st), reps)
        for what in passes:
            if what == "usage":
                t = timed(lambda: proc.index_usage_device(m.data_ptr(), n, F.Index8, k, d_usage.data_ptr(), st), reps)
                usage_ms[name] = t
                bpp = 1.0
            else:
                bits = 8 if what.endswith("8") else 4
                out = torch.empty(n * bits // 8, dtype=torch.uint8, device="cuda")
                t = timed(lambda: proc.index_remap_device(m.data_ptr(), F.Index8, W, W, k, remap, bits, out.data_ptr(), d_bad.data_ptr(), st), reps)
                bpp = 1.0 + bits / 8.0
            floor = n * bpp / COPY_RATE * 1e3
            rows.append(f"{what:<13} k={k:<3} {name:<10}: {t * 1e3:8.1f} us, floor {floor * 1e3:6.1f} us ({100 * floor / t:5.1f} % of the copy rate), "
                        f"{t / t_cmp:5.2f} x kmg_dev_compare ({t_cmp * 1e3:7.1f} us)")
    assert int(d_bad[0]) == 0
rows.append(f"usage pass: constant / noise = {usage_ms['constant'] / usage_ms['noise']:.2f}, photograph / noise = "
            f"{usage_ms['photograph'] / usage_ms['noise']:.2f}")
print("\n".join(rows))
proc.close()
