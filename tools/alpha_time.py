#!/usr/bin/env python3
"""Alpha mode device times (HIP events), for DESIGN.md 4.6:
  kmg_dev_alpha_compact on the tiled photograph of bench.py at 8192^2 with random alpha and cutoff 128 (half the pixels kept) and
  on the default 256^2 shrink; the replace and dither output passes at 8192^2 (k = 64, apply plan runs: the per-pixel kernel
  alone) with alpha mode off and on.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/alpha_time.py` for the
  per-kernel split.
    python tools/alpha_time.py [repeats]"""
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
g = torch.Generator(device="cuda")
g.manual_seed(0xA1FA)
img[:, 3] = torch.randint(0, 256, (n,), generator=g, device="cuda", dtype=torch.uint8)
out = torch.empty_like(img)
d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
p0 = kg.ImageProcessor(shrink_max_dim=0)
p1 = kg.ImageProcessor(shrink_max_dim=0, alpha_cutoff=1)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


small = img[: 256 * 256].clone()
rows = []
for name, src, m in (("8192^2", img, n), ("256^2", small, 256 * 256)):
    ms = timed(lambda: p0.alpha_compact(src.data_ptr(), m, 128, out.data_ptr(), d_n.data_ptr(), st))
    kept = int(d_n.item())
    moved = 4.0 * (2 * m + kept)                                # two reads of the image (count, scatter) + the kept pixels written
    rows.append(f"compact {name:>7} cutoff 128: kept {kept / m:.3f}, {ms * 1000:8.1f} us, {moved / ms / 1e6:7.0f} GB/s over 8 B/px read + 4 B/kept px")

host = img[: 1 << 20].cpu().numpy()
pal = host[np.arange(64, dtype=np.int64) * (host.shape[0] // 64)].copy()
pal[:, 3] = 255
cent = np.zeros((64, 4), np.float32)
kg.lib().kmg_palette_to_centroids(pal.ctypes.data, 64, cent.ctypes.data)
for mode, mname in ((0, "replace"), (1, "dither")):
    t = []
    for p in (p0, p1):
        plan = p.apply_plan(cent, mode, n, st)
        t.append(timed(lambda: plan.run(img.data_ptr(), 8192, 8192, 0, out.data_ptr(), st)))
        plan.close()
    rows.append(f"find {mname:>7} 8192^2 k=64: alpha off {t[0]:.3f} ms, on {t[1]:.3f} ms ({100 * (t[1] / t[0] - 1):+.1f} %)")
print("\n".join(rows))
p0.close(); p1.close()
