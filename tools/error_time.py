#!/usr/bin/env python3
"""Error statistics device times (HIP events), for DESIGN.md 4.8: repeated kmg_dev_compare launches on the tiled photograph of
bench.py at 8192^2 -- RGB only for RGBA8 / INDEX8 / INDEX16, RGB + Lab for RGBA8 and INDEX8 at k = 64 and 256, and the RGBA8 Lab
skip on unchanged (out = src) and fully changed outputs -- each beside the floor of its bytes at 6.29 TB/s; then kmg_reduce_quality
end to end on tokyo.png (three targets, k in [2, 64]) beside the cost of the same search made from outside: its palette runs times
kmg_reduce at k_max.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
    python tools/error_time.py [repeats] > profiles/r10_error_time.txt"""
import os
import sys
import time

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
img = bench.synthetic_image("photo", n, 0, 64, 0x5EED0B10)
proc = kg.ImageProcessor(shrink_max_dim=0)
d_stats = torch.zeros(14, dtype=torch.int64, device="cuda")


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
outs = {}
for k in (64, 256):
    pal = host[np.arange(k, dtype=np.int64) * (host.shape[0] // k)].copy()
    pal[:, 3] = 255
    cent = kg.palette_to_centroids(pal)
    rgba = torch.empty_like(img)
    idx8 = torch.empty(n, dtype=torch.uint8, device="cuda")
    idx16 = torch.empty(n, dtype=torch.int16, device="cuda")
    proc.apply(img.data_ptr(), W, W, 0, cent, 0, rgba.data_ptr(), st)
    proc.apply(img.data_ptr(), W, W, 0, cent, 0, idx8.data_ptr(), st, format=kg.OutputFormat.Index8)
    proc.apply(img.data_ptr(), W, W, 0, cent, 0, idx16.data_ptr(), st, format=kg.OutputFormat.Index16)
    # the palette the indices stand for: the bytes of the RGBA8 pass (lab_to_rgb.wgsl of each centroid)
    first = {}
    h_idx, h_rgba = idx8[: 1 << 22].cpu().numpy(), rgba[: 1 << 22].cpu().numpy().reshape(-1, 4)
    P = np.zeros((k, 4), np.uint8)
    for i in range(k):
        hit = np.flatnonzero(h_idx == i)
        if hit.size:
            P[i] = h_rgba[hit[0]]
    outs[k] = (rgba, idx8, idx16, P)
torch.cuda.synchronize()


def run(out, fmt, pal, what):
    proc.compare_device(img.data_ptr(), out.data_ptr(), n, d_stats.data_ptr(), fmt, pal, 0, what, st)


RGB, LAB = kg.ERROR_RGB, kg.ERROR_LAB
F = kg.OutputFormat
rows = [f"8192^2 tiled photograph, kmg_dev_compare, mean of {reps} launches after one warm-up (index formats: with the palette's upload "
        f"and its q launch); floor = bytes / 6.29 TB/s"]
base = {}
rgba, idx8, idx16, P = outs[256]
for name, out, fmt, pal, bpp in (("RGBA8", rgba, F.RGBA8, None, 8), ("INDEX8 k=256", idx8, F.Index8, P, 5), ("INDEX16 k=256", idx16, F.Index16, P, 6)):
    t = timed(lambda: run(out, fmt, pal, RGB), reps)
    base[name.split()[0]] = t
    floor = n * bpp / COPY_RATE * 1e3
    rows.append(f"RGB only    {name:<14}: {t * 1e3:8.1f} us, floor {floor * 1e3:6.1f} us ({100 * floor / t:5.1f} % of the copy rate)")
for k in (64, 256):
    rgba, idx8, idx16, P = outs[k]
    for name, out, fmt, pal, bpp in ((f"RGBA8 k={k}", rgba, F.RGBA8, None, 8), (f"INDEX8 k={k}", idx8, F.Index8, P, 5)):
        t = timed(lambda: run(out, fmt, pal, RGB | LAB), reps)
        floor = n * bpp / COPY_RATE * 1e3
        rows.append(f"RGB + Lab   {name:<14}: {t * 1e3:8.1f} us, floor {floor * 1e3:6.1f} us, {t / base[name.split()[0]]:5.2f} x the RGB-only time")
same = img
flipped = (img.view(torch.int32) ^ 0x00FFFFFF).view(torch.uint8)
for name, out in (("unchanged (out = src)", same), ("fully changed", flipped)):
    for what, wname in ((LAB, "Lab only "), (RGB | LAB, "RGB + Lab")):
        t = timed(lambda: run(out, F.RGBA8, None, what), reps)
        rows.append(f"{wname}   RGBA8 {name:<22}: {t * 1e3:8.1f} us, {t / base['RGBA8']:5.2f} x the RGB-only time")
d_stats.zero_()
run(outs[256][0], F.RGBA8, None, RGB | LAB)
torch.cuda.synchronize()
rows.append("record of RGBA8 k=256: " + repr(kg.ErrorStats.from_array(d_stats.cpu().numpy().view(np.uint64))))
proc.close()

# ---- kmg_reduce_quality end to end ---------------------------------------------------------------------------------------------
from PIL import Image
tokyo = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "tokyo.png")).convert("RGBA"))
proc = kg.ImageProcessor()
L = kg.lib()
import ctypes as C


def quality(k_min, k_max, target):
    h, w = tokyo.shape[:2]
    out = np.empty((h, w), np.uint8)
    pal = np.zeros((k_max, 4), np.uint8)
    cnt, reached, stats = C.c_uint32(), C.c_int(), kg.ErrorStats()
    rc = L.kmg_reduce_quality(proc.handle, C.c_void_p(tokyo.ctypes.data), w, h, k_min, k_max, int(target), 0, 1, C.c_void_p(pal.ctypes.data),
                              C.byref(cnt), C.c_void_p(out.ctypes.data), C.byref(stats), C.byref(reached))
    assert rc == 0, L.kmg_last_error()
    return cnt.value, bool(reached.value), stats


def wall(fn, r):
    fn()
    t0 = time.perf_counter()
    for _ in range(r):
        fn()
    return (time.perf_counter() - t0) / r * 1e3


E = {}


def e_of(k):
    if k not in E:
        E[k] = quality(k, k, 0)[2]
    return int(E[k].lab_sse), int(E[k].pixels)


def runs_of(target):
    """palette runs of the fixed search, from E(k) at single counts"""
    npx = e_of(64)[1]
    ok = lambda k: e_of(k)[0] <= target * npx
    runs = 1
    if not ok(64):
        return runs
    lo, hi = 2, 64
    while lo < hi:
        mid = (lo + hi) // 2
        runs += 1
        if ok(mid):
            hi = mid
        else:
            lo = mid + 1
    return runs


npx = e_of(64)[1]
t_reduce = wall(lambda: proc.reduce(64, tokyo), 10)
rows.append(f"kmg_reduce_quality on tokyo.png (768 x 513, working image {npx} pixels), k in [2, 64], replace, INDEX8; kmg_reduce at k = 64: "
            f"{t_reduce:.2f} ms")
for name, target in (("E(12)", -(-e_of(12)[0] // npx)), ("E(64) - 1", (e_of(64)[0] - 1) // npx), ("E(2)", -(-e_of(2)[0] // npx))):
    k, reached, stats = quality(2, 64, target)
    t = wall(lambda: quality(2, 64, target), 5)
    r = runs_of(target)
    rows.append(f"target {name:<9} = {target:>8}: k* = {k:>2}, reached = {int(reached)}, dE76 rms {stats.delta_e_rms:.3f}: {t:7.2f} ms end to end, "
                f"{r} palette runs x kmg_reduce(64) = {r * t_reduce:7.2f} ms from outside")
print("\n".join(rows))
proc.close()
