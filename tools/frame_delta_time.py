#!/usr/bin/env python3
"""Device time of the delta pass (kmg_dev_frame_delta) at 8192^2, beside device-to-device copies of the same bytes.

Two index maps A and B that differ in about a tenth of their pixels are passed in turn, so every launch finds a tenth of the
canvas changed: `scattered` spreads the changes over the whole frame (nearly every 16-byte chunk of the canvas is rewritten),
`block` puts them into one rectangle (what an animation looks like: the canvas is rewritten only there).  The copy beside it is two
hipMemcpyAsync device-to-device copies of one map each: two streams read, two written, as the pass reads index and canvas and writes
delta and canvas.  HIP events around windows of `launches` calls after a warm-up, pass and copy alternating, the median window of
each.
    python tools/frame_delta_time.py [windows] [launches] > profiles/seq_frame_delta_time.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python"))
import numpy as np
import torch
import kmeans_gpu_amd as kg

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 200
W = 8192
n = W * W
st = torch.cuda.current_stream().cuda_stream
proc = kg.ImageProcessor()
fresh = torch.from_numpy(np.frombuffer(kg.FrameDelta.fresh_bytes(), np.int64).copy()).cuda()
info = fresh.clone()


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(launches):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3          # us per call


rows = [f"8192^2 pixels, k = 255, about a tenth of the pixels changed per launch; median of {windows} windows of {launches} calls (HIP events), "
        f"pass and copy alternating; copy = two hipMemcpyAsync device-to-device of one map each"]
for fmt, tdtype, size, name in ((kg.OutputFormat.Index8, torch.uint8, 1, "INDEX8"), (kg.OutputFormat.Index16, torch.int16, 2, "INDEX16")):
    g = torch.Generator(device="cuda").manual_seed(7)
    A = torch.randint(0, 255, (W, W), generator=g, device="cuda", dtype=torch.int16).to(tdtype)
    for pattern in ("scattered", "block"):
        B = A.clone()
        if pattern == "scattered":
            m = torch.rand((W, W), generator=g, device="cuda") < 0.1
            B[m] = ((A[m].to(torch.int32) + 1) % 255).to(tdtype)
        else:
            s = int(W * 0.1 ** 0.5)
            B[1000:1000 + s, 2000:2000 + s] = ((A[1000:1000 + s, 2000:2000 + s].to(torch.int32) + 1) % 255).to(tdtype)
        maps = (A, B)
        canvas, delta, spare = B.clone(), torch.empty_like(A), torch.empty_like(A)

        def run_pass(i):
            proc.frame_delta(maps[i & 1].data_ptr(), canvas.data_ptr(), W, W, 0, fmt, 255, delta.data_ptr(), info.data_ptr(), st)

        def run_copy(i):
            delta.copy_(maps[i & 1], non_blocking=True)
            spare.copy_(canvas, non_blocking=True)

        # one checked launch: the record is the difference of the two maps
        info.copy_(fresh)
        run_pass(0)
        torch.cuda.synchronize()
        rec = kg.FrameDelta.from_array(info.cpu().numpy())
        assert int(rec.changed) == int((A != B).sum()) and bool((canvas == A).all()), rec
        for i in range(1, 21):                                 # warm-up (an odd start: the canvas holds A)
            run_pass(i)
            run_copy(i)
        torch.cuda.synchronize()
        t_pass, t_copy = [], []
        for _ in range(windows):
            t_pass.append(window(lambda i: run_pass(i + 1)))   # `launches` is even: every window starts from a canvas of A
            t_copy.append(window(run_copy))
        p, c = float(np.median(t_pass)), float(np.median(t_copy))
        moved = 4 * n * size
        rows.append(f"{name:<8} {pattern:<10} changed {int(rec.changed):>9} px, box {rec.rect}: pass {p:7.1f} us (min {min(t_pass):.1f}, max {max(t_pass):.1f}), "
                    f"copies {c:7.1f} us (min {min(t_copy):.1f}, max {max(t_copy):.1f}), ratio {p / c:5.2f}; "
                    f"{moved / 2**20:.0f} MiB moved: {moved / p / 1e6:.2f} TB/s pass, {moved / c / 1e6:.2f} TB/s copies")
print("\n".join(rows))
proc.close()
