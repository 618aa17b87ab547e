#!/usr/bin/env python3
"""Device time of the lossy delta pass (kmg_dev_frame_delta_lossy) at 8192^2, beside the exact delta pass
(kmg_dev_frame_delta) on the same index maps and device-to-device copies.

Three cases, each in a steady state (every launch of a case finds what the one before it found):
  still   every source word equals its held word, the indices equal the canvas: no conversion, nothing stored but the delta map
  noise   every pixel's source differs from its held source by one level per channel, under the tolerance, and the index maps A and F
          (F = A flickered in 60 % of the pixels) are passed in turn: two Lab conversions per pixel, every pixel held
  block   the sources S_A / S_B and the maps A / B differ, far beyond the tolerance, in one rectangle of a tenth of the frame and are
          passed in turn: the rectangle is sent and re-anchored, the rest is still
The exact pass gets the same maps in the same order on a canvas of its own (the parent's pass: the yardstick, not the code under
test).  The copies are one RGBA8 frame and one index map, device to device: 8 + 2 e bytes per pixel moved against the 8 + 3 e the
lossy pass moves at least (e = bytes per index); `floor` is the pass's bytes at the copies' rate.  HIP events around windows of
`launches` calls after a warm-up, the three alternating, the median window of each.
    python tools/frame_hold_time.py [windows] [launches] [output file]      (default: profiles/seq_frame_hold_time.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python"))
import numpy as np
import torch
import kmeans_gpu_amd as kg

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 50
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "seq_frame_hold_time.txt")
assert launches % 2 == 0
W = 8192
n = W * W
K = 255
TOL = kg.tolerance_of(3.0)
st = torch.cuda.current_stream().cuda_stream
proc = kg.ImageProcessor()
fresh = torch.from_numpy(np.frombuffer(kg.FrameHold.fresh_bytes(), np.int64).copy()).cuda()
info = fresh.clone()


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(launches):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3          # us per call


g = torch.Generator(device="cuda").manual_seed(11)
# mid-range colours (bytes 64 .. 191): one level per channel stays far below TOL, 64 levels per channel lie far above it
S_A = torch.randint(64, 192, (W, W, 4), generator=g, device="cuda", dtype=torch.int16).to(torch.uint8)
S_A[..., 3] = 255
S_N = S_A.clone()
S_N[..., :3] ^= 1                                         # the noise: every channel one level off
side = int(W * 0.1 ** 0.5)
S_B = S_A.clone()
S_B[1000:1000 + side, 2000:2000 + side, :3] ^= 0x40

rows = [f"8192^2 pixels, k = {K}, tolerance {TOL} (dE76 3.0); median of {windows} windows of {launches} calls (HIP events), lossy pass, exact "
        f"pass and copies alternating; copies = one RGBA8 frame and one index map, device to device"]
for fmt, tdtype, size, name in ((kg.OutputFormat.Index8, torch.uint8, 1, "INDEX8"), (kg.OutputFormat.Index16, torch.int16, 2, "INDEX16")):
    A = torch.randint(0, K, (W, W), generator=g, device="cuda", dtype=torch.int16).to(tdtype)
    F = torch.where(torch.rand((W, W), generator=g, device="cuda") < 0.6, ((A.to(torch.int32) + 1) % K).to(tdtype), A)
    B = A.clone()
    B[1000:1000 + side, 2000:2000 + side] = ((A[1000:1000 + side, 2000:2000 + side].to(torch.int32) + 1) % K).to(tdtype)
    for case, sources, maps in (("still", (S_A, S_A), (A, A)), ("noise", (S_N, S_N), (A, F)), ("block", (S_A, S_B), (A, B))):
        canvas, held, delta = A.clone(), S_A.clone(), torch.empty_like(A)
        canvas_x, delta_x = A.clone(), torch.empty_like(A)
        spare_f, spare_m = torch.empty_like(S_A), torch.empty_like(A)

        def run_hold(i):
            proc.frame_delta_lossy(sources[i & 1].data_ptr(), maps[i & 1].data_ptr(), canvas.data_ptr(), held.data_ptr(), W, W, 0, fmt, K, TOL,
                                   delta.data_ptr(), info.data_ptr(), st)

        def run_exact(i):
            proc.frame_delta(maps[i & 1].data_ptr(), canvas_x.data_ptr(), W, W, 0, fmt, K, delta_x.data_ptr(), info.data_ptr(), st)

        def run_copy(i):
            spare_f.copy_(sources[i & 1], non_blocking=True)
            spare_m.copy_(maps[i & 1], non_blocking=True)

        # one checked launch of the odd kind: the record is what the case is there to show
        info.copy_(fresh)
        run_hold(1)
        torch.cuda.synchronize()
        rec = kg.FrameHold.from_array(info.cpu().numpy())
        moved = int((maps[0] != maps[1]).sum())
        if case == "still":
            assert rec.as_tuple() == kg.FrameHold.FRESH, rec
        elif case == "noise":
            assert rec.changed == 0 and rec.held == moved and rec.held_sse > 0 and bool((canvas == A).all()) and bool((held == S_A).all()), rec
        else:
            assert rec.changed == moved == side * side and rec.held == 0 and rec.rect == (2000, 1000, 2000 + side, 1000 + side), rec
            assert bool((canvas == B).all()) and bool((held == S_B).all())
        for i in range(2, 12):                                 # warm-up (an even start: the next launch is of the even kind)
            run_hold(i)
            run_exact(i)
            run_copy(i)
        torch.cuda.synchronize()
        t_hold, t_exact, t_copy = [], [], []
        for _ in range(windows):
            t_hold.append(window(run_hold))
            t_exact.append(window(run_exact))
            t_copy.append(window(run_copy))
        h, x, c = float(np.median(t_hold)), float(np.median(t_exact)), float(np.median(t_copy))
        pass_bytes, copy_bytes = (8 + 3 * size) * n, (8 + 2 * size) * n
        floor = pass_bytes / (copy_bytes / c)
        rows.append(f"{name:<8} {case:<6} changed {int(rec.changed):>8} held {int(rec.held):>9}: lossy {h:7.1f} us (min {min(t_hold):.1f}, max {max(t_hold):.1f}), "
                    f"exact {x:7.1f} us (min {min(t_exact):.1f}, max {max(t_exact):.1f}), copies {c:7.1f} us (min {min(t_copy):.1f}, "
                    f"max {max(t_copy):.1f}); lossy moves >= {pass_bytes / 2**20:.0f} MiB: {pass_bytes / h / 1e6:.2f} TB/s, floor at the copies' "
                    f"rate {floor:7.1f} us, lossy / floor {h / floor:5.2f}, lossy / exact {h / x:5.2f}")
text = "\n".join(rows)
print(text)
with open(out_path, "w") as f:
    f.write(text + "\n")
proc.close()
