#!/usr/bin/env python3
"""Clip output: kmg_sequence_output_frames against the same frames one call at a time, and the device time of
kmg_dev_frame_delta_clip against kmg_dev_frame_delta_lossy called per frame.

(a) End to end, host buffers in, host buffers out.  T = 2, 8, 32, 128 frames of 256 x 256 (tokyo.png shifted a pixel per frame, plus
    noise of two levels), k = 8 / 64 / 255, replace and dither, exact and lossy (dE76 3.0), INDEX8.  Two sequences of one warm
    processor with the same palette: one takes the clip in one call, the other the same frames through kmg_sequence_output_frame /
    _lossy (the per-frame path: the yardstick, not the code under test).  They take turns; the minimum of five wall-clock times each.
(b) The walk alone: 8 resident frames of 8192^2, INDEX8, k = 255, in the three cases of tools/frame_hold_time.py (still, noise,
    block), HIP events around one clip call against eight per-frame calls, per frame; beside them the device-to-device copies of
    4 + 2 e bytes per pixel and frame (one RGBA8 frame and two index maps), the bytes a frame of the clip has to move.
    python tools/frame_clip_time.py [repeats] [output file]      (default: profiles/r12_clip_time.txt)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python"))
import numpy as np
import torch
from PIL import Image
import kmeans_gpu_amd as kg

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r12_clip_time.txt")
TOL = kg.tolerance_of(3.0)
proc = kg.ImageProcessor()
rows = []


def say(line):
    rows.append(line)
    print(line, flush=True)


# ---- (a) end to end -----------------------------------------------------------------------------------------------------------------
tokyo = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "tokyo.png")).convert("RGBA"))
rng = np.random.default_rng(5)
S = 256
frames = []
for t in range(128):
    f = np.ascontiguousarray(tokyo[100:100 + S, 200 + t:200 + t + S]).astype(np.int64)
    f[..., :3] = np.clip(f[..., :3] + rng.integers(-2, 3, (S, S, 3)), 0, 255)
    frames.append(f.astype(np.uint8))

say(f"(a) frames of {S} x {S}, INDEX8; wall clock of the whole clip, minimum of {repeats}, clip call and per-frame calls taking turns; "
    "ms per clip, ratio = clip call / per-frame calls")
worst = {}
for k in (8, 64, 255):
    for mode, mname in ((kg.ReduceMode.Replace, "replace"), (kg.ReduceMode.Dither, "dither")):
        with proc.sequence() as a, proc.sequence() as b:
            for f in frames[:2]:
                a.add(f); b.add(f)
            assert np.array_equal(a.output(k, mode, kg.OutputFormat.Index8, S, S), b.output(k, mode, kg.OutputFormat.Index8, S, S))
            for tol, tname in ((None, "exact"), (TOL, "lossy")):
                for T in (2, 8, 32, 128):
                    clip = frames[:T]
                    got = a.frames(clip, tolerance=tol)                # warm, and checked once
                    want = [b.frame(f, tolerance=tol) for f in clip]
                    assert all(np.array_equal(g[0], w[0]) and g[1].as_tuple() == w[1].as_tuple() and g[2] == w[2] for g, w in zip(got, want))
                    t_clip, t_each = [], []
                    for _ in range(repeats):
                        t0 = time.perf_counter()
                        a.frames(clip, tolerance=tol)
                        t1 = time.perf_counter()
                        for f in clip:
                            b.frame(f, tolerance=tol)
                        t2 = time.perf_counter()
                        t_clip.append(t1 - t0); t_each.append(t2 - t1)
                    c, e = min(t_clip) * 1e3, min(t_each) * 1e3
                    worst[T] = max(worst.get(T, 0.0), c / e)
                    r = a.last_clip_report
                    say(f"k {k:>3} {mname:<7} {tname:<5} T {T:>3}: clip {c:8.3f} ms, per frame {e:8.3f} ms, ratio {c / e:5.2f}  "
                        f"(launches {r.launches}, batched {r.batched}, per image {r.per_image})")
say("(a) worst ratio per T: " + ", ".join(f"T {T}: {v:.2f}" for T, v in sorted(worst.items())))

# ---- (b) the walk alone ---------------------------------------------------------------------------------------------------------------
W, K, T = 8192, 255, 8
n = W * W
st = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda").manual_seed(11)
S_A = torch.randint(64, 192, (W, W, 4), generator=g, device="cuda", dtype=torch.int16).to(torch.uint8)
S_A[..., 3] = 255
S_N = S_A.clone()
S_N[..., :3] ^= 1
side = int(W * 0.1 ** 0.5)
S_B = S_A.clone()
S_B[1000:1000 + side, 2000:2000 + side, :3] ^= 0x40
A = torch.randint(0, K, (W, W), generator=g, device="cuda", dtype=torch.int16).to(torch.uint8)
F = torch.where(torch.rand((W, W), generator=g, device="cuda") < 0.6, ((A.to(torch.int32) + 1) % K).to(torch.uint8), A)
B = A.clone()
B[1000:1000 + side, 2000:2000 + side] = ((A[1000:1000 + side, 2000:2000 + side].to(torch.int32) + 1) % K).to(torch.uint8)
fresh = torch.from_numpy(np.tile(np.frombuffer(kg.FrameHold.fresh_bytes(), np.int64), T).copy()).cuda()
info, info1 = fresh.clone(), fresh[:6].clone()
outs = [torch.empty_like(A) for _ in range(T)]
spare_f, spare_m, spare_d = torch.empty_like(S_A), torch.empty_like(A), torch.empty_like(A)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / T                   # us per frame


say(f"(b) {T} resident frames of {W}^2, INDEX8, k = {K}, tolerance {TOL}; HIP events, us per frame, median of {repeats}; copies = one "
    "RGBA8 frame and two index maps per frame, device to device")
for case, sources, maps in (("still", (S_A, S_A), (A, A)), ("noise", (S_N, S_N), (A, F)), ("block", (S_A, S_B), (A, B))):
    src = [sources[t & 1] for t in range(T)]
    idx = [maps[t & 1] for t in range(T)]
    canvas, held = A.clone(), S_A.clone()
    canvas_x, held_x, delta_x = A.clone(), S_A.clone(), torch.empty_like(A)

    def run_clip():
        proc.frame_delta_clip([s.data_ptr() for s in src], [m.data_ptr() for m in idx], canvas.data_ptr(), held.data_ptr(), W, W,
                              kg.OutputFormat.Index8, K, [TOL] * T, [o.data_ptr() for o in outs], info.data_ptr(), 0, 0, st)

    def run_each():
        for t in range(T):
            proc.frame_delta_lossy(src[t].data_ptr(), idx[t].data_ptr(), canvas_x.data_ptr(), held_x.data_ptr(), W, W, 0, kg.OutputFormat.Index8, K,
                                   TOL, delta_x.data_ptr(), info1.data_ptr(), st)

    def run_copy():
        for t in range(T):
            spare_f.copy_(src[t], non_blocking=True)
            spare_m.copy_(idx[t], non_blocking=True)
            spare_d.copy_(idx[t], non_blocking=True)

    info.copy_(fresh)
    run_clip(); run_each(); run_copy()                      # warm-up; the states agree afterwards
    torch.cuda.synchronize()
    assert bool((canvas == canvas_x).all()) and bool((held == held_x).all()) and bool((outs[T - 1] == delta_x).all())
    recs = [kg.FrameHold.from_array(info.cpu().numpy()[6 * t:6 * t + 6]) for t in range(T)]
    t_clip, t_each, t_copy = [], [], []
    for _ in range(repeats):
        t_clip.append(timed(run_clip)); t_each.append(timed(run_each)); t_copy.append(timed(run_copy))
    c, e, f = float(np.median(t_clip)), float(np.median(t_each)), float(np.median(t_copy))
    say(f"{case:<6} changed/frame {int(recs[-1].changed):>8} held/frame {int(recs[-1].held):>9}: clip {c:7.1f} us (min {min(t_clip):.1f}), per-frame "
        f"passes {e:7.1f} us (min {min(t_each):.1f}), copies {f:7.1f} us (min {min(t_copy):.1f}); clip / per-frame {c / e:5.2f}, clip / copies "
        f"{c / f:5.2f}; clip moves >= {6 * n / 2**20:.0f} MiB a frame: {6 * n / c / 1e6:.2f} TB/s")
with open(out_path, "w") as fh:
    fh.write("\n".join(rows) + "\n")
proc.close()
