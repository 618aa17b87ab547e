#!/usr/bin/env python3
"""Device time of the colour-keyed delta passes (kmg_dev_frame_delta_colour / _colour_lossy) at 8192^2, k = 255,
beside the index passes (kmg_dev_frame_delta / _lossy) on the same index maps and device-to-device copies of the same bytes.

A tenth of the pixels changes per frame, in two layouts, each in a steady state (the maps A / B and the sources S_A / S_B are passed
in turn, so every launch finds what the one before it found):
  block    one rectangle of a tenth of the frame
  scatter  every tenth pixel of the flat frame
One palette of distinct colours serves both maps, so the colour passes and the index passes send the same pixels.  The copies are,
device to device, what each pass reads at least: the index map and the shown canvas (exact: e + 4 bytes per pixel, e = bytes per
index), plus the source and the held source (lossy: e + 12); `floor` is the pass's bytes, its delta map and the changed tenth of its
canvases included, at the copies' rate.  HIP events around windows of `launches` calls after a warm-up, the passes alternating, the
median window of each.

Then the warm start on a still scene with noise, cold beside warm: the Lloyd iterations of every frame -- from a kmg_lloyd object
driven as the sequence drives its own (farthest-point initialisation for a cold frame, a seeded one with all k of the previous
frame's centroids for a warm frame) -- and, from Sequence.output_local itself, the changed pixels of the exact delta frames and
the palette entries that differ from the previous frame's.  Reported, not asserted.
    python tools/frame_local_time.py [windows] [launches] [output file]      (default: profiles/local_frame_time.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python"))
import numpy as np
import torch
import kmeans_gpu_amd as kg

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 40
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "local_frame_time.txt")
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
S_A = torch.randint(64, 192, (W, W, 4), generator=g, device="cuda", dtype=torch.int16).to(torch.uint8)
S_A[..., 3] = 255
side = int(W * 0.1 ** 0.5)
block = torch.zeros((W, W), dtype=torch.bool, device="cuda")
block[1000:1000 + side, 2000:2000 + side] = True
scatter = (torch.arange(n, device="cuda") % 10 == 0).reshape(W, W)
# K distinct opaque colours: index i shows (i, 255 - i, 7 i mod 256, 255)
idx = np.arange(K)
pal_host = np.stack([idx, 255 - idx, (7 * idx) % 256, np.full(K, 255)], axis=1).astype(np.uint8)
palette = torch.from_numpy(pal_host).cuda()
pal_words = torch.from_numpy(np.concatenate([pal_host.view("<u4").reshape(-1).astype(np.int64), [0]])).cuda()

rows = [f"8192^2 pixels, k = {K}, a tenth of the pixels changed per frame, tolerance {TOL} (dE76 3.0); median of {windows} windows of {launches} "
        f"calls (HIP events), colour pass, index pass and copies alternating"]
for fmt, tdtype, size, name in ((kg.OutputFormat.Index8, torch.uint8, 1, "INDEX8"), (kg.OutputFormat.Index16, torch.int16, 2, "INDEX16")):
    A = torch.randint(0, K, (W, W), generator=g, device="cuda", dtype=torch.int16).to(tdtype)
    for layout, mask in (("block", block), ("scatter", scatter)):
        B = torch.where(mask, ((A.to(torch.int32) + 1) % K).to(tdtype), A)
        S_B = torch.where(mask[..., None], S_A ^ torch.tensor([0x40, 0x40, 0x40, 0], dtype=torch.uint8, device="cuda"), S_A)
        maps, sources = (A, B), (S_A, S_B)
        moved = int(mask.sum())
        for lossy in (False, True):
            shown = pal_words[A.to(torch.int64) & 0xFFFF].to(torch.int32)
            held, delta = S_A.clone(), torch.empty_like(A)
            canvas_x, held_x, delta_x = A.clone(), S_A.clone(), torch.empty_like(A)
            spare_w, spare_m = torch.empty_like(shown), torch.empty_like(A)
            spare_f, spare_h = torch.empty_like(S_A), torch.empty_like(S_A)

            def run_colour(i):
                if lossy:
                    proc.frame_delta_colour_lossy(sources[i & 1].data_ptr(), maps[i & 1].data_ptr(), palette.data_ptr(), shown.data_ptr(),
                                                  held.data_ptr(), W, W, 0, fmt, K, TOL, delta.data_ptr(), info.data_ptr(), st)
                else:
                    proc.frame_delta_colour(maps[i & 1].data_ptr(), palette.data_ptr(), shown.data_ptr(), W, W, 0, fmt, K, delta.data_ptr(),
                                            info.data_ptr(), st)

            def run_index(i):
                if lossy:
                    proc.frame_delta_lossy(sources[i & 1].data_ptr(), maps[i & 1].data_ptr(), canvas_x.data_ptr(), held_x.data_ptr(), W, W, 0, fmt, K,
                                           TOL, delta_x.data_ptr(), info.data_ptr(), st)
                else:
                    proc.frame_delta(maps[i & 1].data_ptr(), canvas_x.data_ptr(), W, W, 0, fmt, K, delta_x.data_ptr(), info.data_ptr(), st)

            def run_copy(i):
                spare_m.copy_(maps[i & 1], non_blocking=True)
                spare_w.copy_(shown, non_blocking=True)
                if lossy:
                    spare_f.copy_(sources[i & 1], non_blocking=True)
                    spare_h.copy_(held, non_blocking=True)

            # one checked launch of the odd kind: the tenth is sent, nothing else
            info.copy_(fresh)
            run_colour(1)
            torch.cuda.synchronize()
            rec = kg.FrameHold.from_array(info.cpu().numpy())
            assert rec.changed == moved and rec.cleared == 0 and rec.held == 0, rec
            assert bool((shown == pal_words[B.to(torch.int64) & 0xFFFF].to(torch.int32)).all())
            run_index(1)
            for i in range(2, 10):                                 # warm-up (an even start)
                run_colour(i)
                run_index(i)
                run_copy(i)
            torch.cuda.synchronize()
            t_col, t_idx, t_copy = [], [], []
            for _ in range(windows):
                t_col.append(window(run_colour))
                t_idx.append(window(run_index))
                t_copy.append(window(run_copy))
            c, x, cp = float(np.median(t_col)), float(np.median(t_idx)), float(np.median(t_copy))
            copy_bytes = 2 * (size + 4 + (8 if lossy else 0)) * n                       # read and written
            pass_bytes = (size + 4 + (8 if lossy else 0)) * n + size * n + (4 + (4 if lossy else 0)) * moved
            floor = pass_bytes / (copy_bytes / cp)
            rows.append(f"{name:<8} {'lossy' if lossy else 'exact':<5} {layout:<8} changed {moved:>8}: colour {c:7.1f} us (min {min(t_col):.1f}, max {max(t_col):.1f}), "
                        f"index pass {x:7.1f} us (min {min(t_idx):.1f}, max {max(t_idx):.1f}), copies {cp:7.1f} us (min {min(t_copy):.1f}, "
                        f"max {max(t_copy):.1f}); colour moves >= {pass_bytes / 2**20:.0f} MiB: {pass_bytes / c / 1e6:.2f} TB/s, floor at the copies' "
                        f"rate {floor:7.1f} us, colour / floor {c / floor:5.2f}, colour / index {c / x:5.2f}")
            del shown, held, delta, canvas_x, held_x, delta_x, spare_w, spare_m, spare_f, spare_h
        del B, S_B
    del A
del S_A, block, scatter
torch.cuda.empty_cache()

# ---- the warm start on a still scene with noise ----------------------------------------------------------------------------------
h, w, k, frames_n = 256, 384, 64, 6
rng = np.random.default_rng(3)
y, x = np.mgrid[0:h, 0:w]
base = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y) * 255) // (w + h - 2), np.full((h, w), 255)], axis=2).astype(np.int64)
frames = []
for t in range(frames_n):
    f = base.copy()
    f[..., :3] += rng.integers(-2, 3, (h, w, 3))
    frames.append(np.clip(f, 0, 255).astype(np.uint8))
for warm in (False, True):
    # the Lloyd loop of every frame, as kmg_sequence_output_frame_local runs it (the frames fit shrink_max_dim: no shrink)
    iterations, prev_c = [], None
    for f in frames:
        d = torch.from_numpy(f).cuda()
        lloyd = kg.Lloyd(proc, k)
        if warm and prev_c is not None:
            lloyd.init_centroids_seeded(d.data_ptr(), w, h, prev_c, st)
        else:
            lloyd.init_centroids(d.data_ptr(), w, h, st)
        iterations.append(int(lloyd.run(d.data_ptr(), w * h, 0, st)))
        prev_c = lloyd.get_centroids(st)
        lloyd.close()
    with proc.sequence() as seq:
        seq.output_local(k, kg.ReduceMode.Replace, kg.OutputFormat.Index8, w, h, warm=warm)
        changed, moved_entries, prev = [], [], None
        for f in frames:
            m, pal, rec, full = seq.frame_local(f)
            changed.append(int(rec.changed))
            moved_entries.append(k if prev is None else int((pal != prev).any(axis=1).sum()))
            prev = pal
    rows.append(f"still scene with noise +-2, {w}x{h}, k = {k}, exact delta frames, {'warm' if warm else 'cold'}: Lloyd iterations per frame {iterations}, "
                f"changed pixels per frame {changed}, palette entries that differ from the previous frame's {moved_entries}")
text = "\n".join(rows)
print(text)
with open(out_path, "w") as f:
    f.write(text + "\n")
proc.close()
