#!/usr/bin/env python3
"""Host time of making an apply plan: kmg_apply_plan_create + a synchronise of its stream + kmg_apply_plan_destroy, the fastest of
`reps` after one warm-up, for k = 8, 256 and 3072 in each of the four modes, once with a hint of 65 536 pixels (the scan routes,
and the lists of k >= 128) and once with 8192^2 (the colour table, the lists, the mask words).  No image: a plan is built from the
centroid table alone.  One JSON line, microseconds.
    python tools/apply_plan_time.py [reps]          (KMG_LIBRARY selects another build of the library)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python"))
import numpy as np
import torch
import kmeans_gpu_amd as kg

MODES = (("replace", kg.ReduceMode.Replace), ("dither", kg.ReduceMode.Dither), ("meld", kg.ReduceMode.Meld),
         ("diffuse", kg.ReduceMode.Diffuse))
HINTS = (("64k", 65536), ("8192sq", 8192 * 8192))


def plan_times(reps=20):
    rng = np.random.default_rng(8192)
    proc = kg.ImageProcessor()
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for k in (8, 256, 3072):
        rgb = rng.choice(1 << 24, k, replace=False).astype(np.uint32) | np.uint32(0xFF000000)
        cent = kg.palette_to_centroids(rgb.view(np.uint8).reshape(k, 4))
        for mode_name, mode in MODES:
            for hint_name, hint in HINTS:
                best = None
                for i in range(reps + 1):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    plan = proc.apply_plan(cent, int(mode), hint, st)
                    torch.cuda.current_stream().synchronize()
                    plan.close(synchronise=False)
                    dt = (time.perf_counter() - t) * 1e6
                    if i and (best is None or dt < best):
                        best = dt
                out[f"plan_{mode_name}_k{k}_{hint_name}_us"] = round(best, 2)
    proc.close()
    return out


if __name__ == "__main__":
    print(json.dumps(plan_times(int(sys.argv[1]) if len(sys.argv) > 1 else 20)))
