#!/usr/bin/env python3
"""Alpha weighting (kmg_processor_set_weighting) against the same call without it, for DESIGN.md 4.15: whole host-buffer calls of
one warm processor on the reference's test image (tests/golden/tokyo.png, 1200 x 800: shrunk to 256 x 171 first), host clock around
calls that return synchronised.
  reduce -c 8 (replace) and palette at k = 256, each with the weighting off and on, on the opaque image (every pixel weighs 255:
  the weighted loop alone) and with a random importance map 1 .. 255 in the alpha byte (the centroids move; no compaction: every
  pixel is kept in both settings).  Three settings alternate -- off; alpha mode at cutoff 1 without weighting, which runs the same
  compaction and read-back of the kept count as the weighting does (its reduce also keeps the input's alpha in the output); on --
  in `rounds` rounds of `calls` calls each: the mean of the round means and their lowest and highest.
    python tools/weight_time.py [rounds] [calls]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python"))
import numpy as np
from PIL import Image
import kmeans_gpu_amd as kg

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 40
tokyo = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "tokyo.png")).convert("RGBA"))
rng = np.random.default_rng(0xA1FA)
mapped = kg.with_weights(tokyo, rng.integers(1, 256, tokyo.shape[:2], dtype=np.uint8))
proc = kg.ImageProcessor()
out = np.empty_like(tokyo)


def round_ms(fn):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1000.0 / calls


SETTINGS = (("off", 0, False), ("cutoff 1", 1, False), ("on", 0, True))


def setting(t, on):
    proc.set_alpha_cutoff(t)
    proc.set_alpha_weight(on)


for what, img in (("opaque", tokyo), ("importance map", mapped)):
    for name, fn in (("reduce -c 8 replace", lambda: proc.reduce(8, img, out=out)), ("palette k = 256", lambda: proc.palette(256, img))):
        ms = {s[0]: [] for s in SETTINGS}
        for _, t, on in SETTINGS:                                      # warm every setting
            setting(t, on)
            fn()
        for _ in range(rounds):
            for key, t, on in SETTINGS:
                setting(t, on)
                ms[key].append(round_ms(fn))
        m = {key: np.array(v) for key, v in ms.items()}
        print(f"{name:>20}, {what:>14}: " + "   ".join(f"{key} {v.mean():6.3f} ms [{v.min():.3f}, {v.max():.3f}]" for key, v in m.items())
              + f"   on / off = {m['on'].mean() / m['off'].mean():.3f}, on / cutoff 1 = {m['on'].mean() / m['cutoff 1'].mean():.3f}")
proc.close()
