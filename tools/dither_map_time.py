#!/usr/bin/env python3
"""KMG_MODE_DITHER device time (HIP events) on the tiled photograph of bench.py at 8192^2, with palettes of k = 8, 64 and 256 seeded
random colours, for the default choice and for the Bayer 8, Bayer 16 (as 16 x 16 and tiled to 64 x 64: the LDS table's width alone)
and blue-noise maps, on the scan route (KMG_STRATEGY_SCAN) and the list route (KMG_STRATEGY_TABLE): the pass alone
(kmg_apply_plan_run) and the plan's build with it (kmg_apply_plan_create + run).  Warm, the choices alternating inside every
repeat in one process, median and spread (min .. max) over the repeats, and the ratio of each map to the default of the same
route.

With --parent-lib PATH (a libkmeans_hip.so built from the parent commit) fresh child processes then time, parent library and this
one in turn (A B A B): the default choice on both routes and, on the scan route, Bayer 8, the blue-noise map and the replace pass
at the same k, and the dither pass of a 256 x 256 image at k = 256 (the reference's default call).  Per pass the medians of the
four turns, B's excess over A beside the difference of A's own two medians, and whether the SHA-256 of the outputs agree.  "This
one" is what KMG_LIBRARY names when the tool starts, else the tree's build.
    python tools/dither_map_time.py [repeats] [--parent-lib PATH]        (writes the table to stdout)"""
import hashlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python")); sys.path.insert(0, ROOT)
import numpy as np, torch
import kmeans_gpu_amd as kg
import bench

args = [a for a in sys.argv[1:]]
parent_lib = None
if "--parent-lib" in args:
    i = args.index("--parent-lib"); parent_lib = args[i + 1]; del args[i:i + 2]
child = "--child" in args                               # (the child processes: the passes below through whatever library KMG_LIBRARY names)
args = [a for a in args if a != "--child"]
reps = int(args[0]) if args else 7
SIDE = 8192
KS = [8, 64, 256]
ROUTES = ["scan", "table"]

proc = kg.ImageProcessor(shrink_max_dim=0)
st = torch.cuda.current_stream().cuda_stream
photo = bench.synthetic_image("photo", SIDE * SIDE, 0, 64, 0x5EED0B10)
out = torch.empty((SIDE * SIDE, 4), dtype=torch.uint8, device="cuda")


def centroids(k):
    """k seeded random sRGB colours (distinct with near certainty: pixels sampled from the photograph repeat each other, and a
    palette with equal entries spends the pass in its near-tie repair)"""
    pal = np.full((k, 4), 255, np.uint8)
    pal[:, :3] = np.random.default_rng(1000 + k).integers(0, 256, (k, 3))
    return kg.palette_to_centroids(pal)


def one_pass(cent, mode=kg.ReduceMode.Dither, side=SIDE):
    """(pass ms, build + pass ms) on the first side x side pixels"""
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    torch.cuda.synchronize()
    e0.record()
    plan = proc.apply_plan(cent, mode, side * side, st)
    e1.record()
    plan.run(photo.data_ptr(), side, side, 0, out.data_ptr(), st)
    e2.record()
    torch.cuda.synchronize()
    plan.close()
    return e1.elapsed_time(e2), e0.elapsed_time(e2)


def digest(side=SIDE):
    return hashlib.sha256(out[:side * side].cpu().numpy().tobytes()).hexdigest()


if child:
    # (route, k, what, mode, map, side): the default choice on both routes; on the scan route, where one kernel body serves them
    # all, also two maps, the replace pass, and the reference's default call (a 256 x 256 working image at k = 256)
    D, R = kg.ReduceMode.Dither, kg.ReduceMode.Replace
    cases = [(route, k, "", D, "bayer4", SIDE) for route in ROUTES for k in KS]
    cases += [("scan", k, what, mode, m, SIDE) for k in KS for what, mode, m in ((" bayer8", D, "bayer8"), (" blue64", D, "blue"), (" replace", R, "bayer4"))]
    cases += [("scan", 256, " 256^2", D, "bayer4", 256), ("scan", 256, " 256^2 blue64", D, "blue", 256)]
    res = {}
    for route, k, what, mode, m, side in cases:
        kg.set_strategy(route)
        proc.set_dither(m, 1.0)
        cent = centroids(k)
        t = [one_pass(cent, mode, side) for _ in range(reps + 1)][1:]
        res[f"{route} {k}{what}"] = {"ms": [a for a, _ in t], "total": [b for _, b in t], "sha256": digest(side)}
    print("CHILD " + json.dumps(res), flush=True)
    sys.exit(0)

# bayer16 as 16 x 16 and tiled to 64 x 64: the same offsets for every pixel, so the pair differs in the LDS table's width alone (the
# dword reads at stride four across the wave conflict four ways on a 64-wide table and not at all on a 16-wide one)
BAYER16 = kg.dither_map_values("bayer16")[0]
CHOICES = [("default", "bayer4"), ("bayer8", "bayer8"), ("bayer16", "bayer16"), ("b16 64w", np.tile(BAYER16, (4, 4))), ("blue64", "blue")]
print(f"# dither pass (HIP events), tiled photograph {SIDE}x{SIDE}, palettes of seeded random colours, {reps} warm repeats, choices alternating",
      flush=True)
print(f"{'route':>6s} {'k':>4s} {'map':>8s} {'pass ms':>9s} {'min':>8s} {'max':>8s} {'vs default':>10s} {'build+pass':>10s} {'min':>8s} {'max':>8s} {'vs default':>10s}",
      flush=True)
for route in ROUTES:
    kg.set_strategy(route)
    for k in KS:
        cent = centroids(k)
        times = {name: [] for name, _ in CHOICES}
        for r in range(reps + 1):
            for name, m in CHOICES:
                proc.set_dither(m, 1.0, levels=256 if isinstance(m, np.ndarray) else None)
                t = one_pass(cent)
                if r:
                    times[name].append(t)
        base = np.median(np.array(times["default"]), axis=0)
        for name, _ in CHOICES:
            t = np.array(times[name])
            med = np.median(t, axis=0)
            print(f"{route:>6s} {k:4d} {name:>8s} {med[0]:9.3f} {t[:, 0].min():8.3f} {t[:, 0].max():8.3f} {med[0] / base[0]:10.3f} "
                  f"{med[1]:10.3f} {t[:, 1].min():8.3f} {t[:, 1].max():8.3f} {med[1] / base[1]:10.3f}", flush=True)
proc.set_dither(0, 1.0)

if parent_lib:
    print(f"# fresh processes in turn: the parent commit's library (A) and this one (B), {reps} warm repeats each; medians in ms", flush=True)
    print("# excess: median of B's repeats over both turns - the same of A; A/A: |A's first median - A's second|; ok: excess <= A/A", flush=True)
    runs = []
    for tag, lib_path in (("A", parent_lib), ("B", None), ("A", parent_lib), ("B", None)):
        env = dict(os.environ)
        if lib_path:
            env["KMG_LIBRARY"] = os.path.abspath(lib_path)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(reps), "--child"], env=env, capture_output=True, text=True,
                           timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
        if r.returncode != 0 or not line:
            print(f"# child {tag} failed ({r.returncode}): {r.stderr[-400:]}", flush=True)
            sys.exit(1)
        runs.append(json.loads(line[0][6:]))
    print(f"{'route k pass':>24s} {'A':>9s} {'B':>9s} {'A':>9s} {'B':>9s} {'excess':>9s} {'A/A':>8s} {'ok':>4s}  outputs", flush=True)
    for key in runs[0]:
        med = [float(np.median(res[key]["ms"])) for res in runs]
        excess = float(np.median(runs[1][key]["ms"] + runs[3][key]["ms"]) - np.median(runs[0][key]["ms"] + runs[2][key]["ms"]))
        spread = abs(med[0] - med[2])
        same = len({res[key]["sha256"] for res in runs}) == 1
        print(f"{key:>24s} {med[0]:9.4f} {med[1]:9.4f} {med[2]:9.4f} {med[3]:9.4f} {excess:+9.4f} {spread:8.4f} {'yes' if excess <= spread else 'NO':>4s}  "
              f"{'identical' if same else 'DIFFER'}", flush=True)
