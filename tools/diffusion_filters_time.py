#!/usr/bin/env python3
"""KMG_MODE_DIFFUSE device time (HIP events) of kmg_apply_plan_run -- the diffusion pass alone -- for every filter of kmg_diffusion,
on the tiled photograph of bench.py at 8192^2 and at 256^2 (a clip's frame), k = 64: warm, the filters alternating inside every
repeat in one process, median and spread (min .. max) over the repeats, the step count W + SKEW (H - 1) of the filter's schedule
and the time per step.

With --parent-lib PATH (a libkmeans_hip.so built from the parent commit) Floyd-Steinberg is also timed in fresh child processes,
parent library and this one in turn (A B A B), and the SHA-256 of their outputs compared: its kernel is meant to be untouched.
    python tools/diffusion_filters_time.py [repeats] [--parent-lib PATH]        (writes the table to stdout)"""
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
fs_only = "--fs-only" in args                           # (the child processes: filter 0 through whatever library KMG_LIBRARY names)
args = [a for a in args if a != "--fs-only"]
reps = int(args[0]) if args else 7
SIZES = [8192, 256]
K = 64

proc = kg.ImageProcessor(shrink_max_dim=0)
st = torch.cuda.current_stream().cuda_stream
photo = bench.synthetic_image("photo", 8192 * 8192, 0, 64, 0x5EED0B10)
host = photo[: 1 << 20].cpu().numpy()
pal = host[np.arange(K, dtype=np.int64) * (host.shape[0] // K)].copy(); pal[:, 3] = 255
cent = kg.palette_to_centroids(pal)
out = torch.empty((8192 * 8192, 4), dtype=torch.uint8, device="cuda")


def one_pass(side):
    e1, e2 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    plan = proc.apply_plan(cent, kg.ReduceMode.Diffuse, side * side, st)
    torch.cuda.synchronize()                            # (the tables are built: the pass alone is timed)
    e1.record()
    plan.run(photo.data_ptr(), side, side, 0, out.data_ptr(), st)
    e2.record()
    torch.cuda.synchronize()
    plan.status()
    plan.close()
    return e1.elapsed_time(e2)


def digest(side):
    return hashlib.sha256(out[: side * side].cpu().numpy().tobytes()).hexdigest()


if fs_only:
    res = {}
    for side in SIZES:
        t = [one_pass(side) for _ in range(reps + 1)][1:]
        res[str(side)] = {"ms": t, "sha256": digest(side)}
    print("FS " + json.dumps(res), flush=True)
    sys.exit(0)

names = sorted(kg.DIFFUSION_NAMES, key=kg.DIFFUSION_NAMES.get)
print(f"# diffusion pass alone (kmg_apply_plan_run, HIP events), tiled photograph, k = {K}, {reps} warm repeats, filters alternating", flush=True)
print(f"{'shape':>10s} {'filter':>16s} {'skew':>4s} {'steps':>7s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'us/step':>8s} {'vs FS':>6s}", flush=True)
for side in SIZES:
    times = {f: [] for f in range(len(names))}
    for r in range(reps + 1):
        for f in range(len(names)):
            proc.set_diffusion(f)
            t = one_pass(side)
            if r:
                times[f].append(t)
    fs = float(np.median(times[0]))
    for f, name in enumerate(names):
        w, _ = kg.diffusion_weights(f)
        skew = 3 if (w[2] or w[7]) else 2
        steps = side + skew * (side - 1)
        t = np.array(times[f])
        med = float(np.median(t))
        print(f"{side:>4d}x{side:<5d} {name:>16s} {skew:4d} {steps:7d} {med:10.3f} {t.min():9.3f} {t.max():9.3f} {med * 1e3 / steps:8.3f} "
              f"{med / fs:6.2f}", flush=True)
proc.set_diffusion(0)

if parent_lib:
    print(f"# Floyd-Steinberg, fresh processes in turn: the parent commit's library (A) and this one (B), {reps} warm repeats each", flush=True)
    runs = []
    for tag, lib_path in (("A", parent_lib), ("B", None), ("A", parent_lib), ("B", None)):
        env = dict(os.environ)
        if lib_path:
            env["KMG_LIBRARY"] = os.path.abspath(lib_path)
        else:
            env.pop("KMG_LIBRARY", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(reps), "--fs-only"], env=env, capture_output=True, text=True,
                           timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("FS ")]
        if r.returncode != 0 or not line:
            print(f"# child {tag} failed ({r.returncode}): {r.stderr[-400:]}", flush=True)
            sys.exit(1)
        runs.append((tag, json.loads(line[0][3:])))
    for side in SIZES:
        for tag, res in runs:
            t = np.array(res[str(side)]["ms"])
            print(f"{side:>4d}x{side:<5d} {tag} median {np.median(t):9.3f} ms  min {t.min():9.3f}  max {t.max():9.3f}", flush=True)
        same = len({res[str(side)]["sha256"] for _, res in runs}) == 1
        print(f"{side:>4d}x{side:<5d} outputs of A and B {'identical' if same else 'DIFFER'}", flush=True)
