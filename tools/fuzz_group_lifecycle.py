#!/usr/bin/env python3
"""Random call sequences on the multi-device layer against the oracle (tests/group_harness.py): per world ONE group that stays alive
across the sequences -- one rank with every RCCL collective forced, one rank without collectives, two, three and five ranks sharing
device 0 through the loopback exchange -- group Lloyd objects bound again and again with random bands (uneven, without rows, in any
owner order, with and without label maps) and flags, batches, the host calls and single-device passes on the member processors in
between.  Every label map, every rank's centroid table, every iteration count and every host output is compared bit for bit with
the stateless model, every refused call with the status include/kmeans_hip.h names.  A mismatch prints the op list (replay() of the
harness runs it) and ends the run: nothing more is started on the device.
usage: fuzz_group_lifecycle.py [sequences] [seed]   |   fuzz_group_lifecycle.py scenarios"""
import os, sys, time
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import group_harness as G

env = G.KgGroupEnv()
if len(sys.argv) > 1 and sys.argv[1] == "scenarios":
    jobs = [(name, G.SCENARIO_SEED, 0, ops) for name, ops in G.scenarios().items()]
else:
    sequences = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 201
    jobs = [(f"sequence {seq}", seed, seq, None) for seq in range(sequences)]
ops_total, t0 = 0, time.time()
for i, (name, seed, seq, ops) in enumerate(jobs):
    t1 = time.time()
    try:
        n_ops, allocated, reused = G.run_sequence(env, seed, seq, ops)
    except G.Mismatch as e:
        print(f"MISMATCH {name}: {e}", flush=True)
        print(f"{i + 1} sequences, {ops_total} ops, 1 mismatching")
        sys.exit(1)                                   # (without closing the groups: nothing more runs on the device)
    ops_total += n_ops
    print(f"{name}: {n_ops} ops, {allocated} blocks allocated, {reused} blocks re-used, {time.time() - t1:.1f} s", flush=True)
env.close()
print(f"{time.time() - t0:.1f} s")
print(f"{len(jobs)} sequences, {ops_total} ops, 0 mismatching")
