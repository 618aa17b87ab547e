#!/usr/bin/env python3
"""Random sessions on ONE long-lived processor against the stateless model (tests/session_harness.py): the sticky switches (alpha
cutoff, fixed colours, strategy), host calls, output passes and plans, error records combined over bands, caller-owned delta
canvases, two Lloyd objects with seeds and n_fixed, two Sequence objects with their outputs -- all closed and re-created in each
other's blocks, every result compared byte for byte after every call, every refused call with the status include/kmeans_hip.h
names.  Surface 2 adds outputs with per-frame palettes (cold and warm), colour-keyed canvases of the caller's and the index-map
optimisation (usage records, plans, remaps, kmg_index_optimize) to the same objects, switches and blocks.  Surface 3 adds alpha
weighting: kmg_processor_set_weighting turned on and off between all of those calls, kmg_lloyd_set_weighting on the two Lloyd
objects, with the bindings of the initialisation and of the caller around it, and the refusals of both.  Surface 4 adds the batched
calls -- kmg_palette_batch, kmg_reduce_batch, kmg_reduce_indexed_batch, kmg_find_batch, kmg_dev_palette_batch, kmg_dev_apply_batch
-- with lists of 1 to 9 images, three classes of max_resident_bytes, their reports and their refusals.  A mismatch prints the op
list (replay() of the harness runs it) and ends the run: nothing more is started on the device.
usage: fuzz_session.py [sequences] [seed] [surface]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmeans-gpu_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import session_harness as H

sequences = int(sys.argv[1]) if len(sys.argv) > 1 else 6
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 201
surface = int(sys.argv[3]) if len(sys.argv) > 3 else 1
extra = {} if surface == 1 else {"surface": surface}     # (surface 1 is the call as it always was)
env = H.KgEnv()
ops_total, t0 = 0, time.time()
for seq in range(sequences):
    try:
        n_ops, allocated, reused = H.run_sequence(env, seed, seq, **extra)
    except H.Mismatch as e:
        print(f"MISMATCH {e}", flush=True)
        print(f"{seq + 1} sequences, {ops_total} ops, 1 mismatching")
        sys.exit(1)
    ops_total += n_ops
    print(f"sequence {seq}: {n_ops} ops, {allocated} blocks allocated, {reused} blocks re-used", flush=True)
print(f"{time.time() - t0:.1f} s")
print(f"{sequences} sequences, {ops_total} ops, 0 mismatching")
