"""Long-lived processors and Lloyd objects on the device (tests/lifecycle_harness.py): the random sequences of
tools/fuzz_lifecycle.py on the seeds tests/test_lifecycle_model.py vouches for, and the scenarios that are too rare for a
generator -- each an op list of the harness, run against its oracle model on ONE processor that stays alive across all of them
(so every scenario works in the blocks the ones before it left).  Everything is compared bit for bit after every op."""
import os
import re
import subprocess
import sys

import pytest

import lifecycle_harness as H
from test_lifecycle_model import SEEDS, SEQUENCES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SEQ = 7, 0                      # the images of the scenarios: H.make_images(SEED, SEQ)
MEGA, NOISE, BLOBS, TOKYO = (H.IMAGE_KINDS.index(k) for k in ("mega", "noise", "blobs", "tokyo"))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sequences_equal_the_model(seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_lifecycle.py"), str(SEQUENCES), str(seed)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert re.search(rf"^{SEQUENCES} sequences, \d+ ops, 0 mismatching$", r.stdout, re.M), r.stdout[-2000:]
    reused = [int(x) for x in re.findall(r"(\d+) blocks re-used", r.stdout)]
    assert len(reused) == SEQUENCES and sum(reused) > 0 and all(x > 0 for x in reused), reused     # else nothing ran on recycled memory


def _n(i):
    h, w = H.make_images(SEED, SEQ)[i][1].shape[:2]
    return w * h


@pytest.fixture(scope="module")
def world(torch_cuda):
    env = H.KgEnv()
    proc = env.processor()
    yield env, proc
    proc.close()


def _run(world, ops):
    env, proc = world
    done = H.run_sequence(env, SEED, SEQ, ops, proc=proc)[0]
    assert done == len(ops)
    proc.set_strategy(0)


def test_k8_k300_k8_alternate_on_one_buffer(world):
    n = _n(BLOBS)
    ops = [("upload", 1, BLOBS), ("strategy", 2), ("create", 0, 8)]
    for i, k in enumerate((8, 300, 8, 300, 8)):
        if i:
            ops.append(("recreate", 0, k))
        ops += [("set_cent", 0, "rand", i, 0), ("bind", 0, 1, 0, n, 0), ("labels", 0, 1, 0, n, 0), ("assign", 0, 1, 0, n, 1, 1, 0),
                ("iterate", 0, 1, 0, n, 1, 2, 1, 1, 1), ("lft", 0, 5, n - 5, 0)]
    _run(world, ops + [("close", 0)])


@pytest.mark.parametrize("strategy", [1, 2])
def test_a_megapixel_then_100_pixels_then_the_megapixel_on_one_object(world, strategy):
    """1024 x 1024 is where the per-pixel scan takes four pixels per thread on 1024 partial rows (reduction and update in launches of
    their own) and kmg_lloyd_run its general loop; 100 pixels take one partial row and the one-launch loop, which keeps its sums and
    its second centroid table in the partial rows -- alternately on one warm object, per-pixel scan and colour table"""
    n = _n(MEGA)
    assert n == 1 << 20
    ops = [("upload", 0, MEGA), ("strategy", strategy), ("create", 0, 24), ("set_cent", 0, "init", 1, TOKYO)]
    for m in (n, 100, n):
        ops += [("prepare", 0, 0, 0, m, 1, 0), ("assign", 0, 0, 0, m, 1, 1, 0), ("partials", 0, 0, 0, m, 1, 1),
                ("assign_update", 0, 0, 0, m, 1, 1, 0), ("labels", 0, 0, 0, m, 1), ("run", 0, 0, 0, m, 1, 0),
                ("iterate", 0, 0, 0, m, 1, 2, 1, 1, 0)]
    _run(world, ops + [("close", 0)])


def test_every_refusal_is_followed_by_a_correct_pass(world):
    n = _n(NOISE)
    ops = [("upload", 1, NOISE), ("strategy", 2), ("create", 0, 40), ("set_cent", 0, "rand", 3, 0), ("create", 1, 300),
           ("set_cent", 1, "rand", 4, 0), ("bind", 1, 1, 0, n, 0), ("refuse", 1, "lftu_bigk", 0), ("assign", 1, 1, 0, n, 1, 1, 0)]
    for what in ("unbound_lft", "unbound_into", "unbound_share", "unbound_rebuild", "share_bad"):
        ops += [("refuse", 0, what, 1), ("assign", 0, 1, 0, n, 1, 1, 0)]
    ops += [("bind", 0, 1, 0, n, 0), ("share_round", 0, 2, 0, 0, n, 1, 0)]
    for what in ("run", "iterate", "assign_update", "labelmap", "partials"):
        ops += [("refuse", 0, what, 0), ("share_round", 0, 1, 0, 0, n, 0, 0), ("assign", 0, 1, 0, n, 1, 1, 0), ("share_round", 0, 3, 0, 7, n - 7, 1, 1)]
    _run(world, ops + [("close", 0), ("close", 1)])


@pytest.mark.parametrize("k", [24, 256])
def test_fused_cell_share_pair_through_the_binding(world, k):
    n = _n(TOKYO)
    ops = [("upload", 2, TOKYO), ("strategy", 2), ("create", 0, k), ("set_cent", 0, "init", 1, TOKYO), ("bind", 0, 2, 0, n, 0)]
    for parts in (1, 2, 4, 2, 1):
        ops += [("share_round", 0, parts, 1, 0, n, 0, 0), ("get", 0, 0), ("conv", 0, 0), ("share_round", 0, parts, 0, 11, n - 11, 0, 1)]
    _run(world, ops + [("close", 0)])


def test_iterate_set_centroids_iterate_flush(world):
    n = _n(BLOBS)
    ops = [("upload", 1, BLOBS), ("strategy", 2), ("create", 0, 64), ("set_cent", 0, "init", 1, BLOBS), ("bind", 0, 1, 0, n, 0),
           ("assign", 0, 1, 0, n, 0, 1, 0), ("iterate", 0, 1, 0, n, 1, 5, 1, 0, 0), ("set_cent", 0, "rand", 9, 0), ("labels", 0, 1, 0, n, 0),
           ("iterate", 0, 1, 0, n, 1, 2, 1, 1, 1), ("get", 0, 0), ("close", 0)]
    _run(world, ops)


def test_an_output_pass_of_each_mode_between_two_passes_of_a_bound_object(world):
    n = _n(TOKYO)
    ops = [("upload", 2, TOKYO), ("strategy", 2), ("create", 0, 100), ("set_cent", 0, "init", 1, TOKYO), ("bind", 0, 2, 0, n, 0)]
    for mode in range(4):
        for fmt in (None, 2) if mode != 2 else (None,):
            ops += [("assign_update", 0, 2, 0, n, 1, 1, 0), ("apply", 2, mode, fmt, 60 + mode, 5, mode & 1, 0), ("labels", 0, 2, 0, n, 1),
                    ("assign", 0, 2, 0, n, 1, 1, 0)]
    _run(world, ops + [("host", "reduce", 6, 5, 1, 1), ("assign", 0, 2, 0, n, 1, 1, 0), ("close", 0)])


def test_strategy_switched_between_prepare_and_the_pass(world):
    n = _n(NOISE)
    ops = [("upload", 1, NOISE), ("create", 0, 16), ("set_cent", 0, "rand", 2, 0)]
    for a, b in ((2, 1), (1, 2), (2, 0), (0, 6), (6, 1)):
        ops += [("strategy", a), ("prepare", 0, 1, 0, n, 1, 0), ("strategy", b), ("assign", 0, 1, 0, n, 1, 1, 1), ("update", 0, 0),
                ("labels", 0, 1, 0, n, 0), ("run", 0, 1, 0, n, 1, 0)]
    _run(world, ops + [("close", 0)])


def test_next_frame_after_an_initialisation_that_bound_the_buffer(world):
    """init_centroids over the colour table binds the buffer; the next frame arrives in the same buffer (same size) and the caller
    sets centroids and runs: kmg_lloyd_run works from the buffer's CURRENT contents, not from the initialisation's histogram"""
    n = _n(BLOBS)
    ops = [("upload", 1, BLOBS), ("strategy", 2), ("create", 0, 9), ("init", 0, 1, 0), ("upload", 1, BLOBS + H.NI),
           ("set_cent", 0, "init", 1, BLOBS), ("run", 0, 1, 0, n, 1, 0), ("assign", 0, 1, 0, n, 1, 1, 0), ("close", 0)]
    _run(world, ops)


def test_initialisation_with_one_centroid_drops_the_binding_of_its_buffer(world):
    """kmg_lloyd_init_centroids starts a new problem for every k, k = 1 included: an earlier binding of the buffer is dropped"""
    n = _n(BLOBS)
    ops = [("upload", 1, BLOBS), ("strategy", 2), ("create", 0, 1), ("set_cent", 0, "rand", 1, 0), ("bind", 0, 1, 0, n, 0),
           ("assign", 0, 1, 0, n, 1, 1, 0), ("upload", 1, BLOBS + H.NI), ("init", 0, 1, 0), ("assign", 0, 1, 0, n, 1, 1, 0),
           ("refuse", 0, "unbound_lft", 0), ("close", 0)]
    _run(world, ops)


def test_the_next_call_meets_an_iterate_still_in_flight(world):
    """kmg_lloyd_iterate leaves its label pass on the library's side stream; no flush, no device synchronisation, nothing read back
    (flush = 2 of the harness), then at once on the same stream: set_centroids, update, get_centroids, a re-creation in the same
    blocks, close.  The label map it owed is complete and right after the next call's synchronisation"""
    n = _n(BLOBS)
    ops = [("upload", 1, BLOBS), ("strategy", 2), ("create", 0, 64), ("set_cent", 0, "init", 1, BLOBS), ("bind", 0, 1, 0, n, 0),
           ("assign", 0, 1, 0, n, 0, 1, 0)]
    it = ("iterate", 0, 1, 0, n, 1, 3, 1, 2, 0)
    ops += [it, ("set_cent", 0, "rand", 9, 0), ("labels", 0, 1, 0, n, 0), ("assign", 0, 1, 0, n, 1, 1, 0),
            it, ("update", 0, 0), ("labels", 0, 1, 0, n, 0), ("assign", 0, 1, 0, n, 1, 1, 0),
            it, ("get", 0, 0), it, ("recreate", 0, 300), ("set_cent", 0, "rand", 4, 0), ("bind", 0, 1, 0, n, 0), ("labels", 0, 1, 0, n, 0),
            ("assign", 0, 1, 0, n, 1, 1, 0), it, ("close", 0)]
    _run(world, ops)
