"""Long-lived sessions on the device (tests/session_harness.py): the random sessions of tools/fuzz_session.py on the seeds
tests/test_session_model.py vouches for, and named scenarios -- each an op list of the harness, run against its stateless model on
ONE processor that stays alive across all of them (so every scenario works in the blocks the ones before it left): the eight of the
first surface, then the directed passages of surface 2 (local outputs, colour-keyed canvases, the index-map optimisation), then
the seven of surface 3 (alpha weighting turned on and off between the other calls of that processor and of its Lloyd objects), then
the seven of surface 4 (the batched calls, each in the blocks that larger batches, refused batches and other objects gave back).
Everything an op could have touched is compared byte for byte after every op."""
import os
import re
import subprocess
import sys

import pytest

import session_harness as H
from test_session_model import SEEDS, SEEDS_2, SEEDS_3, SEEDS_4, SEQUENCES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SEQ = 7, 0                      # the images of the scenarios: H.make_images(SEED, SEQ)
ODD, ODD_B, SPRITE, NOISY, SHIFT, FEW, FLAT, CLEAR, BIG, MEGA, ROW, COL, MAP = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14
ROW_B, COL_B = 11, 13
# A seed's run took 7.5 and 7.8 s on an MI355X, process start included (profiles/NOTES.md, "Session harness"); about two thirds of
# that is the reference on the host's CPUs.  The limit is forty times the measured time: a host with a quarter of the cores, busy
# with other work, can slow the reference tenfold and still finish; a run that needs longer than that hangs.
SESSION_SECONDS = 7.8
TIMEOUT = 40 * SESSION_SECONDS


# The seeds of surface 2 (per-frame palettes, colour-keyed canvases, index-map optimisation) took 5.2 and 4.8 s in the visit in which
# a seed-201 run took 7.7 s (profiles/NOTES.md): the same rule, forty times the slower of the two.
SESSION_2_SECONDS = 5.2
TIMEOUT_2 = 40 * SESSION_2_SECONDS


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sessions_equal_the_model(seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_session.py"), str(SEQUENCES), str(seed)],
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert re.search(rf"^{SEQUENCES} sequences, \d+ ops, 0 mismatching$", r.stdout, re.M), r.stdout[-2000:]
    reused = [int(x) for x in re.findall(r"(\d+) blocks re-used", r.stdout)]
    assert len(reused) == SEQUENCES and all(x > 0 for x in reused), reused     # else nothing ran on recycled memory


@pytest.mark.parametrize("seed", SEEDS_2)
def test_random_sessions_of_surface_2_equal_the_model(seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_session.py"), str(SEQUENCES), str(seed), "2"],
                       capture_output=True, text=True, timeout=TIMEOUT_2)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert re.search(rf"^{SEQUENCES} sequences, \d+ ops, 0 mismatching$", r.stdout, re.M), r.stdout[-2000:]
    reused = [int(x) for x in re.findall(r"(\d+) blocks re-used", r.stdout)]
    assert len(reused) == SEQUENCES and all(x > 0 for x in reused), reused     # else nothing ran on recycled memory


# The seeds of surface 3 (alpha weighting) took 5.5 and 5.5 s in the visit in which a seed-314 run took 5.3 s (profiles/NOTES.md):
# the same rule, forty times the slower of the two.
SESSION_3_SECONDS = 5.5
TIMEOUT_3 = 40 * SESSION_3_SECONDS


@pytest.mark.parametrize("seed", SEEDS_3)
def test_random_sessions_of_surface_3_equal_the_model(seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_session.py"), str(SEQUENCES), str(seed), "3"],
                       capture_output=True, text=True, timeout=TIMEOUT_3)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert re.search(rf"^{SEQUENCES} sequences, \d+ ops, 0 mismatching$", r.stdout, re.M), r.stdout[-2000:]
    reused = [int(x) for x in re.findall(r"(\d+) blocks re-used", r.stdout)]
    assert len(reused) == SEQUENCES and all(x > 0 for x in reused), reused     # else nothing ran on recycled memory


# The seeds of surface 4 (the batched calls) took 6.7 and 6.3 s in the visit in which a seed-421 run took 5.6 s (profiles/NOTES.md):
# the same rule, forty times the slower of the two.
SESSION_4_SECONDS = 6.7
TIMEOUT_4 = 40 * SESSION_4_SECONDS


@pytest.mark.parametrize("seed", SEEDS_4)
def test_random_sessions_of_surface_4_equal_the_model(seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_session.py"), str(SEQUENCES), str(seed), "4"],
                       capture_output=True, text=True, timeout=TIMEOUT_4)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert re.search(rf"^{SEQUENCES} sequences, \d+ ops, 0 mismatching$", r.stdout, re.M), r.stdout[-2000:]
    reused = [int(x) for x in re.findall(r"(\d+) blocks re-used", r.stdout)]
    assert len(reused) == SEQUENCES and all(x > 0 for x in reused), reused     # else no batch ran in a recycled block


@pytest.fixture(scope="module")
def world(torch_cuda):
    env = H.KgEnv()
    proc = env.session_processor()
    yield env, proc
    proc.close()


def _run(world, ops):
    env, proc = world
    done = H.run_sequence(env, SEED, SEQ, ops, proc=proc)[0]
    assert done == len(ops)


def _order(h, nb, want):
    """an order seed for which session_harness.bands_of runs the bands of h rows from the last to the first (want = "reverse")"""
    for s in range(1000):
        rows = [r0 for r0, _ in H.bands_of(h, nb, s)]
        if len(rows) == nb and rows == sorted(rows, reverse=True):
            return s
    raise AssertionError(want)


def _cutoff_0_128_0_around_palette_reduce_and_a_plan():
    """the results at cutoff 0 before and after the passage at 128 are those of the default path, and the plan made at 128 still
    writes index k for the pixels below it after the switch back"""
    at = [("palette", ODD, 8), ("reduce_indexed", ODD, 8, 0, 1), ("reduce_indexed", SPRITE, 40, 3, 1), ("reduce", ODD, 8, 1)]
    return ([("strategy", 0), ("cutoff", 0)] + at + [("cutoff", 128)] + at +
         [("apply_plan", ODD, 0, 1, 40, 11, 0, 0), ("apply_plan", SPRITE, 3, 2, 300, 12, 128, 1), ("apply_plan", ODD, 1, None, 9, 13, 0, 0)] + at)


def _frames_added_under_three_cutoffs_then_clear():
    frames = [(SPRITE, 0), (ODD, 128), (SHIFT, 0)]
    ops = [("s_new", 0)]
    for i, t in frames:
        ops += [("cutoff", t), ("s_add", 0, i, int(i == ODD), 1)]
    ops += [("s_info", 0), ("s_palette", 0, 12), ("s_centroids", 0, 12), ("cutoff", 255), ("s_centroids", 0, 5), ("s_clear", 0), ("s_info", 0),
            ("cutoff", 128)]
    ops += [("s_add", 0, i, 0, 0) for i, _ in frames]
    return (ops + [("s_info", 0), ("s_palette", 0, 12), ("s_centroids", 0, 12), ("cutoff", 0), ("s_close", 0)])


def _an_output_ends_a_lloyd_object_runs_in_its_block_and_the_next_output_starts_fresh():
    """INDEX8 k = 40, exact / lossy / lossy / exact, end; a Lloyd object created, run and closed in the returned block; INDEX16
    k = 300 at another size: its first delta is the delta against a canvas of k, that is the full map"""
    return ([("cutoff", 1), ("s_new", 0), ("s_add", 0, SPRITE, 0, 0), ("s_add", 0, ODD, 1, 0), ("s_output", 0, 40, 0, 1, 1),
                 ("s_frame", 0, SPRITE, 1, None), ("s_frame", 0, NOISY, 1, 40), ("s_frame", 0, SHIFT, 1, 4096), ("s_frame", 0, SPRITE, 1, None),
                 ("s_end", 0), ("l_new", 0, 24), ("l_set", 0, "rand", 3, ODD), ("l_run", 0, FEW, 1, 0), ("l_close", 0),
                 ("s_output", 0, 300, 0, 2, 0), ("s_frame", 0, ODD, 1, None), ("s_frame", 0, ODD_B, 1, 40), ("s_output", 0, 40, 3, 1, 1),
                 ("s_frame", 0, NOISY, 1, 40), ("s_close", 0), ("cutoff", 0)])


def _frozen_seeds_do_not_outlive_their_object():
    return ([("strategy", 2), ("l_new", 0, 12), ("l_init", 0, FEW, 3, 0), ("l_fix", 0, 3), ("l_run", 0, FEW, 1, 0), ("l_re", 0, 30),
                 ("l_init", 0, ROW, 0, 1), ("l_run", 0, ROW, 1, 1), ("l_assign_update", 0, ODD, 1, 1, 0), ("l_conv", 0, 0), ("l_fix", 0, 2),
                 ("l_iterate", 0, ODD, 2, 0), ("l_conv", 0, 0), ("l_lftu", 0, SPRITE, 1), ("l_fix", 0, 0), ("l_assign_update", 0, ODD, 0, 1, 0),
                 ("l_update", 0, 1), ("l_conv", 0, 1), ("l_close", 0), ("strategy", 0)])


def _quality_search_with_and_without_pins_beside_a_bound_object():
    """the second search equals the unpinned model; the user's Lloyd object stays bound across both, and its next assign is right"""
    q = ("quality", FEW, 4.0, 8, 14, 0, 1, 1)
    return ([("strategy", 2), ("l_new", 1, 9), ("l_set", 1, "rand", 5, ODD), ("l_bind", 1, ODD, 0), ("l_assign", 1, ODD, 0), ("fixed", 3), q,
                 ("l_assign", 1, ODD, 1), ("fixed", 0), q, ("quality", SPRITE, 9.0, 2, 12, 3, 0, 0), ("l_assign_update", 1, ODD, 1, 1, 0),
                 ("l_close", 1), ("strategy", 0)])


def _records_combine_over_bands_in_reverse_on_two_streams():
    h_odd, h_sprite = 61, 72
    return ([("cutoff", 128),
                 ("compare_device", ODD, 0, 1, 40, 21, 3, _order(h_odd, 3, "reverse"), 128, 3, 1, 0),
                 ("compare_device", SPRITE, 0, 2, 300, 22, 2, _order(h_sprite, 2, "reverse"), 0, 3, 0, 1),      # into the same record
                 ("compare_device", FEW, 0, None, 9, 23, 3, 5, 0, 1, 1, 0),                                      # a fresh one
                 ("compare_device", ODD, 0, None, 9, 23, 2, 6, 128, 2, 0, 1),
                 ("pair_open", 0, 1, 1, 40, 24, 0), ("pair_frame", 0, SPRITE, None, 3, _order(h_sprite, 3, "reverse"), 0),
                 ("pair_frame", 0, NOISY, 40, 3, _order(h_sprite, 3, "reverse"), 1), ("pair_frame", 0, SHIFT, 4096, 2, 3, 0),
                 ("pair_frame", 0, SPRITE, 0, 3, 4, 1), ("pair_frame", 0, NOISY, None, 1, 0, 0), ("pair_frame", 0, SPRITE, 400000, 2, 9, 0),
                 ("pair_open", 1, 0, 2, 300, 25, 1), ("pair_frame", 1, ODD, 40, 3, _order(h_odd, 3, "reverse"), 0),
                 ("pair_frame", 1, ODD_B, 40, 2, 1, 1), ("cutoff", 0)])


def _every_refusal_is_followed_by_the_correct_call():
    return ([("cutoff", 0), ("fixed", 3), ("refuse", "k_below_fixed_palette", SPRITE, 7), ("palette", SPRITE, 9),
                 ("refuse", "k_below_fixed_reduce", SPRITE, 3), ("reduce", SPRITE, 10, 0), ("refuse", "octree_fixed", SPRITE, 12),
                 ("palette", SPRITE, 12), ("s_new", 0), ("s_add", 0, FEW, 0, 0), ("refuse", "k_below_fixed_sequence", 0, 7), ("s_palette", 0, 9),
                 ("fixed", 0), ("refuse", "frame_no_output", 0, SPRITE), ("s_output", 0, 5, 0, 0, 1), ("refuse", "delta_on_rgba8", 0, NOISY),
                 ("refuse", "lossy_on_rgba8", 0, NOISY), ("s_frame", 0, NOISY, 0, None), ("s_output", 0, 5, 1, 1, 1),
                 ("refuse", "lossy_without_delta", 0, NOISY), ("s_frame", 0, NOISY, 1, 40), ("s_end", 0), ("refuse", "frame_no_output", 0, SPRITE),
                 ("refuse", "index8_full", ODD, 257), ("apply", ODD, 0, 1, 256, 31, 0), ("cutoff", 128), ("refuse", "index8_full", ODD, 256),
                 ("apply", ODD, 0, 1, 255, 32, 1), ("refuse", "meld_indexed", FLAT, 5), ("apply", FLAT, 2, None, 5, 33, 0), ("s_clear", 0),
                 ("s_add", 0, CLEAR, 0, 0), ("s_info", 0), ("refuse", "empty_sequence", 0, 4), ("s_add", 0, FLAT, 1, 0), ("s_palette", 0, 4),
                 ("s_close", 0), ("cutoff", 0)])


def _two_sequences_alternate_beside_host_calls_on_the_megapixel_image():
    """forced colour table on 1024 x 1024: large blocks enter the idle list and the next output picks them up"""
    return ([("strategy", 2), ("s_new", 0), ("s_new", 1), ("s_add", 0, SPRITE, 0, 0), ("s_add", 1, ODD, 1, 1), ("s_add", 1, BIG, 0, 0),
                 ("s_output", 0, 16, 0, 1, 1), ("s_output", 1, 20, 1, 2, 0), ("s_frame", 0, SPRITE, 1, None), ("reduce", MEGA, 8, 0),
                 ("s_frame", 1, ODD, 1, None), ("s_frame", 0, NOISY, 1, 40), ("reduce_indexed", MEGA, 6, 1, 1), ("s_frame", 1, ODD_B, 1, 40),
                 ("compare_device", MEGA, 0, 1, 12, 41, 3, 2, 0, 3, 1, 0), ("s_end", 0), ("s_output", 0, 30, 0, 2, 1), ("s_frame", 0, SHIFT, 1, None),
                 ("s_frame", 1, ODD, 0, None), ("s_frame", 0, SPRITE, 1, 4096), ("s_close", 0), ("s_close", 1), ("strategy", 0)])


def _a_warm_output_across_a_cutoff_switch_and_back():
    """each warm frame runs on the working image of the cutoff read at its own call, from the centroids of the frame before"""
    return [("cutoff", 0), ("fixed", 0), ("s_new", 0), ("s_output_local", 0, 12, 1, 1, 1, 1), ("s_frame_local", 0, SPRITE, 1, None),
            ("s_frame_local", 0, NOISY, 1, 40), ("cutoff", 128), ("s_frame_local", 0, SHIFT, 1, None), ("cutoff", 0),
            ("s_frame_local", 0, SPRITE, 1, 4096), ("s_frame_local", 0, NOISY, 0, None), ("s_close", 0)]


def _a_refused_frame_leaves_a_warm_output_warm_and_a_failed_palette_step_makes_it_cold():
    """frame / refused frame / frame: status -5 for fixed colours on a warm output, -1 for k below the fixed colours, and the
    frame without a kept pixel, after which the next frame is cold"""
    return [("cutoff", 0), ("fixed", 0), ("s_new", 0), ("s_output_local", 0, 9, 0, 1, 1, 1), ("s_frame_local", 0, SPRITE, 1, None), ("fixed", 2),
            ("s_frame_local", 0, NOISY, 1, None), ("fixed", 0), ("s_frame_local", 0, NOISY, 1, None), ("fixed", 1),
            ("refuse", "warm_with_fixed", 0, SHIFT), ("fixed", 0), ("s_frame_local", 0, SHIFT, 1, 40),
            ("s_output_local", 0, 2, 0, 1, 0, 0), ("s_frame_local", 0, ODD, 1, None), ("fixed", 3), ("s_frame_local", 0, ODD_B, 1, None), ("fixed", 0),
            ("s_frame_local", 0, ODD_B, 1, 40),
            ("s_output_local", 0, 3, 0, 1, 4, 1), ("s_frame_local", 0, CLEAR, 1, None), ("cutoff", 128), ("s_frame_local", 0, CLEAR, 1, None),
            ("cutoff", 0), ("s_frame_local", 0, CLEAR, 1, None), ("s_close", 0)]


def _a_local_output_begins_in_a_used_block_with_a_lossy_first_frame():
    """a shared output ended, a Lloyd object run and closed, then begin_local with a smaller k in the block that came back: shown is
    filled, the held source is not and the lossy first frame must not read it; a second begin_local starts from nothing again"""
    return [("cutoff", 1), ("s_new", 0), ("s_add", 0, SPRITE, 0, 0), ("s_output", 0, 40, 0, 1, 1), ("s_frame", 0, SPRITE, 1, None),
            ("s_frame", 0, NOISY, 1, 40), ("s_end", 0), ("l_new", 0, 24), ("l_set", 0, "rand", 3, ODD), ("l_run", 0, FEW, 1, 0), ("l_close", 0),
            ("s_output_local", 0, 7, 1, 1, 1, 0), ("s_frame_local", 0, SPRITE, 1, 40), ("s_frame_local", 0, NOISY, 1, 4096),
            ("s_frame_local", 0, SHIFT, 1, None), ("s_output_local", 0, 7, 1, 1, 1, 1), ("s_frame_local", 0, NOISY, 1, 40),
            ("s_frame_local", 0, SPRITE, 1, None), ("s_close", 0), ("cutoff", 0)]


def _a_lossy_frame_comes_back_in_full_then_an_exact_and_a_lossy_frame():
    return [("cutoff", 128), ("s_new", 1), ("s_output_local", 1, 16, 0, 2, 1, 0), ("s_frame_local", 1, SPRITE, 1, None),
            ("s_frame_local", 1, SHIFT, 1, 4096), ("s_frame_local", 1, NOISY, 1, None), ("s_frame_local", 1, SPRITE, 1, 4096),
            ("s_frame_local", 1, SHIFT, 1, 400000), ("s_frame_local", 1, NOISY, 1, 40), ("s_close", 1), ("cutoff", 0)]


def _local_shared_local_on_one_sequence_with_the_refusals_between():
    return [("cutoff", 0), ("s_new", 0), ("s_add", 0, SPRITE, 0, 0), ("s_output_local", 0, 8, 0, 1, 1, 0), ("s_frame_local", 0, SPRITE, 1, None),
            ("refuse", "shared_frame_on_local", 0, NOISY), ("s_frame_local", 0, NOISY, 1, None), ("s_output", 0, 8, 0, 1, 1),
            ("s_frame", 0, SPRITE, 1, None), ("refuse", "local_frame_on_shared", 0, NOISY), ("s_frame", 0, NOISY, 1, 40),
            ("s_output_local", 0, 8, 1, 2, 1, 1), ("s_frame_local", 0, SHIFT, 1, None), ("s_frame_local", 0, NOISY, 1, 40), ("s_end", 0),
            ("refuse", "local_frame_no_output", 0, ODD), ("refuse", "local_meld", 0, 5), ("refuse", "local_index8_k256", 0, 256),
            ("s_output_local", 0, 255, 0, 1, 1, 0), ("s_frame_local", 0, SPRITE, 1, None), ("refuse", "local_tolerance_without_delta", 0, NOISY),
            ("s_frame_local", 0, NOISY, 0, None), ("s_close", 0)]


def _the_sequence_optimize_path_counts_plans_remaps_and_replays():
    """one record over the coded frames, one plan by usage with the transparent slot kept, every frame remapped at 8 bits: no bad
    pixel, and the remapped maps through the pruned palette show what the originals show"""
    ops = [("cutoff", 128), ("s_new", 0), ("s_add", 0, SPRITE, 0, 0), ("s_output", 0, 24, 1, 1, 1)]
    for j, i in enumerate((SPRITE, NOISY, SHIFT)):
        ops += [("s_frame", 0, i, 1, None), ("s_usage", 0, 0, int(j == 0), j)]
    return ops + [("plan", 0, 0, 1 | 8)] + [("s_remap", 0, 0, 8, j, 1) for j in range(3)] + [("s_close", 0), ("cutoff", 0)]


def _usage_records_outlive_their_maps_and_the_bad_count_combines():
    return [("cutoff", 0), ("usage_device", ODD, 0, 1, 40, 51, 0, 3, _order(61, 3, "reverse"), 0, 1), ("optimize", SPRITE, 12, 1, 1 | 16, 0),
            ("usage_device", ODD_B, 1, 2, 40, 52, 0, 2, 5, 1, 0), ("optimize", FEW, 6, 0, 1 | 8, 8), ("plan", 0, 0, 2 | 4 | 16),
            ("remap_device", ODD, 0, 1, 40, 53, 0, 8, 1, 1, 0), ("remap_device", ODD, 3, 2, 40, 54, ("rand", 9), 4, 0, 1, 1),
            ("remap_device", ROW, 0, 1, 40, 55, ("rand", 10), 1, 0, 0, 0), ("remap_device", COL, 1, 2, 300, 58, ("rand", 11), 2, 0, 0, 1),
            ("usage_device", ODD, 0, 1, 256, 56, 1, 2, 3, 0, 1), ("refuse", "plan_indices_above_k", 1, 0), ("refuse", "plan_empty_record", 1, 0),
            ("plan", 1, 1, 0), ("refuse", "optimize_bits_too_narrow", FEW, 5), ("optimize", FEW, 5, 0, 4, 0), ("refuse", "remap_bad_bits", FLAT, 3),
            ("usage_device", SPRITE, 0, 2, 300, 57, 0, 2, 4, 1, 1), ("plan", 0, 0, 1), ("remap_device", SPRITE, 0, 2, 300, 57, 0, 16, 1, 0, 0)]


def _a_colour_keyed_canvas_of_the_caller_on_both_routes():
    return [("cutoff", 128), ("cpair_open", 0, 1, 1, 40, 1), ("cpair_frame", 0, SPRITE, 61, None, 3, _order(72, 3, "reverse"), 0),
            ("cpair_frame", 0, NOISY, 61, 40, 3, _order(72, 3, "reverse"), 1), ("cpair_frame", 0, SHIFT, 62, 4096, 2, 3, 0),
            ("cpair_frame", 0, SPRITE, 62, None, 1, 0, 0), ("cpair_open", 1, 0, 2, 300, 4), ("cpair_frame", 1, ODD, 63, 40, 3, _order(61, 3, "reverse"), 0),
            ("cpair_frame", 1, ODD_B, 63, 40, 2, 1, 1), ("cpair_frame", 1, ODD, 64, None, 2, 2, 0), ("cutoff", 0)]


# ---- surface 3: alpha weighting ---------------------------------------------------------------------------------------------------
def _weight_on_cutoff_0_128_0_weight_off_around_the_same_calls():
    """the first and the last results are the default path's; under weighting the working image is cut at max(t, 1) and the outputs
    at t; INDEX8 at k = 256 is legal at t = 0 under weighting"""
    at = [("palette", SPRITE, 8), ("reduce_indexed", SPRITE, 8, 0, 1), ("reduce_indexed", ODD, 40, 3, 1), ("reduce", ODD, 8, 1), ("reduce", MAP, 5, 3)]
    return ([("strategy", 0), ("fixed", 0), ("cutoff", 0), ("weight", 0)] + at + [("weight", 1)] + at + [("cutoff", 128)] + at + [("cutoff", 0)] + at +
            [("reduce_indexed", FEW, 256, 0, 0), ("find", ODD, 9, 0, 71), ("apply", SPRITE, 1, 1, 256, 72, 0), ("weight", 0)] + at)


def _two_frames_added_under_different_weightings_and_the_palette_both_ways():
    """the weighting at an add decides that frame's cutoff (s_info: the frame added under it at t = 0 loses its pixels of alpha 0),
    the weighting at the palette call whether the loop is weighted"""
    ops = [("cutoff", 0), ("fixed", 0), ("s_new", 0)]
    for first in (0, 1):
        ops += [("s_clear", 0), ("weight", first), ("s_add", 0, SPRITE, 0, 0), ("weight", 1 - first), ("s_add", 0, ODD, 1, 1), ("s_info", 0),
                ("s_centroids", 0, 7), ("s_palette", 0, 7), ("weight", first), ("s_centroids", 0, 7), ("s_palette", 0, 7),
                ("s_output", 0, 7, 0, 1, 1), ("s_frame", 0, SPRITE, 1, None), ("s_frame", 0, NOISY, 1, 40), ("s_end", 0)]
    return ops + [("fixed", 2), ("weight", 1), ("s_add", 0, MAP, 0, 0), ("s_info", 0), ("s_centroids", 0, 6), ("fixed", 0), ("weight", 0),
                  ("s_centroids", 0, 6), ("s_close", 0)]


def _a_warm_output_alternates_weighted_and_unweighted_frames_across_a_cutoff_switch():
    """a warm frame reads the weighting at its own call, as it reads the cutoff"""
    return [("cutoff", 0), ("fixed", 0), ("weight", 1), ("s_new", 1), ("s_output_local", 1, 12, 0, 1, 1, 1), ("s_frame_local", 1, SPRITE, 1, None),
            ("weight", 0), ("s_frame_local", 1, NOISY, 1, 40), ("cutoff", 128), ("weight", 1), ("s_frame_local", 1, SHIFT, 1, None), ("weight", 0),
            ("s_frame_local", 1, SPRITE, 1, 4096), ("cutoff", 0), ("weight", 1), ("s_frame_local", 1, NOISY, 1, None),
            ("s_output_local", 1, 5, 1, 2, 0, 0), ("s_frame_local", 1, ODD, 1, None), ("weight", 0), ("s_frame_local", 1, ODD_B, 1, 40),
            ("s_output_local", 1, 3, 0, 1, 4, 1), ("s_frame_local", 1, CLEAR, 1, None), ("weight", 1), ("s_frame_local", 1, CLEAR, 1, None),
            ("weight", 0), ("s_frame_local", 1, CLEAR, 1, None), ("s_close", 1)]


def _the_binding_of_an_initialisation_and_of_the_caller_around_the_lloyd_weighting():
    """forced colour table, so that the initialisation leaves a binding: the weighted run drops it, and so does the setter, in both
    directions; the setter is refused under the caller's binding, bind_image on a weighted object"""
    return [("strategy", 2), ("l_new", 0, 9), ("l_init", 0, ODD, 0, 0), ("l_weight", 0, 1), ("l_run", 0, ODD, 1, 0), ("l_weight", 0, 0),
            ("l_assign_update", 0, ODD, 1, 1, 0), ("l_init", 0, ODD, 1, 1), ("l_weight", 0, 1), ("l_assign", 0, ODD, 1), ("l_weight", 0, 0),
            ("l_assign", 0, ODD, 0), ("l_init", 0, MAP, 0, 0), ("l_weight", 0, 0), ("l_assign", 0, MAP, 0), ("l_bind", 0, MAP, 0),
            ("refuse", "l_weight_under_caller_binding", 0, 1), ("l_assign", 0, MAP, 1), ("l_run", 0, MAP, 1, 0),
            ("refuse", "l_weight_under_caller_binding", 0, 0), ("refuse", "l_weight_bad_value", 0, 2), ("l_unbind", 0), ("l_weight", 0, 1),
            ("refuse", "weighted_bind", 0, MAP), ("refuse", "weighted_lftu", 0, MAP), ("refuse", "weighted_accumulate_into", 0, MAP),
            ("l_run", 0, MAP, 1, 1), ("l_iterate", 0, SPRITE, 2, 0), ("l_conv", 0, 0), ("refuse", "l_weight_bad_value", 0, -1), ("l_assign", 0, SPRITE, 0),
            ("l_weight", 0, 0), ("l_assign_update", 0, SPRITE, 1, 1, 1), ("l_lftu", 0, SPRITE, 0), ("l_close", 0), ("strategy", 0)]


def _weighted_and_unweighted_lloyd_objects_in_each_others_blocks_beside_weighted_host_calls():
    """neither a Lloyd object of the caller's nor the library's own one leaks its weighting into the block's next owner"""
    return [("cutoff", 0), ("fixed", 0), ("l_new", 0, 12), ("l_set", 0, "rand", 81, ODD), ("l_weight", 0, 1), ("l_assign_update", 0, ODD, 1, 1, 0),
            ("weight", 0), ("palette", SPRITE, 6), ("l_close", 0), ("l_new", 0, 12), ("l_set", 0, "rand", 81, ODD), ("l_assign_update", 0, ODD, 1, 1, 0),
            ("weight", 1), ("reduce_indexed", SPRITE, 6, 0, 0), ("l_new", 1, 40), ("l_set", 1, "rand", 82, ODD), ("l_assign_update", 1, MAP, 1, 1, 1),
            ("l_close", 1), ("l_close", 0), ("l_new", 1, 40), ("l_set", 1, "rand", 82, ODD), ("l_weight", 1, 1), ("l_assign_update", 1, MAP, 1, 1, 0),
            ("weight", 0), ("reduce_indexed", SPRITE, 6, 0, 0), ("palette", MAP, 300), ("l_re", 1, 5), ("l_set", 1, "dup", 83, ODD),
            ("l_run", 1, FEW, 1, 0), ("l_close", 1)]


def _fixed_colours_and_weighting_with_clusters_of_weight_0():
    """a pinned entry stays put whatever its members weigh and counts as converged; a free cluster whose members all weigh 0 is an
    empty cluster (60 centroids on the 131 pixels of the row, a quarter of which weigh 0)"""
    return [("cutoff", 0), ("fixed", 3), ("weight", 1), ("palette", SPRITE, 11), ("reduce_indexed", ROW, 12, 0, 0), ("reduce", COL, 9, 1),
            ("refuse", "weight_bad_value", 2), ("refuse", "weight_bad_value", -1), ("palette", SPRITE, 11),
            ("l_new", 0, 60), ("l_init", 0, ROW, 3, 0), ("l_fix", 0, 3), ("l_weight", 0, 1), ("l_assign_update", 0, ROW, 1, 1, 0), ("l_conv", 0, 0),
            ("l_run", 0, COL, 1, 1), ("l_iterate", 0, ROW, 2, 0), ("l_conv", 0, 1), ("l_update", 0, 0), ("l_conv", 0, 0), ("l_close", 0),
            # the refusals of weighting once no colour is fixed, so that nothing else refuses them: the octree in its three calls
            # (reduce: nothing written), and the image without a kept pixel at t = 0
            ("fixed", 0), ("refuse", "octree_weighted", SPRITE, 12, 0), ("refuse", "octree_weighted", SPRITE, 12, 1),
            ("refuse", "octree_weighted", FEW, 6, 2), ("refuse", "weighted_no_kept_pixel", 0), ("refuse", "weighted_no_kept_pixel", 1),
            ("refuse", "weighted_no_kept_pixel", 2), ("palette", SPRITE, 5), ("weight", 0)]


def _the_quality_search_weighted_then_unweighted():
    """weighted palettes, the unweighted record, on the working image cut at max(t, 1); then the same call without weighting"""
    q = ("quality", SPRITE, 4.0, 2, 12, 0, 1, 1)
    return [("cutoff", 0), ("fixed", 0), ("weight", 1), q, ("quality", MAP, 9.0, 2, 10, 3, 0, 0), ("cutoff", 128), q, ("cutoff", 0), ("weight", 0), q,
            ("fixed", 2), ("weight", 1), ("quality", SPRITE, 9.0, 3, 9, 1, 1, 0), ("fixed", 0), ("weight", 0)]


# ---- surface 4: the batched calls ---------------------------------------------------------------------------------------------------
def _batches_of_nine_two_and_one_image_at_k_300_3_and_33():
    """n, k and the sizes shrink from batch to batch, through the palette, the indexed, the find and the device call: every word a
    recycled block still holds -- stop, slots, distances, centroids, records, gather buffer, tables -- differs from the needed one"""
    nine = (ODD, ROW, SPRITE, FLAT, SHIFT, FEW, NOISY, ODD_B, COL)
    steps = ((nine, 300), ((ROW_B, COL_B), 3), ((MAP,), 33))
    ops = [("strategy", 0), ("cutoff", 0), ("fixed", 0), ("weight", 0)]
    ops += [("b_palette", imgs, k, 0, 0) for imgs, k in steps]
    ops += [("b_reduce_indexed", imgs, k, 0, 1, 2 if k > 255 else 1, 0) for imgs, k in steps]
    ops += [("b_find", imgs, k, 91, 1, 2 if k > 255 else 1, 0) for imgs, k in steps]
    ops += [("b_palette_device", imgs, k) for imgs, k in steps]
    return ops + [("b_reduce", (MAP, BIG), 3, 0, 1, 0), ("b_palette", (BIG,), 33, 0, 0)]


def _two_device_batches_with_a_lloyd_object_in_the_block_between():
    return [("b_palette_device", (SPRITE, FEW, ODD, FLAT, MAP), 24), ("l_new", 0, 12), ("l_set", 0, "rand", 3, ODD), ("l_run", 0, FEW, 1, 0),
            ("l_close", 0), ("b_palette_device", (COL, ODD_B, FEW), 5), ("l_new", 1, 300), ("l_set", 1, "rand", 4, ODD), ("l_run", 1, ROW, 1, 1),
            ("l_close", 1), ("b_palette_device", (BIG, ROW, CLEAR), 40), ("b_palette_device", (FLAT,), 1)]


def _cutoff_0_128_0_around_the_indexed_and_the_find_batch_then_device_output_batches():
    """every batched call reads the cutoff when it starts: index k below it, INDEX8 sized for it; the device output call at each
    cutoff with one shared table and with a table per image, at the aligned and the unaligned element offsets"""
    imgs = (SPRITE, ODD, NOISY, ROW, MAP)
    ops = [("fixed", 0), ("weight", 0)]
    for t in (0, 128, 0):
        ops += [("cutoff", t), ("b_reduce_indexed", imgs, 24, 0, 1, 1, 0), ("b_reduce_indexed", imgs, 24, 0, 0, 2, 1),
                ("b_find", imgs + (CLEAR,), 24, 92, 1, 1, 0), ("b_find", imgs, 300, 93, 0, 2, 1)]
    for t in (128, 0):
        ops += [("cutoff", t), ("b_apply_device", imgs, 24, 94, 1, 1, 1, 1), ("b_apply_device", imgs, 24, 94, 0, 0, 2, 4),
                ("b_apply_device", imgs + (CLEAR,), 9, 95, 0, 3, 0, 0), ("b_apply_device", imgs, 255, 96, 0, 1, 1, 1)]
    return ops + [("refuse", "batch_index8_full", "b_apply_device", imgs, 257), ("refuse", "batch_index8_full", "b_find", imgs, 257),
                  ("b_apply_device", imgs, 256, 97, 1, 0, 1, 0)]


def _fixed_colours_and_weighting_around_the_batches():
    """the find batch ignores both switches and equals the unpinned model; the three calls with a palette step refuse; with the
    switch off again the same calls work"""
    imgs, k = (ODD, SPRITE, MAP, FEW), 12
    calls = [("b_reduce_indexed", imgs, k, 0, 1, 1, 0), ("b_palette", imgs, k, 0, 0), ("b_reduce", imgs, k, 0, 0, 1)]
    ops = [("cutoff", 0), ("weight", 0)]
    for what, on, off in (("batch_fixed", ("fixed", 3), ("fixed", 0)), ("batch_weighted", ("weight", 1), ("weight", 0))):
        ops += [on, ("b_find", imgs, k, 98, 1, 1, 0)] + [("refuse", what, c[0], imgs, k) for c in calls] + [off, ("b_find", imgs, k, 98, 1, 1, 0)] + calls
    return ops


def _a_batch_refused_for_an_image_without_a_kept_pixel_then_the_same_list_without_it():
    """refused at bound 0 after the shrinks and at bound 1 in the up-front pass, no output written; the same list without the image
    at bound 1 and at bound 0, in the blocks the refused calls gave back"""
    imgs, k = (ODD, SPRITE, FEW, MAP), 7
    ops = [("fixed", 0), ("weight", 0), ("cutoff", 128)]
    for call in ("b_reduce_indexed", "b_palette", "b_reduce"):
        ops += [("refuse", "batch_no_kept_pixel", call, imgs + (CLEAR,), k, bound) for bound in (0, 1)]
        ops += [{"b_palette": ("b_palette", imgs, k, 0, bound), "b_reduce": ("b_reduce", imgs, k, 0, 1, bound),
                 "b_reduce_indexed": ("b_reduce_indexed", imgs, k, 0, 1, 1, bound)}[call] for bound in (1, 0)]
    return ops + [("refuse", "batch_no_kept_pixel", "b_palette", (CLEAR, ODD), k, 1), ("refuse", "batch_empty", "b_palette"),
                  ("refuse", "batch_empty", "b_apply_device"), ("refuse", "batch_meld_indexed", "b_reduce_indexed", imgs, 5, 1),
                  ("refuse", "batch_bad_tables", imgs, 9, 2), ("refuse", "batch_bad_tables", imgs, 9, 5), ("b_palette", imgs, k, 0, 0), ("cutoff", 0)]


def _batches_between_the_frames_of_an_open_output_and_beside_a_bound_lloyd_object():
    return [("cutoff", 0), ("fixed", 0), ("weight", 0), ("s_new", 0), ("s_add", 0, SPRITE, 0, 0), ("s_output", 0, 16, 1, 1, 1),
            ("s_frame", 0, SPRITE, 1, None), ("l_new", 0, 9), ("l_set", 0, "rand", 5, ODD), ("l_bind", 0, ODD, 0), ("l_assign", 0, ODD, 0),
            ("b_reduce_indexed", (ODD, FEW, SPRITE, ROW), 40, 0, 1, 1, 0), ("s_frame", 0, NOISY, 1, 40), ("l_assign", 0, ODD, 1),
            ("b_palette_device", (MAP, FLAT, COL), 33), ("b_apply_device", (NOISY, ODD), 40, 99, 0, 1, 2, 1), ("s_frame", 0, SHIFT, 1, None),
            ("l_assign_update", 0, ODD, 1, 1, 0), ("b_palette", (SPRITE, SPRITE, ODD), 8, 0, 1), ("s_frame", 0, SPRITE, 1, 4096), ("l_close", 0),
            ("s_close", 0)]


def _octree_batches_alternate_with_k_means_batches():
    """the octree is the host algorithm per image: no batched launch, palettes of their own sizes"""
    imgs, k = (SPRITE, FEW, ROW, NOISY, COL_B), 13
    ops = [("cutoff", 0), ("fixed", 0), ("weight", 0)]
    for algo in (1, 0, 1):
        ops += [("b_palette", imgs, k, algo, int(algo)), ("b_reduce", imgs, k, 1 - algo, 1, 0)]
    return ops


SCENARIOS = {f.__name__[1:]: f for f in (_cutoff_0_128_0_around_palette_reduce_and_a_plan, _frames_added_under_three_cutoffs_then_clear, _an_output_ends_a_lloyd_object_runs_in_its_block_and_the_next_output_starts_fresh, _frozen_seeds_do_not_outlive_their_object, _quality_search_with_and_without_pins_beside_a_bound_object, _records_combine_over_bands_in_reverse_on_two_streams, _every_refusal_is_followed_by_the_correct_call, _two_sequences_alternate_beside_host_calls_on_the_megapixel_image,
                                         # surface 2, on the same long-lived processor after the eight above
                                         _a_warm_output_across_a_cutoff_switch_and_back,
                                         _a_refused_frame_leaves_a_warm_output_warm_and_a_failed_palette_step_makes_it_cold,
                                         _a_local_output_begins_in_a_used_block_with_a_lossy_first_frame,
                                         _a_lossy_frame_comes_back_in_full_then_an_exact_and_a_lossy_frame,
                                         _local_shared_local_on_one_sequence_with_the_refusals_between,
                                         _the_sequence_optimize_path_counts_plans_remaps_and_replays,
                                         _usage_records_outlive_their_maps_and_the_bad_count_combines,
                                         _a_colour_keyed_canvas_of_the_caller_on_both_routes,
                                         # surface 3, after the sixteen above: the processor ends with weighting off
                                         _weight_on_cutoff_0_128_0_weight_off_around_the_same_calls,
                                         _two_frames_added_under_different_weightings_and_the_palette_both_ways,
                                         _a_warm_output_alternates_weighted_and_unweighted_frames_across_a_cutoff_switch,
                                         _the_binding_of_an_initialisation_and_of_the_caller_around_the_lloyd_weighting,
                                         _weighted_and_unweighted_lloyd_objects_in_each_others_blocks_beside_weighted_host_calls,
                                         _fixed_colours_and_weighting_with_clusters_of_weight_0,
                                         _the_quality_search_weighted_then_unweighted,
                                         # surface 4, after the twenty-three above: the switches end as they began
                                         _batches_of_nine_two_and_one_image_at_k_300_3_and_33,
                                         _two_device_batches_with_a_lloyd_object_in_the_block_between,
                                         _cutoff_0_128_0_around_the_indexed_and_the_find_batch_then_device_output_batches,
                                         _fixed_colours_and_weighting_around_the_batches,
                                         _a_batch_refused_for_an_image_without_a_kept_pixel_then_the_same_list_without_it,
                                         _batches_between_the_frames_of_an_open_output_and_beside_a_bound_lloyd_object,
                                         _octree_batches_alternate_with_k_means_batches)}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenario(world, name):
    """(tests/test_session_model.py runs the same lists on its stand-ins: they are legal sequences of the harness)"""
    _run(world, SCENARIOS[name]())
