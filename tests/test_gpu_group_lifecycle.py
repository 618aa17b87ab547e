"""The multi-device layer under long-lived objects (tests/group_harness.py): the random sequences of tools/fuzz_group_lifecycle.py
on the seeds tests/test_group_model.py vouches for, and the hand-written scenarios -- each an op list of the harness -- run one
after the other on groups that stay alive across them.  Five worlds in one process on device 0: one rank with every RCCL
collective forced, one rank without collectives, two / three / five ranks through the loopback exchange.  Everything -- every
band's label map and its guard, every rank's centroid table, iteration counts, host outputs -- is compared bit for bit with the
oracle after every op; a mismatch ends the subprocess, which starts nothing more on the device.

Measured on one MI355X: see profiles/NOTES.md ("group lifecycle harness")."""
import os
import re
import subprocess
import sys

import pytest

import group_harness as G
from test_group_model import SEEDS, SEQUENCES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "fuzz_group_lifecycle.py")
ENV = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")


def _reused(stdout):
    return [int(x) for x in re.findall(r"(\d+) blocks re-used", stdout)]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sequences_equal_the_model(torch_cuda, seed):
    r = subprocess.run([sys.executable, TOOL, str(SEQUENCES), str(seed)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert re.search(rf"^{SEQUENCES} sequences, \d+ ops, 0 mismatching$", r.stdout, re.M), r.stdout[-2000:]
    reused = _reused(r.stdout)
    assert len(reused) == SEQUENCES and max(reused) > 0, reused      # else nothing ran on recycled blocks of a member processor


def test_hand_written_scenarios_on_groups_that_stay_alive(torch_cuda):
    names = list(G.scenarios())
    r = subprocess.run([sys.executable, TOOL, "scenarios"], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    for name in names:
        assert re.search(rf"^{name}: \d+ ops", r.stdout, re.M), (name, r.stdout[-2000:])
    assert re.search(rf"^{len(names)} sequences, \d+ ops, 0 mismatching$", r.stdout, re.M), r.stdout[-2000:]
    assert max(_reused(r.stdout)) > 0
