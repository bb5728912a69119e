"""The host's guarded spin wait (jobset_amd/csrc/jsp_wait.h) on the CPU:
tools/wait_check.cc drives every result of the loop (ready, abandoned, gone,
failed, late), its 256-spin beat and the query's pacing with a scripted
stream query and a clock of its own, built with ASan + UBSan into the program
itself (make wait-asan). No GPU: the branches a dead or hung stream would take
run nowhere else."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_every_branch_of_the_guarded_wait():
    r = subprocess.run(["make", "-s", "wait-asan"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "wait_check: ok" in r.stdout.splitlines(), r.stdout[-2000:]
