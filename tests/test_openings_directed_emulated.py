"""tests/test_openings_directed_gpu.py where there is no GPU: shapes A and C in a single context, and two ranks over shape A, against
tests/emu/_build/libdistaff_emu.so (the library's own sources compiled for the host, see tests/test_emulated_kernels.py).  The opening
plan, the owners, the batched gather's addresses and the slots of the proof are host code and index arithmetic: all of it is checked here
bit for bit against the oracle, at the directed position sets of tests/openings_sets.py."""
import os
import subprocess
import sys

import pytest

from openings_sets import FAMILIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libdistaff_emu.so")

SELECTION = ["test_position_sets_hold_what_they_are_meant_to"] + [
    "test_single_context_openings[%s-%s]" % (shape, family) for shape in ("A", "C") for family in FAMILIES] + [
    "test_verifier_at_given_positions_is_not_vacuous",
    "test_sharded_openings[2-A-None-False]",
    "test_refused_positions_leave_the_context_usable[A]",
    "test_refused_positions_leave_the_context_usable[C]",
    "test_no_position_at_all",
]


@pytest.fixture(scope="module")
def emulated_library():
    subprocess.check_call(["make", "-C", EMU_DIR, "-j8"], stdout=subprocess.DEVNULL)
    assert os.path.exists(EMU_LIB)
    return EMU_LIB


def test_directed_openings_on_the_emulated_build(emulated_library):
    env = dict(os.environ, DISTAFF_HIP_LIB=emulated_library, DISTAFF_HIP_RUNTIME="none", DISTAFF_EMU_THREADS="2")
    ids = ["tests/test_openings_directed_gpu.py::" + t for t in SELECTION]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu"] + ids,
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:]
    assert "%d passed" % len(SELECTION) in out, out[-2000:]
