"""The Rescue kernels' own source (distaff_amd/csrc/rescue_dev.h, the Rescue kernels of kernels_hash.hip) on the host launch emulation:
tests/emu/_build/libdistaff_emu.so with device = 0, against the oracle's hasher_digest.  No GPU.  As in tests/test_emulated_kernels.py this
pins the kernels' logic -- state order, the addition chain's step table, the exchange of the six-lane form, node-array indexing, the check
of the inputs -- and the limb-level dataflow of fe.h on plain integers; the gfx950 instructions themselves are the GPU tests' business.
Trees of this size take the six-lane level kernel on every level; the one-lane-per-digest form is exercised through the digest kernel."""
import ctypes
import os
import random
import subprocess

import pytest

from test_rescue_tree_host import P, check_every_node, edge_tuples, random_leaves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libdistaff_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR, "-j8"], stdout=subprocess.DEVNULL)
    assert os.path.exists(EMU_LIB)
    os.environ.setdefault("DISTAFF_EMU_THREADS", "2")
    return ctypes.CDLL(EMU_LIB)


def test_digest_kernel_equals_the_oracle(oracle, emu):
    import distaff_amd as D
    rnd = random.Random(6)
    tuples = [tuple(rnd.randrange(P) for _ in range(4)) for _ in range(256)] + edge_tuples()
    out = D.arr_to_ints(D.rescue_digest(tuples, device=0, lib=emu))
    for k, t in enumerate(tuples):
        assert out[2 * k:2 * k + 2] == oracle.hasher_digest(list(t)), t


def test_inputs_are_checked_by_the_kernels(emu):
    import distaff_amd as D
    for bad in (P, 2 ** 128 - 1):
        with pytest.raises(D.DistaffError) as e:
            D.rescue_digest([(1, 2, 3, 4)] * 70 + [(5, 6, bad, 8)], device=0, lib=emu)
        assert e.value.code == D.DST_ERR_ARG
        with pytest.raises(D.DistaffError) as e:
            D.RescueTree([(1, 2), (3, 4), (bad, 6), (7, 8)], device=0, lib=emu)
        assert e.value.code == D.DST_ERR_ARG


@pytest.mark.parametrize("log_leaves", range(1, 7))
def test_every_node_of_the_tree_is_the_digest_of_its_children(oracle, emu, log_leaves):
    import distaff_amd as D
    leaves = random_leaves(log_leaves, 200 + log_leaves)
    tree = D.RescueTree(leaves, device=0, lib=emu)
    check_every_node(oracle, D, tree, leaves)
    host = D.RescueTree(leaves, device=-1, lib=emu)
    assert host.root == tree.root and host.path(1) == tree.path(1) and host.tapes(1) == tree.tapes(1)
    tree.close(); host.close()
