"""The update and opening kernels' own source (rescue_tree_update_spread_kernel, rescue_tree_scatter_kernel, rescue_tree_gather_kernel and the
dense level kernels a fully dirty level runs through, kernels_hash.hip) on the host launch emulation: tests/emu/_build/libdistaff_emu.so with
device = 0.  No GPU.  As tests/test_rescue_tree_emulated.py does for the build, this pins the logic of the device path of dst_rtree_update /
dst_rtree_paths -- the dirty lists and their offsets, the indexing through the list, the staging layout -- at log_leaves = 3; trees of this size
never reach the one-lane indexed kernel, which tests/test_rescue_tree_update_gpu.py drives."""
import random

import pytest

from test_rescue_tree_emulated import emu  # noqa: F401  (the fixture that builds and opens the emulated library)
from test_rescue_tree_host import random_leaves
from test_rescue_tree_update_host import check_batched_openings, check_rejections, check_updates, host_tree, update_sets


@pytest.fixture()
def emu_tree(emu):  # noqa: F811
    import distaff_amd as D
    return lambda leaves: D.RescueTree(leaves, device=0, lib=emu)


def test_updated_tree_equals_a_fresh_build_and_the_host_tree(emu_tree):
    check_updates(emu_tree, 3, update_sets(3) + [[5], [4, 1, 7]], 83, also=host_tree)


def test_rejected_updates_leave_the_tree_unchanged(emu_tree):
    check_rejections(emu_tree, 3)


def test_batched_openings_equal_the_single_index_calls(emu_tree):
    tree = emu_tree(random_leaves(3, 84))
    rnd = random.Random(3)
    check_batched_openings(tree, [7, 0, 7] + [rnd.randrange(8) for _ in range(9)])
    tree.update([7, 2], [(7, 8), (9, 10)])
    assert tree.update_ms >= 0
    check_batched_openings(tree, [7, 2, 0])
    tree.close()
