"""The six-lane kernel of the path checks (rescue_path_root_spread_kernel, kernels_hash.hip) and the device path of dst_rescue_path_roots /
dst_rescue_verify_paths / dst_rescue_verify_writes on the host launch emulation: tests/emu/_build/libdistaff_emu.so with device = 0, against the
yardsticks of tests/test_rescue_path_verify_host.py (the reference's walk restated in Python, the roots of host trees).  No GPU.  This pins the
lane mapping, the hand-over of the digest between levels through the group's LDS slots, the launch of both modes over one copy of the paths and
the `bad` word; launches of this size never reach the one-lane kernel, which tests/test_rescue_path_verify_gpu.py drives.  The trees whose paths
and witnesses are checked are host trees of the product library: what is emulated is the checker."""
from test_rescue_path_verify_host import (check_path_roots, check_rejections, check_tampering, check_tree_paths, check_writes_of_apply, host_sparse, host_tree,
                                          path_root_cases)
from test_rescue_tree_emulated import emu  # noqa: F401  (the fixture that builds and opens the emulated library)


def test_path_roots_equal_the_reference_walk(oracle, emu):  # noqa: F811
    """every index of n = 2, 3, 4 in launches of 1, 8, 9 and 17 groups; n = 64 with the ends of the index range; n = 21 at three paths"""
    cases = [(n, indices[:3] if n == 21 else indices) for n, indices in path_root_cases()]
    check_path_roots(0, emu, oracle, cases)


def test_paths_of_dense_and_sparse_trees_resolve_to_their_roots(emu):  # noqa: F811
    check_tree_paths(0, emu, host_tree, host_sparse, log_leaves=(1, 3))


def test_the_witnesses_of_apply_are_accepted_and_the_state_is_followed(emu):  # noqa: F811
    check_writes_of_apply(0, emu, host_tree, host_sparse)


def test_each_single_tampering_is_found_at_its_write(emu):  # noqa: F811
    check_tampering(0, emu, host_tree)


def test_what_is_refused(emu):  # noqa: F811
    check_rejections(0, emu)
