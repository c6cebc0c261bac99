"""The multiproof kernels (rescue_multiproof_level_spread_kernel, rescue_stree_lookup_kernel, the gathers) and the device path of
dst_rtree_multiproof / dst_stree_multiproof / dst_rescue_multiproof_root / dst_rescue_verify_multiproof / dst_rescue_multiproof_paths on the host
launch emulation: tests/emu/_build/libdistaff_emu.so with device = 0, trees and checks alike, against the yardsticks of
tests/test_rescue_multiproof_host.py.  No GPU.  This pins the job indexing, the lane mapping of the six-lane form, the hand-over between level
launches through the pool, the lookup of (level, prefix) pairs and the `bad` word; launches of this size never reach the one-lane kernel, which
tests/test_rescue_multiproof_gpu.py drives."""
from test_rescue_multiproof_host import check_d3_table, check_dense, check_every_single_tampering, check_rejections, check_sizes, check_sparse
from test_rescue_tree_emulated import emu  # noqa: F401  (the fixture that builds and opens the emulated library)


def makers(lib):
    import distaff_amd as D
    return (lambda leaves: D.RescueTree(leaves, device=0, lib=lib)), (lambda depth, empty=(0, 0): D.SparseRescueTree(depth, empty, device=0, lib=lib))


def test_the_reference_cases_of_depth_3_by_heap_position(emu):  # noqa: F811
    check_d3_table(0, emu, makers(emu)[0])


def test_sizes_equal_the_restatement(emu):  # noqa: F811
    check_sizes(emu)


def test_dense_trees_of_2_and_8_leaves(emu):  # noqa: F811
    check_dense(0, emu, makers(emu)[0], log_leaves=(1, 3))


def test_sparse_depth_63_with_3_keys(emu):  # noqa: F811
    check_sparse(0, emu, makers(emu)[1], stored=3, absent=3)


def test_every_single_flipped_leaf_or_node_gives_ok_0(emu):  # noqa: F811
    check_every_single_tampering(0, emu, makers(emu)[0], log_leaves=3, count=3)


def test_what_is_refused_and_the_trees_stay_unchanged(emu):  # noqa: F811
    check_rejections(0, emu, *makers(emu))
