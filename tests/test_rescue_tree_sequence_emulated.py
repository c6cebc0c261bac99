"""The kernels of ordered leaf writes (rescue_seq_level_spread_kernel, rescue_tree_scatter_from_kernel, kernels_hash.hip) and the device path of
dst_rtree_apply / dst_stree_apply on the host launch emulation: tests/emu/_build/libdistaff_emu.so with device = 0, against host trees of the
product library driven one operation at a time.  No GPU.  This pins the plan of host/tree_sequence.h, the source words, the staging layout, the
two version areas taking turns and the order of the scatters; sequences of this size never reach the one-lane kernel, which
tests/test_rescue_tree_sequence_gpu.py drives."""
import pytest

from test_rescue_tree_emulated import emu  # noqa: F401  (the fixture that builds and opens the emulated library)
from test_rescue_tree_sequence_host import (NONZERO_EMPTY, check_dense_rejections, check_dense_sequence, check_sparse_rejections, check_sparse_sequence, index_lists,
                                            random_ops, sparse_cases)


@pytest.fixture()
def emu_tree(emu):  # noqa: F811
    import distaff_amd as D
    return lambda leaves: D.RescueTree(leaves, device=0, lib=emu)


@pytest.fixture()
def emu_sparse(emu):  # noqa: F811
    import distaff_amd as D
    return lambda depth, empty=(0, 0): D.SparseRescueTree(depth, empty, device=0, lib=emu)


def test_dense_sequences_equal_one_operation_at_a_time(emu_tree):
    tree = leaves = None
    for case, indices in enumerate(index_lists(8, 3) + [random_ops(8, 24, 43, 0.3)[0], [6]]):      # all on ONE tree: a stale plan in the staging buffer would show
        new = random_ops(8, len(indices), 300 + case)[1]
        tree, leaves = check_dense_sequence(emu_tree, 3, indices, new, 23, tree=tree, leaves=leaves)
        assert tree.update_ms >= 0
    tree.close()


@pytest.mark.parametrize("depth,empty", [(3, NONZERO_EMPTY), (63, (0, 0))])
def test_sparse_sequences_equal_one_operation_at_a_time(emu_sparse, depth, empty):
    for initial, ops in sparse_cases(depth, empty, 60 + depth):
        tree, _ = check_sparse_sequence(emu_sparse, depth, empty, initial, ops)
        assert tree.info()["last_digests"] == len(ops) * depth + sum(len({k >> (depth - l) for k, _ in ops}) for l in range(depth))
        tree.close()


def test_a_longer_sparse_sequence_and_a_second_one_on_the_same_tree(emu_sparse):
    depth = 63
    keys, new = random_ops(1 << depth, 24, 44, 0.3)
    tree, content = check_sparse_sequence(emu_sparse, depth, NONZERO_EMPTY, {}, list(zip(keys, new)))
    again, new = random_ops(1 << depth, 8, 45, 0.3)
    again[3] = keys[0]                                                                             # a key the first sequence stored
    tree, _ = check_sparse_sequence(emu_sparse, depth, NONZERO_EMPTY, content, list(zip(again, new)), tree=tree)
    tree.close()


def test_rejected_sequences_leave_the_trees_unchanged(emu_tree, emu_sparse):
    check_dense_rejections(emu_tree, 3)
    check_sparse_rejections(emu_sparse, 3)
