"""Ordered leaf writes with a witness for each on the GPU (rescue_seq_level_kernel, rescue_seq_level_spread_kernel, rescue_tree_scatter_from_kernel)
through the library the session binds.  The yardstick is a HOST tree driven through the calls that existed before, one operation at a time --
path, update / set with count 1, root -- and a fresh build over the final leaves; never the new call.  Everything is bit-exact.  Every test has
its own time limit and nothing is run twice."""
import numpy as np
import pytest

from test_rescue_tree_sequence_host import (NONZERO_EMPTY, check_dense_rejections, check_dense_sequence, check_sparse_rejections, check_sparse_sequence, example_roots, index_lists,
                                            random_ops, run_example, sparse_cases)

pytestmark = pytest.mark.gpu
SPREAD_MAX = 1 << 15                       # RESCUE_SPREAD_MAX: launches of more operations run the one-lane kernel


def device_tree(leaves):
    import distaff_amd as D
    return D.RescueTree(leaves, device=0)


def device_sparse(depth, empty=(0, 0)):
    import distaff_amd as D
    return D.SparseRescueTree(depth, empty, device=0)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("log_leaves", [1, 3, 10])
def test_dense_sequences_equal_a_host_tree_driven_one_operation_at_a_time(log_leaves):
    """the host file's lists, all on ONE device tree: a stale plan in the staging buffer would show"""
    n = 1 << log_leaves
    tree = leaves = None
    for case, indices in enumerate(index_lists(n, log_leaves)):
        new = random_ops(n, len(indices), 700 + 10 * log_leaves + case)[1]
        tree, leaves = check_dense_sequence(device_tree, log_leaves, indices, new, 30 + log_leaves, tree=tree, leaves=leaves)
        assert tree.update_ms > 0
    tree.close()


@pytest.mark.timeout(120)
def test_200_random_operations_with_repeats_span_several_workgroups():
    """8 operations per workgroup in the six-lane form: 25 workgroups, versions read across them"""
    indices, new = random_ops(1 << 10, 200, 71)
    assert len(set(indices)) < len(indices)
    tree, _ = check_dense_sequence(device_tree, 10, indices, new, 72)
    assert tree.update_ms > 0
    tree.close()


@pytest.mark.timeout(300)
def test_the_one_lane_kernel_on_more_operations_than_the_spread_form_takes():
    """2^15 + 64 operations on a tree of 4 leaves: 2 digests each, so the host yardstick is some 65 000 digests.  Every root and every final node;
    the paths of the first and the last 64 operations."""
    count = SPREAD_MAX + 64
    rng = np.random.default_rng(73)
    indices = [int(i) for i in rng.integers(0, 4, size=count)]
    new = rng.integers(0, 1 << 64, size=(count, 2, 2), dtype=np.uint64)
    new[..., 1] >>= np.uint64(1)                                                    # high word below 2^63: below p
    import distaff_amd as D
    v = D.arr_to_ints(new)
    pairs = [(v[2 * i], v[2 * i + 1]) for i in range(count)]
    tree, _ = check_dense_sequence(device_tree, 2, indices, pairs, 74, paths_at=set(range(64)) | set(range(count - 64, count)))
    assert tree.update_ms > 0
    tree.close()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("depth,empty", [(1, (0, 0)), (10, NONZERO_EMPTY), (63, (0, 0))])
def test_sparse_sequences_equal_a_host_tree_driven_one_operation_at_a_time(depth, empty):
    for initial, ops in sparse_cases(depth, empty, 80 + depth):
        tree, _ = check_sparse_sequence(device_sparse, depth, empty, initial, ops)
        info = tree.info()
        assert info["last_device_ms"] > 0 and info["last_digests"] == len(ops) * depth + sum(len({k >> (depth - l) for k, _ in ops}) for l in range(depth))
        tree.close()


@pytest.mark.timeout(300)
def test_300_operations_on_a_sparse_tree_of_1000_keys():
    """stored and new keys mixed, repeats among them, against sequential sets on a host tree; the fresh tree of the final content is a device
    tree (a host tree set once with 1 200 keys would double the host's digests and say nothing the second tree does not)"""
    depth = 63
    rng = np.random.default_rng(75)
    stored = [int(k) for k in np.unique(rng.integers(0, 1 << 63, size=1000, dtype=np.uint64))]
    initial = dict(zip(stored, random_ops(4, len(stored), 76)[1]))
    fresh_keys, new = random_ops(1 << depth, 300, 77)
    keys = [stored[(7 * j) % len(stored)] if j % 3 == 0 else k for j, k in enumerate(fresh_keys)]
    assert len(set(keys)) < len(keys) and set(keys) & set(stored) and set(keys) - set(stored)
    tree, _ = check_sparse_sequence(device_sparse, depth, (0, 0), initial, list(zip(keys, new)), fresh_by=(device_sparse,))
    assert tree.info()["last_device_ms"] > 0
    tree.close()


@pytest.mark.timeout(120)
def test_a_second_sequence_on_the_same_sparse_tree():
    """a stale plan in the staging buffer, or witnesses read from the generation before the first sequence's set, would show here"""
    depth = 63
    keys, new = random_ops(1 << depth, 30, 78, 0.3)
    tree, content = check_sparse_sequence(device_sparse, depth, NONZERO_EMPTY, {}, list(zip(keys, new)))
    again, new = random_ops(1 << depth, 12, 79, 0.3)
    again[5] = keys[1]
    tree, _ = check_sparse_sequence(device_sparse, depth, NONZERO_EMPTY, content, list(zip(again, new)), tree=tree)
    assert tree.info()["last_device_ms"] > 0
    tree.close()


@pytest.mark.timeout(120)
def test_rejected_sequences_leave_the_device_trees_unchanged():
    check_dense_rejections(device_tree, 10)
    check_sparse_rejections(device_sparse, 63)


@pytest.mark.timeout(300)
def test_c_example_checks_its_witnesses_on_a_device_tree(tmp_path):
    from test_rescue_tree_update_host import host_tree
    assert run_example(tmp_path, 10, 40, 0) == example_roots(host_tree, 10, 40)
