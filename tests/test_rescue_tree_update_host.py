"""Updates in place and batched openings of Rescue Merkle trees (dst_rtree_update, dst_rtree_paths, dst_rtree_tapes_many) on the host path
(device = -1) of the PRODUCT library.  No GPU.  The yardstick of an update is dst_rtree_build over the modified leaves -- code that
tests/test_rescue_tree_host.py holds against the oracle.  The single-index calls may share their code with the batched openings, so these have
two yardsticks that share none: the node array as dst_rtree_read_nodes copies it, at positions computed here, and tapes_from_path.  The helpers take
the tree's constructor, so tests/test_rescue_tree_update_gpu.py and tests/test_rescue_tree_update_emulated.py run the same cases on device trees."""
import ctypes
import random

import numpy as np
import pytest

from test_rescue_tree_host import P, _product, random_leaves, tapes_from_path


def host_tree(leaves):
    import distaff_amd as D
    return D.RescueTree(leaves, device=-1, lib=_product())


def all_nodes(tree):
    """nodes 1 .. 2^(log_leaves + 1) - 1: the whole tree"""
    return tree.nodes(1, (2 << tree.log_leaves) - 1)


def update_sets(log_leaves):
    """the index sets of one run, applied one after the other to the same tree"""
    n = 1 << log_leaves
    sets = [[0], [n - 1], [n - 2, n - 1],                         # one leaf, the last leaf, two siblings (their parent is computed once)
            [n - 1, 0] if n == 2 else [n // 2 + 1, n // 2 - 2 if n > 4 else 0],      # one leaf in either half, not in ascending order
            list(range(n))[::-1]]                                 # every leaf
    if log_leaves >= 8:
        sets.append(random.Random(37).sample(range(n), 37))
    return sets


def check_updates(make_tree, log_leaves, sets, seed, also=None):
    """after every update the whole node array equals that of a fresh build (make_tree, and `also` when given) over the modified leaves"""
    rnd = random.Random(seed)
    leaves = random_leaves(log_leaves, seed)
    tree = make_tree(leaves)
    for indices in sets:
        new = [(rnd.randrange(P), rnd.randrange(P)) for _ in indices]
        tree.update(indices, new)
        for i, v in zip(indices, new):
            leaves[i] = v
        for build in (make_tree, also) if also else (make_tree,):
            fresh = build(leaves)
            assert np.array_equal(all_nodes(tree), all_nodes(fresh)), (log_leaves, indices[:8], build)
            assert tree.root == fresh.root
            fresh.close()
    tree.close()


def check_rejections(make_tree, log_leaves):
    """every argument error returns DST_ERR_ARG and leaves every node as it was; count = 0 is a no-op"""
    import distaff_amd as D
    n = 1 << log_leaves
    tree = make_tree(random_leaves(log_leaves, 5))
    before = all_nodes(tree).tobytes()
    for indices, new in (([1, 0, 1], [(1, 2), (3, 4), (5, 6)]),           # a repeated index
                         ([0, n], [(1, 2), (3, 4)]),                      # an index = 2^log_leaves
                         ([n - 1, 1 << 40], [(1, 2), (3, 4)]),
                         ([0, 1], [(1, 2), (3, P)]),                      # an element equal to p
                         ([1], [(2 ** 128 - 1, 0)])):
        with pytest.raises(D.DistaffError) as e:
            tree.update(indices, new)
        assert e.value.code == D.DST_ERR_ARG, (indices, new)
        assert all_nodes(tree).tobytes() == before, (indices, new)
    idx, leaf = (ctypes.c_uint64 * 1)(0), ctypes.create_string_buffer(32)
    assert tree.lib.dst_rtree_update(tree._h, None, leaf, ctypes.c_size_t(1)) == D.DST_ERR_ARG
    assert tree.lib.dst_rtree_update(tree._h, idx, None, ctypes.c_size_t(1)) == D.DST_ERR_ARG
    assert tree.lib.dst_rtree_update(None, idx, leaf, ctypes.c_size_t(1)) == D.DST_ERR_ARG
    assert all_nodes(tree).tobytes() == before
    tree.update([], [])
    assert tree.lib.dst_rtree_update(tree._h, None, None, ctypes.c_size_t(0)) == D.DST_OK
    assert all_nodes(tree).tobytes() == before
    with pytest.raises(D.DistaffError):
        tree.update([0, 1], [(1, 2)])
    tree.close()


def check_batched_openings(tree, indices):
    """paths / tapes_many equal the concatenation of the single-index calls, the nodes of the node array at the path's positions (leaf
    2^L + i, then p ^ 1 while p >>= 1) and the tapes restated from those paths; an index past the end is an argument error"""
    import distaff_amd as D
    paths = tree.paths(indices)
    assert paths == [tree.path(i) for i in indices]
    v = D.arr_to_ints(tree.nodes(0, 2 << tree.log_leaves))
    node = [(v[2 * k], v[2 * k + 1]) for k in range(2 << tree.log_leaves)]
    for i, path in zip(indices, paths):
        p = (1 << tree.log_leaves) + i
        want = [node[p]]
        while p > 1:
            want.append(node[p ^ 1])
            p >>= 1
        assert path == want, i
    for what in (1, 2, 3):
        assert tree.tapes_many(indices, what) == [tree.tapes(i, what) for i in indices], what
    assert tree.tapes_many(indices, 3) == [tapes_from_path(path, i) for i, path in zip(indices, paths)]
    assert tree.paths([]) == [] and tree.tapes_many([]) == []
    for call in (tree.paths, tree.tapes_many):
        with pytest.raises(D.DistaffError) as e:
            call([0, 1 << tree.log_leaves])
        assert e.value.code == D.DST_ERR_ARG
    with pytest.raises(D.DistaffError):
        tree.tapes_many([0], what=4)
    n = ctypes.c_size_t(0)
    idx, buf = (ctypes.c_uint64 * 1)(0), ctypes.create_string_buffer(16 * 3 * (tree.log_leaves + 1))
    assert tree.lib.dst_rtree_paths(tree._h, None, ctypes.c_size_t(1), buf) == D.DST_ERR_ARG
    assert tree.lib.dst_rtree_paths(tree._h, idx, ctypes.c_size_t(1), None) == D.DST_ERR_ARG
    assert tree.lib.dst_rtree_tapes_many(tree._h, idx, ctypes.c_size_t(1), 3, buf, None, ctypes.c_size_t(100), ctypes.byref(n)) == D.DST_ERR_ARG
    assert tree.lib.dst_rtree_tapes_many(tree._h, idx, ctypes.c_size_t(1), 3, buf, buf, ctypes.c_size_t(2), ctypes.byref(n)) == D.DST_ERR_ARG      # too small
    assert n.value == 3 * (tree.log_leaves + 1) - 2


@pytest.mark.parametrize("log_leaves", [1, 3, 8])
def test_updated_tree_equals_a_fresh_build(log_leaves):
    check_updates(host_tree, log_leaves, update_sets(log_leaves), 60 + log_leaves)


@pytest.mark.parametrize("log_leaves", [1, 3, 8])
def test_rejected_updates_leave_the_tree_unchanged(log_leaves):
    check_rejections(host_tree, log_leaves)


@pytest.mark.parametrize("log_leaves", [1, 3, 8])
def test_batched_openings_equal_the_single_index_calls(log_leaves):
    n = 1 << log_leaves
    tree = host_tree(random_leaves(log_leaves, 70 + log_leaves))
    rnd = random.Random(log_leaves)
    check_batched_openings(tree, [n - 1, 0, n - 1] + [rnd.randrange(n) for _ in range(9)])
    tree.update([n - 1], [(7, 8)])
    check_batched_openings(tree, [n - 1, 0])
    tree.close()


def test_host_tree_reports_no_device_time_and_the_package_lists_the_calls():
    import distaff_amd as D
    tree = host_tree([(1, 2), (3, 4)])
    tree.update([1], [(5, 6)])
    assert tree.update_ms == 0.0
    assert tree.path(1) == [(5, 6), (1, 2)]
    tree.close()
    assert {"dst_rtree_update", "dst_rtree_update_ms", "dst_rtree_paths", "dst_rtree_tapes_many"} <= set(D.EXPORTS)
