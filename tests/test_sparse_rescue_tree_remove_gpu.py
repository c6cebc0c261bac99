"""Deletion from sparse Rescue Merkle trees on the GPU (dst_stree_remove, dst_stree_compact, dst_stree_get: rescue_stree_carry_kernel and both
level kernels over the dirty lists of a removal, rescue_stree_empty_leaves_kernel, rescue_stree_get_kernel) through the library the session
binds.  Up to depth 20 the yardstick is the dense DEVICE tree over the same leaves after update(removed, empty), node by node; at depth 63 it is
the host sparse tree, which tests/test_sparse_rescue_tree_remove_host.py holds against the dense host tree.  Everything is bit-exact.  Every test
has its own time limit and nothing is run twice."""
import random

import numpy as np
import pytest

from test_sparse_rescue_tree_gpu import SPREAD_MAX, assert_levels_equal_dense, random_words
from test_sparse_rescue_tree_host import assert_same_levels, depth_63_keys, levels_of, random_pairs
from test_sparse_rescue_tree_remove_host import example_lines, run_example, surviving_ancestors

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(120)
def test_depth_12_remove_compact_and_get_equal_the_dense_device_tree_and_the_host_tree():
    import distaff_amd as D
    depth, n = 12, 1 << 12
    rnd = random.Random(1212)
    keys = set(range(2048, 2048 + 300)) | {k ^ b for k in rnd.sample(range(n), 100) for b in (0, 1, 2, 3)}      # clusters ...
    while len(keys) < 1500:
        keys.add(rnd.randrange(n))                                                                              # ... and random keys
    keys = list(keys)
    rnd.shuffle(keys)
    new = random_words(len(keys), 1213)
    leaves = np.zeros((n, 2, 2), dtype=np.uint64)
    leaves[np.array(keys)] = new
    never = sorted(set(range(n)) - set(keys))
    gone = keys[:500]
    asked = gone + never[:40]
    rnd.shuffle(asked)
    rest = keys[500:]
    empties = np.zeros((len(asked), 2, 2), dtype=np.uint64)
    tree, host, dense = D.SparseRescueTree(depth, device=0), D.SparseRescueTree(depth, device=-1), D.RescueTree(leaves, device=0)
    for t in (tree, host):
        t.set(keys, new)
    assert tree.remove(asked) == host.remove(asked) == len(gone)
    dense.update(asked, empties)
    every = list(range(n))

    def check(remaining):
        assert_levels_equal_dense(tree, dense, remaining)
        assert_same_levels(levels_of(tree), levels_of(host))
        assert tree.paths(every) == dense.paths(every)                              # all 4 096 indices, the removed and the never-stored included
        assert (tree.info()["keys"], tree.info()["nodes"]) == (host.info()["keys"], host.info()["nodes"])

    assert tree.info()["last_digests"] == host.info()["last_digests"] == surviving_ancestors(keys, asked, depth)
    check(rest)
    # a witnessed deletion of 200 more keys and of 10 that were never stored: apply of empties, then compact
    hollow = rest[:200] + never[40:50]
    before = tree.root
    paths, roots = tree.apply(hollow, np.zeros((len(hollow), 2, 2), dtype=np.uint64))
    assert D.verify_writes(before, hollow, paths, [(0, 0)] * len(hollow), roots, device=0) == (-1, 0, tree.root)
    dense.update(hollow, np.zeros((len(hollow), 2, 2), dtype=np.uint64))
    host.set(hollow, [(0, 0)] * len(hollow))
    assert tree.info()["keys"] == len(rest) + 10
    assert tree.compact() == host.compact() == len(hollow)
    assert tree.info()["last_digests"] == 0
    check(rest[200:])
    # get: stored, removed by either way, never stored, repeats -- the dense tree's leaves, and the stored flags
    ask = rest[200:260] + gone[:30] + hollow[:30] + never[100:120] + [rest[200]] * 3 + [0, n - 1]
    kept = set(rest[200:])
    got, stored = tree.get_words(ask)
    assert np.array_equal(got, dense.nodes(n, n)[np.array(ask)]) and [bool(s) for s in stored] == [k in kept for k in ask]
    assert tree.get(ask) == host.get(ask)
    tree.close(); host.close(); dense.close()


@pytest.mark.timeout(180)
def test_depth_20_the_one_lane_level_kernel_runs_over_the_dirty_list_of_a_removal():
    """2^19 random keys, the first 2^18 of them removed: levels 19 .. 16 keep 65 458, 112 409, 105 326 and 64 167 touched parents -- more than
    2^15, so the one-lane kernel runs over a dirty list that is not the whole level -- and the levels from 15 up are narrow (the six-lane
    form); 163 890 nodes of level 19 are pruned.  Every stored node equals the dense device tree of 2^20 leaves after update(removed, empty)."""
    import distaff_amd as D
    depth, n = 20, 1 << 20
    perm = np.random.default_rng(2020).permutation(n).astype(np.uint64)
    keys, gone, rest = perm[:1 << 19], perm[:1 << 18], perm[1 << 18:1 << 19]
    at = lambda k, l: np.unique(k >> np.uint64(depth - l))  # noqa: E731
    dirty = [np.intersect1d(at(gone, l), at(rest, l)).size for l in range(depth)]
    assert any(d > SPREAD_MAX for d in dirty) and any(0 < d <= SPREAD_MAX for d in dirty)      # both level kernels, whatever the seed
    assert dirty[19:15:-1] == [65458, 112409, 105326, 64167] and dirty[15] <= SPREAD_MAX
    assert all(dirty[l] < at(rest, l).size for l in range(16, depth))                          # dirty lists, not whole levels
    assert at(keys, 19).size - at(rest, 19).size == 163890
    new = random_words(keys.size, 2021)
    leaves = np.zeros((n, 2, 2), dtype=np.uint64)
    leaves[keys.astype(np.int64)] = new
    tree, dense = D.SparseRescueTree(depth, device=0), D.RescueTree(leaves, device=0)
    tree.set(keys, new)
    nodes = tree.info()["nodes"]
    assert tree.remove(gone) == gone.size
    dense.update(gone, np.zeros((gone.size, 2, 2), dtype=np.uint64))
    info = tree.info()
    assert info["last_digests"] == sum(dirty) and info["keys"] == rest.size and info["last_device_ms"] > 0
    assert info["nodes"] == sum(at(rest, l).size for l in range(depth + 1)) < nodes
    assert_levels_equal_dense(tree, dense, rest)
    ask = [int(gone[0]), int(rest[0]), int(perm[-1]), 0, n - 1]
    assert tree.paths(ask) == dense.paths(ask)
    got, stored = tree.get_words(ask)
    assert np.array_equal(got, dense.nodes(n, n)[np.array(ask)]) and list(stored[:3]) == [0, 1, 0]
    tree.close(); dense.close()


@pytest.mark.timeout(120)
def test_depth_63_equals_the_host_tree_on_stored_removed_and_never_stored_keys():
    import distaff_amd as D
    keys = depth_63_keys(6363)
    gone, rest = keys[:20], keys[20:]
    leaves = random_pairs(len(keys), 6364)
    tree, host = D.SparseRescueTree(63, device=0), D.SparseRescueTree(63, device=-1)
    for t in (tree, host):
        t.set(keys, leaves)
    never = [keys[0] ^ 2, keys[30] ^ (1 << 62), 12345]
    assert not set(never) & set(keys)
    assert tree.remove(gone + never[:1]) == host.remove(gone + never[:1]) == 20
    assert_same_levels(levels_of(tree), levels_of(host))
    assert tree.root == host.root and tree.info()["last_digests"] == host.info()["last_digests"] == surviving_ancestors(keys, gone, 63)
    assert (tree.info()["keys"], tree.info()["nodes"]) == (44, host.info()["nodes"])
    ask = rest[:8] + gone[:8] + never + [rest[0]]
    got = tree.get(ask)
    assert tree.paths(ask) == host.paths(ask) and got == host.get(ask)
    assert got[1] == [True] * 8 + [False] * 11 + [True]
    tree.close(); host.close()


@pytest.mark.timeout(120)
def test_churn_returns_the_node_count_and_the_root_every_round():
    """ten rounds of set 256 keys, remove the same 256, on one device tree that keeps 100 keys throughout"""
    import distaff_amd as D
    rng = np.random.default_rng(77)
    base = np.unique(rng.integers(0, 1 << 63, size=100, dtype=np.uint64))
    tree = D.SparseRescueTree(63, device=0)
    tree.set(base, random_words(base.size, 78))
    root, nodes = tree.root, tree.info()["nodes"]
    for r in range(10):
        batch = np.setdiff1d(np.unique(rng.integers(0, 1 << 63, size=256, dtype=np.uint64)), base)
        tree.set(batch, random_words(batch.size, 100 + r))
        assert tree.info()["nodes"] > nodes and tree.root != root
        assert tree.remove(batch) == batch.size
        assert tree.info()["nodes"] == nodes and tree.info()["keys"] == base.size and tree.root == root, r
    tree.close()


@pytest.mark.timeout(300)
def test_c_example_prints_the_same_roots_on_the_device_and_on_the_host(tmp_path):
    """examples/merkle_remove.c compiles as C99 against include/distaff_hip.h and the product library; device 0 and the host print the same
    lines, which are what the binding computes"""
    import distaff_amd as D
    on_device = run_example(tmp_path, 1000, 300, 0)
    assert on_device == run_example(tmp_path, 1000, 300, -1)
    assert on_device == example_lines(lambda depth: D.SparseRescueTree(depth, device=0), 1000, 300)
