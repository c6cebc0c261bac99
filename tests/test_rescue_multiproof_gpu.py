"""Multiproofs on the GPU (rescue_multiproof_level_spread_kernel, rescue_multiproof_level_kernel, rescue_stree_lookup_kernel and the gathers)
through the library the session binds, on device trees.  The yardsticks are those of tests/test_rescue_multiproof_host.py: the trees' own paths
and roots, and the definition restated in Python.  Everything is bit-exact.  Every test has its own time limit and nothing is run twice."""
import random

import numpy as np
import pytest

from test_rescue_multiproof_host import (check_d3_table, check_rejections, check_tree, example_lines, random_nodes, restate, run_example)
from test_rescue_path_verify_gpu import SPREAD_MAX, bound, device_sparse, device_tree, pairs_of, random_words
from test_rescue_tree_host import P, random_leaves
from test_sparse_rescue_tree_host import NONZERO_EMPTY

pytestmark = pytest.mark.gpu
P_WORDS = (P & (2 ** 64 - 1), P >> 64)


def one_lane_indices():
    """2j for j < RESCUE_SPREAD_MAX + 64, plus 5 and 2 RESCUE_SPREAD_MAX + 1: the parents of the leaf level are more jobs than the spread form
    takes, and both kinds of job occur there -- two members of the set, and a member with a supplied sibling on either side"""
    return [2 * j for j in range(SPREAD_MAX + 64)] + [5, 2 * SPREAD_MAX + 1]


@pytest.mark.timeout(120)
def test_the_reference_cases_of_depth_3_by_heap_position():
    check_d3_table(0, bound(), device_tree)


@pytest.mark.timeout(120)
def test_six_lane_form_on_a_dense_tree_of_2_10_leaves_with_200_indices():
    """the multiproof is the restatement over the tree's paths, verifies, expands into the tree's paths; a tampered node gives ok = 0; other
    leaves over the same nodes give the root after the update"""
    indices = random.Random(401).sample(range(1 << 10), 200)
    check_tree(0, bound(), device_tree(random_leaves(10, 402)), indices, 10, 403, update=True)


@pytest.mark.timeout(120)
def test_six_lane_form_on_a_sparse_depth_63_tree_with_200_stored_and_50_absent_keys():
    rnd = random.Random(404)
    stored = sorted({rnd.randrange(1 << 63) for _ in range(300)} | {0, (1 << 63) - 1})[:300]
    tree = device_sparse(63, NONZERO_EMPTY)
    tree.set(stored, random_nodes(len(stored), 405))
    absent = sorted(({k ^ 1 for k in stored[:25]} | {rnd.randrange(1 << 63) for _ in range(25)}) - set(stored))
    keys = rnd.sample(stored, 200) + absent
    assert len(absent) == 50
    rnd.shuffle(keys)
    check_tree(0, bound(), tree, keys, 63, 406)


@pytest.mark.timeout(180)
def test_one_lane_form_on_a_dense_tree_of_2_17_leaves():
    """level 16 has more jobs than RESCUE_SPREAD_MAX: the root is the tree's, the digest count the restatement's, and the expansion of the
    first, the last and 64 random indices equals dst_rtree_paths"""
    import distaff_amd as D
    rng = np.random.default_rng(407)
    tree = D.RescueTree(random_words(rng, (1 << 17,)), device=0)
    indices = one_lane_indices()
    supplied, digests = restate(indices, 17)
    assert len({i >> 1 for i in indices}) > SPREAD_MAX
    leaves, nodes = tree.multiproof(indices, words=True)
    assert nodes.shape[0] == len(supplied)
    stats = {}
    assert D.multiproof_root(18, indices, leaves, nodes, device=0, stats=stats) == tree.root
    assert stats["digests"] == digests and stats["device_ms"] > 0
    paths, root = D.multiproof_paths(18, indices, leaves, nodes, device=0, words=True)
    assert root == tree.root
    some = [0, len(indices) - 1] + [int(j) for j in rng.integers(0, len(indices), size=64)]
    want = tree.paths([indices[j] for j in some])
    assert [pairs_of(paths[j]) for j in some] == want
    leaves[len(indices) // 2, 0, 0] ^= np.uint64(1)
    assert D.verify_multiproof(tree.root, 18, indices, leaves, nodes, device=0) is False
    tree.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("where", ["leaves", "nodes"])
@pytest.mark.parametrize("shape", ["six-lane", "one-lane"])
def test_an_element_that_is_not_below_p_is_found_on_the_device(shape, where):
    """p in one element of a leaf or of a supplied node, at 5 indices and at the one-lane shape, where the leaf and the first supplied node are
    read by the one-lane kernel: DST_ERR_ARG from all three calls, nothing else is wrong with the arguments"""
    import distaff_amd as D
    rng = np.random.default_rng(408)
    n, indices = (18, one_lane_indices()) if shape == "one-lane" else (11, [3, 1000, 1001, 512, 77])
    m, _ = D.multiproof_size(n, indices)
    leaves, nodes = random_words(rng, (len(indices),)), random_words(rng, (m,))
    D.multiproof_root(n, indices, leaves, nodes, device=0)
    bent = leaves if where == "leaves" else nodes
    bent[0 if shape == "one-lane" else -1, 1] = P_WORDS
    for call in (lambda: D.multiproof_root(n, indices, leaves, nodes, device=0), lambda: D.verify_multiproof((1, 2), n, indices, leaves, nodes, device=0),
                 lambda: D.multiproof_paths(n, indices, leaves, nodes, device=0, words=True)):
        with pytest.raises(D.DistaffError) as e:
            call()
        assert e.value.code == D.DST_ERR_ARG and "not below the modulus" in e.value.reason


@pytest.mark.timeout(120)
def test_device_and_host_give_identical_bytes():
    """the same inputs -- random nodes, no tree needed -- through device 0 and device -1: root, digest count and every expanded path"""
    import distaff_amd as D
    rng = np.random.default_rng(409)
    rnd = random.Random(410)
    for n, indices in ((11, rnd.sample(range(1 << 10), 200)), (64, [0, 1, 1 << 62, (1 << 63) - 1] + [rnd.randrange(1 << 63) for _ in range(20)]), (2, [1]), (2, [1, 0])):
        m, digests = D.multiproof_size(n, indices)
        leaves, nodes = random_words(rng, (len(indices),)), random_words(rng, (m,))
        on_device, on_host = {}, {}
        assert D.multiproof_root(n, indices, leaves, nodes, device=0, stats=on_device) == D.multiproof_root(n, indices, leaves, nodes, device=-1, stats=on_host)
        assert on_device["digests"] == on_host["digests"] == digests
        got, root = D.multiproof_paths(n, indices, leaves, nodes, device=0, words=True)
        want, want_root = D.multiproof_paths(n, indices, leaves, nodes, device=-1, words=True)
        assert root == want_root and got.tobytes() == want.tobytes()


@pytest.mark.timeout(120)
def test_what_is_refused_and_the_trees_stay_unchanged():
    check_rejections(0, bound(), device_tree, device_sparse)


@pytest.mark.timeout(300)
def test_c_example_takes_verifies_and_expands_a_multiproof_on_the_device(tmp_path):
    assert run_example(tmp_path, 12, 500, 0) == example_lines(12, 500)
