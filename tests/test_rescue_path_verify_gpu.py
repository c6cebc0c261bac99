"""Checking paths and witnesses on the GPU (rescue_path_root_spread_kernel, rescue_path_root_kernel) through the library the session binds.  The
yardstick is never one of the new calls: the reference's walk restated in Python (tests/test_rescue_path_verify_host.py) over the oracle and over
the existing host digests, and the roots that trees report.  Everything is bit-exact.  Every test has its own time limit and nothing is run twice."""
import numpy as np
import pytest

from test_rescue_path_verify_host import (BAD_ROOT, OK, P, check_path_roots, check_rejections, check_tampering, check_tree_paths, check_writes_of_apply, example_lines,
                                          flip, host_tree, merkle_roots_batched, random_paths, run_example)
from test_rescue_tree_sequence_host import random_ops

pytestmark = pytest.mark.gpu
SPREAD_MAX = 1 << 15                       # RESCUE_SPREAD_MAX: launches of more chains run the one-lane kernel


def device_tree(leaves):
    import distaff_amd as D
    return D.RescueTree(leaves, device=0)


def device_sparse(depth, empty=(0, 0)):
    import distaff_amd as D
    return D.SparseRescueTree(depth, empty, device=0)


def bound():
    import distaff_amd as D
    return D.load()


def random_words(rng, shape):
    """uint64 words [..., 2, 2] of elements below 2^127: below p"""
    w = rng.integers(0, 1 << 64, size=shape + (2, 2), dtype=np.uint64)
    w[..., 1] >>= np.uint64(1)
    return w


def pairs_of(words):
    import distaff_amd as D
    v = D.arr_to_ints(words)
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


@pytest.mark.timeout(120)
def test_path_roots_equal_the_reference_walk(oracle):
    check_path_roots(0, bound(), oracle)


@pytest.mark.timeout(120)
def test_200_paths_span_25_workgroups_of_the_six_lane_form():
    """8 chains per workgroup; n = 21; with and without substitute leaves, against the host's digests level by level"""
    import distaff_amd as D
    rng = np.random.default_rng(81)
    indices = [int(i) for i in rng.integers(0, 1 << 20, size=200)]
    paths = random_paths(200, 21, 82)
    subs = [node for node, in random_paths(200, 1, 83)]
    stats = {}
    assert D.path_roots(paths, indices, device=0, stats=stats) == merkle_roots_batched(paths, indices)
    assert stats["device_ms"] > 0
    assert D.path_roots(paths, indices, subs, device=0) == merkle_roots_batched(paths, indices, subs)


@pytest.mark.timeout(120)
def test_paths_of_dense_and_sparse_device_trees_resolve_to_their_roots():
    check_tree_paths(0, bound(), device_tree, device_sparse)


@pytest.mark.timeout(120)
def test_the_witnesses_of_apply_on_device_trees_are_accepted_and_the_state_is_followed():
    check_writes_of_apply(0, bound(), device_tree, device_sparse)


@pytest.mark.timeout(120)
def test_a_sparse_depth_63_witness_set_of_200_writes():
    """stored and new keys, repeats among them, from dst_stree_apply on a device tree: 400 chains of 63 digests in one launch"""
    import distaff_amd as D
    keys, new = random_ops(1 << 63, 200, 84)
    tree = device_sparse(63)
    initial = dict(zip(keys[:40], new[:40]))
    tree.set(list(initial), list(initial.values()))
    before = tree.root
    paths, roots = tree.apply(keys, new)
    stats = {}
    assert D.verify_writes(before, keys, paths, new, roots, device=0, stats=stats) == (-1, OK, tree.root)
    assert stats["device_ms"] > 0
    bent = [list(p) for p in paths]
    bent[137][40] = flip(bent[137][40], 1, 77)
    assert D.verify_writes(before, keys, bent, new, device=0)[:2] == (137, BAD_ROOT)
    tree.close()


@pytest.mark.timeout(120)
def test_each_single_tampering_is_found_at_its_write():
    check_tampering(0, bound(), device_tree)


@pytest.mark.timeout(120)
def test_what_is_refused():
    check_rejections(0, bound())


@pytest.mark.timeout(300)
def test_the_one_lane_kernel_on_more_paths_than_the_spread_form_takes():
    """2^15 + 64 distinct random paths with n = 3: two digests per chain, so the level loop runs; random indices 0 .. 3; every root against the
    host's digests, 65 664 of them in two batched calls"""
    import distaff_amd as D
    count = SPREAD_MAX + 64
    rng = np.random.default_rng(85)
    indices = [int(i) for i in rng.integers(0, 4, size=count)]
    words = random_words(rng, (count, 3))
    nodes = pairs_of(words)
    paths = [nodes[3 * i:3 * i + 3] for i in range(count)]
    stats = {}
    got = D.path_roots(words, indices, device=0, stats=stats)
    assert stats["device_ms"] > 0
    assert got == merkle_roots_batched(paths, indices)


@pytest.mark.timeout(300)
def test_the_one_lane_kernel_checks_old_and_new_leaves_in_one_launch():
    """2^14 + 32 ordered writes on a device tree of 4 leaves: 2^15 + 64 chains, own-leaf chains first, then substitute-leaf chains.  The tree
    says what the roots are; one flipped bit in write 2^14 is found there"""
    import distaff_amd as D
    count = SPREAD_MAX // 2 + 32
    rng = np.random.default_rng(86)
    indices = [int(i) for i in rng.integers(0, 4, size=count)]
    new = pairs_of(random_words(rng, (count,)))
    tree = device_tree(pairs_of(random_words(rng, (4,))))
    before = tree.root
    paths, roots = tree.apply(indices, new)
    stats = {}
    assert D.verify_writes(before, indices, paths, new, roots, device=0, stats=stats) == (-1, OK, tree.root)
    assert stats["device_ms"] > 0
    j = SPREAD_MAX // 2
    paths[j][2] = flip(paths[j][2], 0, 100)
    assert D.verify_writes(before, indices, paths, new, roots, device=0)[:2] == (j, BAD_ROOT)
    tree.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("count", [5, SPREAD_MAX + 3], ids=["six-lane", "one-lane"])
def test_an_element_that_is_not_below_p_is_found_on_the_device(count):
    """p in the last element of the last node of the last path, in both kernels' regimes"""
    import distaff_amd as D
    rng = np.random.default_rng(87)
    words = random_words(rng, (count, 3))
    indices = [int(i) for i in rng.integers(0, 4, size=count)]
    words[-1, -1, -1] = (P & (2 ** 64 - 1), P >> 64)
    with pytest.raises(D.DistaffError) as e:
        D.path_roots(words, indices, device=0)
    assert e.value.code == D.DST_ERR_ARG and "not below the modulus" in e.value.reason


@pytest.mark.timeout(300)
def test_c_example_checks_its_witnesses_on_the_device(tmp_path):
    assert run_example(tmp_path, 10, 40, 0) == example_lines(host_tree, 10, 40)
