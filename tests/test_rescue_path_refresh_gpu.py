"""Following ordered writes with held paths on the GPU (rescue_path_root_spread_kernel<K, true>, rescue_path_root_kernel<K, true>,
rescue_path_refresh_kernel) through the library the session binds, on the witnesses of device trees.  The yardsticks are those of
tests/test_rescue_path_refresh_host.py, never the call under test: the tree's own paths after apply, the rule restated in Python over the oracle,
verify_paths.  Everything is bit-exact.  Every test has its own time limit and nothing is run twice."""
import numpy as np
import pytest

from test_rescue_path_refresh_host import (OK, P, check_edge_cases, check_last_wins, check_ordered_batches, check_rejections, check_single_writes, check_sparse_63,
                                           check_tampering, check_wide_127, example_lines, host_tree, raw_refresh, run_example, words_of, SENTINEL)
from test_rescue_path_verify_gpu import bound, device_sparse, device_tree, pairs_of, random_words
from test_rescue_tree_sequence_host import random_ops
from test_wide_sparse_rescue_tree_gpu import device_wide

pytestmark = pytest.mark.gpu
SPREAD_MAX = 1 << 15                       # RESCUE_SPREAD_MAX: launches of more chains run the one-lane kernel


@pytest.mark.timeout(120)
def test_every_single_write_refreshes_every_held_path(oracle):
    check_single_writes(0, bound(), device_tree, oracle, log_leaves=(1, 2, 3, 4, 5))


@pytest.mark.timeout(120)
def test_ordered_batches_with_repeats_follow_the_tree_and_change_one_position_per_write():
    check_ordered_batches(0, bound(), device_tree, log_leaves=(1, 2, 3, 4, 5))


@pytest.mark.timeout(120)
def test_the_last_write_under_a_sibling_subtree_wins(oracle):
    check_last_wins(0, bound(), device_tree, oracle)


@pytest.mark.timeout(120)
def test_sparse_depth_63_absent_inserted_and_emptied(oracle):
    check_sparse_63(0, bound(), device_sparse, oracle)


@pytest.mark.timeout(120)
def test_wide_depth_127_across_the_split_of_the_index_halves(oracle):
    check_wide_127(0, bound(), device_wide, oracle)


@pytest.mark.timeout(120)
def test_nothing_is_written_from_witnesses_that_do_not_hold():
    check_tampering(0, bound(), device_tree)


@pytest.mark.timeout(120)
def test_no_write_no_held_path_repeated_keys_and_in_place():
    check_edge_cases(0, bound(), device_tree)


@pytest.mark.timeout(120)
def test_what_is_refused():
    check_rejections(0, bound())


@pytest.mark.timeout(120)
def test_200_writes_span_25_workgroups_of_the_six_lane_form():
    """400 chains, 8 per workgroup, the 200 storing ones in workgroups 25 .. 49; a sparse depth-63 tree, 64 held keys, a quarter of them written"""
    import distaff_amd as D
    keys, new = random_ops(1 << 63, 200, 381)
    tree = device_sparse(63)
    initial = dict(zip(keys[:40], new[:40]))
    tree.set(list(initial), list(initial.values()))
    rng = np.random.default_rng(382)
    held_keys = keys[100:116] + [int(k) for k in rng.integers(0, 1 << 63, size=48)]
    before, held = tree.root, tree.paths(held_keys)
    paths, roots = tree.apply(keys, new)
    stats = {}
    first, why, after, got = D.refresh_paths(before, keys, paths, new, held_keys, held, roots, device=0, stats=stats)
    assert (first, why, after) == (-1, OK, tree.root) and stats["device_ms"] > stats["gather_ms"] > 0
    assert got == tree.paths(held_keys)
    assert D.verify_paths(after, got, held_keys, device=0) == (-1, OK)
    tree.close()


@pytest.mark.timeout(300)
def test_the_one_lane_form_stores_the_same_chain_nodes():
    """2^14 + 1 ordered writes with repeats on a tree of 8 leaves, all 8 held: 2 count > RESCUE_SPREAD_MAX chains at n = 4, three levels, two stored
    nodes per write.  Against the tree and against the host path, whose chains are those of the six-lane form's yardstick"""
    import distaff_amd as D
    count = SPREAD_MAX // 2 + 1
    rng = np.random.default_rng(383)
    every = list(range(8))
    indices = [int(i) for i in rng.integers(0, 8, size=count)]
    new = pairs_of(random_words(rng, (count,)))
    tree = device_tree(pairs_of(random_words(rng, (8,))))
    before, held = tree.root, words_of(tree.paths(every))
    paths, roots = tree.apply(indices, new)
    stats = {}
    first, why, after, got = D.refresh_paths(before, indices, paths, new, every, held, roots, device=0, stats=stats)
    assert (first, why, after) == (-1, OK, tree.root) and stats["device_ms"] > 0
    assert got == tree.paths(every)
    assert got == D.refresh_paths(before, indices, paths, new, every, held, roots, device=-1)[3]
    tree.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("where", ["witness", "held-path"])
def test_an_element_that_is_not_below_p_is_found_on_the_device_and_nothing_is_written(where):
    """p in the last element of the last node of the last witness (the chain launch reads it) or of the last held path (the gather reads it)"""
    import distaff_amd as D
    rng = np.random.default_rng(384)
    paths, held = random_words(rng, (5, 4)), random_words(rng, (3, 4))
    (paths if where == "witness" else held)[-1, -1, -1] = (P & (2 ** 64 - 1), P >> 64)
    code, first, why, after, out = raw_refresh(bound(), 0, (1, 2), [0, 7, 3, 3, 5], paths, pairs_of(random_words(rng, (5,))), None, [1, 6, 1], held)
    assert code == D.DST_ERR_ARG and "not below the modulus" in D.lib._rtree_error(bound())
    assert out.tobytes() == bytes([SENTINEL]) * out.nbytes


@pytest.mark.timeout(300)
def test_c_example_follows_two_batches_on_the_device(tmp_path):
    assert run_example(tmp_path, 0) == example_lines(host_tree)
