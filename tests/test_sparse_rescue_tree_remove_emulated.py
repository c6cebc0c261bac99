"""Deletion from sparse trees on the host launch emulation: tests/emu/_build/libdistaff_emu.so with device = 0 -- rescue_stree_get_kernel, the
leaf-flag kernel of compact, and the plan application without new leaves (carry-over and level launches over the dirty lists of a removal, a
next generation of zero nodes) -- against the host path of the same library.  No GPU.  After every remove, compact and get the two trees have
the same levels, roots, paths of every index, info() figures and get results."""
import random

import pytest

from test_rescue_tree_emulated import emu  # noqa: F401  (the fixture that builds and opens the emulated library)
from test_sparse_rescue_tree_host import NONZERO_EMPTY, assert_same_levels, depth_63_keys, levels_of, random_pairs
from test_sparse_rescue_tree_remove_host import check_apply_compact_equals_remove, check_removals, removal_cases, surviving_ancestors


@pytest.fixture()
def make(emu):  # noqa: F811
    import distaff_amd as D
    return (lambda depth, empty=(0, 0): D.SparseRescueTree(depth, empty, device=0, lib=emu),
            lambda depth, empty=(0, 0): D.SparseRescueTree(depth, empty, device=-1, lib=emu))


def assert_twins(a, b, ask):
    """the emulated device tree and the host tree: levels, root, the paths and the leaves of `ask`, the figures of info()"""
    assert_same_levels(levels_of(a), levels_of(b))
    assert a.root == b.root and a.paths(ask) == b.paths(ask) and a.get(ask) == b.get(ask)
    ia, ib = a.info(), b.info()
    assert [ia[f] for f in ("depth", "keys", "nodes", "last_digests")] == [ib[f] for f in ("depth", "keys", "nodes", "last_digests")]


def run_twins(a, b, stored, removals, empty, ask, seed):
    """set, then every removal; then some keys emptied by a set and by an apply, compact, get -- on both trees, compared after every step"""
    leaves = random_pairs(len(stored), seed)
    assert_twins(a, b, ask)                                                         # no keys: the generation of zero nodes
    a.set(stored, leaves); b.set(stored, leaves)
    assert_twins(a, b, ask)
    left = set(stored)
    for asked in removals:
        want = surviving_ancestors(left, asked, a.depth)
        assert a.remove(asked) == b.remove(asked) == len(left & set(asked))
        left -= set(asked)
        assert a.info()["last_digests"] == want
        assert_twins(a, b, ask)
    # what is left (or the first keys again, when nothing is): half of them emptied, a third of those through apply
    again = sorted(left) or stored[:3]
    for t in (a, b):
        t.set(again, random_pairs(len(again), seed + 1))
    hollow = again[::2]
    by_apply = hollow[::3]
    out_a = a.apply(by_apply, [tuple(empty)] * len(by_apply))
    out_b = b.apply(by_apply, [tuple(empty)] * len(by_apply))
    assert out_a == out_b
    for t in (a, b):
        t.set(hollow, [tuple(empty)] * len(hollow))
    assert_twins(a, b, ask)
    assert a.compact() == b.compact() == len(hollow)
    assert a.info()["last_digests"] == 0 and a.info()["keys"] == len(again) - len(hollow)
    assert_twins(a, b, ask)
    assert a.compact() == b.compact() == 0
    assert a.remove(again) == b.remove(again) == len(again) - len(hollow)            # down to zero nodes again
    assert a.info()["nodes"] == 0
    assert_twins(a, b, ask)


@pytest.mark.parametrize("depth", range(1, 7))
def test_remove_compact_and_get_equal_the_host_path(make, depth):
    emu_tree, host_tree = make
    empty = NONZERO_EMPTY if depth & 1 else (0, 0)
    every = list(range(1 << depth))
    for case, (stored, removals) in enumerate(removal_cases(depth, 1100 + depth)):
        a, b = emu_tree(depth, empty), host_tree(depth, empty)
        run_twins(a, b, stored, removals, empty, every + every[:2], 3000 * depth + case)
        a.close(); b.close()


@pytest.mark.parametrize("depth", [2, 5])
def test_emulated_removals_equal_a_fresh_emulated_tree(make, depth):
    """the host test's own sweep with the emulated device tree on both sides: a removal leaves what create + set of the rest builds"""
    emu_tree, _ = make
    for case, (stored, removals) in enumerate(removal_cases(depth, 1200 + depth)):
        check_removals(emu_tree, depth, NONZERO_EMPTY, stored, removals, 4000 * depth + case, dense=False)


def test_depth_63_with_four_keys_equals_the_host_path(make, emu):  # noqa: F811
    import distaff_amd as D
    emu_tree, host_tree = make
    keys = list(dict.fromkeys(depth_63_keys(7, 6)[:4] + [0]))[:4]
    k = keys[0]
    stored = keys + [k ^ 1]                                                          # a sibling pair among them
    ask = stored + [keys[1] ^ (1 << 62), 2 ** 63 - 2, k, k]
    a, b = emu_tree(63), host_tree(63)
    run_twins(a, b, stored, [[k], [k ^ 1, k, 5], [keys[1], keys[2]], stored], (0, 0), ask, 63)
    a.close(); b.close()
    check_apply_compact_equals_remove(emu_tree, 63, NONZERO_EMPTY, keys, keys[:2] + [12345], lambda *w: D.verify_writes(*w, device=-1, lib=emu))


def test_argument_errors_leave_the_emulated_tree_unchanged(make):
    import distaff_amd as D
    emu_tree, _ = make
    tree = emu_tree(6)
    tree.set([1, 2, 40], random_pairs(3, 5))
    before = [(p.tolist(), n.tolist()) for p, n in levels_of(tree)]
    for call in (lambda: tree.remove([1, 1]), lambda: tree.remove([64]), lambda: tree.get([64])):
        with pytest.raises(D.DistaffError) as e:
            call()
        assert e.value.code == D.DST_ERR_ARG
    assert tree.remove([]) == 0 and tree.remove([3, 63]) == 0 and tree.compact() == 0 and tree.get([]) == ([], [])
    assert [(p.tolist(), n.tolist()) for p, n in levels_of(tree)] == before
    tree.close()
