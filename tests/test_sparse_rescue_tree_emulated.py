"""The sparse-tree kernels' own source (rescue_stree_level_spread_kernel, rescue_stree_carry_kernel, rescue_stree_open_kernel and the scatter of
the new leaves, kernels_hash.hip) on the host launch emulation: tests/emu/_build/libdistaff_emu.so with device = 0, against the host path of the
same library.  No GPU.  This pins the child search, the default sides, the carry-over, the opening kernel and the six-lane form's indexing;
trees of this size never reach the one-lane level kernel, which tests/test_sparse_rescue_tree_gpu.py drives."""
import random

import pytest

from test_rescue_tree_emulated import emu  # noqa: F401  (the fixture that builds and opens the emulated library)
from test_sparse_rescue_tree_host import NONZERO_EMPTY, assert_same_levels, check_set_sequence, depth_63_keys, levels_of, random_pairs, set_sequence


@pytest.fixture()
def make(emu):  # noqa: F811
    import distaff_amd as D
    return (lambda depth, empty=(0, 0): D.SparseRescueTree(depth, empty, device=0, lib=emu),
            lambda depth, empty=(0, 0): D.SparseRescueTree(depth, empty, device=-1, lib=emu))


@pytest.mark.parametrize("depth", range(1, 7))
def test_random_subsets_and_a_set_sequence_equal_the_host_path(make, depth):
    emu_tree, host_tree = make
    rnd = random.Random(400 + depth)
    empty = NONZERO_EMPTY if depth & 1 else (0, 0)
    n = 1 << depth
    every = list(range(n))
    for count in sorted({1, max(1, n // 3), n}):
        keys = rnd.sample(range(n), count)
        leaves = random_pairs(count, 500 + depth)
        a, b = emu_tree(depth, empty), host_tree(depth, empty)
        assert a.root == b.root and a.paths(every) == b.paths(every)               # no keys: every node is a default
        a.set(keys, leaves); b.set(keys, leaves)
        assert_same_levels(levels_of(a), levels_of(b))
        assert a.root == b.root and a.paths(every + [keys[0]]) == b.paths(every + [keys[0]]) and a.tapes_many(every) == b.tapes_many(every)
        assert a.info()["last_digests"] == b.info()["last_digests"] and a.info()["nodes"] == b.info()["nodes"]
        a.close(); b.close()
    content = check_set_sequence(emu_tree, depth, set_sequence(depth, 600 + depth, empty), empty, also=host_tree)
    a, b = emu_tree(depth, empty), host_tree(depth, empty)
    for t in (a, b):
        t.set(list(content), list(content.values()))
    assert a.paths(every) == b.paths(every)
    a.close(); b.close()


def test_depth_63_with_four_keys_equals_the_host_path(make):
    emu_tree, host_tree = make
    keys = depth_63_keys(7, 6)[:4] + [0]
    keys = list(dict.fromkeys(keys))[:4]
    leaves = random_pairs(4, 8)
    a, b = emu_tree(63), host_tree(63)
    a.set(keys, leaves); b.set(keys, leaves)
    assert_same_levels(levels_of(a), levels_of(b))
    ask = keys + [keys[0] ^ 1, keys[1] ^ (1 << 62), 2 ** 63 - 2]
    assert a.root == b.root and a.paths(ask) == b.paths(ask) and a.tapes_many(ask, what=1) == b.tapes_many(ask, what=1)
    a.close(); b.close()
