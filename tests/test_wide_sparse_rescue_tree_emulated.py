"""The wide instantiations of the sparse-tree and path-root kernels (rescue_stree_*_kernel<stree_wide>, rescue_path_root_*_kernel<stree_wide>,
kernels_hash.hip) and the device path of dst_wtree_* / dst_rescue_*_w on the host launch emulation: tests/emu/_build/libdistaff_emu.so with
device = 0.  No GPU.  The checks are those of tests/test_wide_sparse_rescue_tree_host.py -- the oracle's digest under merkle_root, the levels as
the sorted distinct prefixes -- at depths 65 and 127 with small key counts, and the emulated tree is held against the host tree node by node.
Launches of this size take the six-lane forms.  Both forms of the audit are forced the way tests/test_rescue_tree_restore_emulated.py forces the
narrow ones: a tree of fewer and a tree of more than 2^15 stored parents.  The one-lane level and path-root kernels need more than 2^15 parents
of ONE level, or as many chains -- millions of emulated digests -- and run in tests/test_wide_sparse_rescue_tree_gpu.py."""
import pytest

from test_rescue_tree_emulated import emu  # noqa: F401  (the fixture that builds and opens the emulated library)
from test_sparse_rescue_tree_host import NONZERO_EMPTY, random_pairs
from test_wide_sparse_rescue_tree_host import (BOUNDARY_SETS, boundary_keys, check_boundary_set, check_audit_reports_the_nearer_of_two_changed_nodes, check_tree_less_calls,
                                               check_tree_less_writes, figures, int_levels, some_absent)

SPREAD_MAX = 1 << 15                       # RESCUE_SPREAD_MAX: launches of more parents run the one-lane kernels


@pytest.fixture()
def make(emu):  # noqa: F811
    import distaff_amd as D
    return (lambda depth, empty=(0, 0): D.WideSparseRescueTree(depth, empty, device=0, lib=emu),
            lambda depth, empty=(0, 0): D.WideSparseRescueTree(depth, empty, device=-1, lib=emu))


@pytest.mark.parametrize("name", BOUNDARY_SETS)
@pytest.mark.parametrize("depth", [65, 127])
def test_the_boundary_sets_through_the_device_code_path(oracle, make, depth, name):
    empty = NONZERO_EMPTY if name in ("sibling-pair", "shared-top", "random-200") else (0, 0)
    check_boundary_set(oracle, make[0], depth, name, empty, 100 * depth + BOUNDARY_SETS.index(name), random_count=24)


@pytest.mark.parametrize("depth", [65, 127])
def test_set_apply_remove_compact_get_and_audit_equal_the_host_path(make, depth):
    emu_tree, host_tree = make
    keys = boundary_keys(depth, "random-200", 70 + depth, 20) + boundary_keys(depth, "equal-low-halves", depth) + boundary_keys(depth, "shared-top", depth)[:6]
    a, b = emu_tree(depth, NONZERO_EMPTY), host_tree(depth, NONZERO_EMPTY)
    ask = keys[:8] + some_absent(depth, keys, depth) + keys[:1]

    def same():
        assert int_levels(a) == int_levels(b) and a.root == b.root and figures(a) == figures(b)
        assert a.paths(ask) == b.paths(ask) and a.get(ask) == b.get(ask) and a.tapes_many(ask[:3]) == b.tapes_many(ask[:3])
        assert a.audit() is None and b.audit() is None
    same()                                                                          # no keys: the generation of zero nodes
    leaves = random_pairs(len(keys), depth)
    a.set(keys, leaves); b.set(keys, leaves)
    same()
    batch = [keys[0], ask[9], keys[0], keys[21], ask[9], keys[3]]
    values = random_pairs(5, depth + 1) + [NONZERO_EMPTY]
    assert a.apply(batch, values) == b.apply(batch, values)
    assert a.info()["last_digests"] > b.info()["last_digests"] > 0                  # a device tree counts the witnesses' digests too, as dst_stree_apply does
    a.set(keys[:1], values[:1]); b.set(keys[:1], values[:1])
    same()
    assert a.remove(keys[::3] + [ask[10]]) == b.remove(keys[::3] + [ask[10]])
    same()
    assert a.compact() == b.compact()
    same()
    a.close(); b.close()


@pytest.mark.parametrize("n", [65, 128])
def test_roots_and_verdicts_without_a_tree_through_the_device_code_path(oracle, make, emu, n):  # noqa: F811
    check_tree_less_calls(oracle, make[0], n, 500 + n, 0, emu, count=5)
    check_tree_less_writes(oracle, make[0], n, 600 + n, 0, emu)


@pytest.mark.parametrize("count,one_lane", [(30, False), (290, True)], ids=["six-lane", "one-lane"])
def test_both_audit_kernels_report_the_nearer_of_two_changed_nodes(make, count, one_lane):
    """depth 127: 30 random keys store fewer than 2^15 parents and 290 more (asserted), so the launcher takes rescue_stree_audit_spread_kernel
    and rescue_stree_audit_kernel, both over stree_wide.  One node of level 70 and one of level 3 are changed in place"""
    tree = make[0](127, NONZERO_EMPTY)
    tree.set(boundary_keys(127, "random-200", 127, count), random_pairs(count, 3))
    assert (tree.info()["nodes"] - tree.info()["keys"] > SPREAD_MAX) == one_lane
    check_audit_reports_the_nearer_of_two_changed_nodes(tree, thorough=not one_lane)
    tree.close()
