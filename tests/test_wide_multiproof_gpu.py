"""Multiproofs and save / load of wide-key sparse Rescue trees on the GPU: rescue_stree_locate_kernel<stree_wide> and rescue_stree_pack_kernel
(the two tree-side launches of dst_wtree_multiproof), the level and gather kernels of the checks reading E-table pool entries, and dst_wtree_save
/ dst_wtree_load on a device tree, through the library the session binds.  Everything is bit-exact.  The yardstick is the host path of the same
library, which tests/test_wide_multiproof_host.py and tests/test_wide_tree_restore_host.py hold against the definition, the narrow tree and the
tree's own paths.  Every test has its own time limit and nothing is run twice."""
import numpy as np
import pytest

from test_sparse_rescue_tree_gpu import random_words
from test_sparse_rescue_tree_host import NONZERO_EMPTY, random_pairs
from test_wide_multiproof_host import check_case, check_empty_tree, check_refusals, check_stored_empty_value, supplied_positions
from test_wide_sparse_rescue_tree_host import BOUNDARY_SETS, boundary_keys, int_levels, some_absent
from test_wide_tree_restore_host import batch_example_lines, check_audit_on_load_names_the_node, check_round_trip, run_batch_example

pytestmark = pytest.mark.gpu
SPREAD_MAX = 1 << 15                       # RESCUE_SPREAD_MAX: levels of more jobs run the one-lane kernel
BLOCK = 256                                # RESCUE_LOCATE_BLOCK: nodes per block of the two tree-side launches


def device_wide(depth, empty=(0, 0)):
    import distaff_amd as D
    return D.WideSparseRescueTree(depth, empty, device=0)


def host_wide(depth, empty=(0, 0)):
    import distaff_amd as D
    return D.WideSparseRescueTree(depth, empty, device=-1)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", BOUNDARY_SETS)
def test_depth_127_proofs_from_the_device_tree_equal_the_host_trees_and_check_on_the_device(name):
    """the boundary sets plus 6 absent keys: compact and plain proofs byte-equal to the host tree's; root, paths and digests of the device checks
    equal the host path's"""
    import distaff_amd as D
    depth, n = 127, 128
    keys = boundary_keys(depth, name, 127000 + BOUNDARY_SETS.index(name), random_count=60)
    values = random_pairs(len(keys), 5)
    a, b = device_wide(depth, NONZERO_EMPTY), host_wide(depth, NONZERO_EMPTY)
    a.set(keys, values); b.set(keys, values)
    ask = list(dict.fromkeys(keys + some_absent(depth, keys, 9)))
    assert len(ask) >= len(keys) + 6
    table = D.empty_nodes(n, NONZERO_EMPTY)
    for compact in (True, False):
        got, want = a.batch_proof(ask, compact=compact, words=True), b.batch_proof(ask, compact=compact, words=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        proof = (got[0], got[1], got[2], table if compact else None)
        on_device, on_host = {}, {}
        assert D.multiproof_root_wide(n, ask, *proof, device=0, stats=on_device) == D.multiproof_root_wide(n, ask, *proof, device=-1, stats=on_host) == a.root == b.root
        assert (on_device["digests"], on_device["levels"]) == (on_host["digests"], on_host["levels"]) and on_device["device_ms"] > 0
        p0, r0 = D.multiproof_paths_wide(n, ask, *proof, device=0, words=True)
        assert r0 == a.root and np.array_equal(p0, b.paths_words(ask))
        assert D.verify_multiproof_wide(a.root, n, ask, *proof, device=0)
    a.close(); b.close()


@pytest.mark.timeout(120)
def test_every_property_of_one_key_set_through_the_device():
    import distaff_amd as D
    check_case(D, device_wide, D.load(), 127, "random-200", 0)
    check_case(D, device_wide, D.load(), 65, "equal-low-halves", 0)
    check_stored_empty_value(D, device_wide, D.load(), 0)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("count", [1, 3, 40], ids=["fewer-than-64-nodes", "more-than-one-block", "several-blocks"])
def test_the_tree_side_launches_at_block_boundaries(count):
    """m = count + M asked nodes: below 64, and across several blocks of 256 without being a multiple of it (asserted)"""
    depth = 127 if count > 1 else 40
    keys = boundary_keys(depth, "random-200", 77 + count, 50)
    a, b = device_wide(depth), host_wide(depth)
    values = random_pairs(len(keys), count)
    a.set(keys, values); b.set(keys, values)
    ask = keys[:count // 2 + 1] + some_absent(depth, keys, count)[2:2 + count // 2]      # the random absent keys, not the two siblings of stored ones
    m = len(ask) + len(supplied_positions(depth, ask))
    assert (m < 64) if count == 1 else (m > BLOCK * (1 if count == 3 else 3) and m % BLOCK != 0)
    for compact in (True, False):
        assert a.batch_proof(ask, compact=compact) == b.batch_proof(ask, compact=compact)
    a.close(); b.close()


@pytest.mark.timeout(60)
def test_an_absent_only_batch_in_an_empty_tree_launches_nothing():
    import distaff_amd as D
    check_empty_tree(D, device_wide, D.load(), 0)


@pytest.mark.timeout(300)
def test_a_level_of_more_jobs_than_the_six_lane_form_takes_reads_the_table():
    """2^15 + 1 stored keys at depth 65, asked together: their parents are more than RESCUE_SPREAD_MAX jobs of one level (asserted), which the
    one-lane kernel hashes, each from a leaf and -- the sibling of a random key is not stored -- the E-table entry of the leaf level.  The root
    is the device tree's, the digest count the plain one (every asked leaf is stored: no parent is known-empty)"""
    import distaff_amd as D
    depth, n = 65, 66
    rng = np.random.default_rng(65)
    raw = rng.integers(0, 1 << 63, size=((1 << 15) + 1, 2), dtype=np.uint64)
    raw[:, 1] &= np.uint64(1)                                                       # below 2^65
    ask = np.ascontiguousarray(np.unique(raw, axis=0))
    assert len(ask) == (1 << 15) + 1
    parents = np.stack([(ask[:, 0] >> np.uint64(1)) | (ask[:, 1] << np.uint64(63)), ask[:, 1] >> np.uint64(1)], axis=1)
    assert len(np.unique(parents, axis=0)) > SPREAD_MAX
    tree = device_wide(depth, NONZERO_EMPTY)
    tree.set(ask, random_words(len(ask), 651))
    leaves, nodes, bits = tree.batch_proof(ask, words=True)
    M, plain_digests = D.multiproof_size_wide(n, ask)
    absent = int(np.unpackbits(np.frombuffer(bits, dtype=np.uint8)).sum())
    assert absent > SPREAD_MAX // 2 and len(nodes) == M - absent                    # most leaf-level siblings are empty subtrees
    table = D.empty_nodes(n, NONZERO_EMPTY)
    s = {}
    assert D.multiproof_root_wide(n, ask, leaves, nodes, bits, table, device=0, stats=s) == tree.root
    assert s["digests"] == plain_digests and s["levels"] == depth
    plain = tree.batch_proof(ask, compact=False, words=True)
    assert D.multiproof_root_wide(n, ask, plain[0], plain[1], device=0) == tree.root
    bent = leaves.copy()
    bent[12345, 0, 0] ^= np.uint64(1)
    assert not D.verify_multiproof_wide(tree.root, n, ask, bent, nodes, bits, table, device=0)
    tree.close()


@pytest.mark.timeout(120)
def test_refusals_on_the_device_path():
    import distaff_amd as D
    check_refusals(D, device_wide, D.load(), 0)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["equal-low-halves", "random-200"])
def test_save_on_the_device_equals_save_on_the_host_and_load_restores_the_tree(name):
    import distaff_amd as D
    depth = 127
    keys = boundary_keys(depth, name, 31, 60)
    values = random_pairs(len(keys), 31)
    a, b = device_wide(depth, NONZERO_EMPTY), host_wide(depth, NONZERO_EMPTY)
    a.set(keys, values); b.set(keys, values)
    blob = a.to_blob()
    assert blob == b.to_blob()
    loaded = D.WideSparseRescueTree.from_blob(blob, device=0, audit=True)
    ask = keys[:9] + some_absent(depth, keys, 3)
    assert loaded.info()["device"] == 0 and loaded.audit() is None and int_levels(loaded) == int_levels(a) and loaded.root == a.root
    assert loaded.batch_proof(ask) == a.batch_proof(ask) == b.batch_proof(ask)
    a.close(); b.close(); loaded.close()
    check_round_trip(D, device_wide, lambda blob, audit: D.WideSparseRescueTree.from_blob(blob, device=0, audit=audit), 65, name)


@pytest.mark.timeout(120)
def test_audit_on_a_device_load_names_a_node_changed_in_the_blob():
    import distaff_amd as D
    check_audit_on_load_names_the_node(D, device_wide, lambda blob, audit: D.WideSparseRescueTree.from_blob(blob, device=0, audit=audit))


@pytest.mark.timeout(120)
def test_c_example_runs_on_the_device(oracle, tmp_path):
    assert run_batch_example(tmp_path, 40, 0) == batch_example_lines(oracle, 40)
