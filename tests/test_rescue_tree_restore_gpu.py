"""Save, restore and audit of the Rescue Merkle trees on the GPU (dst_rtree_save / load / audit, dst_stree_save / load / audit:
rescue_tree_audit_kernel, rescue_stree_audit_kernel and their six-lane forms, one launch per audit) through the library the session binds and the
checks of tests/test_rescue_tree_restore_host.py; the other side is the host path of the same library, which the host tests hold against the
trees' own yardsticks.  Everything is bit-exact.  Parent counts up to 2^15 take the six-lane form and 2^13 leaves are 8 191 parents, so the
one-lane forms run in two cases of their own: 2^16 dense leaves, and a depth-63 tree of 2 048 keys."""
import pytest

from test_rescue_tree_restore_host import (DENSE_LOGS, Side, check_argument_errors, check_dense_audit_names_the_parent, check_dense_round_trip, check_loaded_dense_lives,
                                           check_loaded_sparse_lives, check_one_lane_dense_audit, check_one_lane_sparse_audit, check_refusals, check_sparse_audit_names_the_parent, check_sparse_round_trip, example_lines,
                                           run_example, sparse_cases)

pytestmark = pytest.mark.gpu


def sides():
    import distaff_amd as D
    return Side(0, D.load()), Side(-1, D.load())


@pytest.mark.timeout(120)
@pytest.mark.parametrize("log_leaves", DENSE_LOGS)
def test_a_loaded_dense_tree_is_the_saved_tree(log_leaves):
    check_dense_round_trip(*sides(), log_leaves)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", sparse_cases(), ids=lambda c: "depth%d-%dkeys" % (c[0], len(c[2])))
def test_a_loaded_sparse_tree_is_the_saved_tree(case):
    check_sparse_round_trip(*sides(), case)


@pytest.mark.timeout(120)
def test_a_host_blob_loads_on_the_device_and_the_other_way_round():
    device, host = sides()
    check_dense_round_trip(host, device, 3)
    check_sparse_round_trip(host, device, sparse_cases()[1])


@pytest.mark.timeout(120)
def test_a_loaded_dense_tree_lives():
    check_loaded_dense_lives(sides()[0])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", sparse_cases(), ids=lambda c: "depth%d-%dkeys" % (c[0], len(c[2])))
def test_a_loaded_sparse_tree_lives(case):
    check_loaded_sparse_lives(sides()[0], case)


@pytest.mark.timeout(120)
def test_dense_audit_reports_the_parent_of_every_changed_node():
    check_dense_audit_names_the_parent(sides()[0])


@pytest.mark.timeout(180)
def test_sparse_audit_reports_the_parent_of_every_changed_node():
    check_sparse_audit_names_the_parent(sides()[0])


@pytest.mark.timeout(120)
def test_the_one_lane_dense_audit_finds_changed_nodes_among_65535_parents():
    """2^16 leaves: more parents than the six-lane form takes, so rescue_tree_audit_kernel runs -- on the clean tree, on single changed nodes,
    on two at once, and inside the load with audit"""
    device, _ = sides()
    check_one_lane_dense_audit(device, device, thorough=True)


@pytest.mark.timeout(120)
def test_the_one_lane_sparse_audit_finds_changed_nodes_in_a_depth_63_tree_of_2048_keys():
    """about 1.1e5 stored parents: rescue_stree_audit_kernel, the kernel that audits every tree of real size -- its level from the level table,
    its key, its comparison -- on the clean tree, on a changed leaf, mid-level node and root, on two at once, and inside the load with audit"""
    device, _ = sides()
    check_one_lane_sparse_audit(device, device, 2048, thorough=True)


@pytest.mark.timeout(120)
def test_malformed_blobs_and_bad_arguments_are_refused_on_the_device():
    check_refusals(sides()[0])
    check_argument_errors(sides()[0])


@pytest.mark.timeout(300)
def test_c_example_prints_the_same_lines_on_the_device_and_on_the_host(tmp_path):
    """examples/merkle_restore.c compiles as C99 against include/distaff_hip.h and the product library; device 0 and the host print the same
    lines, which are what the binding computes"""
    on_device = run_example(tmp_path, 10, 0)
    assert on_device == run_example(tmp_path, 10, -1)
    assert on_device == example_lines(sides()[0], 10)
