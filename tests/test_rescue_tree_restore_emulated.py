"""Save, restore and audit on the host launch emulation: tests/emu/_build/libdistaff_emu.so with device = 0 -- the audit kernels' own source
(rescue_tree_audit_kernel, rescue_stree_audit_kernel and their six-lane forms: the level of a flat position from the level table, the search for
the children, the comparison, the atomicMin key; the one-lane forms in two cases above 2^15 parents) and the device side of load (the generation's layout, filled from the blob) -- through the checks of
tests/test_rescue_tree_restore_host.py, the host path of the same library being the other side.  No GPU."""
import pytest

from test_rescue_tree_emulated import emu  # noqa: F401  (the fixture that builds and opens the emulated library)
from test_rescue_tree_restore_host import (DENSE_LOGS, Side, check_argument_errors, check_dense_audit_names_the_parent, check_dense_round_trip, check_loaded_dense_lives,
                                           check_loaded_sparse_lives, check_one_lane_dense_audit, check_one_lane_sparse_audit, check_refusals, check_sparse_audit_names_the_parent, check_sparse_round_trip, sparse_cases)


@pytest.fixture()
def sides(emu):  # noqa: F811
    return Side(0, emu), Side(-1, emu)


@pytest.mark.parametrize("log_leaves", DENSE_LOGS)
def test_a_loaded_dense_tree_is_the_saved_tree(sides, log_leaves):
    check_dense_round_trip(*sides, log_leaves)


@pytest.mark.parametrize("case", sparse_cases(), ids=lambda c: "depth%d-%dkeys" % (c[0], len(c[2])))
def test_a_loaded_sparse_tree_is_the_saved_tree(sides, case):
    check_sparse_round_trip(*sides, case)


def test_a_host_blob_loads_on_the_emulated_device_and_the_other_way_round(sides):
    device, host = sides
    check_dense_round_trip(host, device, 3)
    check_sparse_round_trip(host, device, sparse_cases()[1])


def test_a_loaded_dense_tree_lives(sides):
    check_loaded_dense_lives(sides[0])


@pytest.mark.parametrize("case", sparse_cases(), ids=lambda c: "depth%d-%dkeys" % (c[0], len(c[2])))
def test_a_loaded_sparse_tree_lives(sides, case):
    check_loaded_sparse_lives(sides[0], case)


def test_dense_audit_reports_the_parent_of_every_changed_node(sides):
    check_dense_audit_names_the_parent(sides[0])


def test_sparse_audit_reports_the_parent_of_every_changed_node(sides):
    check_sparse_audit_names_the_parent(sides[0])


def test_the_one_lane_dense_audit_reports_the_nearer_of_two_changed_nodes(sides):
    """65 535 parents: the launcher takes rescue_tree_audit_kernel.  The host path builds and saves, the emulated device loads (no hashing) and
    audits once"""
    check_one_lane_dense_audit(sides[0], sides[1], thorough=False)


def test_the_one_lane_sparse_audit_reports_the_nearer_of_two_changed_nodes(sides):
    """depth 63 with 700 keys, more than 2^15 stored parents: the launcher takes rescue_stree_audit_kernel"""
    check_one_lane_sparse_audit(sides[0], sides[1], 700, thorough=False)


def test_malformed_blobs_are_refused_and_nothing_stays_allocated(sides, emu):  # noqa: F811
    """the emulation's ledger of live device allocations, events and streams: a refused load, and a load with audit that finds a bad node, leave
    nothing behind"""
    import ctypes
    import distaff_amd as D
    from test_rescue_tree_restore_host import HEADER, bump, random_words
    live = (ctypes.c_long * 5)()
    emu.emu_live_counts(live)
    before = list(live)
    check_refusals(sides[0])
    check_argument_errors(sides[0])
    tree = sides[0].dense(random_words(8, 900))
    blob = tree.save()
    tree.close()
    with pytest.raises(D.DistaffError):
        sides[0].load_dense(bump(blob, HEADER + 32 * 4), audit=True)
    emu.emu_live_counts(live)
    assert list(live) == before
