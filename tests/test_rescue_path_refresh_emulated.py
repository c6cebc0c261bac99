"""The storing six-lane chain kernel (rescue_path_root_spread_kernel<K, true>), the gather (rescue_path_refresh_kernel) and the device path of
dst_rescue_refresh_paths / dst_rescue_refresh_paths_w on the host launch emulation: tests/emu/_build/libdistaff_emu.so with device = 0, against the
yardsticks of tests/test_rescue_path_refresh_host.py (the tree's own paths after apply, the rule restated in Python over the oracle, verify_paths).
No GPU.  This pins which lanes store which chain node where, that the nodes follow the roots in one buffer, the gather's indexing for both key widths,
the `bad` word of both launches and the all-or-nothing rule for out_paths; launches of this size never reach the one-lane kernel, which
tests/test_rescue_path_refresh_gpu.py drives.  The trees whose witnesses are followed are host trees of the product library: what is emulated is
the follower."""
from test_rescue_path_refresh_host import (check_edge_cases, check_last_wins, check_ordered_batches, check_rejections, check_single_writes, check_sparse_63, check_tampering,
                                           check_wide_127, host_sparse, host_tree, host_wide)
from test_rescue_tree_emulated import emu  # noqa: F401  (the fixture that builds and opens the emulated library)


def test_every_single_write_refreshes_every_held_path(oracle, emu):  # noqa: F811
    check_single_writes(0, emu, host_tree, oracle)


def test_ordered_batches_with_repeats_follow_the_tree_and_change_one_position_per_write(emu):  # noqa: F811
    check_ordered_batches(0, emu, host_tree)


def test_the_last_write_under_a_sibling_subtree_wins(oracle, emu):  # noqa: F811
    check_last_wins(0, emu, host_tree, oracle)


def test_sparse_depth_63_absent_inserted_and_emptied(oracle, emu):  # noqa: F811
    check_sparse_63(0, emu, host_sparse, oracle)


def test_wide_depth_127_across_the_split_of_the_index_halves(oracle, emu):  # noqa: F811
    check_wide_127(0, emu, host_wide, oracle)


def test_nothing_is_written_from_witnesses_that_do_not_hold(emu):  # noqa: F811
    check_tampering(0, emu, host_tree)


def test_no_write_no_held_path_repeated_keys_and_in_place(emu):  # noqa: F811
    check_edge_cases(0, emu, host_tree)


def test_what_is_refused(emu):  # noqa: F811
    check_rejections(0, emu)
