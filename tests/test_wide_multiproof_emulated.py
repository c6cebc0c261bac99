"""The device code path of the wide multiproofs and of dst_wtree_load on the host launch emulation (tests/emu/_build/libdistaff_emu.so, device =
0): both tree-side launches of dst_wtree_multiproof (rescue_stree_locate_kernel<stree_wide>, rescue_stree_pack_kernel -- LDS and barriers only,
which the emulation runs), the level launches of the checks over pools with an E table, the gather launch of the expansion, and the uploads of a
load.  No GPU.  Depths 65 and 127 with at most a dozen keys; the checks are those of tests/test_wide_multiproof_host.py and
tests/test_wide_tree_restore_host.py, and every output is also held against the host path of the same library."""
import pytest

from test_rescue_tree_emulated import emu  # noqa: F401  (the fixture that builds and opens the emulated library)
from test_sparse_rescue_tree_host import NONZERO_EMPTY, random_pairs
from test_wide_multiproof_host import check_empty_tree, check_stored_empty_value
from test_wide_sparse_rescue_tree_host import boundary_keys, int_levels, some_absent


@pytest.fixture()
def make(emu):  # noqa: F811
    import distaff_amd as D
    return (lambda depth, empty=(0, 0): D.WideSparseRescueTree(depth, empty, device=0, lib=emu),
            lambda depth, empty=(0, 0): D.WideSparseRescueTree(depth, empty, device=-1, lib=emu))


@pytest.mark.parametrize("depth", [65, 127])
def test_proofs_checks_expansion_and_load_equal_the_host_path(make, emu, depth):  # noqa: F811
    import distaff_amd as D
    n = depth + 1
    keys = list(dict.fromkeys(boundary_keys(depth, "random-200", depth, 8) + boundary_keys(depth, "equal-low-halves", depth + 1)))
    values = random_pairs(len(keys), depth)
    a, b = make[0](depth, NONZERO_EMPTY), make[1](depth, NONZERO_EMPTY)
    a.set(keys, values); b.set(keys, values)
    ask = keys[:6] + some_absent(depth, keys, depth)[:6]
    table = D.empty_nodes(n, NONZERO_EMPTY, lib=emu)
    for compact in (True, False):
        proof = a.batch_proof(ask, compact=compact)
        assert proof == b.batch_proof(ask, compact=compact)
        proof = proof + ((table,) if compact else (None,))
        on_device, on_host = {}, {}
        assert D.multiproof_root_wide(n, ask, *proof, device=0, lib=emu, stats=on_device) == D.multiproof_root_wide(n, ask, *proof, device=-1, lib=emu, stats=on_host) == b.root
        assert (on_device["digests"], on_device["levels"]) == (on_host["digests"], on_host["levels"])
        assert D.multiproof_paths_wide(n, ask, *proof, device=0, lib=emu) == (b.paths(ask), b.root)
        assert D.verify_multiproof_wide(b.root, n, ask, *proof, device=0, lib=emu)
        bent = [(proof[0][0][0] ^ 1, proof[0][0][1])] + proof[0][1:]
        assert not D.verify_multiproof_wide(b.root, n, ask, bent, *proof[1:], device=0, lib=emu)
    blob = a.to_blob()
    assert blob == b.to_blob()
    loaded = D.WideSparseRescueTree.from_blob(blob, device=0, audit=True, lib=emu)
    assert int_levels(loaded) == int_levels(b) and loaded.root == b.root and loaded.batch_proof(ask) == b.batch_proof(ask)
    loaded.set(ask[-1:], [(5, 6)]); b.set(ask[-1:], [(5, 6)])
    assert loaded.root == b.root and loaded.audit() is None
    a.close(); b.close(); loaded.close()


def test_an_empty_tree_and_a_stored_empty_value_through_the_device_code_path(make, emu):  # noqa: F811
    import distaff_amd as D
    check_empty_tree(D, make[0], emu, 0)
    check_stored_empty_value(D, make[0], emu, 0)
