"""Multiproofs of wide-key sparse Rescue trees, plain and compact (dst_wtree_multiproof, dst_rescue_empty_nodes, dst_rescue_multiproof_size_w and
the three dst_rescue_multiproof_*_w checks) on the host path (device = -1) of the PRODUCT library.  No GPU.  Everything is bit-exact.  The
yardsticks, none of them the code under test: the narrow tree's multiproof up to depth 63; the tree's own root and paths (which
tests/test_wide_sparse_rescue_tree_host.py holds against the oracle) above it; the definition of the supplied nodes and the known-empty rule,
restated here over Python ints; and the stored (level, prefix) set read back through level().  Also here: the helpers the emulated and the GPU
tests share."""
import ctypes
import os

import numpy as np
import pytest

from test_rescue_tree_host import _product
from test_sparse_rescue_tree_host import NONZERO_EMPTY, empty_chain, host_sparse, random_pairs
from test_wide_sparse_rescue_tree_host import BOUNDARY_SETS, boundary_keys, host_wide, int_levels, some_absent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = [1, 2, 63, 64, 65, 127]
P = (1 << 128) - 45 * (1 << 40) + 1


# ---- the definition, over Python ints ------------------------------------------------------------------------------------------------------------------
def supplied_positions(depth, keys):
    """(level, position) of the supplied nodes in proof order: level `depth` first, ascending within a level"""
    out, level = [], sorted(set(keys))
    for l in range(depth, 0, -1):
        have = set(level)
        out += [(l, p ^ 1) for p in level if p ^ 1 not in have]
        level = sorted({p >> 1 for p in level})
    return out


def known_empty_model(depth, keys, leaf_empty, absent):
    """(digests, levels with a job) of the compact check: a leaf is known-empty when leaf_empty[key], supplied node m when absent[m], a parent
    exactly when both children are, and such a parent is not hashed"""
    known = {k: bool(leaf_empty[k]) for k in keys}
    m = digests = levels = 0
    for _ in range(depth, 0, -1):
        up, made = {}, 0
        for p in sorted(known):
            if p ^ 1 in known:
                if p & 1:
                    continue
                e = known[p] and known[p ^ 1]
            else:
                e = known[p] and bool(absent[m])
                m += 1
            up[p >> 1] = e
            made += 0 if e else 1
        digests += made
        levels += 1 if made else 0
        known = up
    return digests, levels


def bits_of(flags):
    out = bytearray((len(flags) + 7) // 8)
    for m, f in enumerate(flags):
        if f:
            out[m >> 3] |= 1 << (m & 7)
    return bytes(out)


def flags_of(bits, count):
    return [bool(bits[m >> 3] >> (m & 7) & 1) for m in range(count)]


def stored_set(tree):
    return {(l, q) for l, (prefixes, _) in enumerate(int_levels(tree)) for q in prefixes}


def expand(nodes, flags, positions, table):
    """the plain node list a compact proof stands for: E_l wherever a bit is set"""
    it = iter(nodes)
    return [table[l] if f else next(it) for f, (l, _) in zip(flags, positions)]


def sets_of(depth):
    """(name, random count) of the boundary sets that exist at this depth"""
    out = []
    for name in BOUNDARY_SETS:
        if (name == "equal-low-halves" and depth <= 64) or (name.startswith("shared") and depth < 9):
            continue
        out.append(name)
    return out


def case_keys(depth, name, seed):
    return boundary_keys(depth, name, seed, random_count=min(24, 1 << depth))


def asked(depth, keys, seed):
    """some members and some absent keys, distinct, members first"""
    return list(dict.fromkeys(keys[:10] + some_absent(depth, keys, seed)))


CASES = [(d, name) for d in DEPTHS for name in sets_of(d)]


def check_case(D, make, lib, depth, name, device, narrow=None):
    """every property of one key set, with the tree made by `make` and the checks run on `device`"""
    seed = 1000 * depth + BOUNDARY_SETS.index(name)
    empty = NONZERO_EMPTY if BOUNDARY_SETS.index(name) % 2 else (0, 0)
    keys = case_keys(depth, name, seed)
    values = random_pairs(len(keys), seed)
    tree = make(depth, empty)
    tree.set(keys, values)
    ask = asked(depth, keys, seed)
    got, stored = tree.get(ask)
    assert [s for k, s in zip(ask, stored) if k not in keys] == [False] * (len(ask) - len([k for k in ask if k in keys]))      # the absent keys are not stored
    n, root = depth + 1, tree.root
    table = D.empty_nodes(n, empty, lib=lib)
    assert table[depth] == tuple(empty) and len(table) == n
    positions = supplied_positions(depth, ask)
    M, plain_digests = D.multiproof_size_wide(n, ask, lib=lib)
    assert M == len(positions)
    leaves, nodes, none = tree.batch_proof(ask, compact=False)
    assert none is None and leaves == got and len(nodes) == M
    if narrow is not None:                                                          # byte-equal to the narrow tree where both exist
        other = narrow(depth, empty)
        other.set(keys, values)
        assert other.multiproof(ask) == (leaves, nodes)
        other.close()
    cleaves, cnodes, bits = tree.batch_proof(ask)
    have = stored_set(tree)
    flags = [pos not in have for pos in positions]
    assert cleaves == leaves and bits == bits_of(flags) and len(cnodes) == M - sum(flags)
    assert expand(cnodes, flags, positions, table) == nodes
    leaf_empty = {k: v == tuple(empty) for k, v in zip(ask, leaves)}
    digests, levels = known_empty_model(depth, ask, leaf_empty, flags)
    s = {}
    assert D.multiproof_root_wide(n, ask, leaves, nodes, device=device, lib=lib, stats=s) == root and s["digests"] == plain_digests and s["levels"] == depth
    s = {}
    assert D.multiproof_root_wide(n, ask, cleaves, cnodes, bits, table, device=device, lib=lib, stats=s) == root
    assert (s["digests"], s["levels"]) == (digests, levels) and digests <= plain_digests
    want_paths = tree.paths(ask)
    for proof in ((leaves, nodes, None, None), (cleaves, cnodes, bits, table)):
        paths, r = D.multiproof_paths_wide(n, ask, *proof, device=device, lib=lib)
        assert r == root and paths == want_paths
        assert D.verify_multiproof_wide(root, n, ask, *proof, device=device, lib=lib)
    assert D.verify_paths_wide(root, want_paths, ask, leaves=leaves, device=device, lib=lib) == (-1, D.DST_PATH_OK)
    # tampering: a verdict, not an error
    bent = list(cleaves)
    bent[-1] = (bent[-1][0] ^ 1, bent[-1][1])
    assert not D.verify_multiproof_wide(root, n, ask, bent, cnodes, bits, table, device=device, lib=lib)
    if cnodes:
        changed = list(cnodes)
        changed[len(changed) // 2] = (changed[len(changed) // 2][0], changed[len(changed) // 2][1] ^ 2)
        assert not D.verify_multiproof_wide(root, n, ask, cleaves, changed, bits, table, device=device, lib=lib)
        m = flags.index(False)                                                      # one flipped bit: a stored sibling claimed to be an empty subtree
        fewer = [v for i, v in enumerate(expand(cnodes, flags, positions, table)) if not flags[i] and i != m]
        assert not D.verify_multiproof_wide(root, n, ask, cleaves, fewer, bits_of(flags[:m] + [True] + flags[m + 1:]), table, device=device, lib=lib)
    if any(flags):
        m = flags.index(True)                                                       # ... and an empty subtree claimed to be something else
        more = expand(cnodes, flags, positions, table)
        more[m] = (7, 7)
        more = [v for i, v in enumerate(more) if not flags[i] or i == m]
        assert not D.verify_multiproof_wide(root, n, ask, cleaves, more, bits_of(flags[:m] + [False] + flags[m + 1:]), table, device=device, lib=lib)
    # other leaves over the same nodes: the root after those writes
    fresh = random_pairs(len(ask), seed + 1)
    fresh[0] = tuple(empty)                                                         # one write of the empty value: known-empty by value
    after = D.multiproof_root_wide(n, ask, fresh, cnodes, bits, table, device=device, lib=lib)
    tree.set(ask, fresh)
    assert tree.root == after != root
    tree.close()


@pytest.mark.parametrize("depth,name", CASES)
def test_plain_and_compact_proofs_of_the_boundary_sets(depth, name):
    import distaff_amd as D
    check_case(D, host_wide, _product(), depth, name, -1, narrow=host_sparse if depth <= 63 else None)


def check_empty_tree(D, make, lib, device, oracle=None):
    for depth, empty in ((1, (0, 0)), (65, NONZERO_EMPTY), (127, (0, 0))):
        tree = make(depth, empty)
        ask = [0, (1 << depth) - 1] + ([5, 1 << 64, (1 << 64) + 4] if depth > 64 else [])
        leaves, nodes, bits = tree.batch_proof(ask)
        M = len(supplied_positions(depth, ask))
        assert nodes == [] and leaves == [tuple(empty)] * len(ask) and bits == bits_of([True] * M)
        table = D.empty_nodes(depth + 1, empty, lib=lib)
        if oracle is not None:
            assert table == empty_chain(oracle, empty, depth)
        s = {}
        assert D.multiproof_root_wide(depth + 1, ask, leaves, nodes, bits, table, device=device, lib=lib, stats=s) == table[0] == tree.root
        assert (s["digests"], s["levels"], s["device_ms"]) == (0, 0, 0.0)
        paths, root = D.multiproof_paths_wide(depth + 1, ask, leaves, nodes, bits, table, device=device, lib=lib)
        assert root == table[0] and paths == tree.paths(ask) and paths[0] == table[::-1][:1] + table[:0:-1]
        tree.close()


def test_an_empty_tree_with_absent_keys_needs_no_digest(oracle):
    import distaff_amd as D
    check_empty_tree(D, host_wide, _product(), -1, oracle)


def check_stored_empty_value(D, make, lib, device):
    """a key stored with the empty value has stored ancestors: its siblings' bits are by absence, its own leaf is known-empty by value"""
    depth, empty = 100, NONZERO_EMPTY
    tree = make(depth, empty)
    a, b = (1 << 99) | 12345, 12344
    tree.set([a, b], [(1, 2), empty])
    table = D.empty_nodes(depth + 1, empty, lib=lib)
    leaves, nodes, bits = tree.batch_proof([b ^ 1])
    flags = flags_of(bits, depth)
    assert leaves == [tuple(empty)] and flags[0] is False and nodes[0] == tuple(empty)       # the sibling b is stored, with the empty value
    assert flags[1:-1] == [True] * (depth - 2) and flags[-1] is False
    s = {}
    assert D.multiproof_root_wide(depth + 1, [b ^ 1], leaves, nodes, bits, table, device=device, lib=lib, stats=s) == tree.root
    assert s["digests"] == depth                                                    # a shipped node is not known-empty, whatever its value
    leaves, nodes, bits = tree.batch_proof([b])
    assert leaves == [tuple(empty)] and flags_of(bits, depth) == [True] * (depth - 1) + [False]
    s = {}
    assert D.multiproof_root_wide(depth + 1, [b], leaves, nodes, bits, table, device=device, lib=lib, stats=s) == tree.root
    assert (s["digests"], s["levels"]) == (1, 1)                                    # the leaf is known-empty by value: only the root is hashed
    assert tree.compact() == 1
    leaves, nodes, bits = tree.batch_proof([b ^ 1])
    assert flags_of(bits, depth) == [True] * (depth - 1) + [False] and len(nodes) == 1
    tree.close()


def test_a_key_stored_with_the_empty_value_is_flagged_by_absence_and_known_empty_by_value():
    import distaff_amd as D
    check_stored_empty_value(D, host_wide, _product(), -1)


# ---- what is refused: DST_ERR_ARG with its text, the outputs and the tree untouched ----------------------------------------------------------------------
def words(pairs):
    import distaff_amd as D
    return D.ints_to_arr([x for p in pairs for x in p]).reshape(-1, 2, 2) if pairs else np.zeros((0, 2, 2), dtype=np.uint64)


def check_refusals(D, make, lib, device):
    depth, n, empty = 65, 66, NONZERO_EMPTY
    keys = boundary_keys(depth, "random-200", 65, 12)
    tree = make(depth, empty)
    tree.set(keys, random_pairs(12, 65))
    ask = keys[:5] + [keys[0] ^ (1 << 64)]
    leaves, nodes, bits = tree.batch_proof(ask)
    table = D.empty_nodes(n, empty, lib=lib)
    M = len(supplied_positions(depth, ask))
    assert M % 8 != 0                                                               # there are padding bits to set
    padded = bits[:-1] + bytes([bits[-1] | 0x80])
    big = list(table)
    big[3] = (P, 0)
    plain_leaves, plain_nodes, _ = tree.batch_proof(ask, compact=False)
    cases = [((leaves, nodes[:-1], bits, table), "less the bits set"), ((leaves, nodes + [(1, 1)], bits, table), "less the bits set"),
             ((leaves, nodes, padded, table), "padding bit"), ((leaves, nodes, bits, None), "absent_bits without empties"),
             ((leaves, nodes, bits, big), "empties is not below the modulus"), ((plain_leaves, plain_nodes[:-1], None, None), "number of supplied nodes"),
             ((plain_leaves, plain_nodes, None, table), "empties without absent_bits"), ((leaves, [(P, 0)] + nodes[1:], bits, table), "not below the modulus"),
             (([(0, P + 1)] + leaves[1:], nodes, bits, table), "not below the modulus")]
    root = tree.root
    for proof, text in cases:
        for call in (lambda: D.multiproof_root_wide(n, ask, *proof, device=device, lib=lib), lambda: D.verify_multiproof_wide(root, n, ask, *proof, device=device, lib=lib),
                     lambda: D.multiproof_paths_wide(n, ask, *proof, device=device, lib=lib)):
            with pytest.raises(D.DistaffError) as e:
                call()
            assert e.value.code == D.DST_ERR_ARG and text in str(e.value), (text, str(e.value))
    for bad, text in (([5, 5], "repeated"), ([1 << 65], "past the end"), ([], "no leaf")):
        with pytest.raises(D.DistaffError) as e:
            D.multiproof_root_wide(n, bad, [(0, 0)] * len(bad), [], bits_of([True] * 65) if bad else b"", table, device=device, lib=lib)
        assert e.value.code == D.DST_ERR_ARG and text in str(e.value)
    for bad_n in (1, 129):
        with pytest.raises(D.DistaffError) as e:
            D.empty_nodes(bad_n, lib=lib)
        assert "2 .. 128" in str(e.value)
        with pytest.raises(D.DistaffError) as e:
            D.multiproof_size_wide(bad_n, [0], lib=lib)
        assert "2 .. 128" in str(e.value)
    # straight through the C-ABI: the outputs are as they were
    idx = D.ints_to_arr(ask)
    a, b, t = words(leaves), words(nodes[:-1]), words(table)
    raw = np.frombuffer(bits, dtype=np.uint8).copy()
    out = np.full((2, 2), 0xAA, dtype=np.uint64)
    d, ms = ctypes.c_uint64(77), ctypes.c_double(5.0)
    pt = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    r = lib.dst_rescue_multiproof_root_w(ctypes.c_int(device), ctypes.c_uint32(n), pt(idx), pt(a), ctypes.c_size_t(len(ask)), pt(b), ctypes.c_size_t(len(nodes) - 1), pt(raw), pt(t), pt(out),
                                         ctypes.byref(d), ctypes.byref(ms))
    assert r == D.DST_ERR_ARG and (out == 0xAA).all() and d.value == 77 and ms.value == 0.0
    # the tree-side call
    with pytest.raises(D.DistaffError) as e:
        tree.batch_proof([keys[0], keys[0]])
    assert e.value.code == D.DST_ERR_ARG and "repeated" in str(e.value)
    with pytest.raises(D.DistaffError) as e:
        tree.batch_proof([1 << 65])
    assert e.value.code == D.DST_ERR_ARG and "past the end" in str(e.value)
    kidx = D.ints_to_arr(ask)
    lv, nd, small = np.full((len(ask), 2, 2), 0xBB, dtype=np.uint64), np.full((len(nodes), 2, 2), 0xBB, dtype=np.uint64), np.full(len(bits), 0xCC, dtype=np.uint8)
    got, total = ctypes.c_size_t(9), ctypes.c_size_t(9)
    r = lib.dst_wtree_multiproof(tree._h, pt(kidx), ctypes.c_size_t(len(ask)), pt(lv), pt(nd), ctypes.c_size_t(len(nodes) - 1), ctypes.byref(got), pt(small), ctypes.byref(total))
    assert r == D.DST_ERR_ARG and "too small" in tree._error(tree._h) and (lv == 0xBB).all() and (nd == 0xBB).all() and (small == 0xCC).all()
    assert tree.root == root and tree.audit() is None and tree.batch_proof(ask) == (leaves, nodes, bits)
    assert tree.batch_proof([]) == ([], [], b"")
    tree.close()


def test_every_refusal_has_its_text_and_leaves_the_outputs_and_the_tree_untouched():
    import distaff_amd as D
    check_refusals(D, host_wide, _product(), -1)


def test_plan_for_128_bit_positions_against_a_model_under_sanitizers(tmp_path):
    """tests/multiproof/multiproof_wide_plan_check.cpp drives host/multiproof_plan.h alone over stree_wide positions, with and without known-empty
    flags, against a model over std::set; built with -fsanitize=address,undefined and run as a program: exit status 0, nothing on stderr"""
    import subprocess
    exe = str(tmp_path / "multiproof_wide_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-w", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "multiproof", "multiproof_wide_plan_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    assert b"sets ok" in r.stdout


def test_the_new_calls_are_in_the_package_the_header_and_both_libraries():
    import re
    import distaff_amd as D
    names = ["dst_rescue_empty_nodes", "dst_rescue_multiproof_size_w", "dst_wtree_multiproof", "dst_rescue_multiproof_root_w", "dst_rescue_verify_multiproof_w",
             "dst_rescue_multiproof_paths_w", "dst_wtree_save", "dst_wtree_load"]
    assert set(names) <= set(D.EXPORTS)
    header = open(os.path.join(ROOT, "include", "distaff_hip.h")).read()
    assert "NOT YET AVAILABLE" not in header
    for name in names:
        assert re.search(r"DST_API int %s\(" % name, header), name
        assert hasattr(_product(), name) and hasattr(ctypes.CDLL(D.HOOKS_LIB), name), name
    # one call beyond the issue's list: the levels that had a job, for `stats`
    assert "dst_rescue_multiproof_last_levels" in D.EXPORTS and re.search(r"DST_API uint32_t dst_rescue_multiproof_last_levels\(void\);", header)
    assert hasattr(_product(), "dst_rescue_multiproof_last_levels") and hasattr(ctypes.CDLL(D.HOOKS_LIB), "dst_rescue_multiproof_last_levels")
    assert all(hasattr(D.WideSparseRescueTree, f) for f in ("batch_proof", "to_blob", "from_blob"))
