"""Deletion from sparse Rescue Merkle trees (dst_stree_remove, dst_stree_compact, dst_stree_get) on the host path (device = -1) of the PRODUCT
library.  No GPU.  After a removal the tree must BE the tree created fresh and set once with the remaining keys -- prefixes, node values, key and
node counts -- and stand for the dense tree with the empty leaf at the removed positions: up to depth 8 the dense host RescueTree is the second
yardstick, root and the paths of all 2^depth indices.  Everything is bit-exact.  Also here: the helpers the emulated and the GPU tests of
deletion share."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from test_rescue_tree_host import P, _product
from test_sparse_rescue_tree_host import (NONZERO_EMPTY, assert_same_levels, check_against_dense, dense_leaves, depth_63_keys, host_dense, host_sparse,
                                          levels_of, random_pairs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def surviving_ancestors(stored, asked, depth):
    """digests one removal computes: per level l < depth the distinct key >> (depth - l) of the removed stored keys that remain on the level"""
    gone = set(stored) & set(asked)
    rest = set(stored) - gone
    return sum(len({k >> (depth - l) for k in gone} & {k >> (depth - l) for k in rest}) for l in range(depth))


def removal_cases(depth, seed):
    """(stored keys, [removal sets, applied one after the other]): none; one key (stored, then absent); every key (and absent ones); a sibling
    pair k, k ^ 1 with one of them removed, then both; random thirds with stored and not-stored keys"""
    rnd = random.Random(seed)
    n = 1 << depth
    some = rnd.sample(range(n), max(1, (2 * n) // 3))
    absent = [k for k in range(n) if k not in some]
    k = rnd.randrange(n) & ~1
    pair = list({k, k ^ 1} | set(rnd.sample(range(n), max(1, n // 3))))
    cases = [(some, [[]]),
             (some, [[some[0]], absent[:1]]),
             (some, [some + absent[:2]]),
             (list(range(n)), [list(range(n))]),
             (pair, [[k], [k ^ 1, k]]),
             ([k, k ^ 1], [[k ^ 1], [k]]),
             (some, [rnd.sample(range(n), max(1, n // 3)), rnd.sample(range(n), max(1, n // 3)), rnd.sample(range(n), max(1, n // 3))])]
    for _, removals in cases:
        for r in removals:
            rnd.shuffle(r)
    return cases


def check_removals(make, depth, empty, stored, removals, seed, dense=True):
    """after every remove: levels, info and root are those of a fresh tree (by `make`) set with the remaining keys; removed and last_digests are
    computed from the key sets; with `dense` the root and every path are the dense host tree's with the empty leaf at the removed keys"""
    content = dict(zip(stored, random_pairs(len(stored), seed)))
    tree = make(depth, empty)
    tree.set(stored, [content[k] for k in stored])
    for asked in removals:
        want_removed, want_digests = len(set(content) & set(asked)), surviving_ancestors(content, asked, depth)
        assert tree.remove(asked) == want_removed, asked
        for k in asked:
            content.pop(k, None)
        info = tree.info()
        assert info["last_digests"] == want_digests, (sorted(content), asked)
        fresh = make(depth, empty)
        fresh.set(list(content), list(content.values()))
        assert_same_levels(levels_of(tree), levels_of(fresh))
        assert tree.root == fresh.root and (info["keys"], info["nodes"]) == (fresh.info()["keys"], fresh.info()["nodes"])
        fresh.close()
        if dense:
            d = host_dense(dense_leaves(depth, content, empty))
            check_against_dense(tree, d, list(content))
            every = list(range(1 << depth))
            assert tree.paths(every) == d.paths(every)
            d.close()
    tree.close()


@pytest.mark.parametrize("empty", [(0, 0), NONZERO_EMPTY])
@pytest.mark.parametrize("depth", range(1, 9))
def test_after_a_removal_the_tree_is_the_fresh_tree_of_the_remaining_keys_and_the_dense_tree_with_empty_leaves(depth, empty):
    for case, (stored, removals) in enumerate(removal_cases(depth, 900 + depth)):
        check_removals(host_sparse, depth, empty, stored, removals, 2000 * depth + case)


@pytest.mark.parametrize("depth,empty", [(1, (0, 0)), (5, NONZERO_EMPTY), (63, (0, 0))])
def test_remove_everything_then_set_again_equals_a_fresh_tree_of_the_second_set(depth, empty, oracle):
    from test_sparse_rescue_tree_host import empty_chain
    first = list(range(1 << depth)) if depth < 6 else depth_63_keys(5, 12)
    second = first[1::2] + ([] if depth < 6 else depth_63_keys(6, 8)[-4:])
    second = list(dict.fromkeys(second))
    tree = host_sparse(depth, empty)
    tree.set(first, random_pairs(len(first), 31))
    assert tree.remove(first) == len(first)
    info = tree.info()
    assert (info["keys"], info["nodes"], info["last_digests"]) == (0, 0, 0)
    assert tree.root == empty_chain(oracle, empty, depth)[0] and all(len(p) == 0 for p, _ in levels_of(tree))
    assert tree.path(first[0])[0] == tuple(empty)
    leaves = random_pairs(len(second), 32)
    tree.set(second, leaves)
    fresh = host_sparse(depth, empty)
    fresh.set(second, leaves)
    assert_same_levels(levels_of(tree), levels_of(fresh))
    assert tree.root == fresh.root and tree.info() == fresh.info()
    tree.close(); fresh.close()


@pytest.mark.parametrize("depth,empty", [(1, (0, 0)), (4, NONZERO_EMPTY), (63, NONZERO_EMPTY)])
def test_a_key_set_to_the_empty_value_stays_stored_until_compact_drops_it(depth, empty):
    keys = list(range(1 << depth))[:7] if depth < 63 else depth_63_keys(9, 7)
    leaves = random_pairs(len(keys), 41)
    without = host_sparse(depth, empty)
    without.set(keys[1:], leaves[1:])
    tree = host_sparse(depth, empty)
    tree.set(keys, leaves)
    tree.set([keys[0]], [empty])
    assert tree.root == without.root                                               # the root does not depend on it ...
    assert tree.info()["keys"] == len(keys) and tree.get([keys[0]]) == ([tuple(empty)], [True])      # ... and it is stored
    nodes_before = [n.copy() for _, n in levels_of(tree)]
    assert tree.compact() == 1
    assert tree.info()["last_digests"] == 0
    assert_same_levels(levels_of(tree), levels_of(without))
    assert tree.root == without.root and (tree.info()["keys"], tree.info()["nodes"]) == (without.info()["keys"], without.info()["nodes"])
    assert tree.get([keys[0]]) == ([tuple(empty)], [False])
    assert sum(len(n) for n in nodes_before) > tree.info()["nodes"]
    assert tree.compact() == 0 and tree.info()["last_digests"] == 0               # nothing left to drop: the tree is unchanged
    assert_same_levels(levels_of(tree), levels_of(without))
    tree.close(); without.close()


def check_apply_compact_equals_remove(make, depth, empty, keys, gone, verify):
    """apply(gone, empties) + compact() on one tree and remove(gone) on a twin leave identical levels; the last root apply returned is the twin's
    root and `verify` (verify_writes bound to a device and a library) accepts apply's witnesses"""
    leaves = random_pairs(len(keys), 51)
    a, b = make(depth, empty), make(depth, empty)
    a.set(keys, leaves); b.set(keys, leaves)
    before = a.root
    stored = len(set(keys) & set(gone))
    empties = [tuple(empty)] * len(gone)
    paths, roots = a.apply(gone, empties)
    assert b.remove(gone) == stored
    assert roots[-1] == b.root == a.root
    assert verify(before, gone, paths, empties, roots) == (-1, 0, b.root)
    assert a.info()["keys"] == len(set(keys) | set(gone))                           # an absent key written with the empty value is stored too
    assert a.compact() == len(gone) and a.info()["last_digests"] == 0
    assert_same_levels(levels_of(a), levels_of(b))
    assert a.root == b.root and (a.info()["keys"], a.info()["nodes"]) == (b.info()["keys"], b.info()["nodes"])
    a.close(); b.close()


@pytest.mark.parametrize("depth,empty", [(3, (0, 0)), (6, NONZERO_EMPTY), (63, (0, 0))])
def test_apply_of_empties_then_compact_equals_remove_and_its_witnesses_verify(depth, empty):
    import distaff_amd as D
    rnd = random.Random(depth)
    keys = rnd.sample(range(1 << depth), 6) if depth < 63 else depth_63_keys(11, 10)
    never = next(k for k in range(1 << min(depth, 10)) if k not in keys)
    gone = keys[:3] + [never]
    check_apply_compact_equals_remove(host_sparse, depth, empty, keys, gone, lambda *a: D.verify_writes(*a, device=-1, lib=_product()))


def check_get(tree, content, empty, asked):
    leaves, stored = tree.get(asked)
    assert leaves == [content.get(k, tuple(empty)) for k in asked] and stored == [k in content for k in asked]
    words, flags = tree.get_words(asked)
    assert words.shape == (len(asked), 2, 2) and flags.dtype == np.uint8 and [bool(f) for f in flags] == stored
    assert [tuple(p[0]) for p in tree.paths(asked)] == leaves                       # the first node of every path


@pytest.mark.parametrize("depth,empty", [(2, (0, 0)), (7, NONZERO_EMPTY), (63, NONZERO_EMPTY)])
def test_get_returns_stored_absent_and_removed_keys_with_repeats(depth, empty):
    rnd = random.Random(70 + depth)
    keys = rnd.sample(range(1 << depth), min(1 << depth, 40) * 3 // 4) if depth < 63 else depth_63_keys(13, 20)
    content = dict(zip(keys, random_pairs(len(keys), 71)))
    tree = host_sparse(depth, empty)
    assert tree.get([]) == ([], []) and tree.get([0, 0]) == ([tuple(empty)] * 2, [False, False])
    tree.set(keys, [content[k] for k in keys])
    others = [k ^ 1 for k in keys[:5]] + [0, (1 << depth) - 1]
    asked = keys + others + keys[:3] + [keys[0]] * 3
    check_get(tree, content, empty, asked)
    for k in keys[:len(keys) // 2]:
        del content[k]
    assert tree.remove(keys[:len(keys) // 2]) == len(keys) // 2
    check_get(tree, content, empty, asked)
    tree.close()


def test_depth_63_a_sibling_pair_keeps_its_62_upper_ancestors_until_both_are_removed():
    keys = depth_63_keys(17, 8)
    k = next(x for x in keys if x ^ 1 in keys and x not in (0, 2 ** 63 - 1))
    others = [x for x in keys if x not in (k, k ^ 1)]
    assert not any(x >> 2 == k >> 2 for x in others)
    content = dict(zip(keys, random_pairs(len(keys), 18)))
    tree = host_sparse(63)
    tree.set(keys, [content[x] for x in keys])
    value = lambda l: [n.tolist() for q, n in zip(*tree.level(l)) if int(q) == k >> (63 - l)]  # noqa: E731
    before = [value(l) for l in range(64)]
    assert all(len(v) == 1 for v in before)
    nodes = tree.info()["nodes"]
    assert tree.remove([k]) == 1
    after = [value(l) for l in range(64)]
    # the leaf is gone; the common parent (level 62) and the 62 ancestors above it stay, every one with a new value
    assert after[63] == [] and tree.info()["nodes"] == nodes - 1 and tree.info()["last_digests"] == 63
    assert all(len(after[l]) == 1 and after[l] != before[l] for l in range(63))
    shared = sum(1 for l in range(63) if any(x >> (63 - l) == k >> (63 - l) for x in others))     # ancestors other keys keep alive
    assert tree.remove([k ^ 1]) == 1
    assert tree.info()["last_digests"] == shared and tree.info()["nodes"] == nodes - 2 - (63 - shared)
    assert [len(value(l)) for l in range(64)] == [1] * shared + [0] * (64 - shared)
    fresh = host_sparse(63)
    fresh.set(others, [content[x] for x in others])
    assert_same_levels(levels_of(tree), levels_of(fresh))
    tree.close(); fresh.close()


def test_argument_errors_never_abort_and_leave_the_tree_unchanged():
    """a handle that was destroyed is NULL in the binding: DST_ERR_ARG.  (DST_ERR_STATE needs a HIP error inside a call; every entry point
    begins with the same check of the handle as dst_stree_set.)"""
    import distaff_amd as D
    lib = _product()
    n, buf, flag = ctypes.c_uint64(77), ctypes.create_string_buffer(64), ctypes.create_string_buffer(2)
    idx = np.array([3, 3], dtype=np.uint64)
    ip = idx.ctypes.data_as(ctypes.c_void_p)
    assert lib.dst_stree_remove(None, ip, ctypes.c_size_t(1), ctypes.byref(n)) == D.DST_ERR_ARG
    assert lib.dst_stree_compact(None, ctypes.byref(n)) == D.DST_ERR_ARG
    assert lib.dst_stree_get(None, ip, ctypes.c_size_t(1), buf, flag) == D.DST_ERR_ARG
    for depth in (5, 63):
        tree = host_sparse(depth, NONZERO_EMPTY)
        top = 1 << depth
        tree.set([1, 3, top - 1], [(1, 2), (3, 4), NONZERO_EMPTY])
        snapshot = lambda: (tree.root, tree.info(), [(p.tolist(), q.tolist()) for p, q in levels_of(tree)])  # noqa: E731
        before = snapshot()
        bad = [[top], [1, top], [1, 3, 1], [7, 7]] + ([[1 << 63]] if depth < 63 else [])
        for keys in bad:
            with pytest.raises(D.DistaffError) as e:
                tree.remove(keys)
            assert e.value.code == D.DST_ERR_ARG, keys
        for keys in ([top], [1, top]) + (([1 << 63],) if depth < 63 else ()):
            with pytest.raises(D.DistaffError) as e:
                tree.get(keys)
            assert e.value.code == D.DST_ERR_ARG, keys
        assert lib.dst_stree_remove(tree._h, None, ctypes.c_size_t(1), ctypes.byref(n)) == D.DST_ERR_ARG
        assert lib.dst_stree_remove(tree._h, ip, ctypes.c_size_t(2), None) == D.DST_ERR_ARG             # repeated, and no counter to write
        assert lib.dst_stree_get(tree._h, None, ctypes.c_size_t(1), buf, flag) == D.DST_ERR_ARG
        assert lib.dst_stree_get(tree._h, ip, ctypes.c_size_t(1), None, flag) == D.DST_ERR_ARG
        assert snapshot() == before
        # no-ops: count = 0, no index stored -- DST_OK, the tree as it was, last_digests = 0
        assert lib.dst_stree_remove(tree._h, None, ctypes.c_size_t(0), None) == D.DST_OK
        assert tree.remove([]) == 0 and tree.remove([0, 2, top - 2]) == 0
        assert tree.info()["last_digests"] == 0
        assert (tree.root, snapshot()[2]) == (before[0], before[2])
        assert lib.dst_stree_get(tree._h, ip, ctypes.c_size_t(2), buf, None) == D.DST_OK                # the flags are optional, repeats allowed
        assert lib.dst_stree_remove(tree._h, ip, ctypes.c_size_t(1), None) == D.DST_OK and tree.info()["keys"] == 2      # the counter is optional
        assert lib.dst_stree_compact(tree._h, None) == D.DST_OK and tree.info()["keys"] == 1
        tree.close()
        for call in (lambda: tree.remove([1]), tree.compact, lambda: tree.get([1])):
            with pytest.raises(D.DistaffError) as e:
                call()
            assert e.value.code == D.DST_ERR_ARG
        tree.close()


def test_removal_plan_against_a_map_model_under_sanitizers(tmp_path):
    """tests/sparse_host/stree_remove_check.cpp drives host/stree_levels.h alone -- random interleavings of stree_plan_set and stree_plan_remove,
    with and without rehashing: the pruned shape, the carry sources, the dirty lists per level -- against a std::map model, built with
    -fsanitize=address,undefined and run as a program: exit status 0, nothing on stderr"""
    exe = str(tmp_path / "stree_remove_check")
    subprocess.check_call(["g++", "-std=c++17", "-w", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sparse_host", "stree_remove_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    assert b"rounds ok" in r.stdout


def example_lines(make, k, m):
    """what examples/merkle_remove.c prints for k and m, through the binding"""
    keys = [((i + 1) * 0x9E3779B97F4A7C15) & (2 ** 63 - 1) for i in range(k)]
    leaves = [(2 * i + 1, 2 * i + 2) for i in range(k)]
    fmt = lambda label, r: "%s %032x %032x" % ((label,) + tuple(r))  # noqa: E731
    says = lambda label, t: "%s: %d keys in %d stored nodes, %d digests" % (label, t.info()["keys"], t.info()["nodes"], t.info()["last_digests"])  # noqa: E731
    tree = make(63)
    tree.set(keys, leaves)
    lines = [fmt("root", tree.root), says("set", tree)]
    removed = tree.remove(keys[:m])
    lines += [fmt("root after remove", tree.root), "%d removed" % removed, says("remove", tree)]
    tree.set([keys[m]], [(0, 0)])
    lines += [fmt("root after the witnessed deletion", tree.root), "witness: first_bad -1 why 0, the root follows: yes",
              "before compact: %d keys in %d stored nodes, the key is stored and its leaf is empty" % (tree.info()["keys"], tree.info()["nodes"])]
    compacted = tree.compact()
    lines += [fmt("root after compact", tree.root), "%d compacted" % compacted, says("compact", tree), "after compact: the key is not stored and its leaf is empty"]
    tree.close()
    return lines


def run_example(tmp_path, k, m, device):
    import distaff_amd as D
    exe = tmp_path / "merkle_remove"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_remove.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    r = subprocess.run([str(exe), str(k), str(m), str(device)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()
    return r.stdout.decode().splitlines()


def test_c_example_removes_keys_and_compacts_after_a_witnessed_deletion(tmp_path):
    """examples/merkle_remove.c compiles as C99 against include/distaff_hip.h and the product library and runs on the host"""
    lines = run_example(tmp_path, 40, 15, -1)
    assert lines == example_lines(host_sparse, 40, 15)
    assert "15 removed" in lines and "1 compacted" in lines


def test_package_lists_the_calls():
    import distaff_amd as D
    assert {"dst_stree_remove", "dst_stree_compact", "dst_stree_get"} <= set(D.EXPORTS)
    assert all(hasattr(D.SparseRescueTree, f) for f in ("remove", "compact", "get", "get_words"))
