"""Ordered leaf writes with a witness for each (dst_rtree_apply, dst_stree_apply, dst_rescue_path_tapes) on the host path (device = -1) of the
PRODUCT library.  No GPU.  The yardstick is never the new call: it is a SECOND tree driven through the calls that existed before, one operation
at a time -- path, then update / set with count 1, then root -- and, for the final state, a tree built fresh from the final leaves, node by
node.  Everything is bit-exact.  The checkers take the trees' constructors, so tests/test_rescue_tree_sequence_emulated.py and
tests/test_rescue_tree_sequence_gpu.py run the same cases on device trees."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from test_rescue_tree_host import P, _product, random_leaves
from test_rescue_tree_update_host import all_nodes, host_tree
from test_sparse_rescue_tree_host import NONZERO_EMPTY, assert_same_levels, host_sparse, levels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def index_lists(n, seed):
    """the index lists of one tree of n leaf positions: one operation; the same index twice in a row (the old leaf is a version); a leaf and
    then its sibling leaf, and back (the sibling at the leaf level is a version); two indices in different halves (they meet at the root only);
    an index, others, then the first index again"""
    rnd = random.Random(seed)
    x = n - 2 if n > 2 else 0
    y = x ^ (n >> 1)
    others = [rnd.randrange(n) for _ in range(3)]
    return [[x], [x, x], [x, x ^ 1], [x ^ 1, x, x ^ 1, x ^ 1], [x, y], [x] + others + [y, x]]


def random_ops(n, count, seed, repeats=0.1):
    """`count` indices below n, about a tenth of them repeats of earlier ones, and as many leaves"""
    rnd = random.Random(seed)
    indices = []
    for _ in range(count):
        indices.append(rnd.choice(indices) if indices and rnd.random() < repeats else rnd.randrange(n))
    return indices, [(rnd.randrange(P), rnd.randrange(P)) for _ in indices]


def check_dense_sequence(make, log_leaves, indices, new, seed, yard=host_tree, paths_at=None, tree=None, leaves=None):
    """tree.apply against a second tree (built by `yard`) that takes the operations one by one through path / update / root: every path (or
    those at the positions `paths_at`), every root; then every node against fresh builds, by `make` and by `yard`, over the final leaves.
    -> (tree, leaves) for a further sequence on the same tree"""
    leaves = list(leaves) if leaves is not None else random_leaves(log_leaves, seed)
    tree = tree or make(leaves)
    second = yard(leaves)
    assert tree.root == second.root
    paths, roots = tree.apply(indices, new)
    assert len(paths) == len(roots) == len(indices)
    for k, (i, v) in enumerate(zip(indices, new)):
        if paths_at is None or k in paths_at:
            assert paths[k] == second.path(i), (k, i)
        second.update([i], [v])
        assert roots[k] == second.root, (k, i)
        leaves[i] = tuple(v)
    assert np.array_equal(all_nodes(tree), all_nodes(second))
    for build in {make, yard}:
        fresh = build(leaves)
        assert np.array_equal(all_nodes(tree), all_nodes(fresh)), build
        fresh.close()
    assert tree.root == second.root and (not indices or tree.root == roots[-1])
    second.close()
    return tree, leaves


def check_sparse_sequence(make, depth, empty, initial, ops, yard=host_sparse, tree=None, fresh_by=None):
    """the same for a sparse tree that holds `initial` (key -> leaf): path / set / root on the second tree; then every level (prefixes and
    nodes) and the key count against the second tree and against fresh trees (by `make` and `yard`, or by `fresh_by`) set once with the final
    content.  -> (tree, content)"""
    content = dict(initial)
    if tree is None:
        tree = make(depth, empty)
        tree.set(list(content), list(content.values()))
    second = yard(depth, empty)
    second.set(list(content), list(content.values()))
    assert tree.root == second.root
    paths, roots = tree.apply([k for k, _ in ops], [v for _, v in ops])
    assert len(paths) == len(roots) == len(ops)
    for j, (k, v) in enumerate(ops):
        assert paths[j] == second.path(k), (j, k)
        assert len(paths[j]) == depth + 1 and paths[j][0] == content.get(k, tuple(empty))
        second.set([k], [v])
        assert roots[j] == second.root, (j, k)
        content[k] = tuple(v)
    assert_same_levels(levels_of(tree), levels_of(second))
    assert tree.info()["keys"] == second.info()["keys"] == len(content) and tree.info()["nodes"] == second.info()["nodes"]
    for build in fresh_by or {make, yard}:
        fresh = build(depth, empty)
        fresh.set(list(content), list(content.values()))
        assert_same_levels(levels_of(tree), levels_of(fresh))
        assert tree.root == fresh.root
        fresh.close()
    second.close()
    return tree, content


def sparse_cases(depth, empty, seed):
    """(initial content, operations) pairs: the index lists on an empty tree and on one that holds keys; a key whose sibling subtree is absent;
    a key whose sibling subtree an earlier operation of the same sequence created; keys that differ in the lowest bit only and in the top bit
    only; a key written with the empty value, stored before or not"""
    rnd = random.Random(seed)
    n = 1 << depth
    leaf = lambda: (rnd.randrange(P), rnd.randrange(P))  # noqa: E731
    stored = {rnd.randrange(n): leaf() for _ in range(6)}
    cases = []
    for initial in ({}, stored):
        for indices in index_lists(n, seed):
            cases.append((initial, [(i, leaf()) for i in indices]))
    k = rnd.randrange(n)
    top = 1 << (depth - 1)
    mid = 1 << (depth // 2)
    cases.append(({}, [(k, leaf())]))                                                               # every sibling subtree absent
    cases.append((stored, [(k, leaf()), (k ^ mid, leaf()), (k, leaf())]))                           # ... created by the operation before
    cases.append((stored, [(k, leaf()), (k ^ 1, leaf()), (k ^ top, leaf()), (k ^ top ^ 1, leaf()), (k ^ 1, leaf())]))
    some = next(iter(stored))
    cases.append((stored, [(some, tuple(empty)), (k, tuple(empty)), (some, leaf()), (k, tuple(empty))]))
    return cases


@pytest.mark.parametrize("log_leaves", [1, 2, 3])
def test_dense_sequences_equal_one_operation_at_a_time(log_leaves):
    n = 1 << log_leaves
    for case, indices in enumerate(index_lists(n, log_leaves) + [random_ops(n, 12, 40 + log_leaves, 0.3)[0]]):
        new = random_ops(n, len(indices), 100 * log_leaves + case)[1]
        tree, _ = check_dense_sequence(host_tree, log_leaves, indices, new, 20 + log_leaves)
        assert tree.update_ms == 0.0
        tree.close()


@pytest.mark.parametrize("depth,empty", [(1, (0, 0)), (3, NONZERO_EMPTY), (63, (0, 0)), (63, NONZERO_EMPTY)])
def test_sparse_sequences_equal_one_operation_at_a_time(depth, empty):
    for initial, ops in sparse_cases(depth, empty, 50 + depth):
        tree, _ = check_sparse_sequence(host_sparse, depth, empty, initial, ops)
        assert tree.info()["last_digests"] == len(ops) * depth and tree.info()["last_device_ms"] == 0.0      # a host tree: one set per operation
        tree.close()


def check_dense_rejections(make, log_leaves):
    """every argument error returns DST_ERR_ARG, names its cause and leaves every node as it was; count = 0 is a no-op; paths or roots may be NULL"""
    import distaff_amd as D
    n = 1 << log_leaves
    leaves = random_leaves(log_leaves, 6)
    tree = make(leaves)
    before = all_nodes(tree).tobytes()
    for indices, new, cause in (([0, n], [(1, 2), (3, 4)], "past the end"), ([n - 1, 0, 1 << 40], [(1, 2), (3, 4), (5, 6)], "past the end"),
                                ([0, 0], [(1, 2), (3, P)], "not below the modulus"), ([1], [(2 ** 128 - 1, 0)], "not below the modulus")):
        with pytest.raises(D.DistaffError) as e:
            tree.apply(indices, new)
        assert e.value.code == D.DST_ERR_ARG and cause in e.value.reason, (indices, e.value.reason)
        assert all_nodes(tree).tobytes() == before, indices
    idx, leaf, out = (ctypes.c_uint64 * 1)(0), ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * (log_leaves + 1))
    apply = tree.lib.dst_rtree_apply
    assert apply(tree._h, None, leaf, ctypes.c_size_t(1), out, out) == D.DST_ERR_ARG and "null pointer" in D.lib._rtree_error(tree.lib, tree._h)
    assert apply(tree._h, idx, None, ctypes.c_size_t(1), out, out) == D.DST_ERR_ARG
    assert apply(None, idx, leaf, ctypes.c_size_t(1), out, out) == D.DST_ERR_ARG
    assert apply(tree._h, idx, leaf, ctypes.c_size_t(1 << 31), out, out) == D.DST_ERR_ARG and "2^31" in D.lib._rtree_error(tree.lib, tree._h)
    assert all_nodes(tree).tobytes() == before
    assert tree.apply([], []) == ([], []) and apply(tree._h, None, None, ctypes.c_size_t(0), None, None) == D.DST_OK
    assert all_nodes(tree).tobytes() == before
    with pytest.raises(D.DistaffError):
        tree.apply([0, 1], [(1, 2)])
    # paths = NULL, roots = NULL, both: the tree takes the writes all the same
    second = host_tree(leaves)
    want_path = second.path(1)
    second.update([1], [(7, 8)])
    root = np.zeros((1, 2, 2), dtype=np.uint64)
    idx[0] = 1
    new = D.ints_to_arr([7, 8])
    assert apply(tree._h, idx, new.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1), None, root.ctypes.data_as(ctypes.c_void_p)) == D.DST_OK
    assert tuple(D.arr_to_ints(root)) == second.root == tree.root
    want2 = second.path(0)
    second.update([0], [(9, 10)])
    new = D.ints_to_arr([9, 10])
    idx[0] = 0
    path = np.zeros((log_leaves + 1, 2, 2), dtype=np.uint64)
    assert apply(tree._h, idx, new.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1), path.ctypes.data_as(ctypes.c_void_p), None) == D.DST_OK
    v = D.arr_to_ints(path)
    assert [(v[2 * k], v[2 * k + 1]) for k in range(log_leaves + 1)] == want2 and want_path[0] == leaves[1]
    second.update([1], [(11, 12)])
    new = D.ints_to_arr([11, 12])
    idx[0] = 1
    assert apply(tree._h, idx, new.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1), None, None) == D.DST_OK
    assert np.array_equal(all_nodes(tree), all_nodes(second))
    tree.close(); second.close()


def check_sparse_rejections(make, depth):
    import distaff_amd as D
    top = 1 << depth
    tree = make(depth, (0, 0))
    tree.set([1, top - 1], [(1, 2), (3, 4)])
    state = lambda: (tree.root, tree.info()["keys"], tree.info()["nodes"], [(p.tolist(), n.tolist()) for p, n in levels_of(tree)])  # noqa: E731
    before = state()
    bad = [([top], [(1, 1)], "past the end"), ([0, 0], [(1, 1), (P, 2)], "not below the modulus"), ([1], [(2 ** 128 - 1, 0)], "not below the modulus")]
    if depth < 63:
        bad.append(([3, 1 << 63], [(1, 1), (2, 2)], "past the end"))
    for keys, new, cause in bad:
        with pytest.raises(D.DistaffError) as e:
            tree.apply(keys, new)
        assert e.value.code == D.DST_ERR_ARG and cause in e.value.reason, (keys, e.value.reason)
        assert state() == before, keys
    idx, leaf, out = (ctypes.c_uint64 * 1)(0), ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * (depth + 1))
    apply = tree.lib.dst_stree_apply
    assert apply(tree._h, None, leaf, ctypes.c_size_t(1), out, out) == D.DST_ERR_ARG and "null pointer" in tree._error(tree._h)
    assert apply(tree._h, idx, None, ctypes.c_size_t(1), out, out) == D.DST_ERR_ARG
    assert apply(None, idx, leaf, ctypes.c_size_t(1), out, out) == D.DST_ERR_ARG
    assert apply(tree._h, idx, leaf, ctypes.c_size_t(1 << 31), out, out) == D.DST_ERR_ARG and "2^31" in tree._error(tree._h)
    assert tree.apply([], []) == ([], []) and apply(tree._h, None, None, ctypes.c_size_t(0), None, None) == D.DST_OK
    assert state() == before
    second = host_sparse(depth)
    second.set([1, top - 1], [(1, 2), (3, 4)])
    for keys_out in ((False, True), (True, False), (False, False)):                                # paths = NULL, roots = NULL, both
        idx[0] = 2 if keys_out[0] else 1
        new = D.ints_to_arr([5, 6 + idx[0]])
        path, root = np.zeros((depth + 1, 2, 2), dtype=np.uint64), np.zeros((1, 2, 2), dtype=np.uint64)
        want = second.path(idx[0])
        second.set([idx[0]], [(5, 6 + idx[0])])
        assert apply(tree._h, idx, new.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1), path.ctypes.data_as(ctypes.c_void_p) if keys_out[0] else None,
                     root.ctypes.data_as(ctypes.c_void_p) if keys_out[1] else None) == D.DST_OK
        if keys_out[0]:
            v = D.arr_to_ints(path)
            assert [(v[2 * k], v[2 * k + 1]) for k in range(depth + 1)] == want
        if keys_out[1]:
            assert tuple(D.arr_to_ints(root)) == second.root
        assert_same_levels(levels_of(tree), levels_of(second))
    tree.close(); second.close()


@pytest.mark.parametrize("log_leaves", [1, 3])
def test_rejected_dense_sequences_leave_the_tree_unchanged(log_leaves):
    check_dense_rejections(host_tree, log_leaves)


@pytest.mark.parametrize("depth", [3, 63])
def test_rejected_sparse_sequences_leave_the_tree_unchanged(depth):
    check_sparse_rejections(host_sparse, depth)


def test_path_tapes_equal_tapes_many_on_the_same_tree_state():
    import distaff_amd as D
    lib = _product()
    tree = host_tree(random_leaves(3, 9))
    indices = [5, 0, 5, 7]
    paths = tree.paths(indices)
    sparse = host_sparse(63, NONZERO_EMPTY)
    sparse.set([3, 1 << 62], [(1, 2), (3, 4)])
    keys = [3, 2 ** 63 - 1, 1 << 62]
    for what in (1, 2, 3):
        assert D.path_tapes(paths, indices, what, lib=lib) == tree.tapes_many(indices, what)
        assert D.path_tapes(sparse.paths(keys), keys, what, lib=lib) == sparse.tapes_many(keys, what)
        assert D.path_tapes(sparse.paths_words(keys), keys, what, lib=lib) == sparse.tapes_many(keys, what)
    # the witnesses of an apply are the tapes of the tree BEFORE each write
    second = host_tree(random_leaves(3, 9))
    witnesses, _ = tree.apply([5, 5], [(1, 2), (3, 4)])
    want = [second.tapes(5)]
    second.update([5], [(1, 2)])
    want.append(second.tapes(5))
    assert D.path_tapes(witnesses, [5, 5], lib=lib) == want
    assert D.path_tapes([], [], lib=lib) == []
    # the size query, and what is refused
    n, idx, buf = ctypes.c_size_t(0), (ctypes.c_uint64 * 2)(5, 8), ctypes.create_string_buffer(32 * 4 * 2)
    f = lib.dst_rescue_path_tapes
    size = lambda what, count=1: f(None, 4, idx, ctypes.c_size_t(count), what, None, None, ctypes.c_size_t(0), ctypes.byref(n))  # noqa: E731
    assert size(3) == D.DST_OK and n.value == 10 and size(1) == D.DST_OK and n.value == 7 and size(2) == D.DST_OK and n.value == 3
    assert size(0) == D.DST_ERR_ARG and size(4) == D.DST_ERR_ARG
    assert size(3, 2) == D.DST_ERR_ARG and "past the end" in D.lib._rtree_error(lib)                # index 8 in a path of 4 nodes
    assert f(buf, 4, idx, ctypes.c_size_t(1), 3, buf, None, ctypes.c_size_t(10), ctypes.byref(n)) == D.DST_ERR_ARG
    assert f(buf, 4, idx, ctypes.c_size_t(1), 3, buf, buf, ctypes.c_size_t(9), ctypes.byref(n)) == D.DST_ERR_ARG and n.value == 10      # too small
    assert f(None, 4, idx, ctypes.c_size_t(1), 3, buf, buf, ctypes.c_size_t(10), ctypes.byref(n)) == D.DST_ERR_ARG
    assert f(buf, 4, None, ctypes.c_size_t(1), 3, buf, buf, ctypes.c_size_t(10), ctypes.byref(n)) == D.DST_ERR_ARG
    assert f(buf, 1, idx, ctypes.c_size_t(1), 3, buf, buf, ctypes.c_size_t(10), ctypes.byref(n)) == D.DST_ERR_ARG
    assert f(buf, 4, idx, ctypes.c_size_t(1), 3, buf, buf, ctypes.c_size_t(10), None) == D.DST_ERR_ARG
    with pytest.raises(D.DistaffError) as e:
        D.path_tapes([[(1, 2), (P, 0)]], [0], lib=lib)
    assert e.value.code == D.DST_ERR_ARG and "not below the modulus" in e.value.reason
    tree.close(); second.close(); sparse.close()


def test_plan_against_a_two_loop_model_under_sanitizers(tmp_path):
    """tests/tree_sequence/tree_sequence_check.cpp drives host/tree_sequence.h alone (the source words of every operation and level, the touched
    nodes and their last operations) against the definition restated with two nested loops, built with -fsanitize=address,undefined and run as
    a program: exit status 0, nothing on stderr"""
    exe = str(tmp_path / "tree_sequence_check")
    subprocess.check_call(["g++", "-std=c++17", "-w", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "tree_sequence", "tree_sequence_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    assert b"rounds ok" in r.stdout


def example_roots(make, k, count):
    """what examples/merkle_sequence.c prints for k and count, through the calls that existed before it"""
    n = 1 << k
    tree = make([(2 * i + 1, 2 * i + 2) for i in range(n)])
    lines = ["root before 0 %032x %032x" % tree.root]
    indices = []
    for j in range(count):
        indices.append(indices[-1] if j & 3 == 3 else (7 * j + 3) & (n - 1))
        tree.update([indices[-1]], [(2 ** 64 + j, 2 ** 65 + j)])
        lines.append("root after write %d %032x %032x" % ((j,) + tree.root))
    tree.close()
    return lines + ["%d writes, %d witnesses of %d nodes checked" % (count, count, k + 1)]


def run_example(tmp_path, k, count, device):
    import distaff_amd as D
    exe = tmp_path / "merkle_sequence"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_sequence.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    r = subprocess.run([str(exe), str(k), str(count), str(device)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()
    return r.stdout.decode().splitlines()


def test_c_example_checks_its_witnesses_and_prints_the_roots_python_computes(tmp_path):
    """examples/merkle_sequence.c compiles as C99 against include/distaff_hip.h and the product library and runs on the host"""
    assert run_example(tmp_path, 3, 9, -1) == example_roots(host_tree, 3, 9)


def test_package_lists_the_calls():
    import distaff_amd as D
    assert D.path_tapes is not None and {"dst_rtree_apply", "dst_stree_apply", "dst_rescue_path_tapes"} <= set(D.EXPORTS)
