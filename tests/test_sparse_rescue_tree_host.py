"""Sparse Rescue Merkle trees (dst_stree_*) on the host path (device = -1) of the PRODUCT library.  No GPU.  A sparse tree of depth D is defined
as the dense tree over 2^D leaves with the empty leaf wherever no key was set, so the yardstick up to depth 8 is the dense host RescueTree
(which tests/test_rescue_tree_host.py holds against the oracle), node by node and path by path; at depth 63, where no dense tree exists, it is
the oracle's hasher_digest.  Everything is bit-exact.  Also here: the helpers the emulated and the GPU tests of the sparse trees share."""
import os
import random
import subprocess

import numpy as np
import pytest

from test_rescue_tree_host import P, _product, merkle_root, random_leaves  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONZERO_EMPTY = (7, P - 1)


def host_sparse(depth, empty=(0, 0)):
    import distaff_amd as D
    return D.SparseRescueTree(depth, empty, device=-1, lib=_product())


def host_dense(leaves):
    import distaff_amd as D
    return D.RescueTree(leaves, device=-1, lib=_product())


def random_pairs(count, seed):
    rnd = random.Random(seed)
    return [(rnd.randrange(P), rnd.randrange(P)) for _ in range(count)]


def dense_leaves(depth, content, empty):
    """the leaf array of the dense tree a sparse tree with `content` (key -> leaf) stands for"""
    return [content.get(i, tuple(empty)) for i in range(1 << depth)]


def ancestors(keys, depth):
    """digests one set of `keys` computes: the distinct index >> (depth - l) over the levels l < depth"""
    return sum(len({k >> (depth - l) for k in keys}) for l in range(depth))


def levels_of(tree):
    return [tree.level(l) for l in range(tree.depth + 1)]


def assert_same_levels(a, b):
    assert len(a) == len(b)
    for l, ((pa, na), (pb, nb)) in enumerate(zip(a, b)):
        assert np.array_equal(pa, pb), l
        assert np.array_equal(na, nb), l


def check_against_dense(tree, dense, keys):
    """every level's prefixes are the sorted distinct key >> (D - l), every stored node is the dense tree's node (1 << l) + prefix, equal roots"""
    depth = tree.depth
    for l in range(depth + 1):
        prefixes, nodes = tree.level(l)
        want = sorted({k >> (depth - l) for k in keys})
        assert [int(q) for q in prefixes] == want, l
        for q, node in zip(want, nodes):
            assert np.array_equal(node, dense.nodes((1 << l) + q, 1)[0]), (l, q)
    assert tree.root == dense.root
    info = tree.info()
    assert info["keys"] == len(set(keys)) and info["nodes"] == sum(len({k >> (depth - l) for k in keys}) for l in range(depth + 1))


def check_all_openings(tree, dense):
    """paths and tapes of ALL 2^D indices, absent ones included"""
    every = list(range(1 << tree.depth))
    assert tree.paths(every) == dense.paths(every)
    assert tree.tapes_many(every) == dense.tapes_many(every)
    assert tree.path(every[-1]) == dense.path(every[-1]) and tree.tapes(0, what=2) == dense.tapes(0, what=2)
    assert tree.paths([]) == [] and tree.tapes_many([]) == []


def key_sets(depth, seed):
    rnd = random.Random(seed)
    n = 1 << depth
    k = rnd.randrange(n) & ~1
    sets = [[], [rnd.randrange(n)], list(range(n)), [k, k ^ 1]]                    # none, one, all, a cluster that shares all but the last bit
    sets += [rnd.sample(range(n), max(1, n // 3)), rnd.sample(range(n), max(1, (2 * n) // 3))]
    for s in sets:
        rnd.shuffle(s)
    return sets


@pytest.mark.parametrize("empty", [(0, 0), NONZERO_EMPTY])
@pytest.mark.parametrize("depth", range(1, 9))
def test_every_node_path_and_tape_equals_the_dense_tree(depth, empty):
    for case, keys in enumerate(key_sets(depth, 300 + depth)):
        content = dict(zip(keys, random_pairs(len(keys), 1000 * depth + case)))
        tree = host_sparse(depth, empty)
        tree.set(keys, [content[k] for k in keys])
        assert tree.info()["last_digests"] == ancestors(keys, depth)
        dense = host_dense(dense_leaves(depth, content, empty))
        check_against_dense(tree, dense, keys)
        check_all_openings(tree, dense)
        tree.close(); dense.close()


def empty_chain(O, empty, depth):
    """[E_0 .. E_depth] by the oracle"""
    e = [tuple(empty)]
    for _ in range(depth):
        e.append(tuple(O.hasher_digest([*e[-1], *e[-1]])))
    return e[::-1]


@pytest.mark.parametrize("empty", [(0, 0), NONZERO_EMPTY])
def test_depth_63_empty_tree_has_the_root_of_63_digests_of_the_empty_leaf(oracle, empty):
    tree = host_sparse(63, empty)
    chain = empty_chain(oracle, empty, 63)
    assert tree.root == chain[0]
    assert tree.info() == {"depth": 63, "device": -1, "keys": 0, "nodes": 0, "last_digests": 0, "last_device_ms": 0.0}
    path = tree.path(2 ** 63 - 1)                                                   # a proof that the key is empty
    assert path == [chain[63]] + [chain[63 - k] for k in range(63)]
    assert all(len(tree.level(l)[0]) == 0 for l in range(64))
    tree.close()


def depth_63_keys(seed, count=64):
    """0, 2^63 - 1, a pair k, k ^ 1, a pair that differs only in the top bit, random ones"""
    rnd = random.Random(seed)
    k, t = rnd.randrange(1 << 63), rnd.randrange(1 << 62)
    keys = {0, 2 ** 63 - 1, k, k ^ 1, t, t | (1 << 62)}
    while len(keys) < count:
        keys.add(rnd.randrange(1 << 63))
    keys = list(keys)
    rnd.shuffle(keys)
    return keys


def test_depth_63_paths_of_present_and_absent_keys_recompute_to_the_root(oracle):
    import distaff_amd as D
    rnd = random.Random(63)
    keys = depth_63_keys(64)
    content = dict(zip(keys, random_pairs(64, 65)))
    tree = host_sparse(63)
    tree.set(keys, [content[k] for k in keys])
    assert tree.info()["last_digests"] == ancestors(keys, 63) and tree.info()["keys"] == 64
    root = tree.root
    absent = [keys[0] ^ 2, keys[1] ^ (1 << 62)] + [rnd.randrange(1 << 63) for _ in range(14)]
    assert not set(absent) & set(keys)
    for i, path in zip(keys + absent, tree.paths(keys + absent)):
        assert len(path) == 64 and path[0] == content.get(i, (0, 0))
        assert merkle_root(path, i)(oracle.hasher_digest) == root, i
    # one path digest by digest: the stored ancestors of keys[0] are the oracle's digests of (node, path sibling) all the way up
    i, path = keys[0], tree.path(keys[0])
    v = content[i]
    for k in range(1, 64):
        q = i >> (k - 1)
        v = tuple(oracle.hasher_digest([*v, *path[k]] if q & 1 == 0 else [*path[k], *v]))
        prefixes, nodes = tree.level(63 - k)
        at = [int(x) for x in prefixes].index(q >> 1)
        assert tuple(D.arr_to_ints(nodes[at])) == v, k
    assert v == root
    tree.close()


def check_set_sequence(make, depth, steps, empty=(0, 0), also=None):
    """after every set of `steps` (lists of (key, leaf)): all levels equal a fresh tree set once with the union (built by `make`, and by `also`),
    last_digests is the distinct-ancestor count of that set"""
    tree = make(depth, empty)
    content = {}
    for step in steps:
        keys = [k for k, _ in step]
        tree.set(keys, [v for _, v in step])
        content.update(step)
        assert tree.info()["last_digests"] == ancestors(keys, depth), keys
        for build in (make, also) if also else (make,):
            fresh = build(depth, empty)
            fresh.set(list(content), list(content.values()))
            assert_same_levels(levels_of(tree), levels_of(fresh))
            assert tree.root == fresh.root
            fresh.close()
    tree.close()
    return content


def set_sequence(depth, seed, empty=(0, 0)):
    """new keys only, stored keys only, a mix, a key set to the empty value, count = 0, more new keys"""
    rnd = random.Random(seed)
    n = 1 << depth
    first = rnd.sample(range(n), min(n, 5)) if depth < 63 else depth_63_keys(seed, 6)
    rest = [k for k in (range(n) if depth < 63 else {rnd.randrange(n) for _ in range(8)}) if k not in first]
    rnd.shuffle(rest)
    leaf = lambda: (rnd.randrange(P), rnd.randrange(P))  # noqa: E731
    steps = [[(k, leaf()) for k in first],
             [(k, leaf()) for k in first[::2]],
             [(k, leaf()) for k in first[1:3] + rest[:3]],
             [(first[0], tuple(empty))],
             [],
             [(k, leaf()) for k in rest[3:7]]]
    return steps


@pytest.mark.parametrize("depth,empty", [(1, (0, 0)), (3, NONZERO_EMPTY), (6, (0, 0)), (63, NONZERO_EMPTY)])
def test_set_sequences_equal_a_fresh_tree_of_the_union(depth, empty):
    content = check_set_sequence(host_sparse, depth, set_sequence(depth, 70 + depth, empty), empty)
    if depth <= 6:                                                                  # ... and the dense tree, the key set to the empty value included
        tree = host_sparse(depth, empty)
        tree.set(list(content), list(content.values()))
        dense = host_dense(dense_leaves(depth, content, empty))
        check_against_dense(tree, dense, list(content))
        check_all_openings(tree, dense)
        tree.close(); dense.close()


def test_argument_errors_never_abort_and_leave_the_tree_unchanged():
    import ctypes
    import distaff_amd as D
    lib = _product()
    h = ctypes.c_void_p()
    for depth in (0, 64, 1 << 20):
        assert lib.dst_stree_create(-1, depth, None, ctypes.byref(h)) == D.DST_ERR_ARG and not h.value
    assert lib.dst_stree_create(-1, 5, None, None) == D.DST_ERR_ARG
    with pytest.raises(D.DistaffError) as e:
        host_sparse(5, (P, 0))
    assert e.value.code == D.DST_ERR_ARG
    buf = ctypes.create_string_buffer(64 * 32)
    assert lib.dst_stree_root(None, buf) == D.DST_ERR_ARG and lib.dst_stree_set(None, None, None, ctypes.c_size_t(0)) == D.DST_ERR_ARG
    for depth in (5, 63):
        tree = host_sparse(depth)
        top = 1 << depth
        tree.set([1, top - 1], [(1, 2), (3, 4)])
        before = (tree.root, tree.info(), [(p.tolist(), n.tolist()) for p, n in levels_of(tree)])
        bad_sets = [([top], [(1, 1)]), ([3, top], [(1, 1), (2, 2)]), ([3, 4, 3], [(1, 1), (2, 2), (3, 3)]), ([1, 1], [(1, 1), (2, 2)]),
                    ([3], [(P, 0)]), ([3, 4], [(1, 1), (5, P)]), ([6], [(2 ** 128 - 1, 0)])]
        if depth < 63:
            bad_sets.append(([1 << 63], [(1, 1)]))
        for keys, leaves in bad_sets:
            with pytest.raises(D.DistaffError) as e:
                tree.set(keys, leaves)
            assert e.value.code == D.DST_ERR_ARG, keys
        idx = np.array([3], dtype=np.uint64)
        assert lib.dst_stree_set(tree._h, None, buf, ctypes.c_size_t(1)) == D.DST_ERR_ARG
        assert lib.dst_stree_set(tree._h, idx.ctypes.data_as(ctypes.c_void_p), None, ctypes.c_size_t(1)) == D.DST_ERR_ARG
        assert lib.dst_stree_paths(tree._h, None, ctypes.c_size_t(1), buf) == D.DST_ERR_ARG
        assert lib.dst_stree_paths(tree._h, idx.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1), None) == D.DST_ERR_ARG
        assert lib.dst_stree_root(tree._h, None) == D.DST_ERR_ARG and lib.dst_stree_info(tree._h, None) == D.DST_ERR_ARG
        for call in (lambda: tree.path(top), lambda: tree.tapes(top), lambda: tree.tapes(0, what=0), lambda: tree.tapes(0, what=4), lambda: tree.level(depth + 1)):
            with pytest.raises(D.DistaffError) as e:
                call()
            assert e.value.code == D.DST_ERR_ARG
        m = ctypes.c_uint64(77)
        assert lib.dst_stree_read_level(tree._h, depth, ctypes.c_uint64(1), ctypes.c_uint64(2), None, None, ctypes.byref(m)) == D.DST_ERR_ARG and m.value == 2
        assert (tree.root, tree.info(), [(p.tolist(), n.tolist()) for p, n in levels_of(tree)]) == before
        assert lib.dst_stree_set(tree._h, None, None, ctypes.c_size_t(0)) == D.DST_OK and tree.root == before[0]      # a set of nothing is no error
        tree.close()
        tree.close()


def test_levels_bookkeeping_against_a_map_model_under_sanitizers(tmp_path):
    """tests/sparse_host/stree_levels_check.cpp drives host/stree_levels.h alone (the merge, the carry-over sources, the dirty lists, the lookups)
    against a std::map model, built with -fsanitize=address,undefined and run as a program: exit status 0, nothing on stderr"""
    exe = str(tmp_path / "stree_levels_check")
    subprocess.check_call(["g++", "-std=c++17", "-w", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sparse_host", "stree_levels_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    assert b"rounds ok" in r.stdout


def test_package_reexports_the_binding():
    import distaff_amd as D
    assert D.SparseRescueTree is not None
    assert {"dst_stree_create", "dst_stree_set", "dst_stree_root", "dst_stree_paths", "dst_stree_tapes_many", "dst_stree_read_level", "dst_stree_info",
            "dst_stree_destroy", "dst_stree_last_error"} <= set(D.EXPORTS)
