"""Compressed batch openings (dst_rescue_multiproof_size, dst_rtree_multiproof, dst_stree_multiproof, dst_rescue_multiproof_root,
dst_rescue_verify_multiproof, dst_rescue_multiproof_paths) on the host path (device = -1) of the PRODUCT library.  No GPU.  The yardsticks are
independent of the new code: the trees' own node arrays, paths and roots (read_nodes, paths, root -- calls that existed before), the reference's
walk restated in tests/test_rescue_path_verify_host.py, and a restatement here of the definition -- K_l, the supplied positions and the digest
count of a set -- with which the expected multiproof is assembled out of full paths.  Everything is bit-exact.  The checkers take `device`, `lib`
and the trees' constructors, so tests/test_rescue_multiproof_emulated.py and tests/test_rescue_multiproof_gpu.py run the same cases on the
device path."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

from test_rescue_path_verify_host import flip, merkle_roots_batched
from test_rescue_tree_host import P, _product, random_leaves
from test_rescue_tree_update_host import host_tree
from test_sparse_rescue_tree_host import NONZERO_EMPTY, host_sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the expectations of the reference's own tests (src/crypto/merkle.rs:427-493 and :513), re-ordered level by level: indices -> heap positions, digests
D3_TABLE = [([1], [8, 5, 3], 3), ([1, 2], [8, 11, 3], None), ([1, 6], [8, 15, 5, 6], None), ([1, 3, 6], [8, 10, 15, 6], 6), (list(range(8)), [], 7)]


# ---- the definition, restated ----------------------------------------------------------------------------------------------------------------
def restate(indices, depth):
    """-> (supplied [(level, position)] in the order of `nodes`, digests): K_D = S, K_{l-1} = {p >> 1}; the supplied siblings of level l are the
    (l, p ^ 1) with p in K_l and p ^ 1 not in K_l, ascending by position, level D first; digests = sum of |K_l| over l < D"""
    level = set(indices)
    assert len(level) == len(indices)
    supplied, digests = [], 0
    for l in range(depth, 0, -1):
        supplied += [(l, q) for q in sorted(p ^ 1 for p in level if p ^ 1 not in level)]
        level = {p >> 1 for p in level}
        digests += len(level)
    return supplied, digests


def expected_multiproof(indices, paths, depth):
    """the multiproof assembled out of full paths: leaves[i] = node 0 of path i; node k >= 1 of the path of index i is the sibling
    (depth - k + 1, (i >> (k - 1)) ^ 1), so the supplied (l, q) is node depth - l + 1 of any path whose index has i >> (depth - l) == q ^ 1"""
    supplied, digests = restate(indices, depth)
    owner = {}
    for i, path in zip(indices, paths):
        for l in range(1, depth + 1):
            owner.setdefault((l, (i >> (depth - l)) ^ 1), path[depth - l + 1])
    return [tuple(p[0]) for p in paths], [tuple(owner[s]) for s in supplied], digests


def random_nodes(count, seed):
    rnd = random.Random(seed)
    return [(rnd.randrange(P), rnd.randrange(P)) for _ in range(count)]


def sparse_case(make_sparse, stored_count, absent_count, seed, depth=63):
    """a sparse tree with `stored_count` random keys (the ends of the key range among them) and the distinct keys to open: all stored ones and
    `absent_count` that are not, neighbours of stored keys among them, shuffled"""
    rnd = random.Random(seed)
    top = (1 << depth) - 1
    stored = set([0, top][:stored_count])
    while len(stored) < stored_count:
        stored.add(rnd.randrange(1 << depth))
    stored = sorted(stored)
    absent = {k ^ 1 for k in stored[:absent_count // 2]} - set(stored)
    while len(absent) < absent_count:
        k = rnd.randrange(1 << depth)
        if k not in stored:
            absent.add(k)
    tree = make_sparse(depth, NONZERO_EMPTY)
    tree.set(stored, random_nodes(len(stored), seed + 1))
    keys = stored + sorted(absent)
    rnd.shuffle(keys)
    return tree, keys


# ---- the checkers: device and lib say which path runs the tree-less calls, make / make_sparse where the trees live ----------------------------
def check_d3_table(device, lib, make):
    """1. the five D = 3 cases by heap position against the tree's node array"""
    import distaff_amd as D
    tree = make(random_leaves(3, 301))
    node = D.lib._pairs(tree.nodes(0, 16))
    for indices, heap, digests in D3_TABLE:
        leaves, nodes = tree.multiproof(indices)
        assert nodes == [node[h] for h in heap], indices
        assert leaves == [node[8 + i] for i in indices], indices
        stats = {}
        assert D.multiproof_root(4, indices, leaves, nodes, device=device, lib=lib, stats=stats) == tree.root, indices
        assert D.multiproof_size(4, indices, lib=lib) == (len(heap), stats["digests"])
        assert digests is None or stats["digests"] == digests, indices
        assert [(l, p) for l, p in restate(indices, 3)[0]] == [(h.bit_length() - 1, h - (1 << (h.bit_length() - 1))) for h in heap]
    tree.close()


def check_sizes(lib):
    """2. multiproof_size against the restatement: every non-empty subset for D = 1, 2, 3; the ends of the key range at D = 63"""
    import distaff_amd as D
    sets = 0
    for depth in (1, 2, 3):
        every = list(range(1 << depth))
        for r in range(1, len(every) + 1):
            for subset in itertools.combinations(every, r):
                supplied, digests = restate(subset, depth)
                assert D.multiproof_size(depth + 1, list(subset), lib=lib) == (len(supplied), digests), (depth, subset)
                sets += depth == 3
    assert sets == 255
    keys = [0, 1, 1 << 62, (1 << 63) - 1]
    supplied, digests = restate(keys, 63)
    assert D.multiproof_size(64, keys, lib=lib) == (len(supplied), digests)
    assert D.multiproof_size(64, keys[::-1], lib=lib) == (len(supplied), digests)
    assert D.multiproof_size(4, [], lib=lib) == (0, 0)


def check_tree(device, lib, tree, indices, depth, seed, update=False):
    """3. one tree and one set: the multiproof is the restatement over the tree's paths and does not depend on the order of the indices; it
    resolves to the tree's root in `digests` digests; it expands into the tree's paths byte for byte; (dense) with new leaves it gives the root
    after dst_rtree_update of those leaves.  Closes the tree."""
    import distaff_amd as D
    n = depth + 1
    paths = tree.paths(indices)
    want_leaves, want_nodes, want_digests = expected_multiproof(indices, paths, depth)
    leaves, nodes = tree.multiproof(indices)
    assert (leaves, nodes) == (want_leaves, want_nodes)
    shuffled = list(range(len(indices)))
    random.Random(seed).shuffle(shuffled)
    again_leaves, again_nodes = tree.multiproof([indices[j] for j in shuffled])
    assert again_nodes == nodes and again_leaves == [leaves[j] for j in shuffled]          # the nodes stay, the leaves follow the shuffle
    stats = {}
    root = tree.root
    assert D.multiproof_root(n, indices, leaves, nodes, device=device, lib=lib, stats=stats) == root
    assert stats["digests"] == want_digests and stats["device_ms"] >= 0 and (device >= 0 or stats["device_ms"] == 0)
    assert D.multiproof_size(n, indices, lib=lib) == (len(nodes), want_digests)
    assert D.verify_multiproof(root, n, indices, leaves, nodes, device=device, lib=lib) is True
    assert D.verify_multiproof(flip(root), n, indices, leaves, nodes, device=device, lib=lib) is False
    if nodes:
        bent = list(nodes)
        bent[len(nodes) // 2] = flip(bent[len(nodes) // 2], 1, 70)
        assert D.verify_multiproof(root, n, indices, leaves, bent, device=device, lib=lib) is False      # one tampered node: ok = 0, not an error
    assert D.multiproof_paths(n, indices, leaves, nodes, device=device, lib=lib) == (paths, root)
    assert D.multiproof_paths(n, [indices[j] for j in shuffled], again_leaves, nodes, device=device, lib=lib) == ([paths[j] for j in shuffled], root)
    if update:
        new = random_nodes(len(indices), seed + 1)
        after = D.multiproof_root(n, indices, new, nodes, device=device, lib=lib)
        tree.update(indices, new)
        assert after == tree.root != root
    tree.close()


def check_dense(device, lib, make, log_leaves=(1, 4)):
    for k in log_leaves:
        rnd = random.Random(310 + k)
        for count in sorted({1, min(5, 1 << k), 1 << k}):
            indices = rnd.sample(range(1 << k), count)
            check_tree(device, lib, make(random_leaves(k, 320 + k)), indices, k, 330 + k, update=True)


def check_sparse(device, lib, make_sparse, stored=3, absent=3):
    tree, keys = sparse_case(make_sparse, stored, absent, 340)
    check_tree(device, lib, tree, keys, 63, 341)
    tree = make_sparse(63, NONZERO_EMPTY)                                                    # a tree without keys: every node is an E_l
    check_tree(device, lib, tree, [5, 1 << 62], 63, 342)


def check_every_single_tampering(device, lib, make, log_leaves=4, count=5):
    """4. one flipped byte in any single leaf or any single supplied node: ok = 0 with DST_OK, every one of them"""
    import distaff_amd as D
    tree = make(random_leaves(log_leaves, 350))
    indices = random.Random(351).sample(range(1 << log_leaves), count)
    leaves, nodes = tree.multiproof(indices)
    root, n = tree.root, log_leaves + 1
    tree.close()
    assert D.verify_multiproof(root, n, indices, leaves, nodes, device=device, lib=lib) is True
    for j in range(len(leaves)):
        bent = list(leaves)
        bent[j] = flip(bent[j], j & 1, 8 * (j % 15))
        assert D.verify_multiproof(root, n, indices, bent, nodes, device=device, lib=lib) is False, j
    assert nodes
    for j in range(len(nodes)):
        bent = list(nodes)
        bent[j] = flip(bent[j], 1 - (j & 1), 8 * (j % 15) + 3)
        assert D.verify_multiproof(root, n, indices, leaves, bent, device=device, lib=lib) is False, j
        assert D.multiproof_root(n, indices, leaves, bent, device=device, lib=lib) != root


def check_rejections(device, lib, make, make_sparse):
    """5. every DST_ERR_ARG case; after a refused tree-side call the tree is unchanged"""
    import distaff_amd as D
    k, n = 3, 4
    tree = make(random_leaves(k, 360))
    sparse = make_sparse(k, NONZERO_EMPTY)
    sparse.set([1, 6], random_nodes(2, 361))
    before = (D.lib._pairs(tree.nodes(0, 16)), [sparse.level(l)[1].tolist() for l in range(k + 1)])
    indices = [6, 1, 3]
    leaves, nodes = tree.multiproof(indices)
    root = tree.root
    calls = {"root": lambda i=indices, v=leaves, s=nodes, nn=n: D.multiproof_root(nn, i, v, s, device=device, lib=lib),
             "verify": lambda i=indices, v=leaves, s=nodes, nn=n: D.verify_multiproof(root, nn, i, v, s, device=device, lib=lib),
             "paths": lambda i=indices, v=leaves, s=nodes, nn=n: D.multiproof_paths(nn, i, v, s, device=device, lib=lib),
             "size": lambda i=indices, v=leaves, s=nodes, nn=n: D.multiproof_size(nn, i, lib=lib),
             "rtree": lambda i=indices, v=leaves, s=nodes, nn=n: tree.multiproof(i),
             "stree": lambda i=indices, v=leaves, s=nodes, nn=n: sparse.multiproof(i)}
    hashing = ("root", "verify", "paths")

    def refused(what, cause, **kw):
        with pytest.raises(D.DistaffError) as e:
            calls[what](**kw)
        assert e.value.code == D.DST_ERR_ARG and cause in e.value.reason, (what, kw.keys(), e.value.reason)

    for what in calls:
        calls[what]()                                                                               # the untouched arguments are accepted
        refused(what, "past the end", i=[6, 1, 8])
        refused(what, "repeated", i=[6, 1, 6])
        if what in hashing or what == "size":
            for bad_n in (1, 65, 0):
                refused(what, "2 .. 64 nodes", nn=bad_n, i=[0, 0, 0][:len(indices)])
        if what in hashing:
            refused(what, "num_nodes", s=nodes[:-1])
            refused(what, "num_nodes", s=nodes + nodes[:1])
            refused(what, "proves nothing", i=[], v=[], s=[])
            refused(what, "as many leaves", v=leaves[:-1])                                          # found by the binding
            for big in (P, 2 ** 128 - 1):
                refused(what, "not below the modulus", v=leaves[:-1] + [(leaves[-1][0], big)])
                refused(what, "not below the modulus", v=[(big, leaves[0][1])] + leaves[1:])
                refused(what, "not below the modulus", s=nodes[:-1] + [(nodes[-1][0], big)])
                refused(what, "not below the modulus", s=[(big, nodes[0][1])] + nodes[1:])
    assert tree.multiproof([]) == ([], []) and sparse.multiproof([]) == ([], [])                   # count = 0: DST_OK with 0 nodes
    # the C-ABI itself: null pointers with count > 0, a node buffer that is too small, count >= 2^31, before anything is read
    idx, buf, m, d = (ctypes.c_uint64 * 3)(*indices), ctypes.create_string_buffer(32 * 8), ctypes.c_size_t(7), ctypes.c_uint64(7)
    three, dev, ok = ctypes.c_size_t(3), ctypes.c_int(device), ctypes.c_int(7)
    error = lambda: D.lib._rtree_error(lib)  # noqa: E731
    assert lib.dst_rescue_multiproof_size(4, None, three, ctypes.byref(m), ctypes.byref(d)) == D.DST_ERR_ARG and "null pointer" in error()
    assert lib.dst_rescue_multiproof_size(4, idx, three, None, ctypes.byref(d)) == D.DST_ERR_ARG
    assert lib.dst_rescue_multiproof_size(4, idx, three, ctypes.byref(m), None) == D.DST_ERR_ARG
    assert lib.dst_rescue_multiproof_size(4, idx, ctypes.c_size_t(1 << 31), ctypes.byref(m), ctypes.byref(d)) == D.DST_ERR_ARG and "2^31" in error()
    assert lib.dst_rescue_multiproof_size(4, idx, three, ctypes.byref(m), ctypes.byref(d)) == D.DST_OK and (m.value, d.value) == (len(nodes), restate(indices, 3)[1])
    two = ctypes.c_size_t(len(nodes))
    assert lib.dst_rescue_multiproof_root(dev, 4, None, buf, three, buf, two, buf, None, None) == D.DST_ERR_ARG and "null pointer" in error()
    assert lib.dst_rescue_multiproof_root(dev, 4, idx, None, three, buf, two, buf, None, None) == D.DST_ERR_ARG
    assert lib.dst_rescue_multiproof_root(dev, 4, idx, buf, three, None, two, buf, None, None) == D.DST_ERR_ARG
    assert lib.dst_rescue_multiproof_root(dev, 4, idx, buf, three, buf, two, None, None, None) == D.DST_ERR_ARG
    assert lib.dst_rescue_multiproof_root(dev, 4, idx, buf, ctypes.c_size_t(1 << 31), buf, two, buf, None, None) == D.DST_ERR_ARG and "2^31" in error()
    assert lib.dst_rescue_verify_multiproof(dev, None, 4, idx, buf, three, buf, two, ctypes.byref(ok), None) == D.DST_ERR_ARG
    assert lib.dst_rescue_verify_multiproof(dev, buf, 4, idx, buf, three, buf, two, None, None) == D.DST_ERR_ARG
    assert lib.dst_rescue_multiproof_paths(dev, 4, idx, buf, three, buf, two, None, buf, None) == D.DST_ERR_ARG
    assert lib.dst_rescue_multiproof_paths(dev, 4, idx, buf, three, buf, two, buf, None, None) == D.DST_ERR_ARG
    for t, call in ((tree, tree.lib.dst_rtree_multiproof), (sparse, sparse.lib.dst_stree_multiproof)):
        assert call(t._h, None, three, buf, buf, ctypes.c_size_t(8), ctypes.byref(m)) == D.DST_ERR_ARG
        assert call(t._h, idx, three, buf, buf, ctypes.c_size_t(8), None) == D.DST_ERR_ARG
        assert call(t._h, idx, three, None, buf, ctypes.c_size_t(8), ctypes.byref(m)) == D.DST_ERR_ARG
        assert call(t._h, idx, three, buf, buf, ctypes.c_size_t(len(nodes) - 1), ctypes.byref(m)) == D.DST_ERR_ARG and m.value == len(nodes)
        assert call(t._h, idx, ctypes.c_size_t(1 << 31), buf, buf, ctypes.c_size_t(8), ctypes.byref(m)) == D.DST_ERR_ARG
        assert call(t._h, idx, three, None, None, ctypes.c_size_t(0), ctypes.byref(m)) == D.DST_OK and m.value == len(nodes)      # the size query
        assert call(None, idx, three, buf, buf, ctypes.c_size_t(8), ctypes.byref(m)) == D.DST_ERR_ARG
    assert (D.lib._pairs(tree.nodes(0, 16)), [sparse.level(l)[1].tolist() for l in range(k + 1)]) == before
    assert tree.root == root and tree.multiproof(indices) == (leaves, nodes)
    tree.close(); sparse.close()


def check_pool_limit(lib):
    """count + M + digests >= 2^32 is refused by the size query and by the hashing calls before they read a leaf: 2^26 keys spread over the 63-bit
    range share almost nothing, so M + digests is about 2^26 * 2 * 37"""
    import numpy as np
    import distaff_amd as D
    count = 1 << 26
    keys = (np.arange(count, dtype=np.uint64) << np.uint64(37)) | np.uint64(1)
    m, d = ctypes.c_size_t(0), ctypes.c_uint64(0)
    ip = keys.ctypes.data_as(ctypes.c_void_p)
    assert lib.dst_rescue_multiproof_size(64, ip, ctypes.c_size_t(count), ctypes.byref(m), ctypes.byref(d)) == D.DST_ERR_ARG
    assert "2^32" in D.lib._rtree_error(lib)
    buf = ctypes.create_string_buffer(32)
    assert lib.dst_rescue_multiproof_root(ctypes.c_int(-1), 64, ip, buf, ctypes.c_size_t(count), buf, ctypes.c_size_t(1), buf, None, None) == D.DST_ERR_ARG
    assert "2^32" in D.lib._rtree_error(lib)


# ---- the host path ----------------------------------------------------------------------------------------------------------------------------
def test_the_reference_cases_of_depth_3_by_heap_position():
    check_d3_table(-1, _product(), host_tree)


def test_sizes_equal_the_restatement_for_every_subset_and_at_depth_63():
    check_sizes(_product())


def test_dense_trees_root_expansion_digest_count_order_and_unordered_writes():
    check_dense(-1, _product(), host_tree)


def test_sparse_depth_63_with_stored_and_absent_keys_mixed():
    check_sparse(-1, _product(), host_sparse, stored=9, absent=8)


def test_every_single_flipped_leaf_or_node_gives_ok_0():
    check_every_single_tampering(-1, _product(), host_tree)


def test_what_is_refused_and_the_trees_stay_unchanged():
    check_rejections(-1, _product(), host_tree, host_sparse)


def test_a_pool_of_2_32_nodes_is_refused_before_anything_is_read():
    check_pool_limit(_product())


def test_expanded_paths_are_what_the_path_checks_and_the_tapes_take():
    """the expansion travels where paths used to: path_roots over it (the reference's walk, existing code) gives the root for every index, and
    path_tapes over it equals the tree's own tapes"""
    import distaff_amd as D
    k = 5
    tree = host_tree(random_leaves(k, 370))
    indices = random.Random(371).sample(range(1 << k), 9)
    leaves, nodes = tree.multiproof(indices)
    paths, root = D.multiproof_paths(k + 1, indices, leaves, nodes, device=-1, lib=_product())
    assert merkle_roots_batched(paths, indices) == [tree.root] * len(indices) and root == tree.root
    assert D.path_tapes(paths, indices, lib=_product()) == tree.tapes_many(indices)
    tree.close()


def test_plan_against_a_model_under_sanitizers(tmp_path):
    """tests/multiproof/multiproof_plan_check.cpp drives host/multiproof_plan.h alone -- supplied positions, job lists, path node indices -- against
    a model over std::set on random and exhaustive small sets, built with -fsanitize=address,undefined and run as a program"""
    exe = str(tmp_path / "multiproof_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-w", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "multiproof", "multiproof_plan_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    assert b"sets ok" in r.stdout


def run_example(tmp_path, k, count, device):
    import distaff_amd as D
    exe = tmp_path / "merkle_multiproof"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_multiproof.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    r = subprocess.run([str(exe), str(k), str(count), str(device)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()
    return r.stdout.decode().splitlines()


def example_lines(k, count):
    """what examples/merkle_multiproof.c prints for k and count: the sizes follow from the restatement over the example's indices"""
    n = 1 << k
    indices = sorted({(7 * j * j + 3 * j + 1) & (n - 1) for j in range(count)})
    supplied, digests = restate(indices, k)
    return ["%d leaves of 2^%d: multiproof %d bytes against %d bytes of paths" % (len(indices), k, 32 * (len(indices) + len(supplied)), 32 * len(indices) * (k + 1)),
            "verified against the root alone: %d digests against %d" % (digests, len(indices) * k),
            "a tampered node is rejected",
            "the expanded paths equal dst_rtree_paths'"]


def test_c_example_takes_verifies_and_expands_a_multiproof(tmp_path):
    """examples/merkle_multiproof.c compiles as C99 against include/distaff_hip.h and the product library and runs on the host"""
    assert run_example(tmp_path, 6, 20, -1) == example_lines(6, 20)


def test_package_lists_the_calls():
    import distaff_amd as D
    assert {"dst_rescue_multiproof_size", "dst_rtree_multiproof", "dst_stree_multiproof", "dst_rescue_multiproof_root", "dst_rescue_verify_multiproof",
            "dst_rescue_multiproof_paths"} <= set(D.EXPORTS)
    assert D.multiproof_size is not None and D.multiproof_root is not None and D.verify_multiproof is not None and D.multiproof_paths is not None
    assert D.RescueTree.multiproof is not None and D.SparseRescueTree.multiproof is not None
