"""Sparse Rescue Merkle trees on the GPU (rescue_stree_level_kernel, rescue_stree_level_spread_kernel, rescue_stree_carry_kernel,
rescue_stree_open_kernel) through the library the session binds.  Up to depth 20 the yardstick is the dense DEVICE tree over the same leaves with
the empty leaf elsewhere -- code that tests/test_rescue_tree_gpu.py holds against the host path and the oracle -- node by node; at depth 63 it is
the host sparse tree, which tests/test_sparse_rescue_tree_host.py holds against the dense host tree and the oracle.  Everything is bit-exact.
Every test has its own time limit and nothing is run twice."""
import os
import random
import subprocess

import numpy as np
import pytest

from test_rescue_tree_host import merkle_root, merkle_source
from test_sparse_rescue_tree_host import ancestors, assert_same_levels, levels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SPREAD_MAX = 1 << 15                       # RESCUE_SPREAD_MAX: launches of more parents run the one-lane kernel


def random_words(count, seed):
    """uint64 words [count, 2, 2] of uniformly random canonical elements"""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(count, 2, 2), dtype=np.uint64)
    a[..., 1] >>= np.uint64(1)                           # high word below 2^63: below p
    return a


def assert_levels_equal_dense(tree, dense, keys):
    """level l's prefixes are the sorted distinct key >> (D - l) and its nodes the dense tree's nodes (1 << l) + prefix: every stored node"""
    depth = tree.depth
    node = dense.nodes(0, 2 << depth)
    keys = np.asarray(keys, dtype=np.uint64)
    for l in range(depth + 1):
        prefixes, nodes = tree.level(l)
        want = np.unique(keys >> np.uint64(depth - l))
        assert np.array_equal(prefixes, want), l
        assert np.array_equal(nodes, node[(1 << l) + want.astype(np.int64)]), l
    assert tree.root == dense.root


@pytest.mark.timeout(120)
def test_depth_12_every_node_and_every_path_equals_the_dense_device_tree_and_the_host_tree():
    import distaff_amd as D
    depth, n = 12, 1 << 12
    rnd = random.Random(12)
    keys = set(range(2048, 2048 + 300)) | {k ^ b for k in rnd.sample(range(n), 100) for b in (0, 1, 2, 3)}      # clusters ...
    while len(keys) < 1500:
        keys.add(rnd.randrange(n))                                                                              # ... and random keys
    keys = list(keys)
    rnd.shuffle(keys)
    new = random_words(len(keys), 121)
    leaves = np.zeros((n, 2, 2), dtype=np.uint64)
    leaves[np.array(keys)] = new
    tree = D.SparseRescueTree(depth, device=0)
    tree.set(keys, new)
    assert tree.info()["last_digests"] == ancestors(keys, depth) and tree.info()["last_device_ms"] > 0
    dense = D.RescueTree(leaves, device=0)
    assert_levels_equal_dense(tree, dense, keys)
    host = D.SparseRescueTree(depth, device=-1)
    host.set(keys, new)
    assert_same_levels(levels_of(tree), levels_of(host))
    every = list(range(n))
    assert tree.paths(every) == dense.paths(every)                                  # all 4 096 indices, the absent ones included
    some = rnd.sample(every, 16)
    assert tree.paths(some) == host.paths(some) and tree.tapes_many(some) == dense.tapes_many(some)
    tree.close(); dense.close(); host.close()


@pytest.mark.timeout(180)
def test_depth_20_both_level_kernels_whole_levels_and_dirty_lists():
    """2^16 + 2^15 random keys: the lowest levels have more than 2^15 parents (the one-lane kernel, whole levels), the top runs the six-lane one;
    then one set of 2^15 + 2^14 keys, half stored and half new: more than 2^15 DIRTY parents on the low levels, so the one-lane kernel runs over a
    dirty list.  Every stored node equals the dense device tree of 2^20 leaves, before and after (dst_rtree_update on the dense side)."""
    import distaff_amd as D
    depth, n = 20, 1 << 20
    rng = np.random.default_rng(20)
    perm = rng.permutation(n).astype(np.uint64)
    keys = perm[:(1 << 16) + (1 << 15)]
    new = random_words(keys.size, 201)
    leaves = np.zeros((n, 2, 2), dtype=np.uint64)
    leaves[keys.astype(np.int64)] = new
    distinct = lambda k, l: np.unique(k >> np.uint64(depth - l)).size  # noqa: E731
    assert distinct(keys, depth - 1) > SPREAD_MAX and distinct(keys, 10) <= SPREAD_MAX
    tree = D.SparseRescueTree(depth, device=0)
    tree.set(keys, new)
    info = tree.info()
    assert info["last_digests"] == sum(distinct(keys, l) for l in range(depth)) and info["keys"] == keys.size and info["last_device_ms"] > 0
    dense = D.RescueTree(leaves, device=0)
    assert_levels_equal_dense(tree, dense, keys)
    half = (1 << 14) + (1 << 13)
    second = np.concatenate([keys[:half], perm[keys.size:keys.size + half]])
    rng.shuffle(second)
    new2 = random_words(second.size, 202)
    assert SPREAD_MAX < distinct(second, depth - 1) < distinct(np.concatenate([keys, second]), depth - 1)       # a dirty list, not the whole level
    tree.set(second, new2)
    dense.update(second, new2)
    info = tree.info()
    assert info["last_digests"] == sum(distinct(second, l) for l in range(depth)) and info["keys"] == keys.size + half and info["last_device_ms"] > 0
    assert_levels_equal_dense(tree, dense, np.concatenate([keys, second]))
    ask = [int(second[0]), int(perm[-1]), 0, n - 1]
    assert tree.paths(ask) == dense.paths(ask)
    tree.close(); dense.close()


@pytest.mark.timeout(180)
def test_depth_63_equals_the_host_tree_and_paths_recompute_to_the_root():
    import distaff_amd as D
    rng = np.random.default_rng(63)
    keys = np.unique(rng.integers(0, 1 << 63, size=1024, dtype=np.uint64))
    keys = np.concatenate([keys, np.setdiff1d(np.array([0, 2 ** 63 - 1, int(keys[5]) ^ 1, int(keys[6]) ^ (1 << 62)], dtype=np.uint64), keys)])
    rng.shuffle(keys)
    new = random_words(keys.size, 631)
    tree, host = D.SparseRescueTree(63, device=0), D.SparseRescueTree(63, device=-1)
    first = keys.size // 2                                                          # two sets: the second merges into every level
    for t in (tree, host):
        t.set(keys[:first], new[:first])
        t.set(keys[first:], new[first:])
    assert_same_levels(levels_of(tree), levels_of(host))
    assert tree.root == host.root and tree.info()["last_digests"] == host.info()["last_digests"] == ancestors([int(k) for k in keys[first:]], 63)
    present = [int(k) for k in keys[:32]]
    absent = [int(k) for k in rng.integers(0, 1 << 63, size=30, dtype=np.uint64)] + [int(keys[0]) ^ 1, int(keys[1]) ^ (1 << 62)]
    assert not set(absent) & {int(k) for k in keys}
    digest = lambda v: D.arr_to_ints(D.rescue_digest([tuple(v)], device=-1))  # noqa: E731
    root = tree.root
    content = {int(k): tuple(D.arr_to_ints(v)) for k, v in zip(keys[:32], new[:32])}
    for i, path in zip(present + absent, tree.paths(present + absent)):
        assert len(path) == 64 and path[0] == content.get(i, (0, 0)), i
        assert merkle_root(path, i)(digest) == root, i
    tree.close(); host.close()


@pytest.mark.timeout(600)
def test_membership_end_to_end_at_depth_63(oracle):
    """sparse tree of depth 63 on the GPU -> tapes of a stored key -> the depth-64 program of src/examples/merkle.rs:46-56 on the oracle VM -> proof
    on the GPU -> dst_verify accepts with outputs (root + root) reversed (merkle.rs:27-30) and rejects when one output limb is changed"""
    import distaff_amd as D
    O = oracle
    rng = np.random.default_rng(64)
    keys = np.unique(rng.integers(0, 1 << 63, size=256, dtype=np.uint64))
    tree = D.SparseRescueTree(63, device=0)
    tree.set(keys, random_words(keys.size, 641))
    root = list(tree.root)
    index = int(keys[100])
    a, b = tree.tapes(index)
    tree.close()
    t = O.Trace(merkle_source(64, index), [], a, b)
    outputs = (root + root)[::-1]
    assert t.outputs(4) == outputs and t.trace_hash() == t.program_hash
    ctx = D.Context(t.length.bit_length() - 1, t.width, t.ctx_depth, t.loop_depth, grinding=8)
    ctx.upload(t.columns)
    proof = ctx.prove([], outputs)
    ctx.close()
    assert D.verify(proof, t.program_hash, [], outputs) == (True, "")
    for k in range(4):
        tampered = list(outputs)
        tampered[k] ^= 1 << (32 * k)
        ok, err = D.verify(proof, t.program_hash, [], tampered)
        assert not ok and err


@pytest.mark.timeout(300)
def test_c_example_prints_the_roots_python_computes(tmp_path):
    """examples/merkle_sparse.c compiles as C99 against include/distaff_hip.h and the product library; its roots and tapes are Python's"""
    import distaff_amd as D
    exe = tmp_path / "merkle_sparse"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_sparse.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    depth, k, m = 63, 1000, 200
    r = subprocess.run([str(exe), str(depth), str(k), str(m), "0", str(tmp_path / "s")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    keys = [((i + 1) * 0x9E3779B97F4A7C15) & (2 ** depth - 1) for i in range(k + m + 1)]      # the example's keys and leaves
    leaves = [(2 * i + 1, 2 * i + 2) for i in range(k + m)]
    tree = D.SparseRescueTree(depth, device=0)
    tree.set(keys[:k], leaves[:k])
    want = tree.root
    tapes = tree.tapes_many([keys[0], keys[k + m]])
    assert tapes[0][0][0] == 1 and tapes[1][0][0] == 0                                        # a stored leaf, an empty one
    assert "root %032x %032x" % want in out, out
    tree.set(keys[k:k + m], leaves[k:])
    assert "new root %032x %032x" % tree.root in out, out
    tree.close()
    assert (tmp_path / "s.root").read_bytes() == b"".join(v.to_bytes(16, "little") for v in want)
    assert (tmp_path / "s.tape_a").read_bytes() == b"".join(v.to_bytes(16, "little") for a, _ in tapes for v in a)
    assert (tmp_path / "s.tape_b").read_bytes() == b"".join(v.to_bytes(16, "little") for _, b in tapes for v in b)
