"""Updates in place and batched openings of Rescue Merkle trees on the GPU (rescue_tree_update_kernel, rescue_tree_update_spread_kernel,
rescue_tree_scatter_kernel, rescue_tree_gather_kernel) through the library the session binds.  An updated tree is compared with a fresh
dst_rtree_build over the modified leaves -- code that tests/test_rescue_tree_gpu.py holds against the host path and the oracle -- never with
itself; small trees also with the host path's tree.  Every test has its own time limit and nothing is run twice."""
import os
import random
import subprocess

import numpy as np
import pytest

from test_rescue_tree_host import P, merkle_root, random_leaves
from test_rescue_tree_update_host import all_nodes, check_batched_openings, check_rejections, check_updates, host_tree, update_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def device_tree(leaves):
    import distaff_amd as D
    return D.RescueTree(leaves, device=0)


def random_words(count, seed):
    """uint64 words [count, 2, 2] of uniformly random canonical elements"""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(count, 2, 2), dtype=np.uint64)
    a[..., 1] >>= np.uint64(1)                           # high word below 2^63: below p
    return a


@pytest.mark.timeout(120)
@pytest.mark.parametrize("log_leaves", [1, 3, 10])
def test_updated_device_tree_equals_a_fresh_build_and_the_host_tree(log_leaves):
    """trees this small take rescue_tree_update_spread_kernel on every partly dirty level"""
    check_updates(device_tree, log_leaves, update_sets(log_leaves), 90 + log_leaves, also=host_tree)


@pytest.mark.timeout(120)
def test_both_indexed_kernels_and_the_dense_levels_in_one_update():
    """2^17 leaves, the leaves 2i for i < 49 152 replaced: 49 152 of 65 536 parents dirty on the lowest level (above RESCUE_SPREAD_MAX = 2^15: the
    one-lane indexed kernel), 24 576 of 32 768 on the next, ... 3 of 4 (the six-lane indexed kernel), then the whole levels of 2 and 1 parents
    (the dense kernels).  All 2^18 - 1 nodes equal a fresh device build over the modified leaves."""
    n, k = 1 << 17, 49152
    leaves = random_words(n, 17)
    tree = device_tree(leaves)
    indices = np.arange(0, 2 * k, 2, dtype=np.uint64)
    new = random_words(k, 18)
    tree.update(indices, new)
    assert tree.update_ms > 0
    leaves[indices.astype(np.int64)] = new
    fresh = device_tree(leaves)
    assert np.array_equal(all_nodes(tree), all_nodes(fresh))
    fresh.close()
    tree.close()


@pytest.mark.timeout(120)
def test_successive_overlapping_updates_equal_one_fresh_build():
    """a stale dirty list in the staging buffer, or a level that does not wait for the one below it, would show here"""
    log_leaves, n = 10, 1 << 10
    rnd = random.Random(10)
    leaves = random_leaves(log_leaves, 95)
    tree = device_tree(leaves)
    for indices in (list(range(100, 400)), list(range(300, 700, 3))[::-1], [350], rnd.sample(range(n), 600)):
        new = [(rnd.randrange(P), rnd.randrange(P)) for _ in indices]
        tree.update(indices, new)
        for i, v in zip(indices, new):
            leaves[i] = v
    for build in (device_tree, host_tree):
        fresh = build(leaves)
        assert np.array_equal(all_nodes(tree), all_nodes(fresh)), build
        fresh.close()
    tree.close()


@pytest.mark.timeout(120)
def test_batched_openings_equal_the_single_index_calls_and_follow_an_update(oracle):
    log_leaves, n = 10, 1 << 10
    rnd = random.Random(11)
    tree = device_tree(random_leaves(log_leaves, 96))
    indices = [n - 1, 0, n - 1] + [rnd.randrange(n) for _ in range(297)]
    assert len(set(indices)) < len(indices)
    check_batched_openings(tree, indices)
    changed = rnd.sample(range(n), 40)
    new = [(rnd.randrange(P), rnd.randrange(P)) for _ in changed]
    tree.update(changed, new)
    assert tree.update_ms > 0
    root = tree.root
    for i, v, path in zip(changed, new, tree.paths(changed)):
        assert path[0] == v and merkle_root(path, i)(oracle.hasher_digest) == root, i
    tree.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("log_leaves", [1, 10])
def test_rejected_updates_leave_the_device_tree_unchanged(log_leaves):
    check_rejections(device_tree, log_leaves)


@pytest.mark.timeout(300)
def test_c_example_prints_the_roots_python_computes(tmp_path):
    """examples/merkle_update.c compiles as C99 against include/distaff_hip.h and the product library; its roots and tapes are Python's"""
    import distaff_amd as D
    exe = tmp_path / "merkle_update"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_update.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    k, index, second = 10, 389, 77
    r = subprocess.run([str(exe), str(k), str(index), str(second), "0", str(tmp_path / "u")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    leaves = [(2 * i + 1, 2 * i + 2) for i in range(1 << k)]              # the example's leaves: node i = (2i + 1, 2i + 2)
    tree = D.RescueTree(leaves, device=0)
    assert "old root %032x %032x" % tree.root in out, out
    tree.close()
    leaves[index] = (2 ** 64 + index, 2 ** 65 + index)
    tree = D.RescueTree(leaves, device=0)                                 # a fresh build of the modified leaves
    want = tree.root
    tapes = [tree.tapes(index), tree.tapes(second)]
    tree.close()
    assert "new root %032x %032x" % want in out, out
    assert (tmp_path / "u.root").read_bytes() == b"".join(v.to_bytes(16, "little") for v in want)
    assert (tmp_path / "u.tape_a").read_bytes() == b"".join(v.to_bytes(16, "little") for a, _ in tapes for v in a)
    assert (tmp_path / "u.tape_b").read_bytes() == b"".join(v.to_bytes(16, "little") for _, b in tapes for v in b)
