"""Rescue digests and Rescue Merkle trees on the GPU (rescue_digest_kernel, rescue_tree_level_kernel, rescue_tree_level_spread_kernel)
through the library the session binds, against the library's own host path and the oracle's hasher_digest; then end to end: tree -> tapes ->
oracle VM trace -> proof on the GPU -> dst_verify.  Every test has its own time limit and nothing is run twice."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from test_rescue_tree_host import P, check_every_node, merkle_root, merkle_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def random_words(count, per_item, seed):
    """uint64 words [count, per_item, 2] of uniformly random canonical elements"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=(count, per_item, 2), dtype=np.uint64)
    a[..., 1] &= np.uint64(0x7FFFFFFFFFFFFFFF)          # high word below 2^63: below p
    return a


def pairs(words):
    import distaff_amd as D
    v = D.arr_to_ints(words)
    return [(v[2 * k], v[2 * k + 1]) for k in range(len(v) // 2)]


@pytest.mark.timeout(300)
def test_device_digests_equal_the_host_path_and_the_oracle(oracle):
    """2^16 random inputs: device == host path (both ours), and the first 1 024 of them == the oracle"""
    import distaff_amd as D
    a = random_words(1 << 16, 4, 1)
    a[:8, :, :] = np.array([0xFFFFD30000000000, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)      # p - 1 in every slot
    a[8:16, 1:3, :] = 0
    dev = D.rescue_digest(a, device=0)
    host = D.rescue_digest(a, device=-1)
    assert np.array_equal(dev, host)
    tuples = [tuple(D.arr_to_ints(a[k])) for k in range(1024)]
    got = pairs(dev[:1024])
    for k in range(1024):
        assert list(got[k]) == oracle.hasher_digest(list(tuples[k])), k
    bad = a[:200].copy()
    bad[137, 2] = np.array([0xFFFFD30000000001, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)        # p itself
    with pytest.raises(D.DistaffError) as e:
        D.rescue_digest(bad, device=0)
    assert e.value.code == D.DST_ERR_ARG


@pytest.mark.timeout(300)
@pytest.mark.parametrize("log_leaves", [10, 12])
def test_every_node_of_a_device_tree(oracle, log_leaves):
    import distaff_amd as D
    leaves = pairs(random_words(1 << log_leaves, 2, log_leaves))
    tree = D.RescueTree(leaves, device=0)
    check_every_node(oracle, D, tree, leaves)
    tree.close()
    leaves[len(leaves) // 3] = (5, P)
    with pytest.raises(D.DistaffError) as e:
        D.RescueTree(leaves, device=0)
    assert e.value.code == D.DST_ERR_ARG


@pytest.mark.timeout(600)
def test_tree_of_2_20_leaves_sampled():
    """The device root equals the root of the library's host path over the same leaves (one core, about 50 s at the rate of
    profiles/rescue_tree.md: inside this test's limit).  Both are ours, so on top of that a SAMPLED check against the oracle: the whole top 8
    levels (nodes 1 .. 255) and 4 096 parent nodes drawn uniformly from the node array -- which puts about half of them on the lowest level, a
    quarter on the next, ... so both level kernels and every launch width are hit -- equal the oracle's digest of their two children as read back
    from the device, the leaf level reads back as uploaded at 4 096 random places, and 64 random authentication paths recompute to the root.
    This is the ONLY test that runs rescue_tree_level_kernel, the one-lane-per-parent level kernel (levels of 2^16 .. 2^19 parents here): smaller
    trees take the six-lane kernel on every level, on the GPU and in tests/test_rescue_tree_emulated.py alike (the emulated build cannot lower the
    threshold), so the node indexing of that kernel has no CPU-side check -- the root equality and the sampled parents of its four levels are it."""
    import distaff_amd as D
    import oracle as O
    log_leaves, n = 20, 1 << 20
    words = random_words(n, 2, 20)
    tree = D.RescueTree(words, device=0)
    rnd = random.Random(20)
    top = pairs(tree.nodes(0, 512))
    for p in range(1, 256):
        assert list(top[p]) == O.hasher_digest([*top[2 * p], *top[2 * p + 1]]), p
    assert tree.root == top[1]
    for p in sorted(rnd.randrange(1, n) for _ in range(4096)):
        parent, kids = pairs(tree.nodes(p, 1))[0], pairs(tree.nodes(2 * p, 2))
        assert list(parent) == O.hasher_digest([*kids[0], *kids[1]]), p
    for i in (rnd.randrange(n) for _ in range(4096)):
        assert np.array_equal(tree.nodes(n + i, 1)[0], words[i])
    digest = lambda v: D.arr_to_ints(D.rescue_digest([tuple(v)], device=-1))
    for i in [0, n - 1] + [rnd.randrange(n) for _ in range(62)]:
        path = tree.path(i)
        assert len(path) == log_leaves + 1 and merkle_root(path, i)(digest) == tree.root, i
    assert tree.build_ms > 0
    host = D.RescueTree(words, device=-1)
    assert host.root == tree.root
    host.close()
    tree.close()


@pytest.mark.timeout(600)
def test_membership_end_to_end(oracle):
    """tree of 2^15 leaves on the GPU -> tapes of a random leaf -> the depth-16 program of src/examples/merkle.rs:46-56 on the oracle VM -> proof
    on the GPU -> dst_verify accepts with outputs (root + root) reversed (merkle.rs:27-30) and rejects when one output limb is changed"""
    import distaff_amd as D
    O = oracle
    log_leaves = 15
    tree = D.RescueTree(random_words(1 << log_leaves, 2, 15), device=0)
    root = list(tree.root)
    index = random.Random(15).randrange(1 << log_leaves)
    a, b = tree.tapes(index)
    tree.close()
    t = O.Trace(merkle_source(log_leaves + 1, index), [], a, b)
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
def test_c_example_prints_the_root_python_computes(tmp_path):
    """examples/merkle_membership.c compiles as C99 against include/distaff_hip.h and the product library; its root and tapes are Python's"""
    import distaff_amd as D
    exe = tmp_path / "merkle_membership"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_membership.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    k, index = 10, 389
    r = subprocess.run([str(exe), str(k), str(index), "0", str(tmp_path / "m")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    leaves = [(2 * i + 1, 2 * i + 2) for i in range(1 << k)]              # the example's leaves: node i = (2i + 1, 2i + 2)
    tree = D.RescueTree(leaves, device=0)
    want = tree.root
    a, b = tree.tapes(index)
    tree.close()
    assert "root %032x %032x" % want in out, out
    assert (tmp_path / "m.root").read_bytes() == b"".join(v.to_bytes(16, "little") for v in want)
    assert (tmp_path / "m.tape_a").read_bytes() == b"".join(v.to_bytes(16, "little") for v in a)
    assert (tmp_path / "m.tape_b").read_bytes() == b"".join(v.to_bytes(16, "little") for v in b)
