"""Rescue digests and Rescue Merkle trees (dst_rescue_digest_many, dst_rtree_*) on the host path (device = -1) of the PRODUCT library
(libdistaff_hip.so, opened here by path: the session itself binds the test build).  No GPU.  The yardstick is the oracle's
hasher_digest, which tests/test_oracle_isa.py pins to the reference, and the oracle's VM, prover and verifier."""
import functools
import random

import pytest

P = 2 ** 128 - 45 * 2 ** 40 + 1


@functools.lru_cache(maxsize=None)
def _product():
    import ctypes
    import distaff_amd as D
    lib = ctypes.CDLL(D.PRODUCT_LIB)
    assert lib.dst_test_hooks() == 0
    return lib


def _digests(D, tuples, device=-1, lib=None):
    out = D.arr_to_ints(D.rescue_digest(tuples, device=device, lib=lib or _product()))
    return [out[2 * k:2 * k + 2] for k in range(len(tuples))]


def edge_tuples():
    """the all-zero tuple, and 0 / p - 1 in every slot beside other values"""
    rnd = random.Random(11)
    t = [(0, 0, 0, 0), (P - 1,) * 4]
    for slot in range(4):
        for v in (0, P - 1):
            for other in (0, P - 1, None):
                t.append(tuple(v if k == slot else (rnd.randrange(P) if other is None else other) for k in range(4)))
    return t


def merkle_root(path, index):
    """compute_merkle_root (src/examples/merkle.rs:112-145) restated: path = [leaf, sibling, uncle, ...] as pairs, with the given digest function"""
    def run(digest):
        n = len(path)
        r = index & 1
        v = digest([path[r][0], path[r][1], path[1 - r][0], path[1 - r][1]])
        idx = (index + 2 ** (n - 1)) >> 1
        for i in range(2, n):
            v = digest([v[0], v[1], path[i][0], path[i][1]]) if idx & 1 == 0 else digest([path[i][0], path[i][1], v[0], v[1]])
            idx >>= 1
        return tuple(v)
    return run


def merkle_source(n, index):
    """generate_merkle_program (src/examples/merkle.rs:46-56)"""
    return "begin read.ab dup.2 smpath.%d swap.2 push.%d roll.4 swap swap.2 pmpath.%d end" % (n, index, n)


def random_leaves(log_leaves, seed):
    rnd = random.Random(seed)
    return [(rnd.randrange(P), rnd.randrange(P)) for _ in range(1 << log_leaves)]


def check_every_node(O, D, tree, leaves):
    """100 % of the node array: the leaf level is the input, every other node is the oracle's digest of its two children"""
    n = len(leaves)
    v = D.arr_to_ints(tree.nodes(0, 2 * n))
    node = [(v[2 * k], v[2 * k + 1]) for k in range(2 * n)]
    assert node[0] == (0, 0) and node[n:] == [tuple(x) for x in leaves]
    for p in range(1, n):
        assert list(node[p]) == O.hasher_digest([*node[2 * p], *node[2 * p + 1]]), p
    assert tree.root == node[1]


def test_digest_equals_the_oracle_on_random_and_edge_tuples(oracle):
    import distaff_amd as D
    rnd = random.Random(5)
    tuples = [tuple(rnd.randrange(P) for _ in range(4)) for _ in range(256)] + edge_tuples()
    got = _digests(D, tuples)
    for t, g in zip(tuples, got):
        assert g == oracle.hasher_digest(list(t)), t
    assert D.rescue_digest([], device=-1, lib=_product()).shape == (0, 2, 2)


def test_element_not_below_the_modulus_is_an_argument_error():
    import distaff_amd as D
    for bad in (P, P + 1, 2 ** 128 - 1):
        for slot in range(4):
            with pytest.raises(D.DistaffError) as e:
                D.rescue_digest([(1, 2, 3, 4), tuple(bad if k == slot else 7 for k in range(4))], device=-1, lib=_product())
            assert e.value.code == D.DST_ERR_ARG
        with pytest.raises(D.DistaffError) as e:
            D.RescueTree([(1, 2), (3, bad), (5, 6), (7, 8)], device=-1, lib=_product())
        assert e.value.code == D.DST_ERR_ARG


def test_argument_errors_never_abort():
    import ctypes
    import distaff_amd as D
    lib = _product()
    h = ctypes.c_void_p()
    buf = ctypes.create_string_buffer(64 * 4)
    assert lib.dst_rescue_digest_many(-1, None, ctypes.c_size_t(1), buf) == D.DST_ERR_ARG
    assert lib.dst_rtree_build(-1, None, 2, ctypes.byref(h)) == D.DST_ERR_ARG
    assert lib.dst_rtree_build(-1, buf, 2, None) == D.DST_ERR_ARG
    for log_leaves in (0, 27, 1 << 20):
        assert lib.dst_rtree_build(-1, buf, log_leaves, ctypes.byref(h)) == D.DST_ERR_ARG and not h.value
    assert lib.dst_rtree_root(None, buf) == D.DST_ERR_ARG
    t = D.RescueTree([(1, 2), (3, 4), (5, 6), (7, 8)], device=-1, lib=lib)
    for bad_index in (4, 5, 1 << 40):
        with pytest.raises(D.DistaffError) as e:
            t.path(bad_index)
        assert e.value.code == D.DST_ERR_ARG
        with pytest.raises(D.DistaffError) as e:
            t.tapes(bad_index)
        assert e.value.code == D.DST_ERR_ARG
    with pytest.raises(D.DistaffError):
        t.nodes(7, 2)
    with pytest.raises(D.DistaffError):
        t.tapes(0, what=0)
    assert lib.dst_rtree_path(t._h, ctypes.c_uint64(0), None) == D.DST_ERR_ARG
    assert t.build_ms == 0.0
    t.close()
    t.close()


@pytest.mark.parametrize("log_leaves", range(1, 9))
def test_every_node_of_the_tree_is_the_digest_of_its_children(oracle, log_leaves):
    import distaff_amd as D
    leaves = random_leaves(log_leaves, 100 + log_leaves)
    tree = D.RescueTree(leaves, device=-1, lib=_product())
    check_every_node(oracle, D, tree, leaves)
    tree.close()


@pytest.mark.parametrize("log_leaves", [3, 5])
def test_every_path_recomputes_to_the_root(oracle, log_leaves):
    import distaff_amd as D
    leaves = random_leaves(log_leaves, 7)
    tree = D.RescueTree(leaves, device=-1, lib=_product())
    root = tree.root
    for i in range(1 << log_leaves):
        path = tree.path(i)
        assert len(path) == log_leaves + 1 and path[0] == leaves[i] and path[1] == leaves[i ^ 1]
        assert merkle_root(path, i)(oracle.hasher_digest) == root, i
    tree.close()


def tapes_from_path(path, index):
    """generate_program_inputs (src/examples/merkle.rs:63-94) restated"""
    n = len(path)
    a, b = [path[0][0]], [path[0][1]]
    idx = index + 2 ** (n - 1)
    for i in range(1, n):
        a += [0, path[i][0]]; b += [idx & 1, path[i][1]]; idx >>= 1
    for i in range(1, n):
        a.append(path[i][0]); b.append(path[i][1])
    return a, b


@pytest.mark.parametrize("depth", [3, 4, 9])
def test_tapes_drive_the_merkle_program_on_the_oracle_vm(oracle, depth):
    """the program of src/examples/merkle.rs:46-56 with the library's tapes leaves (root + root) reversed on the stack (merkle.rs:27-30);
    at depth 3 the oracle also proves and verifies that trace"""
    import distaff_amd as D
    O = oracle
    log_leaves = depth - 1
    leaves = random_leaves(log_leaves, 40 + depth)
    tree = D.RescueTree(leaves, device=-1, lib=_product())
    root = list(tree.root)
    last = (1 << log_leaves) - 1
    for index in sorted({0, 1, last // 2, last - 1, last}):
        a, b = tree.tapes(index)
        assert len(a) == len(b) == 3 * depth - 2 and (a, b) == tapes_from_path(tree.path(index), index)
        a1, b1 = tree.tapes(index, what=1)
        a2, b2 = tree.tapes(index, what=2)
        assert len(a1) == 2 * depth - 1 and len(a2) == depth - 1 and a1 + a2 == a and b1 + b2 == b
        t = O.Trace(merkle_source(depth, index), [], a, b)
        assert t.outputs(4) == (root + root)[::-1], index
        if depth == 3 and index in (0, last):
            p = O.Prover.from_trace(t, 4, grinding=8)
            proof = p.prove()
            assert O.verify(proof, t.program_hash, [], p.outputs) == (True, "")
            assert p.outputs == (root + root)[::-1]
    tree.close()


def test_package_reexports_the_binding():
    import distaff_amd as D
    assert D.rescue_digest is not None and D.RescueTree is not None
    assert {"dst_rescue_digest_many", "dst_rtree_build", "dst_rtree_root", "dst_rtree_path", "dst_rtree_tapes", "dst_rtree_read_nodes", "dst_rtree_destroy",
            "dst_rtree_last_error"} <= set(D.EXPORTS)
