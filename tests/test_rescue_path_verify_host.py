"""Checking paths and witnesses (dst_rescue_path_roots, dst_rescue_verify_paths, dst_rescue_verify_writes) on the host path (device = -1) of the
PRODUCT library.  No GPU.  The yardstick is never one of the new calls: it is compute_merkle_root (src/examples/merkle.rs:112-145 of the reference)
restated here in Python -- over the oracle's hasher_digest for the small cases, over the existing rescue_digest(device=-1), one batched call per
level, where thousands of digests are needed -- and, for positive cases, the roots that existing trees report.  Everything is bit-exact.  The
checkers take `device` and `lib` (and the trees' constructors), so tests/test_rescue_path_verify_emulated.py and
tests/test_rescue_path_verify_gpu.py run the same cases on the device path."""
import os
import random
import subprocess

import pytest

from test_rescue_tree_host import P, _product
from test_rescue_tree_sequence_host import example_roots, index_lists, random_ops
from test_rescue_tree_update_host import host_tree
from test_sparse_rescue_tree_host import NONZERO_EMPTY, host_sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_LEAF, BAD_ROOT, BAD_NEXT_ROOT = 0, 1, 2, 3


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------
def merkle_root(digest, path, index, leaf=None):
    """merkle.rs:112-145 over `digest` (four ints -> two ints); `leaf` replaces the path's first node"""
    n = len(path)
    first = tuple(leaf) if leaf is not None else tuple(path[0])
    pair = (first, tuple(path[1]))
    r = index & 1
    v = digest(list(pair[r]) + list(pair[1 - r]))                                      # :118-124
    index = (index + (1 << (n - 1))) >> 1                                               # :126
    for i in range(2, n):
        v = digest(list(v) + list(path[i])) if index & 1 == 0 else digest(list(path[i]) + list(v))
        index >>= 1
    return tuple(v)


def merkle_roots_batched(paths, indices, leaves=None):
    """the same for many paths of one length through the existing rescue_digest on the host: one call per level for all paths"""
    import distaff_amd as D
    lib = _product()
    n = len(paths[0])
    cur = [tuple(leaves[i]) if leaves is not None else tuple(p[0]) for i, p in enumerate(paths)]
    for k in range(1, n):
        rows = []
        for c, p, i in zip(cur, paths, indices):
            rows.append(tuple(p[k]) + c if (i >> (k - 1)) & 1 else c + tuple(p[k]))
        v = D.arr_to_ints(D.rescue_digest(rows, device=-1, lib=lib))
        cur = [(v[2 * j], v[2 * j + 1]) for j in range(len(rows))]
    return cur


def random_paths(count, n, seed):
    rnd = random.Random(seed)
    return [[(rnd.randrange(P), rnd.randrange(P)) for _ in range(n)] for _ in range(count)]


def flip(node, element=0, bit=0):
    """the node with one bit of one element flipped (still below p: the elements of the tests are nowhere near it)"""
    node = list(node)
    node[element] ^= 1 << bit
    assert node[element] < P
    return tuple(node)


def path_root_cases():
    """(n, indices): n = 2, 3, 4 with EVERY index below 2^(n-1), in lists of 1, 8, 9 and 17 paths (two groups of eight lanes and one more; an
    odd count for the host's two-at-a-time form); n = 21 with random indices; n = 64 with the ends of the index range"""
    rnd = random.Random(11)
    cases = []
    for n in (2, 3, 4):
        every = list(range(1 << (n - 1)))
        for count in (1, 8, 9, 17):
            cases.append((n, [every[(j + count) % len(every)] for j in range(count)]))
        cases.append((n, every))
    cases.append((21, [rnd.randrange(1 << 20) for _ in range(9)]))
    cases.append((64, [0, 1, 1 << 62, (1 << 63) - 1]))
    return cases


# ---- the checkers: device and lib say which path runs ---------------------------------------------------------------------------------------
def check_path_roots(device, lib, oracle=None, cases=None):
    """1. path_roots against the yardstick, with and without substitute leaves"""
    import distaff_amd as D
    seen = {}
    for case, (n, indices) in enumerate(cases or path_root_cases()):
        paths = random_paths(len(indices), n, 100 + case)
        subs = [node for node, in random_paths(len(indices), 1, 200 + case)]
        if oracle is not None and n <= 4:
            want = [merkle_root(oracle.hasher_digest, p, i) for p, i in zip(paths, indices)]
            want_subs = [merkle_root(oracle.hasher_digest, p, i, s) for p, i, s in zip(paths, indices, subs)]
        else:
            want, want_subs = merkle_roots_batched(paths, indices), merkle_roots_batched(paths, indices, subs)
        stats = {}
        assert D.path_roots(paths, indices, device=device, lib=lib, stats=stats) == want, (n, indices)
        assert D.path_roots(paths, indices, subs, device=device, lib=lib) == want_subs, (n, indices)
        assert stats["device_ms"] >= 0 and (device >= 0 or stats["device_ms"] == 0)
        seen.setdefault(n, set()).update(indices)
    for n in (2, 3, 4):
        assert cases or seen[n] == set(range(1 << (n - 1)))
    assert D.path_roots([], [], device=device, lib=lib) == []


def check_tree_paths(device, lib, make, make_sparse, log_leaves=(1, 3, 10)):
    """2. paths of real trees resolve to their roots; absence in a sparse tree"""
    import distaff_amd as D
    from test_rescue_tree_host import random_leaves
    rnd = random.Random(12)
    for k in log_leaves:
        leaves = random_leaves(k, 20 + k)
        tree = make(leaves)
        indices = list(range(1 << k)) if k <= 3 else [0, (1 << k) - 1] + [rnd.randrange(1 << k) for _ in range(15)]
        paths = tree.paths(indices)
        assert D.path_roots(paths, indices, device=device, lib=lib) == [tree.root] * len(indices)
        assert D.verify_paths(tree.root, paths, indices, device=device, lib=lib) == (-1, OK)
        assert D.verify_paths(tree.root, paths, indices, [leaves[i] for i in indices], device=device, lib=lib) == (-1, OK)
        wrong = flip(tree.root)
        assert D.verify_paths(wrong, paths, indices, device=device, lib=lib) == (0, BAD_ROOT)
        tree.close()
    sparse = make_sparse(63, NONZERO_EMPTY)
    stored = [3, 1 << 62, (1 << 63) - 1, rnd.randrange(1 << 63)]
    sparse.set(stored, [(rnd.randrange(P), rnd.randrange(P)) for _ in stored])
    absent = [0, 2, (1 << 62) + 1, rnd.randrange(1 << 63)]
    keys = absent + stored[:2] + absent[:1] + stored[2:]
    for paths in (sparse.paths(keys), sparse.paths_words(keys)):                                  # both shapes
        assert D.path_roots(paths, keys, device=device, lib=lib) == [sparse.root] * len(keys)
        assert D.verify_paths(sparse.root, paths, keys, device=device, lib=lib) == (-1, OK)
        # a claim of absence: the leaf is the empty leaf.  The absent keys hold, the first stored one does not
        assert D.verify_paths(sparse.root, paths[:len(absent)], absent, [NONZERO_EMPTY] * len(absent), device=device, lib=lib) == (-1, OK)
        assert D.verify_paths(sparse.root, paths, keys, [NONZERO_EMPTY] * len(keys), device=device, lib=lib) == (len(absent), BAD_LEAF)
    sparse.close()


def check_writes_of_apply(device, lib, make, make_sparse, sparse_depths=(3, 63)):
    """3. verify_writes accepts what apply returns, with and without the roots, and follows the state"""
    import distaff_amd as D
    from test_rescue_tree_host import random_leaves
    n = 8
    for case, indices in enumerate(index_lists(n, 3) + [random_ops(n, 12, 43, 0.3)[0]]):
        new = random_ops(n, len(indices), 500 + case)[1]
        tree = make(random_leaves(3, 30 + case))
        before = tree.root
        paths, roots = tree.apply(indices, new)
        assert D.verify_writes(before, indices, paths, new, roots, device=device, lib=lib) == (-1, OK, tree.root)
        assert D.verify_writes(before, indices, paths, new, device=device, lib=lib) == (-1, OK, tree.root)
        tree.close()
    for depth in sparse_depths:
        rnd = random.Random(13 + depth)
        tree = make_sparse(depth, NONZERO_EMPTY)
        tree.set([1, (1 << depth) - 2], [(5, 6), (7, 8)])
        for case, keys in enumerate(index_lists(1 << depth, depth) + [random_ops(1 << depth, 12, 44 + depth, 0.3)[0]]):      # one tree: the state is followed
            new = [(rnd.randrange(P), rnd.randrange(P)) for _ in keys]
            before = tree.root
            paths, roots = tree.apply(keys, new)
            stats = {}
            assert D.verify_writes(before, keys, paths, new, roots, device=device, lib=lib, stats=stats) == (-1, OK, tree.root)
            assert D.verify_writes(before, keys, paths, new, device=device, lib=lib) == (-1, OK, tree.root)
            assert stats["device_ms"] >= 0 and (device >= 0 or stats["device_ms"] == 0)
        tree.close()
    root = (1, 2)
    assert D.verify_writes(root, [], [], [], device=device, lib=lib) == (-1, OK, root)             # no write: the state stays
    assert D.verify_writes(root, [], [], [], [], device=device, lib=lib) == (-1, OK, root)


def check_tampering(device, lib, make, log_leaves=3, count=24):
    """4. each single tampering of an accepted batch is found at its write, with its reason"""
    import distaff_amd as D
    from test_rescue_tree_host import random_leaves
    indices, new = random_ops(1 << log_leaves, count, 47)
    tree = make(random_leaves(log_leaves, 48))
    before = tree.root
    paths, roots = tree.apply(indices, new)
    after = tree.root
    tree.close()
    n = log_leaves + 1
    verify = lambda b=before, i=indices, p=paths, v=new, r=roots: D.verify_writes(b, i, p, v, r, device=device, lib=lib)  # noqa: E731
    assert verify() == (-1, OK, after)
    other = (new[0][0] ^ 2, new[0][1])
    for j in (0, count // 2, count - 1):
        for node in (0, 1, n - 1):                                                                  # the old leaf, the sibling, the node below the root
            bent = [list(p) for p in paths]
            bent[j][node] = flip(bent[j][node], node & 1, 5)
            assert verify(p=bent)[:2] == (j, BAD_ROOT), (j, node)
            assert verify(p=bent, r=None)[:2] == (j, BAD_ROOT), (j, node)
        leaves = list(new)
        leaves[j] = flip(leaves[j], 1)
        assert verify(v=leaves)[:2] == (j, BAD_NEXT_ROOT), j
        got = verify(v=leaves, r=None)                                                              # nothing states what the new leaf resolves to ...
        if j < count - 1:
            assert got[:2] == (j + 1, BAD_ROOT), j                                                  # ... so it shows one write later,
        else:
            assert got[:2] == (-1, OK) and got[2] != after                                          # in the last write only in root_after
        claimed = list(roots)
        claimed[j] = other
        assert verify(r=claimed)[:2] == (j, BAD_NEXT_ROOT), j
    for j in (0, count // 2, count - 2):                                                            # writes j and j + 1 swapped: reported at the earlier one
        swap = lambda xs: xs[:j] + [xs[j + 1], xs[j]] + xs[j + 2:]  # noqa: E731
        got = D.verify_writes(before, swap(indices), swap(paths), swap(new), swap(roots), device=device, lib=lib)
        assert got[:2] == (j, BAD_ROOT), j
    assert verify(b=flip(before))[:2] == (0, BAD_ROOT)
    assert verify(b=roots[0])[:2] == (0, BAD_ROOT)


def check_rejections(device, lib, n=4):
    """5. what is refused: DST_ERR_ARG with a reason; count = 0 is accepted"""
    import distaff_amd as D
    indices = [0, 3, (1 << (n - 1)) - 1]
    paths = random_paths(len(indices), n, 51)
    leaves = [node for node, in random_paths(len(indices), 1, 52)]
    roots = [node for node, in random_paths(len(indices), 1, 53)]
    root = (5, 6)
    calls = {"path_roots": lambda p=paths, i=indices, v=None, r=None, b=root: D.path_roots(p, i, v, device=device, lib=lib),
             "path_roots(leaves)": lambda p=paths, i=indices, v=leaves, r=None, b=root: D.path_roots(p, i, v, device=device, lib=lib),
             "verify_paths": lambda p=paths, i=indices, v=leaves, r=None, b=root: D.verify_paths(b, p, i, v, device=device, lib=lib),
             "verify_writes": lambda p=paths, i=indices, v=leaves, r=roots, b=root: D.verify_writes(b, i, p, v, r, device=device, lib=lib)}

    def refused(what, cause, **kw):
        with pytest.raises(D.DistaffError) as e:
            calls[what](**kw)
        assert e.value.code == D.DST_ERR_ARG and cause in e.value.reason, (what, kw.keys(), e.value.reason)

    for what in calls:
        calls[what]()                                                                               # the untouched arguments are accepted
        for nodes in (1, 65):
            refused(what, "2 .. 64 nodes", p=random_paths(len(indices), nodes, 54), i=[0] * len(indices))
        refused(what, "past the end", i=indices[:2] + [1 << (n - 1)])
        for big in (P, 2 ** 128 - 1):
            bent = [list(p) for p in paths]
            bent[-1][-1] = (bent[-1][-1][0], big)                                                   # the last element of the last node of the last path
            refused(what, "not below the modulus", p=bent)
            bent = [list(p) for p in paths]
            bent[0][0] = (big, 1)                                                                   # a first node: read by the device or by the host
            refused(what, "not below the modulus", p=bent)
            if what != "path_roots":
                refused(what, "not below the modulus", v=leaves[:-1] + [(1, big)])
            if what.startswith("verify"):
                refused(what, "not below the modulus", b=(big, 0))
                refused(what, "not below the modulus", b=(0, big))
            if what == "verify_writes":
                refused(what, "not below the modulus", r=roots[:-1] + [(big, 2)])
        # mismatched lengths, found by the binding
        refused(what, "as many paths", p=paths[:-1])
        refused(what, "one length", p=paths[:-1] + [paths[-1][:-1]])
        if what != "path_roots":
            refused(what, "as many leaves", v=leaves[:-1])
        if what == "verify_writes":
            refused(what, "as many roots", r=roots[:-1])
    assert D.path_roots([], [], device=device, lib=lib) == [] and D.path_roots([], [], [], device=device, lib=lib) == []
    assert D.verify_paths(root, [], [], device=device, lib=lib) == (-1, OK) and D.verify_paths(root, [], [], [], device=device, lib=lib) == (-1, OK)
    assert D.verify_writes(root, [], [], [], device=device, lib=lib) == (-1, OK, root)
    # the C-ABI itself: null pointers with count > 0, count >= 2^31 before anything is read
    import ctypes
    idx, buf, first, why = (ctypes.c_uint64 * 1)(0), ctypes.create_string_buffer(32 * 2), ctypes.c_int64(7), ctypes.c_uint32(7)
    one, dev = ctypes.c_size_t(1), ctypes.c_int(device)
    assert lib.dst_rescue_path_roots(dev, None, 2, idx, one, None, buf, None) == D.DST_ERR_ARG and "null pointer" in D.lib._rtree_error(lib)
    assert lib.dst_rescue_path_roots(dev, buf, 2, None, one, None, buf, None) == D.DST_ERR_ARG
    assert lib.dst_rescue_path_roots(dev, buf, 2, idx, one, None, None, None) == D.DST_ERR_ARG
    assert lib.dst_rescue_path_roots(dev, buf, 2, idx, ctypes.c_size_t(1 << 31), None, buf, None) == D.DST_ERR_ARG and "2^31" in D.lib._rtree_error(lib)
    assert lib.dst_rescue_verify_paths(dev, buf, buf, 2, idx, None, one, None, ctypes.byref(why), None) == D.DST_ERR_ARG
    assert lib.dst_rescue_verify_paths(dev, None, buf, 2, idx, None, one, ctypes.byref(first), ctypes.byref(why), None) == D.DST_ERR_ARG
    assert lib.dst_rescue_verify_writes(dev, buf, buf, 2, idx, None, None, one, ctypes.byref(first), ctypes.byref(why), None, None) == D.DST_ERR_ARG
    assert lib.dst_rescue_verify_writes(dev, buf, buf, 2, idx, buf, None, ctypes.c_size_t(1 << 31), ctypes.byref(first), ctypes.byref(why), None, None) == D.DST_ERR_ARG
    assert lib.dst_rescue_verify_writes(dev, buf, None, 2, None, None, None, ctypes.c_size_t(0), ctypes.byref(first), ctypes.byref(why), None, None) == D.DST_OK
    assert (first.value, why.value) == (-1, OK)


# ---- the host path ----------------------------------------------------------------------------------------------------------------------------
def test_path_roots_equal_the_reference_walk(oracle):
    check_path_roots(-1, _product(), oracle)


def test_paths_of_dense_and_sparse_trees_resolve_to_their_roots():
    check_tree_paths(-1, _product(), host_tree, host_sparse)


def test_the_witnesses_of_apply_are_accepted_and_the_state_is_followed():
    check_writes_of_apply(-1, _product(), host_tree, host_sparse)


def test_each_single_tampering_is_found_at_its_write():
    check_tampering(-1, _product(), host_tree)


def test_what_is_refused():
    check_rejections(-1, _product())


def test_decision_against_a_two_loop_model_under_sanitizers(tmp_path):
    """tests/path_verify/path_verify_check.cpp drives host/path_verify.h alone (the index checks, first_bad / why over arrays of computed roots)
    against a model in two loops, built with -fsanitize=address,undefined and run as a program: exit status 0, nothing on stderr"""
    exe = str(tmp_path / "path_verify_check")
    subprocess.check_call(["g++", "-std=c++17", "-w", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "path_verify", "path_verify_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    assert b"rounds ok" in r.stdout


def example_lines(make, k, count):
    """what examples/merkle_verify.c prints for k and count, through calls that existed before it: the roots from a tree updated one write at a
    time (example_roots); the verdict on the tampered write follows from the definition -- its sibling no longer resolves to the root before it"""
    lines = example_roots(make, k, count)
    n = 1 << k
    last = None
    for j in range(count):
        last = last if j & 3 == 3 else (7 * j + 3) & (n - 1)
    return [lines[0].replace("root before 0", "root before"), "root after " + lines[-2].split(" ", 4)[4],
            "%d writes, %d witnesses of %d nodes checked in one call" % (count, count, k + 1),
            "tampered write %d: first_bad %d why %d" % (count // 2, count // 2, BAD_ROOT),
            "3 leaves open under the final root, leaf %d holds the value of write %d" % (last, count - 1)]


def run_example(tmp_path, k, count, device):
    import distaff_amd as D
    exe = tmp_path / "merkle_verify"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_verify.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    r = subprocess.run([str(exe), str(k), str(count), str(device)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()
    return r.stdout.decode().splitlines()


def test_c_example_checks_all_witnesses_in_one_call_and_prints_what_python_computes(tmp_path):
    """examples/merkle_verify.c compiles as C99 against include/distaff_hip.h and the product library and runs on the host"""
    assert run_example(tmp_path, 3, 9, -1) == example_lines(host_tree, 3, 9)


def test_package_lists_the_calls():
    import distaff_amd as D
    assert {"dst_rescue_path_roots", "dst_rescue_verify_paths", "dst_rescue_verify_writes"} <= set(D.EXPORTS)
    assert D.path_roots is not None and D.verify_paths is not None and D.verify_writes is not None
    assert (D.DST_PATH_OK, D.DST_PATH_BAD_LEAF, D.DST_PATH_BAD_ROOT, D.DST_PATH_BAD_NEXT_ROOT) == (OK, BAD_LEAF, BAD_ROOT, BAD_NEXT_ROOT)
    header = open(os.path.join(ROOT, "include", "distaff_hip.h")).read()
    assert "DST_PATH_OK = 0, DST_PATH_BAD_LEAF = 1, DST_PATH_BAD_ROOT = 2, DST_PATH_BAD_NEXT_ROOT = 3" in header
