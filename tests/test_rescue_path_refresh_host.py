"""Following ordered writes with held paths (dst_rescue_refresh_paths, dst_rescue_refresh_paths_w) on the host path (device = -1) of the PRODUCT
library.  No GPU.  Everything is bit-exact.  The yardsticks, none of them the call under test: (a) the tree itself -- paths() of the same keys
after apply(); (b) the rule restated here in Python over the oracle's hasher_digest, independent of the library; (c) verify_paths(root_after,
refreshed), which existed before.  The checkers take `device` and `lib` (and the trees' constructors), so
tests/test_rescue_path_refresh_emulated.py and tests/test_rescue_path_refresh_gpu.py run the same cases on the device path."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from test_rescue_path_verify_host import BAD_NEXT_ROOT, BAD_ROOT, OK, flip, merkle_root, random_paths
from test_rescue_tree_host import P, _product, random_leaves
from test_rescue_tree_sequence_host import random_ops
from test_rescue_tree_update_host import host_tree
from test_sparse_rescue_tree_host import NONZERO_EMPTY, host_sparse
from test_wide_sparse_rescue_tree_host import host_wide

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


# ---- yardstick (b): the rule, restated ------------------------------------------------------------------------------------------------------
def chain(digest, path, index, leaf):
    """c[0] = leaf, c[t] = digest(c[t - 1], path[t]) ordered by bit t - 1 of index"""
    c = [tuple(leaf)]
    for t in range(1, len(path)):
        pair = (tuple(path[t]), c[-1]) if (index >> (t - 1)) & 1 else (c[-1], tuple(path[t]))
        c.append(tuple(digest(list(pair[0]) + list(pair[1]))))
    return c


def refreshed_by_rule(digest, indices, paths, leaves, h, q):
    """the writes in order, so that the last one that supplies a position wins"""
    q = [tuple(node) for node in q]
    for index, path, leaf in zip(indices, paths, leaves):
        c = chain(digest, path, index, leaf)
        if index == h:
            q[0] = tuple(leaf)
        for k in range(1, len(q)):
            if (index >> (k - 1)) == ((h >> (k - 1)) ^ 1):
                q[k] = c[k - 1]
    return q


def raw_refresh(lib, device, before, indices, paths, leaves, roots, held, held_words, out=None, wide=False):
    """the C call itself over arrays the test owns -> (return code, first_bad, why, root_after words, out words): `out` defaults to a new array
    filled with SENTINEL bytes; pass held_words itself for the in-place call"""
    import distaff_amd as D
    L = D.lib
    idx, hidx = L._Keys(indices, wide), L._Keys(held, wide)
    w, n = L._path_words(paths, idx.size)
    n = n if idx.size else held_words.shape[1]
    new = L._nodes_for(leaves, idx.size, "leaves")
    claimed = L._nodes_for(roots, idx.size, "roots") if roots is not None else None
    r0 = L._nodes_for([tuple(before)], 1, "roots")
    if out is None:
        out = np.frombuffer(bytes([SENTINEL]) * held_words.nbytes, dtype=np.uint64).reshape(held_words.shape).copy()
    after = np.zeros((2, 2), dtype=np.uint64)
    first, why = ctypes.c_int64(7), ctypes.c_uint32(7)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    r = getattr(lib, "dst_rescue_refresh_paths" + idx.suffix)(
        ctypes.c_int(device), ptr(r0), ptr(w) if idx.size else None, ctypes.c_uint32(n), idx.ptr, ptr(new) if idx.size else None,
        ptr(claimed) if claimed is not None and idx.size else None, ctypes.c_size_t(idx.size), hidx.ptr, ptr(held_words) if hidx.size else None, ctypes.c_size_t(hidx.size),
        ptr(out), ctypes.byref(first), ctypes.byref(why), ptr(after), None)
    return r, first.value, why.value, after, out


def words_of(paths):
    import distaff_amd as D
    return D.lib._path_words(paths, len(paths))[0].copy()


def changed_positions(old, new):
    return sum(1 for a, b in zip(old, new) if tuple(a) != tuple(b))


# ---- the checkers: device and lib say which path runs ---------------------------------------------------------------------------------------
def check_single_writes(device, lib, make, oracle, log_leaves=(1, 2, 3)):
    """1. every (held, written) pair of a dense tree, the pair with equal keys included, against (a) and (b)"""
    import distaff_amd as D
    for k in log_leaves:
        every = list(range(1 << k))
        leaves = random_leaves(k, 300 + k)
        for w in every:
            tree = make(leaves)
            before, held = tree.root, tree.paths(every)
            new = [(1000 + w, 2000 + k)]
            paths, roots = tree.apply([w], new)
            stats = {}
            got = D.refresh_paths(before, [w], paths, new, every, held, roots, device=device, lib=lib, stats=stats)
            assert got == (-1, OK, tree.root, tree.paths(every)), (k, w)
            assert stats["device_ms"] >= stats["gather_ms"] >= 0 and (device >= 0 or stats["device_ms"] == 0)
            for h in every:
                assert got[3][h] == refreshed_by_rule(oracle.hasher_digest, [w], paths, new, h, held[h]), (k, w, h)
                assert changed_positions(held[h], got[3][h]) <= 1, (k, w, h)
            tree.close()


def check_ordered_batches(device, lib, make, log_leaves=(3, 5), counts=(1, 2, 24)):
    """2. ordered batches with repeats, every leaf held, against (a) and (c); a batch changes at most min(count, n) positions of a path"""
    import distaff_amd as D
    for k in log_leaves:
        every = list(range(1 << k))
        tree = make(random_leaves(k, 310 + k))
        for case, count in enumerate(counts):                                                       # one tree: the state is followed
            indices, new = random_ops(1 << k, count, 320 + 10 * k + case, 0.3)
            before, held = tree.root, tree.paths(every)
            paths, roots = tree.apply(indices, new)
            for claimed in (roots, None):
                first, why, after, got = D.refresh_paths(before, indices, paths, new, every, held, claimed, device=device, lib=lib)
                assert (first, why, after) == (-1, OK, tree.root) and got == tree.paths(every), (k, count)
            assert D.verify_paths(after, got, every, device=-1, lib=_product()) == (-1, OK)
            for h in every:
                assert changed_positions(held[h], got[h]) <= min(count, k + 1), (k, count, h)
        tree.close()


def check_last_wins(device, lib, make, oracle):
    """3. two writes under one sibling subtree of the held key, in both orders; then write x, write h, write x again"""
    import distaff_amd as D
    h, x = 5, 4                                                                                     # log_leaves 3: 6 and 7 lie under h's sibling at height 1
    for case, indices in enumerate(([6, 7], [7, 6], [x, h, x], [7, x, 6, h, 0, 6])):
        tree = make(random_leaves(3, 330))
        new = [(50 + case, j) for j in range(len(indices))]
        before, held = tree.root, tree.paths([h])
        paths, roots = tree.apply(indices, new)
        got = D.refresh_paths(before, indices, paths, new, [h], held, roots, device=device, lib=lib)
        assert got == (-1, OK, tree.root, tree.paths([h])), indices
        assert got[3][0] == refreshed_by_rule(oracle.hasher_digest, indices, paths, new, h, held[0]), indices
        if case < 2:                                                                                # position 2 is the LAST write's chain node at height 1
            assert got[3][0][2] == chain(oracle.hasher_digest, paths[1], indices[1], new[1])[1]
            assert got[3][0][2] != chain(oracle.hasher_digest, paths[0], indices[0], new[0])[1]
        tree.close()


def check_deep_tree(device, lib, make, oracle, depth, bits, refresh, verify):
    """4. / 5. a sparse tree of `depth`: the written keys differ from the held key h at one bit of `bits` each.  h is absent, then inserted, then
    emptied again; a written key and a far key are held beside it.  Against (a), (b) and (c), the state followed over three batches"""
    rnd = random.Random(340 + depth)
    h = rnd.randrange(1 << depth)
    near = [h ^ (1 << b) for b in bits]
    far = h ^ ((1 << depth) - 1)
    tree = make(depth, NONZERO_EMPTY)
    tree.set([near[1], far], [(11, 12), (13, 14)])
    held_keys = [h, near[0], far, h]                                                                # a held key may repeat
    value = lambda: (rnd.randrange(P), rnd.randrange(P))  # noqa: E731
    batches = [(near, [value() for _ in near]),                                                     # h is absent
               ([near[-1], h, near[0]], [value(), value(), value()]),                               # h is inserted between two writes beside it
               ([h, near[2], h, near[2]], [value(), value(), NONZERO_EMPTY, NONZERO_EMPTY])]        # h is written and emptied: the NONZERO_EMPTY leaf
    held = tree.paths(held_keys)
    assert held[0][0] == NONZERO_EMPTY
    for case, (keys, new) in enumerate(batches):
        before = tree.root
        paths, roots = tree.apply(keys, new)
        first, why, after, got = refresh(before, keys, paths, new, held_keys, held, roots, device=device, lib=lib)
        assert (first, why, after) == (-1, OK, tree.root), (depth, case)
        assert got == tree.paths(held_keys), (depth, case)
        for key, old, q in zip(held_keys, held, got):
            assert q == refreshed_by_rule(oracle.hasher_digest, keys, paths, new, key, old), (depth, case, key)
        assert verify(after, got, held_keys, device=-1, lib=_product()) == (-1, OK)
        held = got                                                                                  # the client never goes back to the tree
    assert held[0][0] == NONZERO_EMPTY and verify(tree.root, held[:1], [h], [NONZERO_EMPTY], device=-1, lib=_product()) == (-1, OK)
    tree.close()


def check_sparse_63(device, lib, make_sparse, oracle):
    import distaff_amd as D
    check_deep_tree(device, lib, make_sparse, oracle, 63, (0, 1, 31, 32, 62), D.refresh_paths, D.verify_paths)


def check_wide_127(device, lib, make_wide, oracle):
    import distaff_amd as D
    check_deep_tree(device, lib, make_wide, oracle, 127, (0, 63, 64, 65, 126), D.refresh_paths_wide, D.verify_paths_wide)


def check_tampering(device, lib, make, log_leaves=3, count=24):
    """6. witnesses that do not hold: the verdict of verify_writes, and out_paths still equal to its sentinel fill"""
    import distaff_amd as D
    every = list(range(1 << log_leaves))
    indices, new = random_ops(1 << log_leaves, count, 350)
    tree = make(random_leaves(log_leaves, 351))
    before, held = tree.root, words_of(tree.paths(every))
    paths, roots = tree.apply(indices, new)
    n = log_leaves + 1

    def untouched(p=paths, v=new, r=roots, b=before):
        code, first, why, after, out = raw_refresh(lib, device, b, indices, p, v, r, every, held)
        assert code == D.DST_OK and out.tobytes() == bytes([SENTINEL]) * out.nbytes
        assert (first, why, tuple(D.arr_to_ints(after))) == D.verify_writes(b, indices, p, v, r, device=-1, lib=_product())
        return first, why

    code, first, why, after, out = raw_refresh(lib, device, before, indices, paths, new, roots, every, held)
    assert (code, first, why) == (D.DST_OK, -1, OK) and out.tobytes() == words_of(tree.paths(every)).tobytes()
    for j in (0, count // 2, count - 1):
        for node in (0, 1, n - 1):
            bent = [list(p) for p in paths]
            bent[j][node] = flip(bent[j][node], node & 1, 5)
            assert untouched(p=bent) == (j, BAD_ROOT), (j, node)
            assert untouched(p=bent, r=None) == (j, BAD_ROOT), (j, node)
        leaves = list(new)
        leaves[j] = flip(leaves[j], 1)
        assert untouched(v=leaves) == (j, BAD_NEXT_ROOT), j
        assert D.refresh_paths(before, indices, paths, leaves, every, held, roots, device=device, lib=lib)[3] is None
    assert untouched(b=flip(before)) == (0, BAD_ROOT)
    tree.close()


def check_edge_cases(device, lib, make):
    """7. no write; no held path; repeated held indices; the call in place"""
    import distaff_amd as D
    every = list(range(8))
    indices, new = random_ops(8, 9, 360, 0.3)
    tree = make(random_leaves(3, 361))
    before, held = tree.root, tree.paths(every)
    paths, roots = tree.apply(indices, new)
    want = tree.paths(every)
    assert D.refresh_paths(before, [], [], [], every, held, device=device, lib=lib) == (-1, OK, before, held)            # count = 0
    assert D.refresh_paths(before, [], [], [], every, held, [], device=device, lib=lib) == (-1, OK, before, held)
    for claimed in (roots, None):                                                                   # held = 0: verify_writes
        assert D.refresh_paths(before, indices, paths, new, [], [], claimed, device=device, lib=lib) == D.verify_writes(before, indices, paths, new, claimed, device=-1, lib=_product()) + ([],)
    bent = [list(p) for p in paths]
    bent[4][1] = flip(bent[4][1])
    assert D.refresh_paths(before, indices, bent, new, [], [], roots, device=device, lib=lib)[:2] == (4, BAD_ROOT)
    assert D.refresh_paths((1, 2), [], [], [], [], [], device=device, lib=lib) == (-1, OK, (1, 2), [])
    twice = [3, 3, 0, 3, 7, 0]                                                                      # held indices may repeat
    assert D.refresh_paths(before, indices, paths, new, twice, [held[h] for h in twice], roots, device=device, lib=lib)[3] == [want[h] for h in twice]
    words = words_of(held)                                                                          # out_paths is held_paths
    code, first, why, after, out = raw_refresh(lib, device, before, indices, paths, new, roots, every, words, out=words)
    assert (code, first, why) == (D.DST_OK, -1, OK) and out is words and words.tobytes() == words_of(want).tobytes()
    words = words_of(held)
    code, first, why, after, out = raw_refresh(lib, device, before, indices, bent, new, roots, every, words, out=words)   # in place and refused: as it was
    assert (code, first, why) == (D.DST_OK, 4, BAD_ROOT) and words.tobytes() == words_of(held).tobytes()
    words = words_of(held)
    code, first, why, after, out = raw_refresh(lib, device, before, [], [], [], None, every, words, out=words)            # in place, no write
    assert (code, first, why) == (D.DST_OK, -1, OK) and words.tobytes() == words_of(held).tobytes()
    assert tuple(D.arr_to_ints(after)) == before
    tree.close()


def check_rejections(device, lib, n=4):
    """8. what is refused: DST_ERR_ARG with a reason, before anything is written"""
    import distaff_amd as D
    indices = [0, 3, (1 << (n - 1)) - 1]
    paths = random_paths(len(indices), n, 371)
    leaves = [node for node, in random_paths(len(indices), 1, 372)]
    roots = [node for node, in random_paths(len(indices), 1, 373)]
    held = [5, 0, 5, 2]
    held_paths = random_paths(len(held), n, 374)
    root = (5, 6)

    def call(p=paths, i=indices, v=leaves, r=roots, b=root, h=held, q=held_paths, wide=False):
        return (D.refresh_paths_wide if wide else D.refresh_paths)(b, i, p, v, h, q, r, device=device, lib=lib)

    def refused(cause, **kw):
        with pytest.raises(D.DistaffError) as e:
            call(**kw)
        assert e.value.code == D.DST_ERR_ARG and cause in e.value.reason, (kw.keys(), e.value.reason)

    assert call()[:2] == (0, BAD_ROOT)                                                              # the untouched arguments are accepted: random paths do not verify
    assert call(wide=True)[:2] == (0, BAD_ROOT)
    for nodes in (1, 65):
        refused("2 .. 64 nodes", p=random_paths(len(indices), nodes, 375), i=[0] * len(indices), q=random_paths(len(held), nodes, 376), h=[0] * len(held))
        refused("2 .. 64 nodes", p=[], i=[], v=[], r=None, q=random_paths(len(held), nodes, 376), h=[0] * len(held))
    for nodes in (1, 129):
        refused("2 .. 128 nodes", p=random_paths(len(indices), nodes, 375), i=[0] * len(indices), q=random_paths(len(held), nodes, 376), h=[0] * len(held), wide=True)
    refused("past the end", i=indices[:2] + [1 << (n - 1)])
    refused("past the end", h=held[:3] + [1 << (n - 1)])
    refused("past the end", h=held[:3] + [1 << 100], wide=True)
    refused("past the end", p=[], i=[], v=[], r=None, h=held[:3] + [1 << (n - 1)])
    for big in (P, 2 ** 128 - 1):
        for where in ((-1, -1), (0, 0)):                                                            # the last node of the last path; a first node
            bent = [list(p) for p in paths]
            bent[where[0]][where[1]] = (bent[where[0]][where[1]][0], big)
            refused("not below the modulus", p=bent)
            bent = [list(p) for p in held_paths]
            bent[where[0]][where[1]] = (big, 1)
            refused("not below the modulus", q=bent)
            refused("not below the modulus", q=bent, p=[], i=[], v=[], r=None)                      # no write: the host alone reads the held paths
        refused("not below the modulus", v=leaves[:-1] + [(1, big)])
        refused("not below the modulus", b=(big, 0))
        refused("not below the modulus", b=(0, big))
        refused("not below the modulus", r=roots[:-1] + [(big, 2)])
    refused("as many paths", p=paths[:-1])
    refused("as many paths", q=held_paths[:-1])
    refused("one length", q=[q[:-1] for q in held_paths])
    refused("as many leaves", v=leaves[:-1])
    refused("as many roots", r=roots[:-1])
    # the C-ABI itself: null pointers with a non-zero count, counts of 2^31 or more before anything is read; nothing is written
    idx, buf, first, why = (ctypes.c_uint64 * 1)(0), ctypes.create_string_buffer(32 * 2), ctypes.c_int64(7), ctypes.c_uint32(7)
    out = ctypes.create_string_buffer(bytes([SENTINEL]) * 64, 64)
    one, zero, dev, huge = ctypes.c_size_t(1), ctypes.c_size_t(0), ctypes.c_int(device), ctypes.c_size_t(1 << 31)
    f, w = ctypes.byref(first), ctypes.byref(why)
    narrow = lambda *a: lib.dst_rescue_refresh_paths(dev, *a)  # noqa: E731
    wide = lambda *a: lib.dst_rescue_refresh_paths_w(dev, *a)  # noqa: E731
    key16 = ctypes.create_string_buffer(16)
    for fn, key in ((narrow, idx), (wide, key16)):
        assert fn(buf, None, 2, key, buf, None, one, key, buf, one, out, f, w, None, None) == D.DST_ERR_ARG and "null pointer" in D.lib._rtree_error(lib)
        assert fn(buf, buf, 2, None, buf, None, one, key, buf, one, out, f, w, None, None) == D.DST_ERR_ARG
        assert fn(buf, buf, 2, key, None, None, one, key, buf, one, out, f, w, None, None) == D.DST_ERR_ARG
        assert fn(buf, buf, 2, key, buf, None, one, None, buf, one, out, f, w, None, None) == D.DST_ERR_ARG
        assert fn(buf, buf, 2, key, buf, None, one, key, None, one, out, f, w, None, None) == D.DST_ERR_ARG
        assert fn(buf, buf, 2, key, buf, None, one, key, buf, one, None, f, w, None, None) == D.DST_ERR_ARG
        assert fn(None, buf, 2, key, buf, None, one, key, buf, one, out, f, w, None, None) == D.DST_ERR_ARG
        assert fn(buf, buf, 2, key, buf, None, one, key, buf, one, out, None, w, None, None) == D.DST_ERR_ARG
        assert fn(buf, buf, 2, key, buf, None, one, key, buf, one, out, f, None, None, None) == D.DST_ERR_ARG
        assert fn(buf, buf, 2, key, buf, None, huge, key, buf, one, out, f, w, None, None) == D.DST_ERR_ARG and "2^31" in D.lib._rtree_error(lib)
        assert fn(buf, buf, 2, key, buf, None, one, key, buf, huge, out, f, w, None, None) == D.DST_ERR_ARG and "2^31" in D.lib._rtree_error(lib)
        assert fn(buf, None, 2, None, None, None, zero, None, None, zero, None, f, w, None, None) == D.DST_OK and (first.value, why.value) == (-1, OK)
    assert out.raw == bytes([SENTINEL]) * 64


# ---- the host path ----------------------------------------------------------------------------------------------------------------------------
def test_every_single_write_refreshes_every_held_path(oracle):
    check_single_writes(-1, _product(), host_tree, oracle)


def test_ordered_batches_with_repeats_follow_the_tree_and_change_one_position_per_write():
    check_ordered_batches(-1, _product(), host_tree)


def test_the_last_write_under_a_sibling_subtree_wins(oracle):
    check_last_wins(-1, _product(), host_tree, oracle)


def test_sparse_depth_63_absent_inserted_and_emptied(oracle):
    check_sparse_63(-1, _product(), host_sparse, oracle)


def test_wide_depth_127_across_the_split_of_the_index_halves(oracle):
    check_wide_127(-1, _product(), host_wide, oracle)


def test_nothing_is_written_from_witnesses_that_do_not_hold():
    check_tampering(-1, _product(), host_tree)


def test_no_write_no_held_path_repeated_keys_and_in_place():
    check_edge_cases(-1, _product(), host_tree)


def test_what_is_refused():
    check_rejections(-1, _product())


def test_plan_against_a_two_loop_model_under_sanitizers(tmp_path):
    """tests/path_refresh/path_refresh_check.cpp drives host/path_refresh.h alone (sel for both key widths) against a model in two loops over
    held paths and writes, on random and directed inputs, built with -fsanitize=address,undefined and run as a program: exit status 0, nothing
    on stderr"""
    exe = str(tmp_path / "path_refresh_check")
    subprocess.check_call(["g++", "-std=c++17", "-w", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "path_refresh", "path_refresh_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    assert b"rounds ok" in r.stdout


def run_example(tmp_path, device):
    import distaff_amd as D
    exe = tmp_path / "merkle_follow"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_follow.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    r = subprocess.run([str(exe), str(device)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()
    return r.stdout.decode().splitlines()


def example_lines(make):
    """what examples/merkle_follow.c prints, through calls that existed before it: a tree that takes the same writes and opens the held leaves"""
    k, held = 4, [3, 9, 12]
    n = 1 << k
    tree = make([(i + 1, 2 * i + 1) for i in range(n)])
    lines = ["root before %032x %032x" % tree.root]
    batches = [([3, 2, 8, 3, 13], 100), ([9, 8, 8, 12, 13, 0], 200)]
    for b, (indices, base) in enumerate(batches):
        tree.apply(indices, [(base + j, base + 50 + j) for j in range(len(indices))])
        lines.append("batch %d: %d writes followed, root %032x %032x" % (b, len(indices), tree.root[0], tree.root[1]))
    for h, path in zip(held, tree.paths(held)):
        for j, node in enumerate(path):
            lines.append("leaf %d node %d %032x %032x" % (h, j, node[0], node[1]))
    lines.append("3 held paths of %d nodes equal the tree's after %d writes" % (k + 1, sum(len(i) for i, _ in batches)))
    tree.close()
    return lines


def test_c_example_follows_two_batches_without_the_tree(tmp_path):
    """examples/merkle_follow.c compiles as C99 against include/distaff_hip.h and the product library and runs on the host"""
    assert run_example(tmp_path, -1) == example_lines(host_tree)


def test_package_lists_the_calls():
    import distaff_amd as D
    assert {"dst_rescue_refresh_paths", "dst_rescue_refresh_paths_w", "dst_rescue_refresh_last_gather_ms"} <= set(D.EXPORTS)
    assert D.refresh_paths is not None and D.refresh_paths_wide is not None
    header = open(os.path.join(ROOT, "include", "distaff_hip.h")).read()
    assert "DST_API int dst_rescue_refresh_paths(" in header and "DST_API int dst_rescue_refresh_paths_w(" in header
    assert "HELD PATHS ARE NOT CHECKED" in header
