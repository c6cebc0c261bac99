"""Wide-key sparse Rescue Merkle trees (dst_wtree_*, 16-byte keys, depth <= 127) and the path tools over 16-byte indices (dst_rescue_*_w) on
the host path (device = -1) of the PRODUCT library.  No GPU.  Everything is bit-exact.  The yardsticks, none of them the code under test: the
narrow sparse tree wherever both exist (tests/test_sparse_rescue_tree_host.py holds it against the dense tree and the oracle); above depth 63
the Python merkle_root of tests/test_rescue_tree_host.py over the oracle's hasher_digest, which Python ints carry to 127-bit indices; and the
oracle's VM.  Also here: the helpers the emulated and the GPU tests of the wide trees share."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from test_rescue_tree_host import P, _product, merkle_root, merkle_source, tapes_from_path
from test_sparse_rescue_tree_host import NONZERO_EMPTY, ancestors, depth_63_keys, empty_chain, host_sparse, key_sets, random_pairs


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_wide(depth, empty=(0, 0)):
    import distaff_amd as D
    return D.WideSparseRescueTree(depth, empty, device=-1, lib=_product())


def int_levels(tree):
    """every level as (prefixes as Python ints, nodes as a list of lists of words): the same shape for narrow and wide trees"""
    import distaff_amd as D
    out = []
    for l in range(tree.depth + 1):
        prefixes, nodes = tree.level(l)
        ints = D.arr_to_ints(prefixes) if prefixes.ndim == 2 else [int(q) for q in prefixes]
        out.append((ints, nodes.tolist()))
    return out


def figures(tree):
    i = tree.info()
    return [i[f] for f in ("depth", "keys", "nodes", "last_digests")]


# ---- 1. equal to the narrow tree where both exist ---------------------------------------------------------------------------------------------------
def narrow_cases(depth, seed):
    """the key sets of key_sets() -- none, one, all, a sibling pair, a third, two thirds -- where all 2^depth keys can be listed; at depth 63
    none, a sibling pair and 64 keys with both ends and a pair that differs in the top bit"""
    if depth < 63:
        return key_sets(depth, seed)
    keys = depth_63_keys(seed, 64)
    return [[], [keys[0] & ~1, keys[0] | 1], keys]


def some_absent(depth, keys, seed, count=6):
    rnd = random.Random(seed)
    out = [k ^ 1 for k in keys[:2]] + [rnd.randrange(1 << depth) for _ in range(count)]
    return [k for k in dict.fromkeys(out) if k not in set(keys)]


def check_equals_narrow(make_wide, make_narrow, depth, empty, keys, seed):
    rnd = random.Random(seed)
    leaves = random_pairs(len(keys), seed)
    a, b = make_narrow(depth, empty), make_wide(depth, empty)
    a.set(keys, leaves); b.set(keys, leaves)
    ask = (keys + some_absent(depth, keys, seed))[:48] if depth > 8 else list(range(1 << depth))
    ask += ask[:1]                                                                  # a repeat among the asked keys

    def same():
        assert a.root == b.root and int_levels(a) == int_levels(b) and figures(a) == figures(b)
        assert a.paths(ask) == b.paths(ask) and a.tapes_many(ask) == b.tapes_many(ask) and a.tapes_many(ask[:3], what=2) == b.tapes_many(ask[:3], what=2)
        assert a.get(ask) == b.get(ask)
        assert a.audit() is None and b.audit() is None
    same()
    batch = [ask[i % len(ask)] for i in (0, 1, 0, 2, 1, 0)] + [rnd.randrange(1 << depth) for _ in range(3)]      # ordered, with repeats
    values = random_pairs(len(batch) - 1, seed + 1) + [tuple(empty)]
    assert a.apply(batch, values) == b.apply(batch, values)
    same()
    gone = list(dict.fromkeys(keys[::2] + batch[-2:]))
    assert a.remove(gone) == b.remove(gone)
    same()
    hollow = list(dict.fromkeys(keys[:3] + [batch[0]]))
    for t in (a, b):
        t.set(hollow, [tuple(empty)] * len(hollow))
    assert a.compact() == b.compact()
    same()
    a.close(); b.close()


@pytest.mark.parametrize("empty", [(0, 0), NONZERO_EMPTY], ids=["zero", "nonzero"])
@pytest.mark.parametrize("depth", [1, 2, 8, 63])
def test_the_wide_tree_equals_the_narrow_tree_where_both_exist(depth, empty):
    for case, keys in enumerate(narrow_cases(depth, 300 + depth)):
        check_equals_narrow(host_wide, host_sparse, depth, empty, list(keys), 7000 + 10 * depth + case)


# ---- 2. the limb boundary: depths at which key >> (D - l) crosses the two 64-bit halves ---------------------------------------------------------------
BOUNDARY_DEPTHS = [64, 65, 100, 127]
BOUNDARY_SETS = ["equal-low-halves", "sibling-pair", "zero", "last", "half", "shared-top", "shared-low", "random-200"]


def boundary_keys(depth, name, seed, random_count=200):
    """-> the key set `name` of depth `depth`, or None where it does not exist: k + 2^64 is no key of a depth-64 tree"""
    rnd = random.Random(seed)
    if name == "equal-low-halves":
        if depth == 64:
            return None
        k = rnd.randrange(1 << 64)
        return [k, k + (1 << 64)]
    if name == "sibling-pair":
        k = rnd.randrange(1 << depth)
        return [k, k ^ 1]
    if name in ("zero", "last", "half"):
        return [{"zero": 0, "last": (1 << depth) - 1, "half": 1 << (depth - 1)}[name]]
    if name == "shared-top":                                                        # 40 keys sharing their top D - 8 bits
        high = rnd.randrange(1 << (depth - 8))
        return [(high << 8) | low for low in rnd.sample(range(256), 40)]
    if name == "shared-low":                                                        # 40 keys equal in their low D - 8 bits, different in the top 8
        low = rnd.randrange(1 << (depth - 8))
        return [(top << (depth - 8)) | low for top in rnd.sample(range(256), 40)]
    keys = set()
    while len(keys) < random_count:
        keys.add(rnd.randrange(1 << depth))
    keys = list(keys)
    rnd.shuffle(keys)
    return keys


def check_levels_are_the_distinct_prefixes(tree, keys):
    depth = tree.depth
    for l, (prefixes, _) in enumerate(int_levels(tree)):
        assert prefixes == sorted({k >> (depth - l) for k in keys}), l


def check_paths_resolve(O, tree, keys, absent, content, empty):
    root = tree.root
    for i, path in zip(keys + absent, tree.paths(keys + absent)):
        assert len(path) == tree.depth + 1 and path[0] == content.get(i, tuple(empty)), i
        assert merkle_root(path, i)(O.hasher_digest) == root, i


def check_apply_witnesses(O, tree, batch, values):
    """witness i resolves to the root before write i, and with the new leaf in its place to roots[i]"""
    before = tree.root
    paths, roots = tree.apply(batch, values)
    for i, (index, path) in enumerate(zip(batch, paths)):
        assert merkle_root(path, index)(O.hasher_digest) == before, i
        assert merkle_root([values[i]] + path[1:], index)(O.hasher_digest) == roots[i], i
        before = roots[i]
    assert tree.root == before


def check_removal_equals_fresh(make, tree, keys, content, empty):
    gone, rest = keys[::2], keys[1::2]
    assert tree.remove(gone + [gone[0] ^ 1] if gone[0] ^ 1 not in keys else gone) == len(gone)
    fresh = make(tree.depth, empty)
    fresh.set(rest, [content[k] for k in rest])
    assert int_levels(tree) == int_levels(fresh) and tree.root == fresh.root
    assert tree.info()["keys"] == len(rest)
    fresh.close()


def check_boundary_set(O, make, depth, name, empty, seed, paths_of=None, random_count=200):
    """the checks of one key set on trees that `make` builds; paths_of = how many stored keys are opened (None: all of them)"""
    keys = boundary_keys(depth, name, seed, random_count)
    if keys is None:
        return
    content = dict(zip(keys, random_pairs(len(keys), seed + 1)))
    tree = make(depth, empty)
    tree.set(keys, [content[k] for k in keys])
    assert tree.info()["last_digests"] == ancestors(keys, depth) and tree.info()["keys"] == len(keys)
    check_levels_are_the_distinct_prefixes(tree, keys)
    absent = some_absent(depth, keys, seed + 2) + [k for k in (keys[0] ^ (1 << 64), keys[0] ^ (1 << (depth - 1))) if k >> depth == 0 and k not in content]
    check_paths_resolve(O, tree, keys[:paths_of], absent, content, empty)
    if name == "shared-top":
        # the stored node at level D - 8 is the root of the depth-8 tree over the low bytes; the root is that node folded upward with the E_l
        small = host_sparse(8, empty)
        small.set([k & 255 for k in keys], [content[k] for k in keys])
        prefixes, nodes = int_levels(tree)[depth - 8]
        import distaff_amd as D
        assert prefixes == [keys[0] >> 8] and tuple(D.arr_to_ints(np.array(nodes[0], dtype=np.uint64))) == small.root
        e = empty_chain(O, empty, depth)
        v, high = small.root, keys[0] >> 8
        for l in range(depth - 8, 0, -1):                                           # v is the node of level l with prefix high >> (D - 8 - l)
            bit = (high >> (depth - 8 - l)) & 1
            v = tuple(O.hasher_digest([*e[l], *v] if bit else [*v, *e[l]]))
        assert v == tree.root
        small.close()
    batch = [keys[0], absent[0], keys[0], keys[-1], absent[0]]
    check_apply_witnesses(O, tree, batch, random_pairs(4, seed + 3) + [tuple(empty)])
    tree.close()
    tree = make(depth, empty)                                                       # the removal starts from the set alone
    tree.set(keys, [content[k] for k in keys])
    if len(keys) > 1:
        check_removal_equals_fresh(make, tree, keys, content, empty)
    else:
        assert tree.remove(keys) == 1 and tree.info()["nodes"] == 0 and tree.root == empty_chain(O, empty, depth)[0]
    tree.close()


@pytest.mark.parametrize("name", BOUNDARY_SETS)
@pytest.mark.parametrize("depth", BOUNDARY_DEPTHS)
def test_levels_paths_writes_and_removals_across_the_limb_boundary(oracle, depth, name):
    """levels are the sorted distinct key >> (D - l); every path of a stored or absent key resolves to the root under the oracle's digest and an
    absent key's leaf is the empty leaf; apply's witnesses resolve to the root before and after each write; after the removal of half the keys
    the tree is create + set of the rest.  ({k, k + 2^64} does not exist at depth 64: k + 2^64 is not below 2^64.)"""
    empty = NONZERO_EMPTY if name in ("sibling-pair", "shared-top", "random-200") else (0, 0)
    check_boundary_set(oracle, host_wide, depth, name, empty, 100 * depth + BOUNDARY_SETS.index(name))


# ---- 3. tapes ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 128])
def test_tapes_equal_generate_program_inputs_restated(n):
    import distaff_amd as D
    depth = n - 1
    keys = boundary_keys(depth, "random-200", 900 + n, 12) + [0, (1 << depth) - 1]
    tree = host_wide(depth, NONZERO_EMPTY)
    tree.set(keys, random_pairs(len(keys), n))
    ask = keys + [keys[0] ^ (1 << (depth - 1)), keys[1] ^ 2]
    paths = tree.paths(ask)
    want = [tapes_from_path(path, i) for path, i in zip(paths, ask)]
    assert tree.tapes_many(ask) == want and tree.tapes(ask[0]) == want[0]
    assert D.path_tapes_wide(paths, ask, lib=_product()) == want
    for what, cut in ((1, slice(0, 2 * n - 1)), (2, slice(2 * n - 1, None))):
        assert tree.tapes_many(ask[:3], what=what) == D.path_tapes_wide(paths[:3], ask[:3], what=what, lib=_product()) == [(a[cut], b[cut]) for a, b in want[:3]]
    tree.close()


# ---- 4. the VM accepts them ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [64, 127])
def test_tapes_drive_the_merkle_program_on_the_oracle_vm(oracle, depth):
    """the program of src/examples/merkle.rs:46-56 with n = depth + 1 and push.<index>, on the tapes of one member and one absent key, leaves
    (root + root) reversed on the stack (merkle.rs:27-30): smpath and pmpath both authenticate the wide tree"""
    keys = boundary_keys(depth, "random-200", 40 + depth, 5)
    tree = host_wide(depth)
    tree.set(keys, random_pairs(5, depth))
    root = list(tree.root)
    absent = keys[0] ^ (1 << (depth - 1))
    assert tree.get([keys[0], absent])[1] == [True, False]
    for index in (keys[0], absent):
        a, b = tree.tapes(index)
        t = oracle.Trace(merkle_source(depth + 1, index), [], a, b)
        assert t.outputs(4) == (root + root)[::-1], index
    tree.close()


# ---- 5. the path tools without a tree --------------------------------------------------------------------------------------------------------------------
def wide_paths_case(make, n, seed, count=9):
    """-> (root, keys asked, their paths, the leaves the paths hold): members and absent keys of one tree of depth n - 1"""
    depth = n - 1
    keys = boundary_keys(depth, "random-200", seed, count)
    tree = make(depth, NONZERO_EMPTY)
    leaves = random_pairs(count, seed + 1)
    tree.set(keys, leaves)
    ask = keys + [keys[0] ^ (1 << min(64, depth - 2)), keys[1] ^ (1 << (depth - 1)), keys[2] ^ 1]
    paths = tree.paths(ask)
    root = tree.root
    tree.close()
    return root, ask, paths, [p[0] for p in paths]


def check_tree_less_calls(O, make, n, seed, device, lib, count=9):
    import distaff_amd as D
    root, ask, paths, held = wide_paths_case(make, n, seed, count)
    kw = dict(device=device, lib=lib)
    want = [merkle_root(path, i)(O.hasher_digest) for path, i in zip(paths, ask)]
    assert want == [root] * len(ask)
    assert D.path_roots_wide(paths, ask, **kw) == want
    assert D.verify_paths_wide(root, paths, ask, **kw) == (-1, D.DST_PATH_OK) and D.verify_paths_wide(root, paths, ask, leaves=held, **kw) == (-1, D.DST_PATH_OK)
    # ONE index bit flipped at a position >= 64 -- at n = 65, where an index has the bits 0 .. 63, at 63, the highest there is: another root,
    # BAD_ROOT at that i; two of them: the lowest i
    high = min(64, n - 2)
    for at, bit in ((4, high), (2, n - 2), (len(ask) - 1, 70 if n > 71 else high)):
        bent = list(ask)
        bent[at] ^= 1 << bit
        got = D.path_roots_wide(paths, bent, **kw)
        assert got[at] == merkle_root(paths[at], bent[at])(O.hasher_digest) != root and got[:at] + got[at + 1:] == want[1:]
        assert D.verify_paths_wide(root, paths, bent, **kw) == (at, D.DST_PATH_BAD_ROOT)
    bent = list(ask)
    bent[6] ^= 1 << high
    bent[3] ^= 1 << (n - 2)
    assert D.verify_paths_wide(root, paths, bent, **kw) == (3, D.DST_PATH_BAD_ROOT)
    wrong = list(held)
    wrong[5] = (held[5][0] ^ 1, held[5][1])
    wrong[7] = (1, 2)
    assert D.verify_paths_wide(root, paths, ask, leaves=wrong, **kw) == (5, D.DST_PATH_BAD_LEAF)
    bent[1] ^= 1 << high                                                            # a bad root at 1 comes before the bad leaf at 5
    assert D.verify_paths_wide(root, paths, bent, leaves=wrong, **kw) == (1, D.DST_PATH_BAD_ROOT)
    # with substitute leaves: the root each path gives with another first node
    others = random_pairs(len(ask), seed + 5)
    assert D.path_roots_wide(paths, ask, leaves=others, **kw) == [merkle_root([v] + path[1:], i)(O.hasher_digest) for v, path, i in zip(others, paths, ask)]


def check_tree_less_writes(O, make, n, seed, device, lib):
    import distaff_amd as D
    depth = n - 1
    kw = dict(device=device, lib=lib)
    keys = boundary_keys(depth, "random-200", seed, 6)
    tree = make(depth)
    tree.set(keys[:4], random_pairs(4, seed))
    before = tree.root
    batch = [keys[0], keys[4], keys[0], keys[5] | (1 << 64) if depth > 64 else keys[5], keys[4]]
    values = random_pairs(len(batch), seed + 1)
    paths, roots = tree.apply(batch, values)
    assert D.verify_writes_wide(before, batch, paths, values, roots, **kw) == (-1, D.DST_PATH_OK, tree.root)
    assert D.verify_writes_wide(before, batch, paths, values, **kw) == (-1, D.DST_PATH_OK, tree.root)
    claimed = list(roots)
    claimed[2] = (roots[2][0] ^ 1, roots[2][1])
    claimed[4] = (5, 6)
    assert D.verify_writes_wide(before, batch, paths, values, claimed, **kw)[:2] == (2, D.DST_PATH_BAD_NEXT_ROOT)
    bent = list(batch)
    bent[3] ^= 1 << (depth - 1)
    assert D.verify_writes_wide(before, bent, paths, values, roots, **kw)[:2] == (3, D.DST_PATH_BAD_ROOT)
    bent[2] ^= 1 << min(64, depth - 1)                                              # a stored key: the wrong root before write 2 comes before its wrong claimed root
    assert D.verify_writes_wide(before, bent, paths, values, claimed, **kw)[:2] == (2, D.DST_PATH_BAD_ROOT)
    tree.close()


@pytest.mark.parametrize("n", [65, 128])
def test_roots_and_verdicts_without_a_tree(oracle, n):
    check_tree_less_calls(oracle, host_wide, n, 500 + n, -1, _product())
    check_tree_less_writes(oracle, host_wide, n, 600 + n, -1, _product())


# ---- the audit: a sound tree, then one changed node at level 70 and one at level 3 --------------------------------------------------------------------
def check_audit_reports_the_nearer_of_two_changed_nodes(tree, deep=70, near=3, thorough=True):
    """a changed node of level l is not the digest its parent was hashed from: the parent (l - 1, prefix >> 1) is bad -- and so is the node itself,
    one level further from the root.  Of the two changes the audit reports the one nearest the root, then, that one undone, the other;
    `thorough` audits the sound tree before and after as well, and another element of the deep node"""
    import distaff_amd as D
    assert not thorough or tree.audit() is None
    levels = int_levels(tree)
    spots = []
    for l in (deep, near):
        prefixes, nodes = levels[l]
        i = len(prefixes) // 2
        was = tuple(D.arr_to_ints(np.array(nodes[i], dtype=np.uint64)))
        spots.append((l, i, was, (l - 1, prefixes[i] >> 1)))
        tree.test_set_node(l, i, (was[0] ^ 1, was[1]))
    (dl, di, dwas, dwant), (nl, ni, nwas, nwant) = spots
    assert tree.audit() == nwant
    tree.test_set_node(nl, ni, nwas)
    assert tree.audit() == dwant
    if not thorough:
        return
    tree.test_set_node(dl, di, (dwas[0], dwas[1] ^ (1 << 100)))                     # the other element, another bit
    assert tree.audit() == dwant
    tree.test_set_node(dl, di, dwas)
    assert tree.audit() is None


def test_the_audit_reports_the_changed_node_nearest_the_root():
    import distaff_amd as D
    tree = D.WideSparseRescueTree(127, NONZERO_EMPTY, device=-1, lib=D.load_hooks())
    keys = boundary_keys(127, "random-200", 127, 40)
    tree.set(keys, random_pairs(40, 4))
    check_audit_reports_the_nearer_of_two_changed_nodes(tree)
    tree.close()
    tree = host_wide(127)                                                           # the product library has the entry point and refuses
    tree.set(keys[:2], random_pairs(2, 4))
    with pytest.raises(D.DistaffError) as e:
        tree.test_set_node(127, 0, (1, 2))
    assert e.value.code == D.DST_ERR_STATE and tree.audit() is None
    tree.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def key_bytes(keys):
    import distaff_amd as D
    return D.ints_to_arr(keys)


def test_refusals_leave_the_tree_unchanged_and_the_accepted_pair_is_two_keys():
    import distaff_amd as D
    lib = _product()
    h = ctypes.c_void_p()
    for depth in (0, 128, 1 << 20):
        assert lib.dst_wtree_create(-1, depth, None, ctypes.byref(h)) == D.DST_ERR_ARG and not h.value
        with pytest.raises(D.DistaffError) as e:
            host_wide(depth)
        assert e.value.code == D.DST_ERR_ARG and "127" in str(e.value)
    assert lib.dst_wtree_create(-1, 5, None, None) == D.DST_ERR_ARG
    with pytest.raises(D.DistaffError) as e:
        host_wide(100, (P, 0))
    assert e.value.code == D.DST_ERR_ARG
    buf = ctypes.create_string_buffer(130 * 32)
    assert lib.dst_wtree_root(None, buf) == D.DST_ERR_ARG and lib.dst_wtree_set(None, None, None, ctypes.c_size_t(0)) == D.DST_ERR_ARG
    for depth in (64, 127):
        tree = host_wide(depth)
        top = 1 << depth
        k = 0x0123456789ABCDEF
        tree.set([k, k + (1 << 64)] if depth > 64 else [k, k ^ 1], [(1, 2), (3, 4)])      # equal low halves, different high halves: two keys
        assert tree.info()["keys"] == 2 and tree.get([k]) == ([(1, 2)], [True])
        if depth > 64:
            assert tree.get([k + (1 << 64), k + (1 << 65)]) == ([(3, 4), (0, 0)], [True, False])
        before = (tree.root, tree.info(), int_levels(tree))
        bad_sets = [([top], [(1, 1)]), ([3, top], [(1, 1), (2, 2)]), ([top + 5], [(1, 1)]), ([3, 4, 3], [(1, 1), (2, 2), (3, 3)]), ([k, k], [(1, 1), (2, 2)]),
                    ([top - 1, 7, top - 1], [(1, 1), (2, 2), (3, 3)]), ([3], [(P, 0)]), ([3, 4], [(1, 1), (5, P)]), ([6], [(2 ** 128 - 1, 0)])]
        if depth < 127:
            bad_sets += [([1 << 127], [(1, 1)]), ([(1 << 64) << 40], [(1, 1)])]           # wrong in the high 8 bytes only
        for keys, leaves in bad_sets:
            with pytest.raises(D.DistaffError) as e:
                tree.set(keys, leaves)
            assert e.value.code == D.DST_ERR_ARG, keys
        calls = [lambda: tree.path(top), lambda: tree.get([top]), lambda: tree.remove([top]), lambda: tree.remove([k, k]), lambda: tree.apply([top], [(1, 1)]),
                 lambda: tree.apply([3], [(P, 1)]), lambda: tree.tapes(top), lambda: tree.tapes(0, what=0), lambda: tree.tapes(0, what=4), lambda: tree.level(depth + 1),
                 lambda: tree.set([1 << 128], [(1, 1)]), lambda: tree.set([-1], [(1, 1)])]
        for call in calls:
            with pytest.raises(D.DistaffError) as e:
                call()
            assert e.value.code == D.DST_ERR_ARG
        idx = key_bytes([3])
        ip, one = idx.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1)
        assert lib.dst_wtree_set(tree._h, None, buf, one) == D.DST_ERR_ARG and lib.dst_wtree_set(tree._h, ip, None, one) == D.DST_ERR_ARG
        assert lib.dst_wtree_paths(tree._h, None, one, buf) == D.DST_ERR_ARG and lib.dst_wtree_paths(tree._h, ip, one, None) == D.DST_ERR_ARG
        assert lib.dst_wtree_get(tree._h, None, one, buf, None) == D.DST_ERR_ARG and lib.dst_wtree_remove(tree._h, None, one, None) == D.DST_ERR_ARG
        assert lib.dst_wtree_apply(tree._h, None, buf, one, None, None) == D.DST_ERR_ARG
        assert lib.dst_wtree_root(tree._h, None) == D.DST_ERR_ARG and lib.dst_wtree_info(tree._h, None) == D.DST_ERR_ARG
        assert lib.dst_wtree_audit(tree._h, None, buf, None) == D.DST_ERR_ARG
        assert (tree.root, tree.info(), int_levels(tree)) == before
        assert lib.dst_wtree_set(tree._h, None, None, ctypes.c_size_t(0)) == D.DST_OK and tree.remove([]) == 0 and tree.root == before[0]
        tree.close()
        tree.close()


def test_the_tree_less_calls_refuse_what_their_narrow_forms_refuse():
    import distaff_amd as D
    lib = _product()
    path = lambda n: [[(1, 2)] * n]  # noqa: E731
    for n in (1, 129):
        for call in (lambda: D.path_roots_wide(path(n), [0], device=-1, lib=lib), lambda: D.verify_paths_wide((1, 2), path(n), [0], device=-1, lib=lib),
                     lambda: D.verify_writes_wide((1, 2), [0], path(n), [(3, 4)], device=-1, lib=lib), lambda: D.path_tapes_wide(path(n), [0], lib=lib)):
            with pytest.raises(D.DistaffError) as e:
                call()
            assert e.value.code == D.DST_ERR_ARG and "128" in str(e.value), n
    for n in (2, 65, 128):
        top = 1 << (n - 1)
        assert D.path_roots_wide(path(n), [top - 1], device=-1, lib=lib) and D.path_tapes_wide(path(n), [top - 1], lib=lib)
        for index in (top, top << 1 if n < 128 else top + 1, (1 << 127) | 5 if n < 128 else top):
            for call in (lambda: D.path_roots_wide(path(n), [index], device=-1, lib=lib), lambda: D.path_tapes_wide(path(n), [index], lib=lib),
                         lambda: D.verify_paths_wide((1, 2), path(n), [index], device=-1, lib=lib)):
                with pytest.raises(D.DistaffError) as e:
                    call()
                assert e.value.code == D.DST_ERR_ARG, (n, index)
    with pytest.raises(D.DistaffError) as e:
        D.path_roots_wide([[(1, 2), (P, 0), (3, 4)]], [1], device=-1, lib=lib)      # an element not below p
    assert e.value.code == D.DST_ERR_ARG
    w = np.zeros((1, 65, 2, 2), dtype=np.uint64)
    out = ctypes.create_string_buffer(64)
    ms = ctypes.c_double(0)
    assert lib.dst_rescue_path_roots_w(-1, w.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(65), None, ctypes.c_size_t(1), None, out, ctypes.byref(ms)) == D.DST_ERR_ARG
    assert lib.dst_rescue_path_roots_w(-1, None, ctypes.c_uint32(65), None, ctypes.c_size_t(0), None, out, ctypes.byref(ms)) == D.DST_OK
    assert lib.dst_rescue_path_roots_w(-1, None, ctypes.c_uint32(129), None, ctypes.c_size_t(0), None, out, ctypes.byref(ms)) == D.DST_ERR_ARG


# ---- the C example ----------------------------------------------------------------------------------------------------------------------------------------
def run_wide_example(tmp_path, k, device):
    import distaff_amd as D
    exe = tmp_path / "merkle_wide"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_wide.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    r = subprocess.run([str(exe), str(k), str(device)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()
    return r.stdout.decode().splitlines()


def wide_example_lines(O, k):
    """what examples/merkle_wide.c prints for k keys, from the oracle's digest (the keys), the host tree and the restated tapes"""
    keys = [O.hasher_digest([i, 1, 2, 3])[0] & ((1 << 127) - 1) for i in range(k + 1)]
    tree = host_wide(127)
    tree.set(keys[:k], [(2 * i + 1, 2 * i + 2) for i in range(k)])
    ask = [keys[0], keys[k]]
    paths = tree.paths(ask)
    assert paths[0][0] == (1, 2) and paths[1][0] == (0, 0)
    h = lambda v: "%032x" % v  # noqa: E731
    lines = ["root %s %s" % (h(tree.root[0]), h(tree.root[1])),
             "%d keys of 127 bits in %d stored nodes, %d digests" % (k, tree.info()["nodes"], ancestors(keys[:k], 127)),
             "member %s and absent key %s verified against the root alone; the wrong key is rejected" % (h(ask[0]), h(ask[1]))]
    for name, path, index in zip(("member", "absent"), paths, ask):
        assert merkle_root(path, index)(O.hasher_digest) == tree.root
        a, b = tapes_from_path(path, index)
        lines += ["%s tape a: %s" % (name, " ".join(h(v) for v in a)), "%s tape b: %s" % (name, " ".join(h(v) for v in b))]
    tree.close()
    return lines + ["382 elements per tape and key, smpath.128 / pmpath.128"]


def test_c_example_inserts_hash_derived_keys_and_checks_a_member_and_an_absent_key(oracle, tmp_path):
    """examples/merkle_wide.c compiles as C99 against include/distaff_hip.h and the product library and runs on the host"""
    assert run_wide_example(tmp_path, 9, -1) == wide_example_lines(oracle, 9)


def test_package_reexports_the_binding():
    import distaff_amd as D
    assert D.WideSparseRescueTree is not None and not hasattr(D.WideSparseRescueTree, "multiproof") and not hasattr(D.WideSparseRescueTree, "save")
    assert {"dst_wtree_create", "dst_wtree_set", "dst_wtree_remove", "dst_wtree_compact", "dst_wtree_get", "dst_wtree_root", "dst_wtree_paths", "dst_wtree_apply",
            "dst_wtree_tapes_many", "dst_wtree_read_level", "dst_wtree_info", "dst_wtree_audit", "dst_wtree_destroy", "dst_wtree_last_error",
            "dst_rescue_path_roots_w", "dst_rescue_verify_paths_w", "dst_rescue_verify_writes_w", "dst_rescue_path_tapes_w"} <= set(D.EXPORTS)
    assert all(hasattr(_product(), name) for name in D.EXPORTS if "_wtree_" in name or name.endswith("_w"))
