"""Wide-key sparse Rescue Merkle trees and the path tools over 16-byte indices on the GPU (the stree_wide instantiations of rescue_stree_level_kernel,
rescue_stree_level_spread_kernel, rescue_stree_open_kernel, rescue_stree_get_kernel, both audit kernels and both path-root kernels) through the
library the session binds.  Everything is bit-exact.  The yardsticks: the narrow DEVICE tree at depth 12, where both exist; the host wide tree,
which tests/test_wide_sparse_rescue_tree_host.py holds against the oracle, for the boundary sets at depth 127 and for the path tools; and for
the tree of 2^15 + 2^14 keys the definition itself, restated with numpy over the two 64-bit halves of a prefix and hashed by
dst_rescue_digest_many on the device (which tests/test_rescue_tree_gpu.py holds against the oracle).  That tree has 5.5e6 parents: the host
path, one thread at some 90 microseconds a digest, would take eight minutes to build it, so the host tree is not the yardstick there.
Every test has its own time limit and nothing is run twice."""
import numpy as np
import pytest

from test_rescue_tree_host import merkle_source
from test_sparse_rescue_tree_gpu import random_words
from test_sparse_rescue_tree_host import NONZERO_EMPTY, ancestors, random_pairs
from test_wide_sparse_rescue_tree_host import (BOUNDARY_SETS, boundary_keys, check_audit_reports_the_nearer_of_two_changed_nodes, figures, int_levels, run_wide_example,
                                               some_absent, wide_example_lines)

pytestmark = pytest.mark.gpu
SPREAD_MAX = 1 << 15                       # RESCUE_SPREAD_MAX: launches of more parents, or chains, run the one-lane kernels
ONE = np.uint64(1)


def device_wide(depth, empty=(0, 0)):
    import distaff_amd as D
    return D.WideSparseRescueTree(depth, empty, device=0)


def host_wide(depth, empty=(0, 0)):
    import distaff_amd as D
    return D.WideSparseRescueTree(depth, empty, device=-1)


@pytest.mark.timeout(120)
def test_depth_12_every_node_and_every_path_equals_the_narrow_device_tree():
    import distaff_amd as D
    depth, n = 12, 1 << 12
    rng = np.random.default_rng(12)
    keys = [int(k) for k in np.unique(np.concatenate([rng.integers(0, n, size=1200), np.arange(2048, 2348)]))]
    leaves = random_words(len(keys), 121)
    narrow, wide = D.SparseRescueTree(depth, NONZERO_EMPTY, device=0), device_wide(depth, NONZERO_EMPTY)
    narrow.set(keys, leaves); wide.set(keys, leaves)
    assert int_levels(wide) == int_levels(narrow) and wide.root == narrow.root and figures(wide) == figures(narrow)
    every = list(range(n))
    assert np.array_equal(wide.paths_words(every), narrow.paths_words(every))
    got, want = wide.get_words(every), narrow.get_words(every)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert wide.audit() is None
    narrow.close(); wide.close()


# ---- depth 127, more than 2^15 parents per level: the definition restated over (low, high) halves, hashed by the device's digest kernel --------------
def sorted_keys(lo, hi):
    order = np.lexsort((lo, hi))
    return np.stack([lo[order], hi[order]], axis=1), order


def empties_of(empty, depth):
    """E_l as words [depth + 1, 2, 2]: E_depth = the empty leaf, E_l = digest(E_{l+1}, E_{l+1}), by dst_rescue_digest_many on the host"""
    import distaff_amd as D
    e = [D.ints_to_arr(list(empty))]
    for _ in range(depth):
        e.append(D.rescue_digest(np.concatenate([e[-1], e[-1]]).reshape(1, 4, 2), device=-1)[0])
    return np.stack(e[::-1])


def restated_levels(keys, leaves, empties, depth):
    """keys: words [m, 2] sorted by (high, low), distinct; leaves: words [m, 2, 2] -> per level (prefix words, node words), and the number of parents"""
    import distaff_amd as D
    levels = {depth: (keys, leaves)}
    parents = 0
    for l in range(depth - 1, -1, -1):
        ck, cv = levels[l + 1]
        lo, hi = ck[:, 0], ck[:, 1]
        plo, phi = (lo >> ONE) | (hi << np.uint64(63)), hi >> ONE                   # the shift carries bit 64 across the halves
        first = np.ones(len(ck), dtype=bool)
        first[1:] = (plo[1:] != plo[:-1]) | (phi[1:] != phi[:-1])
        parent = np.cumsum(first) - 1
        m = int(parent[-1]) + 1
        right = (lo & ONE).astype(bool)
        inp = np.empty((m, 4, 2), dtype=np.uint64)
        inp[:, 0:2] = empties[l + 1]; inp[:, 2:4] = empties[l + 1]
        inp[parent[~right], 0:2] = cv[~right]
        inp[parent[right], 2:4] = cv[right]
        levels[l] = (np.stack([plo[first], phi[first]], axis=1), D.rescue_digest(inp, device=0))
        parents += m
    return levels, parents


def assert_tree_is(tree, levels):
    for l in range(tree.depth + 1):
        prefixes, nodes = tree.level(l)
        assert np.array_equal(prefixes, levels[l][0]), l
        assert np.array_equal(nodes, levels[l][1]), l


def merged(keys, leaves, more_keys, more_leaves):
    """content after a set: the later value of a key wins -> sorted distinct keys and their leaves"""
    k, v = np.concatenate([more_keys, keys]), np.concatenate([more_leaves, leaves])
    both, order = sorted_keys(k[:, 0], k[:, 1])
    v = v[order]
    keep = np.ones(len(both), dtype=bool)
    keep[1:] = (both[1:] != both[:-1]).any(axis=1)                                   # lexsort is stable: the first of equal keys is the later value
    return both[keep], v[keep]


def distinct_ancestors(keys, depth, among=None):
    """the number of distinct key >> (depth - l) over the levels l < depth; with `among` (per level prefix words) only those found there"""
    total = 0
    lo, hi = keys[:, 0].copy(), keys[:, 1].copy()
    for l in range(depth - 1, -1, -1):
        lo, hi = (lo >> ONE) | (hi << np.uint64(63)), hi >> ONE
        first = np.ones(len(lo), dtype=bool)
        first[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
        lo, hi = lo[first], hi[first]
        if among is None:
            total += len(lo)
        else:                                                                       # both lists are distinct: a prefix in both shows twice
            _, seen = np.unique(np.concatenate([np.stack([lo, hi], axis=1), among[l][0]]), axis=0, return_counts=True)
            total += int((seen == 2).sum())
    return total


@pytest.mark.timeout(600)
def test_depth_127_set_update_and_removal_of_more_keys_than_the_six_lane_form_takes():
    """2^15 + 2^14 random keys: the low levels have more than RESCUE_SPREAD_MAX parents -- the one-lane kernel over whole levels, the six-lane one
    above.  Then one set of 2^15 + 2^13 keys, half stored and half new (the one-lane kernel over a dirty list), then the removal of a quarter;
    after each step every level equals the definition, last_digests the count of distinct ancestors computed here.  The one-lane audit finds the
    tree sound and names the nearer of two changed nodes."""
    depth = 127
    rng = np.random.default_rng(127)
    count = (1 << 15) + (1 << 14)
    raw = rng.integers(0, 1 << 64, size=(count, 2), dtype=np.uint64)
    raw[:, 1] >>= ONE                                                              # below 2^127
    keys, _ = sorted_keys(raw[:, 0], raw[:, 1])
    assert len(np.unique(keys, axis=0)) == count
    leaves = random_words(count, 1271)
    empties = empties_of((0, 0), depth)
    tree = device_wide(depth)
    shuffled = rng.permutation(count)
    tree.set(keys[shuffled], leaves[shuffled])
    levels, parents = restated_levels(keys, leaves, empties, depth)
    assert len(levels[depth - 1][0]) > SPREAD_MAX > len(levels[12][0])
    assert tree.info()["last_digests"] == parents == distinct_ancestors(keys, depth) and tree.info()["last_device_ms"] > 0
    assert_tree_is(tree, levels)
    # half stored, half new
    half = ((1 << 15) + (1 << 13)) // 2
    fresh = rng.integers(0, 1 << 64, size=(half, 2), dtype=np.uint64)
    fresh[:, 1] >>= ONE
    batch = np.ascontiguousarray(np.concatenate([keys[rng.choice(count, size=half, replace=False)], fresh]))
    values = random_words(len(batch), 1272)
    tree.set(batch, values)
    bkeys, _ = sorted_keys(batch[:, 0], batch[:, 1])
    assert tree.info()["last_digests"] == distinct_ancestors(bkeys, depth) and len(np.unique(bkeys >> np.uint64(1), axis=0)) > SPREAD_MAX
    keys, leaves = merged(keys, leaves, batch, values)
    assert len(keys) == count + half
    levels, _ = restated_levels(keys, leaves, empties, depth)
    assert_tree_is(tree, levels)
    # remove a quarter
    gone = np.zeros(len(keys), dtype=bool)
    gone[rng.choice(len(keys), size=len(keys) // 4, replace=False)] = True
    removed = np.ascontiguousarray(keys[gone][rng.permutation(int(gone.sum()))])
    assert tree.remove(removed) == len(removed)
    levels, _ = restated_levels(keys[~gone], leaves[~gone], empties, depth)
    assert tree.info()["last_digests"] == distinct_ancestors(keys[gone], depth, among=levels)
    assert_tree_is(tree, levels)
    assert tree.info()["nodes"] - tree.info()["keys"] > SPREAD_MAX
    check_audit_reports_the_nearer_of_two_changed_nodes(tree)
    tree.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", BOUNDARY_SETS)
def test_depth_127_boundary_sets_equal_the_host_tree(name):
    """paths, get, apply, audit, removal and every level of the device tree against the host tree, for the key sets at the boundary of the halves"""
    depth = 127
    keys = boundary_keys(depth, name, 100 * depth + BOUNDARY_SETS.index(name))
    leaves = random_pairs(len(keys), 5)
    a, b = device_wide(depth, NONZERO_EMPTY), host_wide(depth, NONZERO_EMPTY)
    a.set(keys, leaves); b.set(keys, leaves)
    absent = some_absent(depth, keys, 9) + [keys[0] ^ (1 << 64), keys[0] ^ (1 << 126)]
    ask = keys + [k for k in absent if k not in keys] + keys[:1]

    def same():
        assert int_levels(a) == int_levels(b) and a.root == b.root and figures(a)[:3] == figures(b)[:3]
        assert a.paths(ask) == b.paths(ask) and a.get(ask) == b.get(ask) and a.tapes_many(ask[:4]) == b.tapes_many(ask[:4])
        assert a.audit() is None
    same()
    assert a.info()["last_digests"] == ancestors(keys, depth)
    batch = [keys[0], ask[len(keys)], keys[0], keys[-1], ask[len(keys)]]
    values = random_pairs(4, 6) + [NONZERO_EMPTY]
    assert a.apply(batch, values) == b.apply(batch, values)
    same()
    gone = keys[::2]
    assert a.remove(gone) == b.remove(gone) == len(gone)
    same()
    assert a.compact() == b.compact()
    same()
    a.close(); b.close()


@pytest.mark.timeout(120)
def test_the_six_lane_audit_reports_the_nearer_of_two_changed_nodes():
    tree = device_wide(127, NONZERO_EMPTY)
    tree.set(boundary_keys(127, "random-200", 127, 40), random_pairs(40, 4))
    assert tree.info()["nodes"] - tree.info()["keys"] <= SPREAD_MAX
    check_audit_reports_the_nearer_of_two_changed_nodes(tree)
    assert tree.audit_ms > 0
    tree.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("count", [3, 40000], ids=["six-lane", "one-lane"])
@pytest.mark.parametrize("n", [65, 128])
def test_path_roots_and_verdicts_on_the_device_equal_the_host(n, count):
    """`count` chains: 3 run the six-lane kernel, 40 000 the one-lane kernel.  The paths are those of 50 keys, stored and absent, of one host tree,
    taken round and round; the host hashes the 50 and the device all of them.  An index with one bit flipped at a position >= 64 (at n = 65,
    where an index ends at bit 63, at 63) gives another root there and is the first bad path; with new leaves the 2 * count chains of
    verify_writes_wide agree with the host as well"""
    import distaff_amd as D
    depth = n - 1
    keys = boundary_keys(depth, "random-200", 50 + n, 30)
    tree = host_wide(depth, NONZERO_EMPTY)
    tree.set(keys, random_pairs(30, n))
    distinct = keys + some_absent(depth, keys, n, 18)[:20]
    words = tree.paths_words(distinct)
    root = tree.root
    host_roots = D.path_roots_wide(words, distinct, device=-1)
    assert host_roots == [root] * len(distinct)
    pick = np.arange(count) % len(distinct)
    indices = [distinct[i] for i in pick]
    paths = np.ascontiguousarray(words[pick])
    stats = {}
    assert D.path_roots_wide(paths, indices, device=0, stats=stats) == [root] * count and stats["device_ms"] > 0
    assert D.verify_paths_wide(root, paths, indices, device=0) == (-1, D.DST_PATH_OK)
    high = min(64, n - 2)
    bent = list(indices)
    early = count // 2
    late = max(i for i in range(early + 1, count) if i % len(distinct) < len(keys))
    bent[late] ^= 1 << high
    bent[early] ^= 1 << (n - 2)
    assert early % len(distinct) < len(keys) and late % len(distinct) < len(keys)   # stored keys: their siblings are no empty subtrees
    got = D.path_roots_wide(paths, bent, device=0)
    want = D.path_roots_wide(words[[early % len(distinct), late % len(distinct)]], [bent[early], bent[late]], device=-1)
    assert [got[early], got[late]] == want and root not in want
    assert [r for i, r in enumerate(got) if i not in (early, late)] == [root] * (count - 2)
    assert D.verify_paths_wide(root, paths, bent, device=0) == (early, D.DST_PATH_BAD_ROOT)
    bent[early] = indices[early]
    assert D.verify_paths_wide(root, paths, bent, device=0) == (late, D.DST_PATH_BAD_ROOT)
    held = paths[:, 0].copy()
    held[late, 0, 0] ^= ONE
    assert D.verify_paths_wide(root, paths, indices, leaves=held, device=0) == (late, D.DST_PATH_BAD_LEAF)
    # substitute leaves: both chains of every path in one launch, against the host over the distinct ones
    others = random_words(len(distinct), n + count)
    want = D.path_roots_wide(words, distinct, leaves=others, device=-1)
    assert D.path_roots_wide(paths, indices, leaves=np.ascontiguousarray(others[pick]), device=0) == [want[i] for i in pick]
    tree.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("n", [65, 128])
def test_verify_writes_on_the_device_equals_the_host(n):
    import distaff_amd as D
    depth = n - 1
    keys = boundary_keys(depth, "random-200", 80 + n, 12)
    tree = device_wide(depth)
    tree.set(keys[:8], random_pairs(8, n))
    before = tree.root
    batch = [keys[0], keys[9], keys[0], keys[10], keys[9], keys[3]]
    values = random_pairs(len(batch), n + 1)
    paths, roots = tree.apply(batch, values)
    for device in (0, -1):
        assert D.verify_writes_wide(before, batch, paths, values, roots, device=device) == (-1, D.DST_PATH_OK, tree.root)
    bent = list(batch)
    bent[2] ^= 1 << min(64, depth - 1)
    claimed = list(roots)
    claimed[4] = (5, 6)
    for device in (0, -1):
        assert D.verify_writes_wide(before, bent, paths, values, roots, device=device)[:2] == (2, D.DST_PATH_BAD_ROOT)
        assert D.verify_writes_wide(before, batch, paths, values, claimed, device=device)[:2] == (4, D.DST_PATH_BAD_NEXT_ROOT)
    tree.close()


@pytest.mark.timeout(300)
def test_c_example_runs_on_the_device(oracle, tmp_path):
    assert run_wide_example(tmp_path, 200, 0) == wide_example_lines(oracle, 200)


@pytest.mark.timeout(300)
def test_membership_in_a_depth_64_tree_is_proven_and_verified_end_to_end(oracle):
    """wide tree of depth 64 on the GPU -> tapes of a stored key -> the depth-65 program of src/examples/merkle.rs:46-56 on the oracle VM -> proof on
    the GPU -> dst_verify accepts with outputs (root + root) reversed (merkle.rs:27-30)"""
    import distaff_amd as D
    O = oracle
    keys = boundary_keys(64, "random-200", 64, 256)
    tree = device_wide(64)
    tree.set(keys, random_words(len(keys), 641))
    root = list(tree.root)
    index = max(keys)
    assert index >> 63 == 1                                                          # a key no depth-63 tree holds
    a, b = tree.tapes(index)
    tree.close()
    t = O.Trace(merkle_source(65, index), [], a, b)
    outputs = (root + root)[::-1]
    assert t.outputs(4) == outputs and t.trace_hash() == t.program_hash
    ctx = D.Context(t.length.bit_length() - 1, t.width, t.ctx_depth, t.loop_depth, grinding=8)
    ctx.upload(t.columns)
    proof = ctx.prove([], outputs)
    ctx.close()
    assert D.verify(proof, t.program_hash, [], outputs) == (True, "")
    tampered = list(outputs)
    tampered[1] ^= 1 << 32
    ok, err = D.verify(proof, t.program_hash, [], tampered)
    assert not ok and err
