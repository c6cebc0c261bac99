"""Save, restore and audit of the Rescue Merkle trees (dst_rtree_save / load / audit, dst_stree_save / load / audit) on the host path (device = -1)
of the PRODUCT library.  No GPU.  The yardsticks are the trees themselves, which tests/test_rescue_tree_host.py and
tests/test_sparse_rescue_tree_host.py hold against the oracle: a loaded tree must BE the tree that was saved -- nodes, levels, paths, multiproofs,
and every later update / apply / set / remove / compact -- and the audit must name the parent whose children were changed.  Everything is
bit-exact.  Also here: the check_* functions the emulated and the GPU tests share; a `Side` says where the trees live."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from test_rescue_tree_host import P, _product
from test_sparse_rescue_tree_host import NONZERO_EMPTY, assert_same_levels, depth_63_keys, levels_of, random_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 64
DENSE_LOGS = (1, 3, 13)                 # 13: 8 191 parents in one launch


class Side:
    """the trees of one library on one device (-1: the host path)"""

    def __init__(self, device, lib):
        self.device, self.lib = device, lib

    def dense(self, leaves):
        import distaff_amd as D
        return D.RescueTree(leaves, device=self.device, lib=self.lib)

    def sparse(self, depth, empty=(0, 0)):
        import distaff_amd as D
        return D.SparseRescueTree(depth, empty, device=self.device, lib=self.lib)

    def load_dense(self, blob, audit=False):
        import distaff_amd as D
        return D.RescueTree.load(blob, device=self.device, audit=audit, lib=self.lib)

    def load_sparse(self, blob, audit=False):
        import distaff_amd as D
        return D.SparseRescueTree.load(blob, device=self.device, audit=audit, lib=self.lib)


def host_side():
    return Side(-1, _product())


def random_words(count, seed):
    """`count` leaves as uint64 words [count, 2, 2], every element below 2^126"""
    return np.random.default_rng(seed).integers(0, 1 << 62, size=(count, 2, 2), dtype=np.uint64)


def sparse_cases():
    """(depth, empty leaf, keys, the key that is stored with the empty value or None): depth 1; depth 8 with 40 keys, among them both children of
    one parent and one key stored with the empty value; depth 63 with 3 keys; no keys; a non-zero empty leaf"""
    rnd = random.Random(88)
    eight = set(rnd.sample(range(256), 38))
    k = next(x for x in range(0, 256, 2) if x not in eight and x ^ 1 not in eight)
    eight = sorted(eight | {k, k ^ 1})
    assert len(eight) == 40
    return [(1, (0, 0), [1], None),
            (8, (0, 0), eight, eight[7]),
            (63, (0, 0), depth_63_keys(3, 6)[:3], None),
            (5, (0, 0), [], None),
            (4, NONZERO_EMPTY, [0, 9, 15, 6], 9)]


def build_sparse(side, case, seed=5):
    depth, empty, keys, hollow = case
    tree = side.sparse(depth, empty)
    leaves = random_pairs(len(keys), seed)
    tree.set(keys, [tuple(empty) if k == hollow else v for k, v in zip(keys, leaves)])
    return tree


def absent_keys(depth, keys):
    return list(dict.fromkeys(k for k in (0, 1, 2, (1 << depth) - 1, (1 << depth) - 2, 1 << (depth - 1)) if k not in keys and k < 1 << depth))


def bump(blob, offset):
    """the blob with the 16-byte element at `offset` replaced by (x + 1) mod p"""
    b = bytearray(blob)
    b[offset:offset + 16] = ((int.from_bytes(b[offset:offset + 16], "little") + 1) % P).to_bytes(16, "little")
    return bytes(b)


def parse_sparse(blob):
    """-> (depth, [(level, prefixes, offset of the level's first node in the blob)], the leaf level first)"""
    depth, nodes = int.from_bytes(blob[12:16], "little"), int.from_bytes(blob[56:64], "little")
    counts = [int.from_bytes(blob[HEADER + 8 * k:HEADER + 8 * k + 8], "little") for k in range(depth + 1)]
    at, out, seen = HEADER + 8 * (depth + 1), [], 0
    for k, c in enumerate(counts):
        prefixes = [int.from_bytes(blob[at + 8 * (seen + i):at + 8 * (seen + i) + 8], "little") for i in range(c)]
        out.append((depth - k, prefixes, at + 8 * nodes + 32 * seen))
        seen += c
    assert seen == nodes and len(blob) == HEADER + 8 * (depth + 1) + 40 * nodes
    return depth, out


def sparse_blob(depth, empty, levels, keys=None, nodes=None):
    """a sparse blob from `levels` = [(prefixes, node bytes)] with the leaf level first; `keys` / `nodes`: the header's counts when they are to lie"""
    total = sum(len(p) for p, _ in levels)
    out = b"DSTTREE1" + (2).to_bytes(4, "little") + depth.to_bytes(4, "little") + b"".join(int(e).to_bytes(16, "little") for e in empty)
    out += (len(levels[0][0]) if keys is None else keys).to_bytes(8, "little") + (total if nodes is None else nodes).to_bytes(8, "little")
    out += b"".join(len(p).to_bytes(8, "little") for p, _ in levels)
    out += b"".join(q.to_bytes(8, "little") for p, _ in levels for q in p)
    return out + b"".join(n for _, n in levels)


# ---- 1. round trip ----------------------------------------------------------------------------------------------------------------------------
def check_dense_round_trip(a, b, log_leaves):
    """load(save(t)) IS t on side a -- root, every node, paths, multiproofs, the blob again -- and side b saves the same bytes and loads a's"""
    import distaff_amd as D
    n = 1 << log_leaves
    leaves = random_words(n, 400 + log_leaves)
    tree = a.dense(leaves)
    blob = tree.save()
    assert len(blob) == HEADER + 32 * (2 * n - 1) and blob[:8] == b"DSTTREE1" and blob[8:16] == (1).to_bytes(4, "little") + log_leaves.to_bytes(4, "little")
    assert blob[16:48] == bytes(32) and blob[48:64] == n.to_bytes(8, "little") + (2 * n - 1).to_bytes(8, "little")
    assert blob[HEADER:] == tree.nodes(1, 2 * n - 1).tobytes()
    assert tree.audit() is None                                                     # a built tree that was never saved
    ask = sorted({0, 1, n // 2, n - 1})
    other = b.dense(leaves)
    assert other.save() == blob
    for loaded in (a.load_dense(blob, audit=True), b.load_dense(blob), a.load_dense(other.save())):
        assert loaded.log_leaves == log_leaves and loaded.root == tree.root
        assert np.array_equal(loaded.nodes(0, 2 * n), tree.nodes(0, 2 * n))
        assert loaded.paths(ask) == tree.paths(ask) and loaded.multiproof(ask) == tree.multiproof(ask) and loaded.tapes(n - 1) == tree.tapes(n - 1)
        assert loaded.save() == blob
        assert loaded.build_ms == 0 and loaded.update_ms == 0                       # nothing was hashed
        assert loaded.audit() is None
        loaded.close()
    tree.close(); other.close()


def check_sparse_round_trip(a, b, case):
    depth, empty, keys, hollow = case
    tree, other = build_sparse(a, case), build_sparse(b, case)
    blob = tree.save()
    info = tree.info()
    assert len(blob) == HEADER + 8 * (depth + 1) + 40 * info["nodes"] and blob[:16] == b"DSTTREE1" + (2).to_bytes(4, "little") + depth.to_bytes(4, "little")
    assert blob[48:64] == len(keys).to_bytes(8, "little") + info["nodes"].to_bytes(8, "little")
    assert [(l, p) for l, p, _ in parse_sparse(blob)[1]] == [(l, [int(q) for q in tree.level(l)[0]]) for l in range(depth, -1, -1)]
    assert other.save() == blob
    assert tree.audit() is None
    ask = list(keys) + absent_keys(depth, keys)
    for loaded in (a.load_sparse(blob), a.load_sparse(blob, audit=True), b.load_sparse(blob), a.load_sparse(other.save())):
        assert loaded.depth == depth and loaded.root == tree.root
        assert_same_levels(levels_of(loaded), levels_of(tree))
        assert loaded.paths(ask) == tree.paths(ask) and loaded.multiproof(ask) == tree.multiproof(ask) and loaded.get(ask) == tree.get(ask)
        assert loaded.save() == blob
        li = loaded.info()
        assert (li["keys"], li["nodes"], li["last_digests"], li["last_device_ms"]) == (len(keys), info["nodes"], 0, 0)
        assert loaded.audit() is None
        loaded.close()
    if hollow is not None:                                                          # the key with the empty value is stored in the blob
        loaded = a.load_sparse(blob)
        assert loaded.get([hollow]) == ([tuple(empty)], [True])
        loaded.close()
    tree.close(); other.close()


# ---- 2. a loaded tree lives ---------------------------------------------------------------------------------------------------------------------
def check_loaded_dense_lives(side, log_leaves=3):
    n = 1 << log_leaves
    built = side.dense(random_words(n, 500))
    loaded = side.load_dense(built.save())
    assert loaded.build_ms == 0 and loaded.update_ms == 0
    idx = [n - 1, 0, n // 2]
    for t in (built, loaded):
        t.update(idx, random_words(3, 501))
    assert loaded.root == built.root and np.array_equal(loaded.nodes(0, 2 * n), built.nodes(0, 2 * n))
    writes = [1, n - 1, 1, 0]
    assert loaded.apply(writes, random_words(4, 502)) == built.apply(writes, random_words(4, 502))
    assert loaded.root == built.root and np.array_equal(loaded.nodes(0, 2 * n), built.nodes(0, 2 * n))
    assert loaded.audit() is None and built.audit() is None                         # trees that have lived through updates
    assert loaded.save() == built.save()
    built.close(); loaded.close()


def check_loaded_sparse_lives(side, case):
    """set, apply, remove and compact on a loaded tree and on the tree it was saved from: equal levels, roots, witnesses and figures"""
    depth, empty, keys, hollow = case
    built = build_sparse(side, case)
    loaded = side.load_sparse(built.save())
    assert loaded.info()["last_digests"] == 0 and loaded.info()["last_device_ms"] == 0
    h = absent_keys(depth, keys)[0]
    last = (1 << depth) - 1 if h != (1 << depth) - 1 else (1 << depth) - 2            # any other key, stored or not

    def same():
        assert_same_levels(levels_of(loaded), levels_of(built))
        a, b = loaded.info(), built.info()
        assert loaded.root == built.root and [a[f] for f in ("keys", "nodes", "last_digests")] == [b[f] for f in ("keys", "nodes", "last_digests")]

    for t in (built, loaded):
        t.set([h, last], random_pairs(2, 600))
    same()
    assert loaded.info()["last_digests"] > 0
    writes, values = [h, last, h], random_pairs(2, 601) + [tuple(empty)]              # h ends with the empty value, and stays stored
    assert loaded.apply(writes, values) == built.apply(writes, values)
    same()
    assert loaded.remove([last]) == built.remove([last]) == 1
    same()
    assert loaded.compact() == built.compact() == (2 if hollow is not None else 1)
    same()
    assert loaded.audit() is None and built.audit() is None
    assert loaded.save() == built.save()
    built.close(); loaded.close()


# ---- 3. audit finds what is wrong, and where ---------------------------------------------------------------------------------------------------
def refused(load, blob):
    """the text with which a load with audit refuses `blob`"""
    import distaff_amd as D
    with pytest.raises(D.DistaffError) as e:
        load(blob, audit=True)
    assert e.value.code == D.DST_ERR_ARG
    return e.value.reason


def check_dense_audit_names_the_parent(side):
    """(x + 1) mod p in one element of every node of the 8-leaf tree, either element by turns"""
    tree = side.dense(random_words(8, 700))
    blob = tree.save()
    tree.close()
    for p in range(1, 16):
        changed = bump(blob, HEADER + 32 * (p - 1) + 16 * (p & 1))
        want = max(p >> 1, 1)                                                       # the changed node and its parent mismatch: the parent is nearer the root
        loaded = side.load_dense(changed)                                           # without audit the blob is believed
        assert loaded.audit() == want, p
        assert loaded.nodes(1, 15).tobytes() == changed[HEADER:]      # ... and the audit changes nothing
        loaded.close()
        text = refused(side.load_dense, changed)
        assert [int(x) for x in re.findall(r"node (\d+)", text)] == [want], text


def check_sparse_audit_names_the_parent(side):
    """the same in every stored node of the depth-8 tree: the audit reports the parent of the changed node, (0, 0) for the root"""
    case = sparse_cases()[1]
    tree = build_sparse(side, case)
    blob = tree.save()
    tree.close()
    depth, levels = parse_sparse(blob)
    assert depth == 8 and sum(len(p) for _, p, _ in levels) > 100
    for l, prefixes, first in levels:
        for i, q in enumerate(prefixes):
            changed = bump(blob, first + 32 * i + 16 * (q & 1))
            want = (l - 1, q >> 1) if l else (0, 0)
            loaded = side.load_sparse(changed)
            assert loaded.audit() == want, (l, q)
            loaded.close()
            text = refused(side.load_sparse, changed)
            assert re.search(r"level (\d+) with prefix (\d+)", text) and tuple(int(x) for x in re.search(r"level (\d+) with prefix (\d+)", text).groups()) == want, text


SPREAD_MAX = 1 << 15                    # RESCUE_SPREAD_MAX: an audit of more parents runs the one-lane kernels


def named_sparse(text):
    m = re.search(r"level (\d+) with prefix (\d+)", text)
    assert m, text
    return int(m.group(1)), int(m.group(2))


def check_one_lane_dense_audit(side, maker, thorough):
    """2^16 leaves are 65 535 parents, more than the six-lane form takes.  `maker` builds and saves the tree, `side` loads and audits it.  Of two
    changed nodes the audit reports the parent of the one nearer the root; `thorough` also audits the clean tree, single changes at the last
    parent, a middle parent and a leaf, and has the load with audit name the same node"""
    n = 1 << 16
    assert n - 1 > SPREAD_MAX
    tree = maker.dense(random_words(n, 1616))
    blob = tree.save()
    tree.close()
    at = lambda p, elem=0: HEADER + 32 * (p - 1) + 16 * elem  # noqa: E731
    both = bump(bump(blob, at(50000)), at(30001, 1))
    loaded = side.load_dense(both)
    assert loaded.audit() == 30001 >> 1 and loaded.build_ms == 0                    # 15 000 before 25 000
    assert loaded.nodes(1, 2 * n - 1).tobytes() == both[HEADER:]                    # the audit changes nothing
    loaded.close()
    if not thorough:
        return
    loaded = side.load_dense(blob)
    assert loaded.audit() is None and loaded.audit_ms > 0
    loaded.close()
    for p in (n - 1, 40001, n + 12345):
        changed = bump(blob, at(p, p & 1))
        loaded = side.load_dense(changed)
        assert loaded.audit() == p >> 1, p
        loaded.close()
        assert [int(x) for x in re.findall(r"node (\d+)", refused(side.load_dense, changed))] == [p >> 1]
    assert [int(x) for x in re.findall(r"node (\d+)", refused(side.load_dense, both))] == [30001 >> 1]


def check_one_lane_sparse_audit(side, maker, key_count, thorough):
    """a depth-63 tree of `key_count` random keys stores more than 2^15 parents (asserted from info()), so its audit is the one-lane sparse kernel.
    One element of a leaf, of a node of level 30 and of the root is changed through the blob: the audit reports (level - 1, prefix >> 1), (0, 0)
    for the root, and of two bad nodes the one nearer the root; `thorough` has the single changes, the clean tree and the load with audit too"""
    rng = np.random.default_rng(6363)
    keys = np.unique(rng.integers(0, 1 << 63, size=key_count, dtype=np.uint64))
    tree = maker.sparse(63)
    tree.set(keys, random_words(keys.size, 6364))
    info = tree.info()
    assert info["nodes"] - info["keys"] > SPREAD_MAX
    blob = tree.save()
    tree.close()
    depth, levels = parse_sparse(blob)
    by_level = {l: (prefixes, first) for l, prefixes, first in levels}

    def change(b, l, i):
        prefixes, first = by_level[l]
        return bump(b, first + 32 * i + 16 * (prefixes[i] & 1)), ((l - 1, prefixes[i] >> 1) if l else (0, 0))

    deep, want_deep = change(blob, 63, keys.size // 3)
    both, want_mid = change(deep, 30, len(by_level[30][0]) // 2)
    assert want_mid[0] == 29 and want_deep[0] == 62
    loaded = side.load_sparse(both)
    assert loaded.audit() == want_mid and loaded.info()["last_digests"] == 0      # level 29 before level 62
    loaded.close()
    if not thorough:
        return
    loaded = side.load_sparse(blob)
    assert loaded.audit() is None and loaded.audit_ms > 0
    loaded.close()
    singles = [(deep, want_deep), change(blob, 30, 0), change(blob, 62, len(by_level[62][0]) - 1), change(blob, 1, 0), change(blob, 0, 0)]
    assert singles[-1][1] == (0, 0)
    for changed, want in singles + [(both, want_mid), (change(singles[0][0], 0, 0)[0], (0, 0))]:
        loaded = side.load_sparse(changed)
        assert loaded.audit() == want, want
        loaded.close()
        assert named_sparse(refused(side.load_sparse, changed)) == want


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------------
def with_u32(blob, at, v):
    return blob[:at] + v.to_bytes(4, "little") + blob[at + 4:]


def dense_refusals(blob):
    """(what, bytes, a word of the error text) for a dense blob of 8 leaves"""
    return [("truncated by one byte", blob[:-1], "truncated"), ("one trailing byte", blob + b"\0", "after the end"), ("shorter than a header", blob[:63], "header"),
            ("a wrong magic", b"DSTTREF" + blob[7:], "magic"), ("another version", blob[:7] + b"2" + blob[8:], "version"),
            ("a wrong kind", with_u32(blob, 8, 3), "unknown kind"), ("the other kind", with_u32(blob, 8, 2), "sparse tree"),
            ("depth 0", with_u32(blob, 12, 0), "1 .. 26"), ("depth 27", with_u32(blob, 12, 27), "1 .. 26"),
            ("a depth the counts do not fit", with_u32(blob, 12, 4), "counts disagree"),
            ("an empty leaf in a dense blob", blob[:16] + b"\1" + blob[17:], "no empty leaf"),
            ("an element equal to p", blob[:HEADER + 32 * 4 + 16] + P.to_bytes(16, "little") + blob[HEADER + 32 * 5:], "not below the modulus"),
            ("an element of all ones", blob[:HEADER] + b"\xff" * 16 + blob[HEADER + 16:], "not below the modulus")]


def sparse_refusals(side):
    """(what, bytes, a word of the error text): the header cases on the blob of a depth-4 tree, the shape cases on blobs put together by hand"""
    tree = side.sparse(4, NONZERO_EMPTY)
    tree.set([2, 3, 9], random_pairs(3, 800))
    blob = tree.save()
    levels = [(p, blob[at:at + 32 * len(p)]) for _, p, at in parse_sparse(blob)[1]]   # [2 3 9] [1 4] [0 2] [0 1] [0]
    tree.close()
    assert [p for p, _ in levels] == [[2, 3, 9], [1, 4], [0, 2], [0, 1], [0]] and sparse_blob(4, NONZERO_EMPTY, levels) == blob
    node = blob[-32:]
    shaped = lambda prefixes, **kw: sparse_blob(4, NONZERO_EMPTY, [(p, node * len(p)) for p in prefixes], **kw)  # noqa: E731
    cases = [("truncated by one byte", blob[:-1], "truncated"), ("one trailing byte", blob + b"\0", "after the end"),
             ("a wrong magic", b"dSTTREE" + blob[7:], "magic"), ("a wrong kind", with_u32(blob, 8, 0), "unknown kind"), ("the other kind", with_u32(blob, 8, 1), "dense tree"),
             ("depth 0", with_u32(blob, 12, 0), "1 .. 63"), ("depth 64", with_u32(blob, 12, 64), "1 .. 63"),
             ("an empty leaf that is not below p", blob[:32] + P.to_bytes(16, "little") + blob[48:], "empty leaf"),
             ("an element equal to p", blob[:-16] + P.to_bytes(16, "little"), "node element"),
             ("two equal prefixes", shaped([[2, 2, 9], [1, 4], [0, 2], [0, 1], [0]]), "stored twice"),
             ("a descending pair", shaped([[3, 2, 9], [1, 4], [0, 2], [0, 1], [0]]), "do not ascend"),
             ("a prefix not below 2^l", shaped([[2, 3, 16], [1, 8], [0, 4], [0, 2], [0]]), "not below 2^level"),
             ("a parent level with one prefix too many", shaped([[2, 3, 9], [1, 4, 5], [0, 2], [0, 1], [0]]), "nothing below it"),
             ("a parent level with one prefix too few", shaped([[2, 3, 9], [1], [0], [0], [0]]), "lacks the parent"),
             ("a parent level with another prefix", shaped([[2, 3, 9], [1, 5], [0, 2], [0, 1], [0]]), "lacks the parent"),
             ("two roots", shaped([[2, 3, 9], [1, 4], [0, 2], [0, 1], [0, 0]]), "more than one root"),
             ("a key count that disagrees with the leaf level", shaped([[2, 3, 9], [1, 4], [0, 2], [0, 1], [0]], keys=2), "key count"),
             ("level counts that disagree with the node count", shaped([[2, 3, 9], [1, 4], [0, 2], [0, 1], [0]], nodes=9)[:-40], "level counts"),
             ("keys in a tree without nodes", sparse_blob(4, NONZERO_EMPTY, [([], b"")] * 5, keys=1), "key count"),
             ("more stored nodes than a set admits", blob[:56] + (2 ** 32 - 1).to_bytes(8, "little") + blob[64:], "2^32 - 2")]
    return cases


def check_refusals(side):
    """every malformed blob is DST_ERR_ARG with its own text, with and without audit, and *out is NULL afterwards"""
    import distaff_amd as D
    tree = side.dense(random_words(8, 801))
    dense = dense_refusals(tree.save())
    tree.close()
    rtree_error = lambda: D.lib._rtree_error(side.lib)  # noqa: E731
    probe = side.sparse(1)
    stree_error = lambda: probe._error(None)  # noqa: E731
    for call, error, cases in ((side.lib.dst_rtree_load, rtree_error, dense), (side.lib.dst_stree_load, stree_error, sparse_refusals(side))):
        texts = {}
        for what, blob, word in cases:
            for audit in (0, 1):
                h = ctypes.c_void_p(0xDEAD)
                a = np.frombuffer(blob, dtype=np.uint8)
                r = call(ctypes.c_int(side.device), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.size), ctypes.c_uint32(audit), ctypes.byref(h))
                assert r == D.DST_ERR_ARG and not h.value, what
                assert word in error(), (what, error())
            texts.setdefault(error(), []).append(what)
        assert all(len(v) <= 2 for v in texts.values()), texts                      # a text is shared by the two depths, the two elements at most
        assert call(ctypes.c_int(side.device), None, ctypes.c_size_t(64), ctypes.c_uint32(0), ctypes.byref(h)) == D.DST_ERR_ARG and not h.value
        assert call(ctypes.c_int(side.device), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.size), ctypes.c_uint32(0), None) == D.DST_ERR_ARG
    probe.close()


def check_argument_errors(side):
    """save: the size query, a buffer that is too small, null pointers; audit: null pointers; a closed tree"""
    import distaff_amd as D
    lib = side.lib
    n, bad, level, prefix, buf = ctypes.c_size_t(0), ctypes.c_int64(7), ctypes.c_int32(7), ctypes.c_uint64(7), ctypes.create_string_buffer(4096)
    dense, sparse = side.dense(random_words(4, 802)), build_sparse(side, sparse_cases()[4])
    for tree, save, audit_null in ((dense, lib.dst_rtree_save, lambda h: lib.dst_rtree_audit(h, None, None)),
                                   (sparse, lib.dst_stree_save, lambda h: lib.dst_stree_audit(h, None, ctypes.byref(prefix), None))):
        assert save(tree._h, None, ctypes.c_size_t(0), ctypes.byref(n)) == D.DST_OK and n.value == len(tree.save())
        assert save(tree._h, buf, ctypes.c_size_t(n.value - 1), ctypes.byref(n)) == D.DST_ERR_ARG and n.value == len(tree.save())
        assert save(tree._h, buf, ctypes.c_size_t(4096), None) == D.DST_ERR_ARG and save(None, buf, ctypes.c_size_t(4096), ctypes.byref(n)) == D.DST_ERR_ARG
        assert audit_null(tree._h) == D.DST_ERR_ARG
        assert save(tree._h, buf, ctypes.c_size_t(4096), ctypes.byref(n)) == D.DST_OK and buf.raw[:n.value] == tree.save()
    assert lib.dst_rtree_audit(None, ctypes.byref(bad), None) == D.DST_ERR_ARG and lib.dst_stree_audit(None, ctypes.byref(level), ctypes.byref(prefix), None) == D.DST_ERR_ARG
    assert lib.dst_stree_audit(sparse._h, ctypes.byref(level), ctypes.byref(prefix), None) == D.DST_OK and (level.value, prefix.value) == (-1, 0)
    assert lib.dst_rtree_audit(dense._h, ctypes.byref(bad), None) == D.DST_OK and bad.value == -1
    dense.close(); sparse.close()
    for call in (dense.save, dense.audit, sparse.save, sparse.audit):
        with pytest.raises(D.DistaffError) as e:
            call()
        assert e.value.code == D.DST_ERR_ARG


# ---- the example ---------------------------------------------------------------------------------------------------------------------------------
def example_lines(side, log_leaves):
    """what examples/merkle_restore.c prints, through the binding"""
    n = 1 << log_leaves
    tree = side.dense([(2 * i + 1, 2 * i + 2) for i in range(n)])
    blob, root = tree.save(), tree.root
    tree.close()
    fmt = lambda label, r: "%s %032x %032x" % ((label,) + tuple(r))  # noqa: E731
    changed = bytearray(blob)
    changed[HEADER + 2 * 32] ^= 1
    lines = [fmt("root", root), "saved %d nodes in %d bytes" % (2 * n - 1, len(blob)), fmt("root after the restart", root),
             "the same root: yes, the same path of leaf %d: yes" % (n - 1),
             "load of the changed file with audit: DST_ERR_ARG, tree NULL: " + refused(side.load_dense, bytes(changed)),
             "loaded without audit, then audited: first bad node 1"]
    return lines


def run_example(tmp_path, log_leaves, device):
    import distaff_amd as D
    exe = tmp_path / "merkle_restore"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_restore.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    r = subprocess.run([str(exe), str(log_leaves), str(tmp_path / ("tree%d.bin" % device)), str(device)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()
    return r.stdout.decode().splitlines()


# ---- the host path ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_leaves", DENSE_LOGS)
def test_a_loaded_dense_tree_is_the_saved_tree(log_leaves):
    check_dense_round_trip(host_side(), host_side(), log_leaves)


@pytest.mark.parametrize("case", sparse_cases(), ids=lambda c: "depth%d-%dkeys" % (c[0], len(c[2])))
def test_a_loaded_sparse_tree_is_the_saved_tree(case):
    check_sparse_round_trip(host_side(), host_side(), case)


def test_a_loaded_dense_tree_lives():
    check_loaded_dense_lives(host_side())


@pytest.mark.parametrize("case", sparse_cases(), ids=lambda c: "depth%d-%dkeys" % (c[0], len(c[2])))
def test_a_loaded_sparse_tree_lives(case):
    check_loaded_sparse_lives(host_side(), case)


def test_dense_audit_reports_the_parent_of_every_changed_node():
    check_dense_audit_names_the_parent(host_side())


def test_sparse_audit_reports_the_parent_of_every_changed_node():
    check_sparse_audit_names_the_parent(host_side())


def test_an_empty_sparse_tree_round_trips_to_the_root_of_the_empty_chain(oracle):
    from test_sparse_rescue_tree_host import empty_chain
    side = host_side()
    tree = side.sparse(63, NONZERO_EMPTY)
    blob = tree.save()
    assert len(blob) == HEADER + 8 * 64 and blob[48:64] == bytes(16)
    loaded = side.load_sparse(blob, audit=True)
    assert loaded.root == tree.root == empty_chain(oracle, NONZERO_EMPTY, 63)[0] and loaded.audit() is None and loaded.info()["nodes"] == 0
    loaded.set([5], [(1, 2)])
    tree.set([5], [(1, 2)])
    assert loaded.root == tree.root
    tree.close(); loaded.close()


def test_malformed_blobs_are_refused_each_with_its_own_text():
    check_refusals(host_side())


def test_argument_errors_never_abort():
    check_argument_errors(host_side())


def test_blob_parser_against_a_model_and_malformed_inputs_under_sanitizers(tmp_path):
    """tests/sparse_host/tree_blob_check.cpp drives host/tree_blob.h alone -- blobs of random key sets made by a std::set model must parse, every
    malformed variant must be refused with its own text, and random damage must never read out of bounds -- built with
    -fsanitize=address,undefined and run as a program: exit status 0, nothing on stderr"""
    exe = str(tmp_path / "tree_blob_check")
    subprocess.check_call(["g++", "-std=c++17", "-w", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sparse_host", "tree_blob_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    assert b"blobs ok" in r.stdout


def test_c_example_restores_a_tree_from_a_file_and_refuses_a_changed_one(tmp_path):
    """examples/merkle_restore.c compiles as C99 against include/distaff_hip.h and the product library and runs on the host"""
    lines = run_example(tmp_path, 6, -1)
    assert lines == example_lines(host_side(), 6)
    assert "audit: node 1 " in lines[4]


def test_the_six_calls_are_in_the_package_the_header_and_both_libraries():
    import distaff_amd as D
    names = ["dst_rtree_save", "dst_rtree_load", "dst_rtree_audit", "dst_stree_save", "dst_stree_load", "dst_stree_audit"]
    assert set(names) <= set(D.EXPORTS)
    header = open(os.path.join(ROOT, "include", "distaff_hip.h")).read()
    for name in names:
        assert re.search(r"DST_API int %s\(" % name, header), name
        assert hasattr(_product(), name) and hasattr(ctypes.CDLL(D.HOOKS_LIB), name), name
    assert all(hasattr(D.RescueTree, f) and hasattr(D.SparseRescueTree, f) for f in ("save", "load", "audit"))
