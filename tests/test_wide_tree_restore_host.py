"""Save and load of wide-key sparse Rescue trees (dst_wtree_save / dst_wtree_load, blob kind 3) on the host path of the PRODUCT library.  No GPU.
The yardsticks: the tree that was saved (every level, the root, batch proofs), the layout as include/distaff_hip.h states it, restated here with
struct, and the refusals of the narrow loader, each with its own text and once more in a high half only.  Also here: the helpers the emulated
and the GPU tests share."""
import os
import struct
import subprocess

import pytest

from test_rescue_tree_host import _product
from test_sparse_rescue_tree_host import NONZERO_EMPTY, host_sparse, random_pairs
from test_wide_multiproof_host import ROOT, asked, case_keys, sets_of
from test_wide_sparse_rescue_tree_host import BOUNDARY_SETS, host_wide, int_levels

HEADER = 64


def blob_of(depth, empty, levels, kind=3, keys=None, nodes=None):
    """the blob of include/distaff_hip.h from (prefixes as ints, node bytes) per level, the leaf level first"""
    import distaff_amd as D
    total = sum(len(p) for p, _ in levels)
    e = D.ints_to_arr(list(empty)).tobytes()
    out = b"DSTTREE1" + struct.pack("<II", kind, depth) + e + struct.pack("<QQ", len(levels[0][0]) if keys is None else keys, total if nodes is None else nodes)
    out += b"".join(struct.pack("<Q", len(p)) for p, _ in levels)
    out += b"".join(int(q).to_bytes(16, "little") for p, _ in levels for q in p)
    return out + b"".join(v for _, v in levels)


def levels_of(tree):
    """(prefixes, node bytes) per level of a tree, the leaf level first"""
    out = []
    for l in range(tree.depth, -1, -1):
        prefixes, nodes = tree.level(l)
        import distaff_amd as D
        out.append((D.arr_to_ints(prefixes), nodes.tobytes()))
    return out


def check_round_trip(D, make, load, depth, name):
    seed = 2000 * depth + BOUNDARY_SETS.index(name)
    keys = case_keys(depth, name, seed)
    tree = make(depth, NONZERO_EMPTY)
    tree.set(keys, random_pairs(len(keys), seed))
    blob = tree.to_blob()
    assert len(blob) == HEADER + 8 * (depth + 1) + 48 * tree.info()["nodes"] and blob == blob_of(depth, NONZERO_EMPTY, levels_of(tree))
    for audit in (False, True):
        loaded = load(blob, audit)
        assert int_levels(loaded) == int_levels(tree) and loaded.root == tree.root and loaded.audit() is None and loaded.info()["last_digests"] == 0
        assert loaded.to_blob() == blob
        loaded.close()
    loaded = load(blob, False)                                                      # the loaded tree lives: set, apply, remove, batch_proof
    ask = asked(depth, keys, seed)
    assert loaded.batch_proof(ask) == tree.batch_proof(ask) and loaded.batch_proof(ask, compact=False) == tree.batch_proof(ask, compact=False)
    fresh = random_pairs(len(ask), seed + 1)
    for t in (loaded, tree):
        t.set(ask[:3], fresh[:3])
    batch = ask[-2:] + ask[:1]                                                      # ordered, with a repeat where there are fewer than three keys
    assert loaded.apply(batch, random_pairs(len(batch), seed + 2)) == tree.apply(batch, random_pairs(len(batch), seed + 2))
    assert loaded.remove(keys[:2]) == tree.remove(keys[:2])
    assert int_levels(loaded) == int_levels(tree) and loaded.root == tree.root and loaded.audit() is None
    loaded.close(); tree.close()


def host_load(blob, audit=False):
    import distaff_amd as D
    return D.WideSparseRescueTree.from_blob(blob, device=-1, audit=audit, lib=_product())


@pytest.mark.parametrize("depth,name", [(d, n) for d in (1, 64, 65, 127) for n in sets_of(d)])
def test_round_trip_of_the_boundary_sets(depth, name):
    import distaff_amd as D
    check_round_trip(D, host_wide, host_load, depth, name)


def test_an_empty_tree_round_trips():
    tree = host_wide(127, NONZERO_EMPTY)
    blob = tree.to_blob()
    assert len(blob) == HEADER + 8 * 128 and blob[48:64] == bytes(16) and blob[8:12] == struct.pack("<I", 3)
    loaded = host_load(blob, audit=True)
    assert loaded.root == tree.root and loaded.info()["nodes"] == 0
    loaded.set([1 << 100], [(1, 2)]); tree.set([1 << 100], [(1, 2)])
    assert loaded.root == tree.root
    loaded.close(); tree.close()


def refusal_cases(D):
    """(what, bytes, a word of the error text): every corruption the narrow loader's tests make, and one that is wrong only in a high half"""
    depth = 70
    tree = host_wide(depth, NONZERO_EMPTY)
    hi = 1 << 64
    keys = [3, hi + 3, hi + 2, 5 * hi + 1]
    tree.set(keys, random_pairs(4, 1))
    good = tree.to_blob()
    levels = levels_of(tree)
    tree.close()

    def with_level(k, prefixes, **kw):
        changed = list(levels)
        changed[k] = (prefixes, levels[k][1][:32] * len(prefixes))
        return blob_of(depth, NONZERO_EMPTY, changed, **kw)

    def with_u32(blob, at, v):
        return blob[:at] + struct.pack("<I", v) + blob[at + 4:]
    leaf = levels[0][0]                                                             # [3, 2^64 + 2, 2^64 + 3, 5 * 2^64 + 1]
    p = (1 << 128) - 45 * (1 << 40) + 1
    return good, [
        ("truncated by one byte", good[:-1], "truncated"), ("one trailing byte", good + b"\0", "after the end"), ("shorter than a header", good[:63], "header"),
        ("a wrong magic", b"dSTTREE" + good[7:], "magic"), ("another version", good[:7] + b"2" + good[8:], "version"), ("a wrong kind", with_u32(good, 8, 0), "unknown kind"),
        ("a dense blob", with_u32(good, 8, 1), "dense tree"), ("a narrow sparse blob", with_u32(good, 8, 2), "8-byte keys"),
        ("depth 0", with_u32(good, 12, 0), "1 .. 127"), ("depth 128", with_u32(good, 12, 128), "1 .. 127"),
        ("an empty leaf not below p", good[:16] + p.to_bytes(16, "little") + good[32:], "empty leaf"),
        ("a node not below p", good[:-16] + p.to_bytes(16, "little"), "node element"),
        ("a key count that disagrees", blob_of(depth, NONZERO_EMPTY, levels, keys=3), "key count"),
        ("a node count that disagrees", blob_of(depth, NONZERO_EMPTY, levels, nodes=sum(len(q) for q, _ in levels) - 1)[:-48], "level counts"),
        ("two roots", blob_of(depth, NONZERO_EMPTY, levels[:-1] + [([0, 1], levels[-1][1] * 2)]), "more than one root"),
        ("leaves that do not ascend", with_level(0, [leaf[1], leaf[0], leaf[2], leaf[3]]), "do not ascend"),
        ("a leaf stored twice", with_level(0, [leaf[0], leaf[1], leaf[1], leaf[3]]), "stored twice"),
        ("leaves that ascend in the low half only", with_level(0, [leaf[0], leaf[3], leaf[1], leaf[2]]), "do not ascend"),
        ("a prefix past 2^level, in the high half only", with_level(0, leaf[:3] + [leaf[3] + (1 << 70)]), "below 2^level"),
        ("a level that lacks a parent", with_level(1, levels[1][0][:-1]), "lacks the parent"),
        ("a level with a node too many", with_level(1, levels[1][0] + [levels[1][0][-1] + 1]), "nothing below it"),
        ("a parent wrong in the high half only", with_level(1, levels[1][0][:-1] + [levels[1][0][-1] ^ (1 << 64)]), "lacks the parent"),
    ]


def check_refusals(D, load):
    good, cases = refusal_cases(D)
    load(good, True).close()
    for what, blob, text in cases:
        with pytest.raises(D.DistaffError) as e:
            load(blob, False)
        assert e.value.code == D.DST_ERR_ARG and text in str(e.value), (what, str(e.value))


def test_malformed_blobs_are_refused_each_with_its_own_text():
    import distaff_amd as D
    check_refusals(D, host_load)


def test_each_loader_refuses_the_other_width():
    import distaff_amd as D
    narrow = host_sparse(20, NONZERO_EMPTY)
    narrow.set([5, 6], [(1, 2), (3, 4)])
    wide = host_wide(20, NONZERO_EMPTY)
    wide.set([5, 6], [(1, 2), (3, 4)])
    assert narrow.root == wide.root
    with pytest.raises(D.DistaffError) as e:
        host_load(narrow.save())
    assert e.value.code == D.DST_ERR_ARG and "8-byte keys" in str(e.value)
    with pytest.raises(D.DistaffError) as e:
        D.SparseRescueTree.load(wide.to_blob(), device=-1, lib=_product())
    assert e.value.code == D.DST_ERR_ARG and "unknown kind" in str(e.value)
    narrow.close(); wide.close()


def check_audit_on_load_names_the_node(D, make, load):
    tree = make(127, NONZERO_EMPTY)
    keys = case_keys(127, "random-200", 9)
    tree.set(keys, random_pairs(len(keys), 9))
    blob = bytearray(tree.to_blob())
    prefixes, _ = tree.level(90)
    prefix = D.arr_to_ints(prefixes)[1]
    at = len(blob) - 32 * sum(len(tree.level(l)[0]) for l in range(90)) - 32 * (len(prefixes) - 1)      # node 1 of level 90
    blob[at] ^= 1
    load(bytes(blob), False).close()                                                # believed without the audit
    with pytest.raises(D.DistaffError) as e:
        load(bytes(blob), True)
    assert e.value.code == D.DST_ERR_ARG and "audit: the node of level 89 with prefix %d " % (prefix >> 1) in str(e.value)
    tree.close()


def test_audit_on_load_names_a_node_changed_in_the_blob():
    import distaff_amd as D
    check_audit_on_load_names_the_node(D, host_wide, host_load)


def run_batch_example(tmp_path, k, device):
    import distaff_amd as D
    exe = tmp_path / "merkle_wide_batch"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "merkle_wide_batch.c"),
                           D.PRODUCT_LIB, "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    r = subprocess.run([str(exe), str(k), str(tmp_path / "tree.blob"), str(device)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()
    return r.stdout.decode().splitlines(), (tmp_path / "tree.blob").read_bytes()


def batch_example_lines(O, k):
    """what examples/merkle_wide_batch.c prints for k keys and the file it writes, from the oracle's digest (the keys) and the host tree"""
    import distaff_amd as D
    keys = [O.hasher_digest([i, 1, 2, 3])[0] & ((1 << 127) - 1) for i in range(k + 3)]
    tree = host_wide(127)
    tree.set(keys[:k], [(2 * i + 1, 2 * i + 2) for i in range(k)])
    ask = [keys[0], keys[k // 2], keys[k - 1]] + keys[k:]
    leaves, nodes, bits = tree.batch_proof(ask)
    assert leaves == [(1, 2), (2 * (k // 2) + 1, 2 * (k // 2) + 2), (2 * k - 1, 2 * k)] + [(0, 0)] * 3
    M, plain = D.multiproof_size_wide(128, ask, lib=_product())
    s = {}
    assert D.multiproof_root_wide(128, ask, leaves, nodes, bits, D.empty_nodes(128, lib=_product()), device=-1, lib=_product(), stats=s) == tree.root
    h = lambda v: "%032x" % v  # noqa: E731
    blob = tree.to_blob()
    lines = ["root %s %s" % (h(tree.root[0]), h(tree.root[1])), "%d keys of 127 bits in %d stored nodes" % (k, tree.info()["nodes"]),
             "6 keys asked, 3 members and 3 absent: %d supplied nodes, %d of them stored; the compact proof has %d bytes, the plain one %d, six paths %d"
             % (M, len(nodes), 32 * 6 + 32 * len(nodes) + len(bits), 32 * 6 + 32 * M, 32 * 6 * 128),
             "verified against the root alone with %d digests; the plain proof takes %d, six paths %d; a changed leaf is rejected" % (s["digests"], plain, 6 * 127),
             "saved %d bytes, loaded with audit: root %s %s, the same proof" % (len(blob), h(tree.root[0]), h(tree.root[1]))]
    tree.close()
    return lines, blob


def test_c_example_proves_a_batch_saves_the_tree_and_proves_it_again_from_the_file(oracle, tmp_path):
    """examples/merkle_wide_batch.c compiles as C99 against include/distaff_hip.h and the product library and runs on the host"""
    assert run_batch_example(tmp_path, 9, -1) == batch_example_lines(oracle, 9)


def test_blob_parser_for_wide_prefixes_against_a_model_under_sanitizers(tmp_path):
    """tests/sparse_host/tree_blob_wide_check.cpp drives the kind-3 parser of host/tree_blob.h alone, built with -fsanitize=address,undefined and
    run as a program: exit status 0, nothing on stderr"""
    exe = str(tmp_path / "tree_blob_wide_check")
    subprocess.check_call(["g++", "-std=c++17", "-w", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sparse_host", "tree_blob_wide_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    assert b"blobs ok" in r.stdout
