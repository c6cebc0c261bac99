#!/usr/bin/env python3
"""Device time of Rescue Merkle trees (dst_rtree_build: events around the level launches), the host path on one core, and the bound the
device's own modular-multiplication rate sets.
    python tools/rescue_tree_time.py [--host-log 12] [--lib path/to/another/build.so] [log_leaves ...]        (default 12 16 20)
    python tools/rescue_tree_time.py --update        updates in place and batched openings on the 2^20 tree instead (dst_rtree_update_ms)
    python tools/rescue_tree_time.py --sparse        sparse trees of depth 63 instead (dst_stree_set, dst_stree_paths), beside a dense 2^20 build
    python tools/rescue_tree_time.py --wide          wide-key sparse trees of depth 127 (dst_wtree_set beside dst_stree_set at depth 63 with as many keys, dst_wtree_paths,
                                                     dst_wtree_apply, dst_rescue_verify_paths_w)
    python tools/rescue_tree_time.py --wide-batch    compact and plain multiproofs of the depth-127 tree of 2^20 keys beside the path check (bytes, digests, levels, device
                                                     time), and dst_wtree_save / dst_wtree_load beside the set that builds the tree
    python tools/rescue_tree_time.py --remove        deletion on the depth-63 tree of 2^20 keys that --sparse builds (dst_stree_remove beside a dst_stree_set of the
                                                     same keys, dst_stree_compact after an apply of empties, dst_stree_get beside dst_stree_paths)
    python tools/rescue_tree_time.py --sequence      ordered writes with a witness each (dst_rtree_apply on the 2^20 tree, dst_stree_apply on a depth-63 tree
                                                     of 2^20 keys), beside the loop of single-leaf updates and single paths they replace
    python tools/rescue_tree_time.py --verify        checking the witnesses of those ordered writes (dst_rescue_verify_writes, one launch) beside the apply that
                                                     made them, the same check on the host for 256 writes, and dst_rescue_verify_paths of 4 096 paths
    python tools/rescue_tree_time.py --refresh       following those writes with held paths (dst_rescue_refresh_paths: the chain launch that also stores its nodes, then
                                                     a gather) beside dst_rescue_verify_writes on the same batches, and beside asking the tree for the paths again
    python tools/rescue_tree_time.py --multiproof    compressed batch openings: bytes, digests and the device time of dst_rescue_multiproof_root beside
                                                     dst_rescue_verify_paths on the full paths of the same leaves (K = 256, 4 096, 65 536; both trees above)
    python tools/rescue_tree_time.py --restore       save, restore, audit: dst_rtree_audit beside dst_rtree_build_ms of the dense 2^20 tree, dst_stree_audit beside the
                                                     one dst_stree_set that builds the depth-63 tree of 2^20 keys, the wall time of a load beside that of the rebuild
One digest is counted as 9 180 field multiplications, the reference's own count per hasher::digest: ten rounds of 6 x 2 for the cubes, 6 x 139
for x^INV_ALPHA by the addition chain (127 squarings + 12 multiplications) and 2 x 36 for the two MDS products."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distaff_amd as D

MULS_PER_DIGEST = 10 * (6 * 2 + 6 * 139 + 2 * 36)

ap = argparse.ArgumentParser()
ap.add_argument("--host-log", type=int, default=12, help="size of the host-path tree (one core); 0: skip")
ap.add_argument("--lib", default=None, help="another build of the library (a different RESCUE_SPREAD_MAX)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--update", action="store_true", help="time dst_rtree_update (k = 1, 256, 65 536 leaves) and dst_rtree_paths on the 2^20 tree instead of builds")
ap.add_argument("--sparse", action="store_true", help="time dst_stree_set (2^12, 2^16, 2^20 keys into an empty depth-63 tree; 1, 256, 65 536 keys into the 2^20-key tree) and dst_stree_paths")
ap.add_argument("--remove", action="store_true", help="time dst_stree_remove of 1, 256, 65 536 stored keys of the 2^20-key depth-63 tree, each just after a dst_stree_set of the same keys; dst_stree_compact after an apply of 65 536 empties; dst_stree_get of 4 096 keys beside dst_stree_paths")
ap.add_argument("--sequence", action="store_true", help="time dst_rtree_apply / dst_stree_apply (1, 256, 4 096, 65 536 ordered writes) and, for 256, the loop of update + path calls")
ap.add_argument("--verify", action="store_true", help="time dst_rescue_verify_writes on the witnesses of dst_rtree_apply / dst_stree_apply (256, 4 096, 65 536 writes), on the host for 256, and dst_rescue_verify_paths of 4 096 paths")
ap.add_argument("--refresh", action="store_true", help="time dst_rescue_refresh_paths (256 and 4 096 held paths across 256, 4 096, 65 536 ordered writes) beside dst_rescue_verify_writes on the same batches: dense 2^20, sparse depth 63 with 2^20 keys, wide depth 127 with 2^16 keys")
ap.add_argument("--multiproof", action="store_true", help="time dst_rescue_multiproof_root of 256, 4 096, 65 536 distinct leaves of the dense 2^20 tree and of the depth-63 tree of 2^20 keys beside dst_rescue_verify_paths on the full paths of the same leaves; bytes and digests of both")
ap.add_argument("--restore", action="store_true", help="time dst_rtree_audit / dst_stree_audit (one launch each) beside the builds of the same trees (dense 2^20; depth 63 with 2^20 keys), and dst_rtree_load / dst_stree_load of their saved forms beside the wall time of the rebuild")
ap.add_argument("--wide", action="store_true", help="time the wide-key sparse trees: create + one dst_wtree_set of 2^16 and 2^20 random keys at depth 127 beside dst_stree_set of as many keys at depth 63, dst_wtree_paths of 2^16 keys, dst_wtree_apply of 2^12 writes, dst_rescue_verify_paths_w of 2^16 paths of 128 nodes")
ap.add_argument("--wide-batch", action="store_true", help="compact and plain multiproofs (dst_wtree_multiproof, dst_rescue_verify_multiproof_w) of 256 and 4 096 keys -- members, absent, half and half -- of the depth-127 tree of 2^20 random keys beside dst_rescue_verify_paths_w on the full paths: bytes, digests, levels launched, device ms; dst_wtree_save / dst_wtree_load beside the set that builds the tree")
ap.add_argument("sizes", nargs="*", type=int)
args = ap.parse_args()
lib = D.lib._open(os.path.abspath(args.lib)) if args.lib else None       # through the binding: one HIP runtime per process


def leaves(log_leaves):
    a = np.random.default_rng(log_leaves).integers(0, 1 << 64, size=(1 << log_leaves, 2, 2), dtype=np.uint64)
    a[..., 1] >>= np.uint64(1)                      # below p
    return a


try:                                                # what was measured: the commit, the digest of the kernel sources, the code objects (build()'s record)
    import json
    info = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distaff_amd", "_build_info.json")))
    print("git HEAD %s, kernel sources %s%s" % (info.get("git_head"), info.get("csrc_sha16"), ", trees built by %s" % args.lib if args.lib else ""))
    for name, k in sorted(info["kernels"].items()):
        if "rescue" in name and not args.lib:
            print("   %s: %d bytes of code, %s" % (name.split("(")[0], k["code_bytes"], ", ".join("%s %s" % (key, k[key]) for key in sorted(k) if key != "code_bytes")))
except (OSError, KeyError, ValueError):
    print("no distaff_amd/_build_info.json: run __graft_entry__.build()")
cal = D.Calibration()
cal.bench_mulmod()                                  # warm-up: clocks, code
lanes, iters = 1 << 20, 1024
mul_ms = min(cal.bench_mulmod(lanes, iters) for _ in range(5))
cal.close()
mul_rate = lanes * iters * 4 / (mul_ms * 1e-3)                       # four multiplication chains per lane and iteration (bench.py counts the same way)
bound = mul_rate / MULS_PER_DIGEST
print("dst_bench_mulmod: %.3e modular multiplications/s (%d lanes x %d iterations x 4 chains in %.3f ms) -> at most %.3e digests/s at %d multiplications per digest"
      % (mul_rate, lanes, iters, mul_ms, bound, MULS_PER_DIGEST))
if args.update:
    import ctypes
    UPDATE_SEED, log_leaves = 2020, 20
    a = leaves(log_leaves)
    D.RescueTree(a, device=0, lib=lib).close()      # warm-up
    t = D.RescueTree(a, device=0, lib=lib)
    print("2^%d leaves: built in %.3f ms on the device (dst_rtree_build_ms of the tree the updates below run on)" % (log_leaves, t.build_ms))
    rng = np.random.default_rng(UPDATE_SEED)
    for k in (1, 256, 65536):
        ms = []
        for _ in range(1 + args.runs):              # the first is the warm-up: stream, staging buffer, code
            idx = rng.permutation(1 << log_leaves)[:k].astype(np.uint64)
            new = rng.integers(0, 1 << 64, size=(k, 2, 2), dtype=np.uint64)
            new[..., 1] >>= np.uint64(1)
            t.update(idx, new)
            ms.append(t.update_ms)
        ms = ms[1:]
        root = t.root
        print("update of %d leaves: %.3f ms on the device (min of %d after one warm-up; all: %s), %.1f x faster than the build, root %032x %032x"
              % (k, min(ms), args.runs, " ".join("%.3f" % v for v in ms), t.build_ms / min(ms), root[0], root[1]))
    count, n = 4096, log_leaves + 1
    idx = rng.integers(0, 1 << log_leaves, size=count).astype(np.uint64)
    t.paths(idx[:16])                               # warm-up
    t0 = time.perf_counter(); many = t.paths(idx); s_many = time.perf_counter() - t0
    t0 = time.perf_counter(); single = [t.path(int(i)) for i in idx]; s_single = time.perf_counter() - t0
    assert many == single
    print("paths() of %d indices: %.2f ms wall; %d calls of path(): %.2f ms wall (both with the binding's conversion to Python ints)" % (count, s_many * 1e3, count, s_single * 1e3))
    out = np.zeros((count * n, 2, 2), dtype=np.uint64)   # the C calls alone
    h, L = t._h, t.lib
    t0 = time.perf_counter(); r = L.dst_rtree_paths(h, idx.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(count), out.ctypes.data_as(ctypes.c_void_p)); c_many = time.perf_counter() - t0
    one = np.zeros((n, 2, 2), dtype=np.uint64)
    po = one.ctypes.data_as(ctypes.c_void_p)
    t0 = time.perf_counter()
    for i in idx.tolist():
        r |= L.dst_rtree_path(h, ctypes.c_uint64(i), po)
    c_single = time.perf_counter() - t0
    assert r == 0 and np.array_equal(out[-n:], one)
    print("dst_rtree_paths of %d indices: %.3f ms wall; %d calls of dst_rtree_path: %.2f ms wall (ctypes, no conversion): %.0f x" % (count, c_many * 1e3, count, c_single * 1e3, c_single / c_many))
    t.close()
    sys.exit(0)
def wide_keys(count, seed, bits=127):
    """-> distinct random keys as words [count, 2] (low half first), shuffled, and as many leaves"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 64, size=(count + count // 8 + 16, 2), dtype=np.uint64)
    k[:, 1] >>= np.uint64(128 - bits)
    k = np.unique(k, axis=0)
    rng.shuffle(k)
    v = rng.integers(0, 1 << 64, size=(count, 2, 2), dtype=np.uint64)
    v[..., 1] >>= np.uint64(1)
    return np.ascontiguousarray(k[:count]), v


if args.wide_batch:
    # compact and plain multiproofs of the depth-127 tree of 2^20 random keys (the keys of --wide), the path check they replace, and save / load
    depth, n, runs = 127, 128, args.runs
    k, v = wide_keys(1 << 20, 320)

    def timed(fn, repeat):
        """-> (the last result, the least wall ms of `repeat` calls after one warm-up)"""
        out, wall = fn(), []
        for _ in range(repeat):
            t0 = time.perf_counter()
            out = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
        return out, min(wall)

    t0 = time.perf_counter()
    tree = D.WideSparseRescueTree(depth, device=0, lib=lib)
    tree.set(k, v)
    set_wall = (time.perf_counter() - t0) * 1e3
    i = tree.info()
    print("dst_wtree_set of 2^20 random keys into an empty depth-127 tree (one run): %.1f ms on the device, %.1f ms wall, %d digests, %d stored nodes = %.1f per key"
          % (i["last_device_ms"], set_wall, i["last_digests"], i["nodes"], i["nodes"] / len(k)))
    root = tree.root
    table = D.empty_nodes(n, lib=lib, words=True)
    absent_all, _ = wide_keys(1 << 12, 9)
    rng = np.random.default_rng(8)
    members_all = np.ascontiguousarray(k[rng.permutation(len(k))[:1 << 12]])
    outcome = {}
    for count in (256, 4096):
        for mix, ask in (("members only", members_all[:count]), ("absent only", absent_all[:count]),
                         ("half and half", np.concatenate([members_all[:count // 2], absent_all[:count // 2]]))):
            ask = np.ascontiguousarray(ask)
            (leaves_c, nodes_c, bits), wall_c = timed(lambda: tree.batch_proof(ask, words=True), runs)
            (leaves_p, nodes_p, _), wall_p = timed(lambda: tree.batch_proof(ask, compact=False, words=True), runs)
            words, wall_paths = timed(lambda: tree.paths_words(ask), runs)
            bytes_c, bytes_p = leaves_c.nbytes + nodes_c.nbytes + len(bits), leaves_p.nbytes + nodes_p.nbytes

            def device_ms(fn):
                s, ms = {}, []
                fn(s)                                   # warm-up
                for _ in range(runs):
                    assert fn(s) in (True, (-1, D.DST_PATH_OK))
                    ms.append(s["device_ms"])
                return min(ms), dict(s)
            ms_c, s_c = device_ms(lambda s: D.verify_multiproof_wide(root, n, ask, leaves_c, nodes_c, bits, table, device=0, lib=lib, stats=s))
            ms_p, s_p = device_ms(lambda s: D.verify_multiproof_wide(root, n, ask, leaves_p, nodes_p, device=0, lib=lib, stats=s))
            ms_v, _ = device_ms(lambda s: D.verify_paths_wide(root, words, ask, leaves=leaves_p, device=0, lib=lib, stats=s))
            d = {}
            D.multiproof_root_wide(n, ask, leaves_c, nodes_c, bits, table, device=-1 if count == 256 else 0, lib=lib, stats=d)
            _, plain_digests = D.multiproof_size_wide(n, ask, lib=lib)
            outcome[(count, mix)] = (ms_c, ms_v)
            print("%d keys, %s: plain %d bytes (%d nodes), compact %d bytes (%d nodes + %d bytes of bits), paths %d bytes; digests compact %d (%.1f per key) in %d levels launched, plain %d in %d; "
                  "device ms: verify_multiproof_wide compact %.3f, plain %.3f, verify_paths_wide on the full paths %.3f (each the min of %d after one warm-up); "
                  "wall ms: batch_proof compact %.2f, plain %.2f, paths %.2f"
                  % (count, mix, bytes_p, len(nodes_p), bytes_c, len(nodes_c), len(bits), words.nbytes, d["digests"], d["digests"] / count, s_c["levels"], plain_digests, s_p["levels"],
                     ms_c, ms_p, ms_v, runs, wall_c, wall_p, wall_paths))
    for count in (256, 4096):
        ms_c, ms_v = outcome[(count, "absent only")]
        print("the condition, %d absent keys: compact check %.3f ms %s verify_paths_wide %.3f ms on the device (factor %.2f)" % (count, ms_c, "<" if ms_c < ms_v else ">=", ms_v, ms_v / ms_c))
    blob, save_wall = timed(tree.to_blob, 3)
    print("to_blob: %d bytes, %.1f ms wall (min of 3 after one warm-up; one copy of the nodes from the device)" % (len(blob), save_wall))
    for audit in (False, True):
        wall, audit_ms = [], []
        for _ in range(1 + 3):
            t0 = time.perf_counter()
            loaded = D.WideSparseRescueTree.from_blob(blob, device=0, audit=audit, lib=lib)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert loaded.root == root
            if audit:
                loaded.audit()
                audit_ms.append(loaded.audit_ms)
            loaded.close()
        print("from_blob %s audit: %.1f ms wall (min of 3 after one warm-up)%s; the set that builds the tree: %.1f ms on the device, %.1f ms wall"
              % ("with" if audit else "without", min(wall[1:]), ", dst_wtree_audit alone %.1f ms on the device" % min(audit_ms[1:]) if audit else "", i["last_device_ms"], set_wall))
    tree.close()
    sys.exit(0)
if args.wide:
    def one_set(make, depth, k, v, runs):
        """create + one set, `runs` times after one warm-up -> (the last tree, device ms of each run, the least wall time in ms)"""
        ms, wall, t = [], [], None
        for _ in range(1 + runs):
            if t is not None:
                t.close()
            t0 = time.perf_counter()
            t = make(depth, device=0, lib=lib)
            t.set(k, v)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(t.info()["last_device_ms"])
        return t, ms[1:], min(wall[1:])

    big = None
    for log_keys in (16, 20):
        count, runs = 1 << log_keys, (args.runs if log_keys < 20 else 1)
        k, v = wide_keys(count, 300 + log_keys)
        narrow_k = np.unique(np.random.default_rng(400 + log_keys).integers(0, 1 << 63, size=count + count // 8, dtype=np.uint64))
        np.random.default_rng(5).shuffle(narrow_k)
        for name, make, depth, keys, per_node, head in (("dst_stree_set", D.SparseRescueTree, 63, narrow_k[:count], 40, 3072), ("dst_wtree_set", D.WideSparseRescueTree, 127, k, 48, 6144)):
            t, ms, wall = one_set(make, depth, keys, v, runs)
            i = t.info()
            within = sum(1 for l in range(depth) if min(1 << l, count) <= (1 << 15))
            print("%s of 2^%d random keys into an empty depth-%d tree: %.3f ms on the device (min of %d after one warm-up; all: %s), %d digests, %.3e digests/s over the level launches; "
                  "%d stored nodes = %.1f per key, %.1f MiB on the device; %d of %d levels within RESCUE_SPREAD_MAX; %.1f ms wall with the plan and the uploads"
                  % (name, log_keys, depth, min(ms), len(ms), " ".join("%.3f" % x for x in ms), i["last_digests"], i["last_digests"] / (min(ms) * 1e-3), i["nodes"], i["nodes"] / count,
                     (per_node * i["nodes"] + head) / 2 ** 20, within, depth, wall))
            if log_keys == 16 and depth == 127:
                big = t
            else:
                t.close()
    rng = np.random.default_rng(8)
    stored = big.level(127)[0]
    absent, _ = wide_keys(1 << 15, 9)
    ask = np.ascontiguousarray(np.concatenate([stored[rng.integers(0, len(stored), size=1 << 15)], absent]))
    big.paths_words(ask[:16])                       # warm-up
    t0 = time.perf_counter(); words = big.paths_words(ask); s_paths = time.perf_counter() - t0
    print("dst_wtree_paths of 2^16 keys (half stored, half absent) on the 2^16-key depth-127 tree: %.3f ms wall (128 nodes of 128 searched levels each, %.0f MiB back)" % (s_paths * 1e3, words.nbytes / 2 ** 20))
    root = big.root
    stats = {}
    D.verify_paths_wide(root, words[:16], ask[:16], device=0, lib=lib)      # warm-up
    ms = []
    for _ in range(args.runs):
        assert D.verify_paths_wide(root, words, ask, device=0, lib=lib, stats=stats) == (-1, D.DST_PATH_OK)
        ms.append(stats["device_ms"])
    chains = len(ask) * 127
    print("dst_rescue_verify_paths_w of 2^16 paths of 128 nodes: %.3f ms on the device (min of %d; all: %s), %d digests, %.3e digests/s"
          % (min(ms), len(ms), " ".join("%.3f" % x for x in ms), chains, chains / (min(ms) * 1e-3)))
    ms, wall = [], []
    for run in range(1 + args.runs):
        fresh, v = wide_keys(1 << 11, 50 + run)
        ops = np.ascontiguousarray(np.concatenate([stored[rng.integers(0, len(stored), size=1 << 11)], fresh]))
        v2 = np.concatenate([v, v])
        import ctypes                               # the C call: the binding's conversion to Python ints is not what is timed
        paths = np.zeros((len(ops) * 128, 2, 2), dtype=np.uint64)
        roots = np.zeros((len(ops), 2, 2), dtype=np.uint64)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        t0 = time.perf_counter()
        big._check(big.lib.dst_wtree_apply(big._h, vp(ops), vp(v2), ctypes.c_size_t(len(ops)), vp(paths), vp(roots)))
        wall.append((time.perf_counter() - t0) * 1e3)
        i = big.info()
        ms.append(i["last_device_ms"])
    ms, wall = ms[1:], wall[1:]
    print("dst_wtree_apply of 2^12 ordered writes (half to stored keys, half to new ones) with paths and roots: %.3f ms on the device (min of %d after one warm-up; all: %s), %d digests, %.3e digests/s; %.1f ms wall"
          % (min(ms), len(ms), " ".join("%.3f" % x for x in ms), i["last_digests"], i["last_digests"] / (min(ms) * 1e-3), min(wall)))
    big.close()
    sys.exit(0)
if args.sparse or args.remove or args.restore:
    DEPTH = 63

    def keys_and_leaves(count, seed):
        rng = np.random.default_rng(seed)
        k = np.unique(rng.integers(0, 1 << DEPTH, size=count + count // 8 + 16, dtype=np.uint64))      # distinct; sorted, so shuffled below
        rng.shuffle(k)
        v = rng.integers(0, 1 << 64, size=(count, 2, 2), dtype=np.uint64)
        v[..., 1] >>= np.uint64(1)
        return k[:count], v

if args.restore:
    import ctypes
    L = lib or D.load()
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def saved(tree, save):
        """the blob in a numpy array, through the C call alone, and the wall milliseconds of the call that wrote it"""
        n = ctypes.c_size_t(0)
        assert save(tree._h, None, ctypes.c_size_t(0), ctypes.byref(n)) == 0
        out = np.zeros(n.value, dtype=np.uint8)
        t0 = time.perf_counter()
        assert save(tree._h, vp(out), ctypes.c_size_t(n.value), ctypes.byref(n)) == 0
        return out, (time.perf_counter() - t0) * 1e3

    def loaded(load, destroy, blob, audit, runs):
        """wall milliseconds of `runs` loads of the blob (each tree destroyed outside the timed part) and the last handle"""
        ms, h = [], None
        for _ in range(runs):
            if h is not None:
                destroy(h)
            h = ctypes.c_void_p()
            t0 = time.perf_counter()
            r = load(ctypes.c_int(0), vp(blob), ctypes.c_size_t(blob.size), ctypes.c_uint32(audit), ctypes.byref(h))
            ms.append((time.perf_counter() - t0) * 1e3)
            assert r == 0, r
        return ms, h

    L.dst_rtree_destroy.restype = L.dst_stree_destroy.restype = None
    log_leaves = 20
    a = leaves(log_leaves)
    D.RescueTree(a, device=0, lib=lib).close()      # warm-up
    t0 = time.perf_counter(); t = D.RescueTree(a, device=0, lib=lib); build_wall = (time.perf_counter() - t0) * 1e3
    build_ms = t.build_ms
    audits = []
    for _ in range(1 + args.runs):                  # the first is the warm-up: the staging word, code
        assert t.audit() is None
        audits.append(t.audit_ms)
    audits = audits[1:]
    blob, save_ms = saved(t, L.dst_rtree_save)
    print("dense 2^%d leaves: build %.3f ms on the device (dst_rtree_build_ms, %d level launches), %.1f ms wall with the upload; audit %.3f ms on the device, ONE launch over %d parents "
          "(min of %d after one warm-up; all: %s): audit / build = %.3f" % (log_leaves, build_ms, log_leaves, build_wall, min(audits), (1 << log_leaves) - 1, args.runs,
                                                                          " ".join("%.3f" % v for v in audits), min(audits) / build_ms))
    ms, h = loaded(L.dst_rtree_load, L.dst_rtree_destroy, blob, 0, 1 + args.runs)
    ms_a, h_a = loaded(L.dst_rtree_load, L.dst_rtree_destroy, blob, 1, args.runs)
    L.dst_rtree_destroy(h_a)
    back = D.RescueTree.__new__(D.RescueTree)
    back.lib, back._h, back.log_leaves = L, h, log_leaves
    assert back.root == t.root and back.build_ms == 0 and back.audit() is None
    print("   saved in %.1f ms wall, %d bytes; dst_rtree_load without audit: %.1f ms wall (min of %d after one warm-up; all: %s), with audit: %.1f ms wall (all: %s); rebuild / load = %.2f, "
          "rebuild / load with audit = %.2f; root %032x %032x" % (save_ms, blob.size, min(ms[1:]), args.runs, " ".join("%.1f" % v for v in ms[1:]), min(ms_a), " ".join("%.1f" % v for v in ms_a),
                                                                   build_wall / min(ms[1:]), build_wall / min(ms_a), back.root[0], back.root[1]))
    back.close(); t.close()
    del blob, a
    k, v = keys_and_leaves(1 << 20, 20)
    s = D.SparseRescueTree(DEPTH, device=0, lib=lib)
    t0 = time.perf_counter(); s.set(k, v); set_wall = (time.perf_counter() - t0) * 1e3
    info = s.info()
    audits = []
    for _ in range(1 + min(args.runs, 3)):
        assert s.audit() is None
        audits.append(s.audit_ms)
    audits = audits[1:]
    blob, save_ms = saved(s, L.dst_stree_save)
    print("sparse depth %d, %d keys, %d stored nodes: the one set that builds it %.3f ms on the device (last_device_ms, one launch per level), %d digests, %.1f ms wall with the plan and the "
          "uploads; audit %.3f ms on the device, ONE launch over %d parents (min of %d after one warm-up; all: %s): audit / set = %.3f"
          % (DEPTH, info["keys"], info["nodes"], info["last_device_ms"], info["last_digests"], set_wall, min(audits), info["nodes"] - info["keys"], len(audits),
             " ".join("%.3f" % x for x in audits), min(audits) / info["last_device_ms"]))
    root = s.root
    s.close()
    ms, h = loaded(L.dst_stree_load, L.dst_stree_destroy, blob, 0, 3)
    ms_a, h_a = loaded(L.dst_stree_load, L.dst_stree_destroy, blob, 1, 2)
    L.dst_stree_destroy(h_a)
    back = D.SparseRescueTree.__new__(D.SparseRescueTree)
    back.lib, back._h, back.depth = L, h, DEPTH
    assert back.root == root and back.info()["last_digests"] == 0 and back.info()["nodes"] == info["nodes"]
    print("   saved in %.1f ms wall, %d bytes; dst_stree_load without audit: %.1f ms wall (min of 2 after one warm-up; all: %s), with audit: %.1f ms wall (all: %s); rebuild / load = %.2f, "
          "rebuild / load with audit = %.2f; root %032x %032x" % (save_ms, blob.size, min(ms[1:]), " ".join("%.1f" % x for x in ms[1:]), min(ms_a), " ".join("%.1f" % x for x in ms_a),
                                                                   set_wall / min(ms[1:]), set_wall / min(ms_a), root[0], root[1]))
    back.close()
    sys.exit(0)
if args.remove:
    import ctypes
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    keys, v = keys_and_leaves(1 << 20, 120)         # the 2^20-key tree of --sparse
    big = D.SparseRescueTree(DEPTH, device=0, lib=lib)
    big.set(keys, v)
    L, h = big.lib, big._h
    print("sparse depth %d: %d keys, %d stored nodes" % (DEPTH, big.info()["keys"], big.info()["nodes"]))

    def timed(call):
        """the C call alone -> (wall ms, device ms, last_digests)"""
        t0 = time.perf_counter()
        r = call()
        wall = (time.perf_counter() - t0) * 1e3
        assert r == 0, big._error(h)
        i = big.info()
        return wall, i["last_device_ms"], i["last_digests"]

    rng = np.random.default_rng(4040)
    live = keys.copy()                              # the stored keys, in random order: every run takes the next `count` of them
    gone = ctypes.c_uint64(0)
    for count in (1, 256, 65536):
        sets, removes = [], []
        for _ in range(1 + args.runs):              # the first is the warm-up: staging buffer, code
            k, live = np.ascontiguousarray(live[:count]), live[count:]
            new = rng.integers(0, 1 << 64, size=(count, 2, 2), dtype=np.uint64)
            new[..., 1] >>= np.uint64(1)
            sets.append(timed(lambda: L.dst_stree_set(h, vp(k), vp(new), ctypes.c_size_t(count))))      # the yardstick: existing code, the same keys, the same tree
            removes.append(timed(lambda: L.dst_stree_remove(h, vp(k), ctypes.c_size_t(count), ctypes.byref(gone))))
            assert gone.value == count
        sets, removes = sets[1:], removes[1:]
        s_ms, r_ms, s_wall, r_wall = min(x[1] for x in sets), min(x[1] for x in removes), min(x[0] for x in sets), min(x[0] for x in removes)
        print("remove of %d stored keys from the 2^20-key tree: %.3f ms on the device (min of %d after one warm-up; all: %s), %d digests, %.1f ms wall (min; all: %s); "
              "the set of the same keys just before: %.3f ms on the device (all: %s), %d digests, %.1f ms wall (all: %s); remove / set = %.3f on the device, %.3f wall; %d stored nodes left"
              % (count, r_ms, len(removes), " ".join("%.3f" % x[1] for x in removes), removes[-1][2], r_wall, " ".join("%.1f" % x[0] for x in removes),
                 s_ms, " ".join("%.3f" % x[1] for x in sets), sets[-1][2], s_wall, " ".join("%.1f" % x[0] for x in sets), r_ms / s_ms, r_wall / s_wall, big.info()["nodes"]))
    count = 65536
    k, live = np.ascontiguousarray(live[:count]), live[count:]
    empties = np.zeros((count, 2, 2), dtype=np.uint64)
    nodes = big.info()["nodes"]
    a_wall, a_ms, a_digests = timed(lambda: L.dst_stree_apply(h, vp(k), vp(empties), ctypes.c_size_t(count), None, None))
    c_wall, c_ms, c_digests = timed(lambda: L.dst_stree_compact(h, ctypes.byref(gone)))
    assert gone.value == count and c_digests == 0
    print("compact after an apply of %d empties: %.1f ms wall, %.3f ms on the device between the events (no level launch), %d digests, %d keys and %d of %d stored nodes dropped; "
          "the apply: %.1f ms wall, %.3f ms on the device, %d digests" % (count, c_wall, c_ms, c_digests, gone.value, nodes - big.info()["nodes"], nodes, a_wall, a_ms, a_digests))
    idx = np.ascontiguousarray(np.concatenate([live[rng.integers(0, live.size, size=2048)], rng.integers(0, 1 << DEPTH, size=2048, dtype=np.uint64)]))
    out, flags, paths = np.zeros((idx.size, 2, 2), dtype=np.uint64), np.zeros(idx.size, dtype=np.uint8), np.zeros((idx.size, DEPTH + 1, 2, 2), dtype=np.uint64)
    g_wall, p_wall = [], []
    for _ in range(1 + args.runs):
        g_wall.append(timed(lambda: L.dst_stree_get(h, vp(idx), ctypes.c_size_t(idx.size), vp(out), vp(flags)))[0])
        p_wall.append(timed(lambda: L.dst_stree_paths(h, vp(idx), ctypes.c_size_t(idx.size), vp(paths)))[0])
    assert np.array_equal(out, paths[:, 0]) and flags[:2048].all() and not flags[2048:].any()
    print("dst_stree_get of %d indices (half stored, half absent) on the %d-key tree: %.3f ms wall (min of %d after one warm-up; all: %s), %d bytes back; dst_stree_paths of the same: %.3f ms wall (all: %s), %d bytes back"
          % (idx.size, big.info()["keys"], min(g_wall[1:]), args.runs, " ".join("%.3f" % x for x in g_wall[1:]), 33 * idx.size, min(p_wall[1:]), " ".join("%.3f" % x for x in p_wall[1:]), 32 * (DEPTH + 1) * idx.size))
    big.close()
    sys.exit(0)
if args.sparse:
    a = leaves(20)
    D.RescueTree(a, device=0, lib=lib).close()      # warm-up
    dense_ms = []
    for _ in range(args.runs):
        t = D.RescueTree(a, device=0, lib=lib)
        dense_ms.append(t.build_ms)
        t.close()
    dense_rate = ((1 << 20) - 1) / (min(dense_ms) * 1e-3)
    print("yardstick, dense tree of 2^20 leaves: %.3f ms on the device (min of %d; all: %s), %.3e digests/s"
          % (min(dense_ms), args.runs, " ".join("%.3f" % v for v in dense_ms), dense_rate))
    big = None
    for log_keys in (12, 16, 20):
        k, v = keys_and_leaves(1 << log_keys, 100 + log_keys)
        ms = []
        for run in range(1 + (args.runs if log_keys < 20 else 1)):      # the first is the warm-up; the 2^20-key tree is built twice only
            t0 = time.perf_counter()
            t = D.SparseRescueTree(DEPTH, device=0, lib=lib)
            t.set(k, v)
            wall = time.perf_counter() - t0
            i = t.info()
            ms.append(i["last_device_ms"])
            root = t.root
            if log_keys == 20 and run == 1:
                big = t                             # the tree the sets below go into
            else:
                t.close()
        ms = ms[1:]
        rate = i["last_digests"] / (min(ms) * 1e-3)
        narrow = sum(1 for l in range(DEPTH) if min(1 << l, 1 << log_keys) <= (1 << 15))
        print("set of 2^%d keys into an empty depth-%d tree: %.3f ms on the device (min of %d after one warm-up; all: %s), %d digests, %.3e digests/s = %.3f of the dense rate; "
              "%d stored nodes; %d of 63 levels within RESCUE_SPREAD_MAX; %.1f ms wall with the plan and the uploads; root %032x %032x"
              % (log_keys, DEPTH, min(ms), len(ms), " ".join("%.3f" % x for x in ms), i["last_digests"], rate, rate / dense_rate, i["nodes"], narrow, wall * 1e3, root[0], root[1]))
    for count in (1, 256, 65536):
        ms, wall = [], []
        for run in range(1 + args.runs):
            k, v = keys_and_leaves(count, 1000 * count + run)
            t0 = time.perf_counter()
            big.set(k, v)
            wall.append((time.perf_counter() - t0) * 1e3)
            i = big.info()
            ms.append(i["last_device_ms"])
        ms, wall = ms[1:], wall[1:]
        print("set of %d keys into the 2^20-key tree: %.3f ms on the device (min of %d after one warm-up; all: %s), %d digests, %.3e digests/s = %.3f of the dense rate, "
              "%.3f ms per level; %.1f ms wall (the carry-over of %d nodes, the plan and the uploads included)"
              % (count, min(ms), len(ms), " ".join("%.3f" % x for x in ms), i["last_digests"], i["last_digests"] / (min(ms) * 1e-3), i["last_digests"] / (min(ms) * 1e-3) / dense_rate,
                 min(ms) / DEPTH, min(wall), i["nodes"]))
    rng = np.random.default_rng(7)
    stored = big.level(DEPTH)[0]
    idx = np.concatenate([stored[rng.integers(0, stored.size, size=2048)], rng.integers(0, 1 << DEPTH, size=2048, dtype=np.uint64)])
    big.paths_words(idx[:16])                       # warm-up
    t0 = time.perf_counter(); w = big.paths_words(idx); s_many = time.perf_counter() - t0
    print("dst_stree_paths of %d indices (half stored, half absent) on the %d-key tree: %.3f ms wall (%d nodes of %d searched levels each)" % (idx.size, big.info()["keys"], s_many * 1e3, DEPTH + 1, DEPTH + 1))
    big.close()
    sys.exit(0)
if args.multiproof:
    import ctypes
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rng = np.random.default_rng(5050)

    def time_multiproofs(name, tree, n, draw, multiproof, open_paths):
        """per K: the tree's multiproof of K random distinct leaves, its bytes and digests beside those of K full paths, and
        dst_rescue_multiproof_root's device_ms beside dst_rescue_verify_paths' on the full paths of the same leaves (existing code: the yardstick)"""
        L = tree.lib
        root = D.ints_to_arr(tree.root)
        for count in (256, 4096, 65536):
            idx = draw(count)
            m, digests, dms = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_double(0)
            assert multiproof(tree._h, vp(idx), ctypes.c_size_t(count), None, None, ctypes.c_size_t(0), ctypes.byref(m)) == 0
            lv, nodes, got = np.zeros((count, 2, 2), dtype=np.uint64), np.zeros((m.value + 1, 2, 2), dtype=np.uint64), np.zeros((2, 2), dtype=np.uint64)
            t0 = time.perf_counter()
            assert multiproof(tree._h, vp(idx), ctypes.c_size_t(count), vp(lv), vp(nodes), ctypes.c_size_t(m.value), ctypes.byref(m)) == 0
            take_wall = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            paths = open_paths(idx)
            paths_wall = (time.perf_counter() - t0) * 1e3
            first, why = ctypes.c_int64(0), ctypes.c_uint32(0)
            mp_ms, mp_wall, pv_ms, pv_wall = [], [], [], []
            for _ in range(1 + args.runs):          # the first is the warm-up: code; the two checks alternate
                t0 = time.perf_counter()
                r = L.dst_rescue_multiproof_root(ctypes.c_int(0), ctypes.c_uint32(n), vp(idx), vp(lv), ctypes.c_size_t(count), vp(nodes), ctypes.c_size_t(m.value), vp(got), ctypes.byref(digests), ctypes.byref(dms))
                mp_wall.append((time.perf_counter() - t0) * 1e3)
                assert r == 0 and np.array_equal(got, root)
                mp_ms.append(dms.value)
                t0 = time.perf_counter()
                r = L.dst_rescue_verify_paths(ctypes.c_int(0), vp(root), vp(paths), ctypes.c_uint32(n), vp(idx), None, ctypes.c_size_t(count), ctypes.byref(first), ctypes.byref(why), ctypes.byref(dms))
                pv_wall.append((time.perf_counter() - t0) * 1e3)
                assert r == 0 and (first.value, why.value) == (-1, 0)
                pv_ms.append(dms.value)
            mp_ms, mp_wall, pv_ms, pv_wall = mp_ms[1:], mp_wall[1:], pv_ms[1:], pv_wall[1:]
            expanded, dms2 = np.zeros((count, n, 2, 2), dtype=np.uint64), ctypes.c_double(0)
            assert L.dst_rescue_multiproof_paths(ctypes.c_int(0), ctypes.c_uint32(n), vp(idx), vp(lv), ctypes.c_size_t(count), vp(nodes), ctypes.c_size_t(m.value), vp(expanded), vp(got), ctypes.byref(dms2)) == 0
            assert np.array_equal(expanded, paths)
            mp_bytes, path_bytes = 32 * (count + m.value), 32 * count * n
            print("%s, K = %d: multiproof %d bytes (%d leaves + %d nodes) against %d bytes of paths = %.2f x fewer; %d digests against %d = %.2f x fewer; "
                  "multiproof_root %.3f ms on the device (min of %d after one warm-up; all: %s), %.2f ms wall (min); verify_paths of the same leaves %.3f ms on the device (all: %s), %.2f ms wall (min); "
                  "multiproof / paths = %.3f on the device, %.3f wall; taking it from the tree %.2f ms wall against %.2f ms for the paths; expansion with the gather %.3f ms on the device"
                  % (name, count, mp_bytes, count, m.value, path_bytes, path_bytes / mp_bytes, digests.value, count * (n - 1), count * (n - 1) / digests.value,
                     min(mp_ms), len(mp_ms), " ".join("%.3f" % v for v in mp_ms), min(mp_wall), min(pv_ms), " ".join("%.3f" % v for v in pv_ms), min(pv_wall),
                     min(mp_ms) / min(pv_ms), min(mp_wall) / min(pv_wall), take_wall, paths_wall, dms2.value))

    log_leaves = 20
    t = D.RescueTree(leaves(log_leaves), device=0, lib=lib)

    def dense_paths(idx):
        out = np.zeros((idx.size, log_leaves + 1, 2, 2), dtype=np.uint64)
        assert t.lib.dst_rtree_paths(t._h, vp(idx), ctypes.c_size_t(idx.size), vp(out)) == 0
        return out

    time_multiproofs("dense 2^%d leaves" % log_leaves, t, log_leaves + 1, lambda count: np.ascontiguousarray(rng.permutation(1 << log_leaves)[:count].astype(np.uint64)),
                     t.lib.dst_rtree_multiproof, dense_paths)
    t.close()
    DEPTH = 63
    keys = np.unique(rng.integers(0, 1 << DEPTH, size=(1 << 20) + (1 << 17), dtype=np.uint64))
    rng.shuffle(keys)
    keys = keys[:1 << 20]
    v = rng.integers(0, 1 << 64, size=(keys.size, 2, 2), dtype=np.uint64)
    v[..., 1] >>= np.uint64(1)
    s = D.SparseRescueTree(DEPTH, device=0, lib=lib)
    s.set(keys, v)
    print("sparse depth %d: %d keys, %d stored nodes" % (DEPTH, s.info()["keys"], s.info()["nodes"]))

    def sparse_draw(count):                         # distinct: half stored keys, half keys that are (almost surely) absent
        half = keys[rng.permutation(keys.size)[:count // 2]]
        other = rng.integers(0, 1 << DEPTH, size=count - count // 2 + 8, dtype=np.uint64)
        return np.ascontiguousarray(rng.permutation(np.unique(np.concatenate([half, other])))[:count])

    time_multiproofs("sparse depth %d, 2^20 keys" % DEPTH, s, DEPTH + 1, sparse_draw, s.lib.dst_stree_multiproof, s.paths_words)
    s.close()
    sys.exit(0)
if args.refresh:
    import ctypes
    REFRESH_SEED = 4040
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def time_refreshes(name, tree, apply, open_paths, n, draw, wide=False):
        """dst_rescue_refresh_paths beside dst_rescue_verify_writes on the same batch, in this process: per repeat the held paths are opened (wall,
        for orientation: what a client without the call would ask the tree for again), the batch is applied, its witnesses are verified and the
        held paths are refreshed; the refreshed paths are then the tree's.  Device ms: events around the chain launch (verify), around the chain
        launch and the gather (refresh), around the gather alone (dst_rescue_refresh_last_gather_ms).  Wall of refresh: the C call with the plan, the upload and the copy back."""
        rng = np.random.default_rng(REFRESH_SEED)
        L = tree.lib
        verify, refresh = (L.dst_rescue_verify_writes_w, L.dst_rescue_refresh_paths_w) if wide else (L.dst_rescue_verify_writes, L.dst_rescue_refresh_paths)
        first, why, dms, after = ctypes.c_int64(0), ctypes.c_uint32(0), ctypes.c_double(0), np.zeros((2, 2), dtype=np.uint64)
        for count in (256, 4096, 65536):
            for held in (256, 4096):
                v_ms, r_ms, g_ms, r_wall, p_wall = [], [], [], [], []
                for _ in range(1 + args.runs):      # the first is the warm-up: code
                    idx, new = draw(rng, count)
                    hidx = np.ascontiguousarray(np.concatenate([idx[rng.integers(0, count, size=held // 4)], draw(rng, held - held // 4)[0]]))   # a quarter of the held keys are written
                    t0 = time.perf_counter()
                    mine = open_paths(hidx)
                    p_wall.append((time.perf_counter() - t0) * 1e3)
                    paths, roots = np.zeros((count, n, 2, 2), dtype=np.uint64), np.zeros((count, 2, 2), dtype=np.uint64)
                    before = D.ints_to_arr(tree.root)
                    assert apply(tree._h, vp(idx), vp(new), ctypes.c_size_t(count), vp(paths), vp(roots)) == 0
                    common = (ctypes.c_int(0), vp(before), vp(paths), ctypes.c_uint32(n), vp(idx), vp(new), vp(roots), ctypes.c_size_t(count))
                    tail = (ctypes.byref(first), ctypes.byref(why), vp(after), ctypes.byref(dms))
                    assert verify(*(common + tail)) == 0 and (first.value, why.value) == (-1, 0)
                    v_ms.append(dms.value)
                    t0 = time.perf_counter()
                    r = refresh(*(common + (vp(hidx), vp(mine), ctypes.c_size_t(held), vp(mine)) + tail))
                    r_wall.append((time.perf_counter() - t0) * 1e3)
                    assert r == 0 and (first.value, why.value) == (-1, 0) and tuple(D.arr_to_ints(after)) == tree.root
                    r_ms.append(dms.value)
                    g_ms.append(D.lib._refresh_gather_ms(L))
                    assert mine.tobytes() == open_paths(hidx).tobytes()
                v_ms, r_ms, g_ms, r_wall, p_wall = v_ms[1:], r_ms[1:], g_ms[1:], r_wall[1:], p_wall[1:]
                print("%s: %d writes, %d held paths of %d nodes (%s): refresh_paths %.3f ms on the device (min of %d after one warm-up; all: %s); verify_writes of the same batches %.3f ms "
                      "(min; all: %s); the gather launch alone %.3f ms (min; all: %s); refresh - verify = %+.3f ms (min - min; the gather and the %d bytes the chains store per write); refresh %.2f ms wall with the plan (min; all: %s); "
                      "tree.paths(held) %.2f ms wall (min)"
                      % (name, count, held, n, "six-lane form" if 2 * count <= (1 << 15) else "one-lane form", min(r_ms), len(r_ms), " ".join("%.3f" % x for x in r_ms), min(v_ms),
                         " ".join("%.3f" % x for x in v_ms), min(g_ms), " ".join("%.3f" % x for x in g_ms), min(r_ms) - min(v_ms), 32 * (n - 2), min(r_wall), " ".join("%.2f" % x for x in r_wall), min(p_wall)))

    def words_draw(draw_keys):
        def draw(rng, count):
            new = rng.integers(0, 1 << 64, size=(count, 2, 2), dtype=np.uint64)
            new[..., 1] >>= np.uint64(1)
            idx = draw_keys(rng, count)
            again = np.nonzero(rng.random(count) < 0.1)[0]          # about a tenth of the writes repeat an earlier key
            again = again[again > 0]
            idx[again] = idx[(rng.random(again.size) * again).astype(np.int64)]
            return np.ascontiguousarray(idx), new
        return draw

    log_leaves = 20
    t = D.RescueTree(leaves(log_leaves), device=0, lib=lib)

    def dense_paths(idx):
        out = np.zeros((idx.shape[0], log_leaves + 1, 2, 2), dtype=np.uint64)
        assert t.lib.dst_rtree_paths(t._h, vp(idx), ctypes.c_size_t(idx.shape[0]), vp(out)) == 0
        return out

    time_refreshes("dense 2^%d leaves" % log_leaves, t, t.lib.dst_rtree_apply, dense_paths, log_leaves + 1, words_draw(lambda rng, count: rng.integers(0, 1 << log_leaves, size=count).astype(np.uint64)))
    t.close()
    rng0 = np.random.default_rng(REFRESH_SEED + 1)
    keys = np.unique(rng0.integers(0, 1 << 63, size=(1 << 20) + (1 << 17), dtype=np.uint64))
    rng0.shuffle(keys)
    keys = keys[:1 << 20]
    v = rng0.integers(0, 1 << 64, size=(keys.size, 2, 2), dtype=np.uint64)
    v[..., 1] >>= np.uint64(1)
    s = D.SparseRescueTree(63, device=0, lib=lib)
    s.set(keys, v)

    def sparse_keys(rng, count):                    # half stored keys, half new ones
        idx = rng.integers(0, 1 << 63, size=count, dtype=np.uint64)
        stored = np.nonzero(rng.random(count) < 0.5)[0]
        idx[stored] = keys[rng.integers(0, keys.size, size=stored.size)]
        return idx

    time_refreshes("sparse depth 63, 2^20 keys", s, s.lib.dst_stree_apply, s.paths_words, 64, words_draw(sparse_keys))
    s.close()
    wk, wv = wide_keys(1 << 16, REFRESH_SEED + 2)
    w = D.WideSparseRescueTree(127, device=0, lib=lib)
    w.set(wk, wv)

    def wide_draw(rng, count):
        idx = rng.integers(0, 1 << 64, size=(count, 2), dtype=np.uint64)
        idx[:, 1] >>= np.uint64(1)
        stored = np.nonzero(rng.random(count) < 0.5)[0]
        idx[stored] = wk[rng.integers(0, len(wk), size=stored.size)]
        return idx

    time_refreshes("wide depth 127, 2^16 keys", w, w.lib.dst_wtree_apply, w.paths_words, 128, words_draw(wide_draw), wide=True)
    w.close()
    sys.exit(0)
if args.sequence or args.verify:
    import ctypes
    SEQUENCE_SEED, DEPTH = 3030, 63
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def operations(rng, count, draw):
        """`count` indices from draw(count), about a tenth of them replaced by an earlier index of the same sequence, and as many leaves"""
        idx = draw(count)
        again = np.nonzero(rng.random(count) < 0.1)[0]
        again = again[again > 0]
        idx[again] = idx[(rng.random(again.size) * again).astype(np.int64)]
        new = rng.integers(0, 1 << 64, size=(count, 2, 2), dtype=np.uint64)
        new[..., 1] >>= np.uint64(1)
        return np.ascontiguousarray(idx), new

    def time_applies(name, tree, apply, n, draw, device_ms, note=lambda: ""):
        """the C call alone: wall = the host clock around it (plan, upload, launches, copy back of count * n nodes and count roots)"""
        rng = np.random.default_rng(SEQUENCE_SEED)
        for count in (1, 256, 4096, 65536):
            ms, wall = [], []
            for _ in range(1 + args.runs):          # the first is the warm-up: staging buffer, code
                idx, new = operations(rng, count, draw)
                paths, roots = np.zeros((count, n, 2, 2), dtype=np.uint64), np.zeros((count, 2, 2), dtype=np.uint64)
                t0 = time.perf_counter()
                r = apply(tree._h, vp(idx), vp(new), ctypes.c_size_t(count), vp(paths), vp(roots))
                wall.append((time.perf_counter() - t0) * 1e3)
                assert r == 0 and tuple(D.arr_to_ints(roots[-1])) == tree.root
                ms.append(device_ms())
            ms, wall = ms[1:], wall[1:]
            print("%s: apply of %d ordered writes (%d distinct indices): %.3f ms on the device (min of %d after one warm-up; all: %s) = %.3f ms per level; %.2f ms wall (min; all: %s)%s"
                  % (name, count, np.unique(idx).size, min(ms), len(ms), " ".join("%.3f" % v for v in ms), min(ms) / (n - 1), min(wall), " ".join("%.2f" % v for v in wall), note()))

    def time_verifies(name, tree, apply, open_paths, n, draw, device_ms, share):
        """dst_rescue_verify_writes on the witnesses an apply just returned, beside that apply's own device time; `share` of the apply's launches
        compute the witnesses (the rest of a sparse apply is the set that follows).  Then the same check on the host for 256 writes, and
        dst_rescue_verify_paths of 4 096 openings against the tree's root."""
        rng = np.random.default_rng(SEQUENCE_SEED + 2)
        first, why, dms, after = ctypes.c_int64(0), ctypes.c_uint32(0), ctypes.c_double(0), np.zeros((2, 2), dtype=np.uint64)
        args_of = lambda device, before, paths, idx, new, roots, count: (ctypes.c_int(device), vp(before), vp(paths), ctypes.c_uint32(n), vp(idx), vp(new), vp(roots), ctypes.c_size_t(count),  # noqa: E731
                                                                         ctypes.byref(first), ctypes.byref(why), vp(after), ctypes.byref(dms))
        for count in (256, 4096, 65536):
            ms, wall, applied = [], [], []
            for _ in range(1 + args.runs):          # the first is the warm-up: code
                idx, new = operations(rng, count, draw)
                paths, roots = np.zeros((count, n, 2, 2), dtype=np.uint64), np.zeros((count, 2, 2), dtype=np.uint64)
                before = D.ints_to_arr(tree.root)
                assert apply(tree._h, vp(idx), vp(new), ctypes.c_size_t(count), vp(paths), vp(roots)) == 0
                applied.append(device_ms())
                t0 = time.perf_counter()
                r = L.dst_rescue_verify_writes(*args_of(0, before, paths, idx, new, roots, count))
                wall.append((time.perf_counter() - t0) * 1e3)
                assert r == 0 and (first.value, why.value) == (-1, 0) and tuple(D.arr_to_ints(after)) == tree.root
                ms.append(dms.value)
            ms, wall, applied = ms[1:], wall[1:], applied[1:]
            print("%s: verify_writes of %d witnesses (%d chains of %d digests, %s): %.3f ms on the device (min of %d after one warm-up; all: %s) = %.3f ms per level; %.2f ms wall (min; all: %s); "
                  "the apply that made them: %.3f ms on the device (min; all: %s); verify / (%.2f x apply) = %.2f"
                  % (name, count, 2 * count, n - 1, "six-lane form" if 2 * count <= (1 << 15) else "one-lane form", min(ms), len(ms), " ".join("%.3f" % v for v in ms), min(ms) / (n - 1),
                     min(wall), " ".join("%.2f" % v for v in wall), min(applied), " ".join("%.3f" % v for v in applied), share, min(ms) / (share * min(applied))))
            if count == 256:
                t0 = time.perf_counter()
                r = L.dst_rescue_verify_writes(*args_of(-1, before, paths, idx, new, roots, count))
                host = (time.perf_counter() - t0) * 1e3
                assert r == 0 and (first.value, why.value) == (-1, 0) and tuple(D.arr_to_ints(after)) == tree.root
                print("%s: the same %d witnesses on the host (device = -1, one core): %.1f ms wall, %.1f us per digest" % (name, count, host, host * 1e3 / (2 * count * (n - 1))))
        idx = np.ascontiguousarray(draw(4096))
        paths, root = open_paths(idx), D.ints_to_arr(tree.root)
        ms, wall = [], []
        for _ in range(1 + args.runs):
            t0 = time.perf_counter()
            r = L.dst_rescue_verify_paths(ctypes.c_int(0), vp(root), vp(paths), ctypes.c_uint32(n), vp(idx), None, ctypes.c_size_t(idx.size), ctypes.byref(first), ctypes.byref(why), ctypes.byref(dms))
            wall.append((time.perf_counter() - t0) * 1e3)
            assert r == 0 and (first.value, why.value) == (-1, 0)
            ms.append(dms.value)
        print("%s: verify_paths of %d paths against the root: %.3f ms on the device (min of %d after one warm-up; all: %s); %.2f ms wall (min)"
              % (name, idx.size, min(ms[1:]), len(ms) - 1, " ".join("%.3f" % v for v in ms[1:]), min(wall[1:])))

    def time_loop(name, count, idx, new, one_write, one_path, n):
        """the baseline: per operation one path of one leaf, then one write of one leaf, through the calls that existed before"""
        path = np.zeros((n, 2, 2), dtype=np.uint64)
        t0 = time.perf_counter()
        r = 0
        for j in range(count):
            r |= one_path(idx[j:j + 1], path)
            r |= one_write(idx[j:j + 1], new[j:j + 1])
        wall = (time.perf_counter() - t0) * 1e3
        assert r == 0
        print("%s: the loop of %d x (single path + single-leaf write): %.1f ms wall, %.3f ms per operation" % (name, count, wall, wall / count))

    log_leaves = 20
    a = leaves(log_leaves)
    t = D.RescueTree(a, device=0, lib=lib)
    L = t.lib
    rng = np.random.default_rng(SEQUENCE_SEED + 1)
    dense_draw = lambda count: rng.integers(0, 1 << log_leaves, size=count).astype(np.uint64)  # noqa: E731
    def dense_paths(idx):
        out = np.zeros((idx.size, log_leaves + 1, 2, 2), dtype=np.uint64)
        assert L.dst_rtree_paths(t._h, vp(idx), ctypes.c_size_t(idx.size), vp(out)) == 0
        return out

    if args.verify:
        time_verifies("dense 2^%d leaves" % log_leaves, t, L.dst_rtree_apply, dense_paths, log_leaves + 1, dense_draw, lambda: t.update_ms, 1.0)
    else:
        time_applies("dense 2^%d leaves" % log_leaves, t, L.dst_rtree_apply, log_leaves + 1, dense_draw, lambda: t.update_ms)
        idx, new = operations(rng, 256, dense_draw)
        time_loop("dense 2^%d leaves" % log_leaves, 256, idx, new, lambda i, v: L.dst_rtree_update(t._h, vp(i), vp(v), ctypes.c_size_t(1)),
                  lambda i, out: L.dst_rtree_path(t._h, ctypes.c_uint64(int(i[0])), vp(out)), log_leaves + 1)
    t.close()
    keys = np.unique(rng.integers(0, 1 << DEPTH, size=(1 << 20) + (1 << 17), dtype=np.uint64))
    rng.shuffle(keys)
    keys = keys[:1 << 20]
    v = rng.integers(0, 1 << 64, size=(keys.size, 2, 2), dtype=np.uint64)
    v[..., 1] >>= np.uint64(1)
    s = D.SparseRescueTree(DEPTH, device=0, lib=lib)
    s.set(keys, v)
    print("sparse depth %d: %d keys, %d stored nodes" % (DEPTH, s.info()["keys"], s.info()["nodes"]))

    def sparse_draw(count):                         # half stored keys, half new ones
        idx = rng.integers(0, 1 << DEPTH, size=count, dtype=np.uint64)
        stored = np.nonzero(rng.random(count) < 0.5)[0]
        idx[stored] = keys[rng.integers(0, keys.size, size=stored.size)]
        return idx

    if args.verify:                                # the witnesses are 63 of the 126 level launches of a sparse apply
        time_verifies("sparse depth %d, 2^20 keys" % DEPTH, s, L.dst_stree_apply, s.paths_words, DEPTH + 1, sparse_draw, lambda: s.info()["last_device_ms"], 0.5)
        s.close()
        sys.exit(0)
    time_applies("sparse depth %d, 2^20 keys" % DEPTH, s, L.dst_stree_apply, DEPTH + 1, sparse_draw, lambda: s.info()["last_device_ms"],
                lambda: "; %d digests: 63 per write, then one dst_stree_set of the distinct keys, whose 63 level launches the device time includes" % s.info()["last_digests"])
    idx, new = operations(rng, 256, sparse_draw)
    time_loop("sparse depth %d, 2^20 keys" % DEPTH, 256, idx, new, lambda i, w: L.dst_stree_set(s._h, vp(i), vp(w), ctypes.c_size_t(1)),
              lambda i, out: L.dst_stree_paths(s._h, vp(i), ctypes.c_size_t(1), vp(out)), DEPTH + 1)
    s.close()
    sys.exit(0)
for log_leaves in args.sizes or [12, 16, 20]:
    a = leaves(log_leaves)
    D.RescueTree(a, device=0, lib=lib).close()      # warm-up
    ms = []
    for _ in range(args.runs):
        t = D.RescueTree(a, device=0, lib=lib)
        ms.append(t.build_ms)
        root = t.root
        t.close()
    best, digests = min(ms), (1 << log_leaves) - 1
    print("2^%d leaves: %.3f ms on the device (min of %d; all: %s), %.3e digests/s, %.1f %% of the multiplication-rate bound, root %032x %032x"
          % (log_leaves, best, args.runs, " ".join("%.3f" % v for v in ms), digests / (best * 1e-3), 100.0 * digests / (best * 1e-3) / bound, root[0], root[1]))
if args.host_log:
    a = leaves(args.host_log)
    t0 = time.perf_counter()
    t = D.RescueTree(a, device=-1, lib=lib)
    s = time.perf_counter() - t0
    print("2^%d leaves on the host path, one core: %.1f ms, %.3e digests/s, root %032x %032x" % ((args.host_log, s * 1e3, ((1 << args.host_log) - 1) / s) + t.root))
    t.close()
