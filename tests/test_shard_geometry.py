"""Which rank and which heap hold a leaf or a node of a sharded Merkle tree (distaff_amd/csrc/host/shard_geometry.h, what the opening plan of
shard.hip asks), walked by a program of its own: tests/shard_geometry/shard_geometry_check.cpp, compiled by g++ with the address and
undefined-behaviour sanitizers.  For every shape the program checks that every leaf and every node has exactly one home and that the home lies
inside the buffer shard.hip reads for it; with the k-range mode off this test compares the homes, line by line, with the Python statement of the
same layout (distaff_amd.sharded.TreeGeometry), which has no k-range mode."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shapes():
    """[(L, Bt, G, krange)]: L leaves in 4 .. 1024, Bt leaves per k in 2 .. 256, over G = 1, 2, 4, 8 ranks with at least one column each.
    L < Bt only on one rank: that is how the opening plan describes a layer of the replicated FRI tail (Geometry(rows, B, 1)); a tree that
    is split over ranks has at least one k (the trace and constraint trees have n of them, a sharded FRI layer at least one row per coset).
    The k-range mode on and off wherever tree_exchange would choose it: K = L / Bt boundary nodes per rank, K >= G and K % G == 0."""
    out = []
    for log_l in range(2, 11):
        for log_bt in range(1, 9):
            for G in (1, 2, 4, 8):
                L, Bt = 1 << log_l, 1 << log_bt
                if Bt % G or (L < Bt and G > 1):
                    continue
                out.append((L, Bt, G, 0))
                K = L // Bt
                if G > 1 and K >= G and K % G == 0:
                    out.append((L, Bt, G, 1))
    return out


def test_every_leaf_and_node_has_one_home_inside_its_heap(tmp_path):
    from distaff_amd.sharded import TreeGeometry
    exe = str(tmp_path / "shard_geometry_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "shard_geometry", "shard_geometry_check.cpp")])
    cases = shapes()
    assert len(cases) == 285 and sum(c[3] for c in cases) == 87 and sum(c[0] < c[1] for c in cases) == 21 and {c[2] for c in cases} == {1, 2, 4, 8}
    r = subprocess.run([exe], input="".join("%d %d %d %d\n" % c for c in cases).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    got, cur = {}, None
    for ln in r.stdout.decode().splitlines():
        if ln.startswith("# "):
            cur = got.setdefault(tuple(int(v) for v in ln[2:].split()), [])
        else:
            cur.append(ln)
    assert sorted(got) == sorted(cases)
    for L, Bt, G, krange in cases:
        if krange:
            assert got[(L, Bt, G, 1)] == []             # checked by the program alone: Python has no such mode
            continue
        geo = TreeGeometry(L, Bt, G)
        want = ["l %d %d %d" % ((i,) + geo.leaf(i)) for i in range(L)]
        for h in range(1, L):
            g, idx = geo.node(h)
            want.append("n %d %d %d" % (h, -1 if g is None else g, idx))
        assert got[(L, Bt, G, 0)] == want, (L, Bt, G)
