"""The opening plan of the library (distaff_amd/csrc/host_proof.h: plan_batch, augmented_positions, constraint_positions) on directed
index sets, without a GPU: tests/openings/open_plan_check.cpp prints what the C++ plans, and that is held against the oracle's
MerkleTree::prove_batch over random leaves (a digest names its leaf or heap node) and against the Python statement of the same plan in
distaff_amd/sharded.py -- both are pinned to the one yardstick.  The program is built with AddressSanitizer and UBSan."""
import json
import os
import subprocess

import numpy as np
import pytest

from openings_sets import position_sets, tree_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = (2, 8, 64, 1024)
DOMAINS = ((256, 16, 1), (4096, 32, 3), (16384, 16, 4))           # (N, B, FRI layers with the remainder): the shapes of the GPU tests


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("openings") / "open_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "openings", "open_plan_check.cpp")])

    def ask(requests):
        text = "".join("%s %s %d %s\n" % (what, " ".join(str(a) for a in args), len(idx), " ".join(str(i) for i in idx)) for what, args, idx in requests)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
        assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])       # sanitizers report on stderr
        lines = [json.loads(l) for l in r.stdout.decode().splitlines()]
        assert lines[-1] == {"served": len(requests)}
        return lines[:-1]
    return ask


@pytest.mark.parametrize("num_leaves", TREES)
def test_plan_batch_on_directed_sets(oracle, plan_check, num_leaves):
    """values, node lists and depth of plan_batch in C++ and in Python name exactly the digests of the oracle's batch proof, in its order
    (node lists by sorted pair, values by input order); at 2 leaves the depth is 1 and no level above the leaves is walked"""
    from distaff_amd import sharded
    O = oracle
    rng = np.random.default_rng(num_leaves)
    leaves = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(num_leaves)]
    heap = O.merkle_nodes(b"".join(leaves))
    name = {leaf: [1, i] for i, leaf in enumerate(leaves)}
    name.update({heap[32 * i:32 * i + 32]: [0, i] for i in range(1, num_leaves)})
    assert len(name) == 2 * num_leaves - 1
    sets = tree_sets(num_leaves)
    assert len(sets) >= (4 if num_leaves == 2 else 20)
    got = plan_check([("batch", (num_leaves,), idx) for _, idx in sets])
    for (label, idx), cpp in zip(sets, got):
        expected = O.merkle_prove_batch(b"".join(leaves), idx)
        want = {"values": [name[v][1] for v in expected["values"]], "nodes": [[name[d] for d in lst] for lst in expected["nodes"]], "depth": expected["depth"]}
        assert all(name[v][0] == 1 for v in expected["values"])
        assert cpp == want, (num_leaves, label)
        values, nodes, depth = sharded.plan_batch(idx, num_leaves)
        assert {"values": values, "nodes": [[[int(is_leaf), i] for is_leaf, i in lst] for lst in nodes], "depth": depth} == want, (num_leaves, label, "python")
    if num_leaves == 2:
        assert all(p["depth"] == 1 and all(ref[0] == 1 for lst in p["nodes"] for ref in lst) for p in got)


@pytest.mark.parametrize("N,B,layers", DOMAINS)
def test_constraint_and_augmented_positions_on_directed_sets(plan_check, N, B, layers):
    """constraint_positions and the chain of augmented_positions over the FRI layers, C++ against Python against the definition: the
    distinct values of p / 2 (of p mod a quarter of the layer) in order of first appearance"""
    from distaff_amd import sharded
    sets = position_sets(N, B)
    got = plan_check([("positions", (N, layers - 1), pos) for _, _, pos in sets])
    collided = {"constraint": 0, "layer": [0] * (layers - 1)}
    for (family, label, pos), cpp in zip(sets, got):
        def first_appearances(values):
            return list(dict.fromkeys(values))
        want = {"constraint": first_appearances(p // 2 for p in pos), "augmented": []}
        cur, size = pos, N
        for d in range(layers - 1):
            nxt = first_appearances(p % (size // 4) for p in cur)
            collided["layer"][d] += len(nxt) < len(cur)
            want["augmented"].append(nxt)
            cur, size = nxt, size // 4
        collided["constraint"] += len(want["constraint"]) < len(pos)
        assert cpp == want, (N, label)
        assert sharded.constraint_positions(pos) == want["constraint"], (N, label, "python")
        cur, size = pos, N
        for d in range(layers - 1):
            cur = sharded.augmented_positions(cur, size)
            assert cur == want["augmented"][d], (N, label, d, "python")
            size //= 4
    assert collided["constraint"] >= 6 and all(c >= 4 for c in collided["layer"]), collided      # the sets do collide where they are meant to


def test_oracle_opens_and_verifies_at_given_positions(oracle):
    """The switch the directed tests stand on, on the oracle alone: `Prover.step(8, positions=...)` keeps seeds and nonce and opens where it
    is told, `verify(..., positions=...)` accepts exactly there; without the argument both do what they did"""
    O = oracle
    t = O.fibonacci_trace(128)
    op = O.Prover.from_trace(t, 1, ext=16, grinding=8)
    for k in range(1, 10):
        op.step(k)
    drawn, proof, seeds, nonce = op.get_u64("positions"), op.get_bytes("proof"), op.get_bytes("query_seeds"), op.get_u64("pow_nonce")
    check = lambda pr, positions=None: O.verify(pr, t.program_hash, t.public_inputs, op.outputs, positions=positions)      # noqa: E731
    assert len(drawn) == 50 and check(proof) == (True, "") and check(proof, drawn) == (True, "")
    S = [2047, 5, 4, 5 + 512, 1030]                                    # N = 2048: siblings, one FRI row, unsorted
    op.step(8, positions=S); op.step(9)
    at_s = op.get_bytes("proof")
    assert op.get_u64("positions") == S and op.get_bytes("query_seeds") == seeds and op.get_u64("pow_nonce") == nonce
    assert at_s != proof and check(at_s, S) == (True, "")
    assert check(at_s)[0] is False and check(at_s, drawn)[0] is False and check(proof, S)[0] is False and check(at_s, S[::-1])[0] is False
    assert check(at_s, [])[0] is False
    for bad in ([2048], [1 << 63], [7, 9, 7]):
        with pytest.raises(RuntimeError):
            op.step(8, positions=bad)
    assert op.get_u64("positions") == S                                # a refused list changes nothing
    with pytest.raises(RuntimeError):
        op.step(7, positions=S)
    op.step(8); op.step(9)
    assert op.get_u64("positions") == drawn and op.get_bytes("proof") == proof
    op.step(8, positions=[]); op.step(9)                               # no position: empty batch openings, a proof all the same
    assert op.get_u64("positions") == [] and len(op.get_bytes("proof")) < len(at_s)


def test_oracle_verifier_on_a_proof_without_layers(oracle):
    """A domain of 256 points is its own remainder: the proof carries no FRI layer, and the verifier takes the domain size from the
    remainder.  Only a 16-row table gives such a domain and no program fills one, so the table is not a valid trace: the verifier must
    say no in words, at the drawn positions and at given ones."""
    O = oracle
    rng = np.random.default_rng(16)
    cols = rng.integers(0, 2**62, size=(17, 16, 2), dtype=np.uint64)
    op = O.Prover(cols, 0, 0, [], [], ext=16, grinding=4)
    for k in range(1, 10):
        op.step(k)
    assert op.get_u64("fri_layers") == [1]
    for positions in (None, [1, 255, 130]):
        if positions is not None:
            op.step(8, positions=positions); op.step(9)
        ok, why = O.verify(op.get_bytes("proof"), bytes(32), [], [], positions=positions)
        assert not ok and why, positions
