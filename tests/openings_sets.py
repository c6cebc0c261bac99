"""Directed query-position sets for the opening tests (tests/test_openings_plan_host.py, tests/test_openings_directed_gpu.py).

The prover draws ~50 uniform positions in a domain of 2^11 or more; such a draw almost never holds two siblings of a tree, two positions
of one constraint leaf, positions that fall into one FRI row, a fully covered subtree, or a lone position (every level of every tree then
supplies exactly one sibling, the top levels included).  The sets below are built from the domain size N, the blowup B and the trace
length n = N / B by formula; R = N / 4 is the row count of FRI layer 0.  Order is part of a set: `values` of a batch proof follow input
order while its node lists follow sorted order."""
import numpy as np

FAMILIES = ("singles", "siblings", "constraint", "fri", "subtrees", "everything", "random")


def position_sets(N, B):
    """-> [(family, label, [positions])], labels unique.  Every position is below N, no set repeats a position."""
    n, R = N // B, N // 4
    out = []

    def add(family, label, positions):
        positions = [int(p) for p in positions]
        assert positions and all(0 <= p < N for p in positions) and len(set(positions)) == len(positions), (label, N)
        assert label not in [l for _, l, _ in out]
        out.append((family, label, positions))

    # one position: every level of every tree supplies exactly one sibling
    add("singles", "p1", [1]); add("singles", "last", [N - 1]); add("singles", "half+1", [N // 2 + 1])
    for j in range(1, B):
        add("singles", "coset%d" % j, [B * ((7 * j + 3) % n) + j])
    # siblings of the trace tree in both input orders (no leaf-level node), and neighbours that are not siblings
    for name, u in (("first", 0), ("middle", N // 4 + 1), ("last", N // 2 - 1)):
        add("siblings", "pair-%s" % name, [2 * u, 2 * u + 1])
        add("siblings", "riap-%s" % name, [2 * u + 1, 2 * u])
        w = min(u, N // 2 - 2)
        add("siblings", "neighbours-%s" % name, [2 * w + 1, 2 * w + 2])
    # two positions of one constraint leaf p / 2 around a third: the leaf is kept at its first appearance
    for name, u, v in (("first", 0, N // 4), ("middle", N // 4 + 1, 2), ("last", N // 2 - 1, N // 8 + 3)):
        add("constraint", "leaf-%s" % name, [2 * u + 1, 2 * u, 2 * v + 1])
        add("constraint", "leaf-%s-between" % name, [2 * u + 1, 2 * v + 1, 2 * u])
    # positions of one FRI row: in layer 0 (p, p + R, p + 2R, p + 3R), only in layer 1 (p, p + R / 4), only in layer 2 (p, p + R / 16)
    for name, p in (("low", 5), ("high", R - 3)):
        add("fri", "row-%s" % name, [p, p + R, p + 2 * R, p + 3 * R])
        add("fri", "row-%s-shuffled" % name, [p + 2 * R, p, p + 3 * R, p + R])
    add("fri", "layer1", [9, 9 + R // 4]); add("fri", "layer1-far", [9 + 3 * (R // 4) + 2 * R, 9])
    add("fri", "layer2", [11, 11 + R // 16])
    mixed = {5, 5 + R, 5 + 3 * R, 9, 9 + R // 4, 11 + R // 16 + R, 11, 3, N - 1}
    add("fri", "mixed-descending", sorted(mixed, reverse=True))
    # covered subtrees: a whole k-row (B positions: every coset, every rank), four of them, and a whole coset (every row from one owner)
    for name, a in (("first", 0), ("inner", n // 2 + 1), ("last", n - 1)):
        add("subtrees", "krow-%s" % name, range(a * B, (a + 1) * B))
    add("subtrees", "krows4", range((n // 4 - 1) * 4 * B, (n // 4) * 4 * B)); add("subtrees", "krows4-reversed", reversed(range(4 * B, 8 * B)))
    for j in (1, B // 2 + 1, B - 1):
        add("subtrees", "whole-coset%d" % j, [B * k + j for k in range(n)])
    add("subtrees", "whole-coset0", [B * k for k in range(n)])
    # everything off the trace domain (every trace-domain leaf is then supplied as a sibling), and everything
    add("everything", "off-trace", [p for p in range(N) if p % B])
    add("everything", "all", range(N))
    # a few seeded draws off the trace domain, in the order drawn
    rng = np.random.default_rng(N + B)
    off = np.array([p for p in range(N) if p % B])
    for count in (1, 2, 7, 128):
        add("random", "draw%d" % count, rng.choice(off, size=min(count, len(off)), replace=False))
    return out


def off_trace(positions, B):
    """no position on the trace domain (the multiples of B), where the prover's transition divisor vanishes"""
    return all(p % B for p in positions)


def tree_sets(L):
    """the same families over a bare tree of L leaves, for the plan of one batch proof: -> [(label, [indexes])]"""
    rng = np.random.default_rng(L)
    cand = [("empty", [])]
    cand += [("single-%d" % i, [i]) for i in sorted({0, 1, L // 2, L // 2 + 1, L - 2, L - 1} & set(range(L)))]
    for u in sorted({0, L // 4, L // 2 - 1}):
        cand += [("pair-%d" % u, [2 * u, 2 * u + 1]), ("riap-%d" % u, [2 * u + 1, 2 * u])]
        if 2 * u + 2 < L:
            cand += [("neighbours-%d" % u, [2 * u + 1, 2 * u + 2]), ("three-%d" % u, [2 * u + 1, 2 * u, 2 * u + 2]), ("three-apart-%d" % u, [2 * u + 1, L - 1 - (u == L // 2 - 1), 2 * u])]
    size = 4
    while size <= L:                                                       # covered subtrees of every size, first / inner / last
        for a in sorted({0, (L // size) // 2, L // size - 1}):
            span = list(range(a * size, (a + 1) * size))
            cand += [("subtree%d-%d" % (size, a), span), ("subtree%d-%d-reversed" % (size, a), span[::-1])]
            if size < L:
                cand.append(("subtree%d-%d-less-one" % (size, a), span[:-1]))
                cand.append(("subtree%d-%d-and-far" % (size, a), span + [(span[-1] + L // 2) % L]))
        size *= 4 if size >= 16 else 2
    if L >= 8:
        cand += [("evens", list(range(0, L, 2))), ("odds-descending", list(range(L - 1, 0, -2))), ("stride4", list(range(1, L, 4)))]
        for count in sorted({1, 2, 7, min(128, L // 2)}):
            cand.append(("draw%d" % count, [int(x) for x in rng.choice(L, size=count, replace=False)]))
    out, seen = [], set()
    for label, idx in cand:
        if all(0 <= i < L for i in idx) and len(set(idx)) == len(idx) and tuple(idx) not in seen:
            seen.add(tuple(idx)); out.append((label, idx))
    return out


def opened_bytes(positions, N, W, layer_sizes, plan_batch, augmented_positions, constraint_positions):
    """bytes of the items a proof at `positions` reads from the prover's buffers (everything but the template): tree nodes and leaves of
    32 bytes (a constraint leaf is its pair of evaluations), rows of W elements, constraint pairs, FRI rows of 4 elements, the remainder.
    `layer_sizes`: the sizes of all FRI layers, the remainder last."""
    def nodes(plan):
        return sum(len(lst) for lst in plan[1])
    total = 32 * nodes(plan_batch(list(positions), N)) + 16 * W * len(positions)
    cpos = constraint_positions(list(positions))
    total += 32 * len(cpos) + 32 * nodes(plan_batch(cpos, N // 2))
    pos = list(positions)
    for size in layer_sizes[:-1]:
        pos = augmented_positions(pos, size)
        total += 64 * len(pos) + 32 * nodes(plan_batch(pos, size // 4))
    return total + 16 * layer_sizes[-1]
