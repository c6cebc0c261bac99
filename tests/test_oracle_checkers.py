"""The whole-array checkers of oracle/check.hpp -- what the whole-domain GPU tests compare the device with -- on the CPU: they accept
every intermediate of the oracle prover's own run, and they fail, naming the index, on one wrong element: +1 at the first, the last,
the (n-1)-th, a tile-aligned and a random index, two adjacent elements swapped, a value replaced by one >= p, one flipped byte in a
leaf or a node."""
import numpy as np
import pytest

P = 2**128 - 45 * 2**40 + 1


@pytest.fixture(scope="module", params=[8, 12])
def run(oracle, request):
    O = oracle
    log_n = request.param
    t = O.fibonacci_trace(1 << log_n)
    p = O.Prover.from_trace(t, 1, grinding=4)
    for k in range(1, 8):
        p.step(k)
    n, N = t.length, p.N
    layers = p.get_u64("fri_layers")[0]
    fri = [p.get("fri_values", d).transpose(1, 0, 2).reshape(-1, 2).copy() for d in range(layers)]     # natural order e[r + q R]
    return dict(O=O, t=t, p=p, n=n, N=N, W=t.width, polys=p.get("polys"), lde=p.get("registers"), cpoly=p.get("constraint_poly"),
                cevals=p.get("constraint_evaluations"), comp_poly=p.get("composition_poly"), comp=p.get("composed_evaluations"),
                fri=fri, xs=O.to_ints(p.get("fri_special_xs")), draws=p.get("deep_draws"))


def _set(a, i, v):
    a[i, 0] = v & (2**64 - 1)
    a[i, 1] = v >> 64


def _get(a, i):
    return int(a[i, 0]) | (int(a[i, 1]) << 64)


def _indices(size, n, rng):
    """first, last, n-1, a tile-aligned index (1024 or the middle), a random one"""
    return sorted({0, size - 1, n - 1, min(1024, size // 2), int(rng.integers(1, size - 1))})


def _mutations(arr, n, rng):
    """(copy with one wrong element, index it should be reported at)"""
    size = arr.shape[0]
    for i in _indices(size, n, rng):
        a = arr.copy(); _set(a, i, (_get(a, i) + 1) % P); yield a, i, "+1"
    i = int(rng.integers(1, size - 2))
    while _get(arr, i) == _get(arr, i + 1):
        i += 1
    a = arr.copy(); a[[i, i + 1]] = a[[i + 1, i]]; yield a, i, "swap"
    i = int(rng.integers(0, size))
    v = _get(arr, i)
    a = arr.copy(); _set(a, i, v + P if v + P < 2**128 else P + v % (2**128 - P)); yield a, i, ">= p"


def test_checker_identity_accepts_every_phase(run):
    O, n, W = run["O"], run["n"], run["W"]
    for c in range(W):
        assert O.check_evaluations(run["polys"][c], run["t"].columns[c], 11 + c) == (-1, ""), ("interpolation", c)
        assert O.check_evaluations(run["polys"][c], run["lde"][c], 97 + c) == (-1, ""), ("extension", c)
    assert O.check_evaluations(run["cpoly"], run["cevals"], 5) == (-1, "")
    assert O.check_evaluations(run["comp_poly"], run["comp"], 6) == (-1, "")
    # degree bounds: composition poly <= get_composition_degree = 7n - 1 (oracle/prover.hpp:46), constraint poly <= 7n (merge_into
    # divides c(x) - c(z) by x - z); both reach their bound, which is what the GPU tests assert on the device's coefficients
    assert not run["cpoly"][7 * n + 1:].any() and run["cpoly"][7 * n].any()
    assert not run["comp_poly"][7 * n:].any() and run["comp_poly"][7 * n - 1].any()


@pytest.mark.parametrize("which", ["interpolation", "extension", "constraints", "composition"])
def test_checker_identity_names_one_wrong_evaluation(run, which):
    O, n = run["O"], run["n"]
    coeffs, evals = {"interpolation": (run["polys"][3], run["t"].columns[3]), "extension": (run["polys"][17], run["lde"][17]),
                     "constraints": (run["cpoly"], run["cevals"]), "composition": (run["comp_poly"], run["comp"])}[which]
    rng = np.random.default_rng(n)
    for bad, i, how in _mutations(np.ascontiguousarray(evals), n, rng):
        idx, msg = O.check_evaluations(coeffs, bad, 12345)
        assert idx == i and str(i) in msg, (which, how, i, idx, msg)
    c = np.ascontiguousarray(coeffs).copy(); _set(c, 1, (_get(c, 1) + 1) % P)
    assert O.check_evaluations(c, evals, 12345)[0] >= 0, "a wrong coefficient"


def test_checker_identity_rejects_p_plus_k_where_k_belongs(run):
    """the trace holds 0 / 1 flags: p + v is the same residue as v, which only the range check notices"""
    O, n = run["O"], run["n"]
    col = np.ascontiguousarray(run["t"].columns[5]).copy()
    small = [k for k in range(n) if _get(col, k) < 2**128 - P]
    for k in (small[0], small[-1]):
        bad = col.copy(); _set(bad, k, _get(col, k) + P)
        idx, msg = O.check_evaluations(run["polys"][5], bad, 3)
        assert idx == k and "not below p" in msg
    assert O.check_noncanonical(col) == -1


def test_checker_merkle_trees(run):
    O, p, N = run["O"], run["p"], run["N"]
    leaves, nodes = p.get_bytes("trace_leaves"), p.get_bytes("trace_nodes")
    cleaves, cnodes = run["cevals"].tobytes(), p.get_bytes("constraint_nodes")        # constraint leaf j = evaluations 2j, 2j+1
    assert O.check_merkle(leaves, nodes) == (-1, "") and O.check_merkle(cleaves, cnodes) == (-1, "")
    rng = np.random.default_rng(N)
    for lv, nd in ((leaves, nodes), (cleaves, cnodes)):
        L = len(lv) // 32
        for k in sorted({1, 2, L // 2 - 1, L // 2, L - 1, int(rng.integers(2, L))}):
            bad = bytearray(nd); bad[32 * k + int(rng.integers(32))] ^= 1 << int(rng.integers(8))
            idx, msg = O.check_merkle(lv, bytes(bad))
            assert idx == k and str(k) in msg, (k, idx, msg)
        for j in (0, L - 1, int(rng.integers(L))):
            bad = bytearray(lv); bad[32 * j + 7] ^= 0x80
            assert O.check_merkle(bytes(bad), nd)[0] == L // 2 + j // 2, j


def test_checker_trace_leaves(run):
    O, p, N, W, n = run["O"], run["p"], run["N"], run["W"], run["n"]
    rows = np.ascontiguousarray(run["lde"].transpose(1, 0, 2))                    # [N, W, 2]
    leaves = p.get_bytes("trace_leaves")
    assert O.check_row_leaves(rows, leaves) == (-1, "")
    assert O.check_row_leaves(rows[1000 % N:], leaves[32 * (1000 % N):]) == (-1, "")           # a block that does not start at 0
    rng = np.random.default_rng(n + 1)
    for i in _indices(N, n, rng):
        bad = rows.copy(); c = int(rng.integers(W)); _set(bad[i], c, (_get(bad[i], c) + 1) % P)
        assert O.check_row_leaves(bad, leaves)[0] == i
        badl = bytearray(leaves); badl[32 * i + 31] ^= 1
        assert O.check_row_leaves(rows, bytes(badl))[0] == i
    bad = rows.copy(); bad[[4, 5]] = bad[[5, 4]]
    assert O.check_row_leaves(bad, leaves)[0] == 4
    bad = rows.copy(); _set(bad[9], 0, P + 1)
    idx, msg = O.check_row_leaves(bad, leaves)
    assert idx == 9 and "not below p" in msg


def test_checker_fri_fold_is_the_quartic_interpolation(oracle):
    """the checker's 4-point inverse DFT with running powers of g^-1 == quartic_interpolate_batch + quartic_evaluate_batch (quartic.rs)"""
    O = oracle
    rng = np.random.default_rng(4)
    for M in (16, 1024, 1 << 14):
        e = O.to_arr([int.from_bytes(rng.bytes(16), "little") % P for _ in range(M)])
        e[:4] = O.to_arr([0, 1, P - 1, P - 2])
        alpha = int.from_bytes(rng.bytes(16), "little") % P
        R = M // 4
        g = O.root_of_unity(M)
        xs = O.to_arr([[pow(g, r + q * R, P) for q in range(4)] for r in range(R)])
        ys = np.ascontiguousarray(e.reshape(4, R, 2).transpose(1, 0, 2))
        want = O.quartic_evaluate_batch(O.quartic_interpolate_batch(xs, ys), alpha)
        assert (O.fri_fold(e, alpha) == want).all(), M


def test_checker_fri_layers(run):
    O, p, n = run["O"], run["p"], run["n"]
    fri, xs = run["fri"], run["xs"]
    assert (fri[0] == run["comp"]).all()
    rng = np.random.default_rng(n + 2)
    for d, e in enumerate(fri):
        R = e.shape[0] // 4
        leaves = b"".join(O.blake3(e[[r, r + R, r + 2 * R, r + 3 * R]].tobytes()) for r in range(R))
        assert O.check_fri_leaves(e, leaves) == (-1, "") and O.check_merkle(leaves, p.get_bytes("fri_nodes", d)) == (-1, ""), d
        r = int(rng.integers(R))
        bad = e.copy(); _set(bad, r + 2 * R, (_get(bad, r + 2 * R) + 1) % P)
        assert O.check_fri_leaves(bad, leaves)[0] == r
        if d + 1 < len(fri):
            assert O.check_fri_fold(e, xs[d], fri[d + 1]) == (-1, ""), d
            for bad, i, how in _mutations(fri[d + 1], min(n, R), rng):
                idx, msg = O.check_fri_fold(e, xs[d], bad)
                assert idx == i and str(i) in msg, (d, how, i, idx, msg)
            bad = e.copy(); _set(bad, R + 1, (_get(bad, R + 1) + 1) % P)
            assert O.check_fri_fold(bad, xs[d], fri[d + 1])[0] == 1, d               # row 1 holds e[R + 1]
    assert fri[-1].shape[0] <= 256


def _deep(run):
    O, n = run["O"], run["n"]
    dr = O.to_ints(run["draws"])
    z, zg = dr[0], dr[0] * O.root_of_unity(n) % P
    z1 = O.to_arr([O.poly_eval_par(run["polys"][c], z) for c in range(run["W"])])
    z2 = O.to_arr([O.poly_eval_par(run["polys"][c], zg) for c in range(run["W"])])
    assert (z1 == run["p"].get("trace_at_z1")).all() and (z2 == run["p"].get("trace_at_z2")).all()      # pins poly_eval_par
    return z1, z2, O.poly_eval_par(run["cpoly"], z)


def test_checker_composition(run):
    O, n, N = run["O"], run["n"], run["N"]
    z1, z2, c_z = _deep(run)
    rows = np.ascontiguousarray(run["lde"].transpose(1, 0, 2))
    args = lambda r, cv, cp, s=0: O.check_composition(r, s, cv, cp, n, N, run["draws"], z1, z2, c_z)     # noqa: E731
    assert args(rows, run["cevals"], run["comp"]) == (-1, "")
    h = N // 2 + 3
    assert args(rows[h:], run["cevals"][h:], run["comp"][h:], h) == (-1, "")       # a block that does not start at 0
    rng = np.random.default_rng(n + 3)
    for bad, i, how in _mutations(run["comp"], n, rng):
        idx, msg = args(rows, run["cevals"], bad)
        assert idx == i and str(i) in msg, (how, i, idx, msg)
    i = int(rng.integers(N))
    bad = rows.copy(); _set(bad[i], 7, (_get(bad[i], 7) + 1) % P)
    assert args(bad, run["cevals"], run["comp"])[0] == i
    bad = run["cevals"].copy(); _set(bad, i, (_get(bad, i) + 1) % P)
    assert args(rows, bad, run["comp"])[0] == i


def _constraint_inputs(run, steps):
    O, t, n, N = run["O"], run["t"], run["n"], run["N"]
    B = N // n
    pos = np.asarray(steps, dtype=np.int64) * (B // 8)
    rows = run["lde"].transpose(1, 0, 2)
    cur, nxt = np.ascontiguousarray(rows[pos]), np.ascontiguousarray(rows[(pos + B) % N])
    col = lambda c: O.to_ints(t.columns[c, n - 1])                           # noqa: E731
    fixed = (n, t.ctx_depth, t.loop_depth, t.stack_depth, run["p"].get("constraint_draws"), [col(1), col(2)], col(0), t.public_inputs, run["p"].outputs)
    return fixed, cur, nxt, np.ascontiguousarray(run["p"].get("t_evaluations")[steps]), np.ascontiguousarray(run["cevals"][pos])


def test_checker_constraint_evaluation(run):
    O, n = run["O"], run["n"]
    steps = np.arange(8 * n) if n <= 256 else np.unique(np.r_[np.arange(2048), np.arange(8 * n - 2048, 8 * n), np.arange(4093, 4200)])
    fixed, cur, nxt, tv, cv = _constraint_inputs(run, steps)
    assert O.check_constraints(*fixed, steps, cur, nxt, tv, cv) == (-1, "")
    rng = np.random.default_rng(n + 4)
    for i in sorted({0, 1, 3, len(steps) - 1, int(rng.integers(len(steps)))}):
        bad = tv.copy(); _set(bad, i, (_get(bad, i) + 1) % P)
        idx, msg = O.check_constraints(*fixed, steps, cur, nxt, bad, cv)
        assert idx == i and "transition" in msg, (i, idx, msg)
        if steps[i] % 8:
            bad = cv.copy(); _set(bad, i, (_get(bad, i) + 1) % P)
            idx, msg = O.check_constraints(*fixed, steps, cur, nxt, tv, bad)
            assert idx == i and "constraint value" in msg, (i, idx, msg)
    bad = cur.copy(); _set(bad[8], 3, (_get(bad[8], 3) + 1) % P)              # step 8: a trace step, its constraints no longer vanish
    idx, msg = O.check_constraints(*fixed, steps, bad, nxt, tv, cv)
    assert idx == 8 and "does not vanish" in msg, msg
    bad = tv.copy(); _set(bad, 5, P + 2)
    assert O.check_constraints(*fixed, steps, cur, nxt, bad, cv)[0] == 5
