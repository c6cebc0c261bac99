"""The constraint kernels with edge values in the op-bit registers: each of the three product instance sets (depth-4, small, deep)
on a 256-row table, the whole 8n evaluation domain, bit for bit against the oracle.

The kernels form their flag tables by subtraction from one product per table and take the bit products of the op-bit constraints from
the flags (air_kernel.h: air_op_flags, air_op_bits), so the rare carry and borrow paths of the device subtraction decide the result.
The ten op-bit registers (cf 0..2, ld 0..4, hd 0..1) cycle through {0, 1, 2, p - 1, p - 2, 2^64, 2^127} with pairwise coprime periods:
on the trace coset the kernels see exactly these values, and the registers that a product pairs -- (ld0, ld1), (ld0, cf1), (ld2, ld3),
(cf0, cf1) -- have the short periods, so every pair of edge values meets within the 256 rows.  On the seven other cosets the bits are
arbitrary elements.  Every other register is uniform below p.  Such a table is no valid trace: both sides record the first failing
step and have written every evaluation by then (tests/test_air_arbitrary_rows.py)."""
import random
from math import gcd

import pytest

P = 2**128 - 45 * 2**40 + 1
EDGE = [0, 1, 2, P - 1, P - 2, 2**64, 2**127]
# register (column of the table) -> period of its cycle through EDGE; every period is at least len(EDGE), so a register takes every value
PERIODS = {8: 7, 6: 8, 9: 9,            # ld0, cf1, ld1
           10: 11, 11: 13,              # ld2, ld3
           5: 17, 13: 19, 14: 23,       # cf0, hd0, hd1
           7: 25, 12: 29}               # cf2, ld4
N = 256


def _columns(O, W, seed):
    rnd = random.Random(seed)
    cols = [[rnd.randrange(P) for _ in range(N)] for _ in range(W)]
    for c, q in PERIODS.items():
        cols[c] = [EDGE[(k % q) % len(EDGE)] for k in range(N)]
    public = [rnd.randrange(P) for _ in range(16)]
    return O.to_arr(cols), public[:8], public[8:]


def test_the_periods_are_pairwise_coprime_and_cover_the_op_bit_registers():
    q = sorted(PERIODS.values())
    assert sorted(PERIODS) == list(range(5, 15)) and min(q) >= len(EDGE)
    assert all(gcd(a, b) == 1 for i, a in enumerate(q) for b in q[i + 1:])
    for a, b in ((8, 9), (8, 6), (10, 11), (5, 6)):                      # the pairs of one product: every pair of edge values within N rows
        seen = {((k % PERIODS[a]) % 7, (k % PERIODS[b]) % 7) for k in range(N)}
        assert len(seen) == 49, (a, b)


# (context, loop, stack depth) -> the instance set the shape selects
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 1, 4), (2, 1, 8), (3, 2, 12)], ids=["sd4", "small", "deep"])
def test_edge_values_in_the_op_bit_registers(oracle, monkeypatch, shape):
    import distaff_amd as D
    from test_air_arbitrary_rows import _first_failing_step
    O = oracle
    cd, ld, sd = shape
    W, log_blowup = 15 + cd + ld + sd, 5
    cols, inputs, outputs = _columns(O, W, 7000 + sd)

    op = O.Prover(cols, cd, ld, inputs, outputs, ext=1 << log_blowup)
    for k in range(1, 6):
        op.step(k)
    assert op.get_u64("constraints_ok") == [0]
    draws = op.get("constraint_draws")
    t_ev = op.get("t_evaluations")
    assert t_ev.shape[0] == 8 * N
    expected_bad = _first_failing_step(O, cols, cd, ld, sd, draws, inputs, outputs)
    assert 0 <= expected_bad < N - 1

    monkeypatch.delenv("DISTAFF_AIR", raising=False)
    monkeypatch.delenv("DISTAFF_BOUNDARY", raising=False)
    ctx = D.Context(N.bit_length() - 1, W, cd, ld, log_blowup=log_blowup)
    ctx.upload(cols)
    assert ctx.commit_trace() == op.get_bytes("roots")[:32]
    with pytest.raises(D.DistaffError) as e:
        ctx.eval_constraints(inputs, outputs, draws)
    assert e.value.code == D.DST_ERR_AIR
    got_t = ctx.read_elements("ceval_t")
    bad_step = ctx.bad_step
    ctx.close()
    assert bad_step == expected_bad
    assert (got_t == t_ev).all(), "ceval_t: first difference at step %d" % int((got_t != t_ev).any(axis=1).argmax())
