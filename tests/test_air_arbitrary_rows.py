"""The constraint kernels on ARBITRARY rows: uniform random columns (no register is a zero, a constant or a copy of another one, so no
term of the evaluation and no boundary / transition coefficient is multiplied by a vanishing extension) at every kernel instance and at
the shapes where the instances meet, up to the widest table `dst_ctx_create` accepts (16 context, 8 loop, 32 stack registers).

Such a table is not a valid trace: the oracle records `constraints_ok = 0` instead of throwing, the library returns DST_ERR_AIR -- and
both have written every evaluation by then, so the vectors are compared bit for bit (integer arithmetic, no tolerance):

  * default route: `ceval_t`, and what was queued behind the evaluation before the verdict was read: `cpoly`, `cevals`, `cnodes[1:]`;
  * DISTAFF_BOUNDARY=eval: `ceval_i`, `ceval_f`, `ceval_t`.  That route waits for the verdict before it combines, so `cpoly`, `cevals`
    and `cnodes` are NOT defined after its DST_ERR_AIR and are not read ("After DST_ERR_AIR").

`bad_step` must be the first trace step at which the oracle's evaluator (O.evaluate_at on the un-extended rows) says that the
transition constraints do not vanish.

Cost of the oracle's share (steps 1 - 5 plus the scan for the first failing step) at (16, 8, 32), n = 256, blowup 32, measured on a
CPU: 0.33 s (inputs 0.03 s, steps 1 - 5 0.30 s, the scan 0.002 s) -- a fraction of a second per case, so no case is cut to n = 128."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 2**128 - 45 * 2**40 + 1
EDGE = [0, 1, P - 1, 2**64, P - 2**40]


def _arbitrary_columns(O, W, n, seed, prefix=None, keep=0):
    """[W, n, 2] words: rows [0, keep) from `prefix` (a valid trace of the same shape), every other row uniform below p; two of the
    arbitrary rows hold the edge values (each value in every fifth register, shifted by two between the rows)"""
    rnd = random.Random(seed)
    cols = O.to_arr([[rnd.randrange(P) for _ in range(n)] for _ in range(W)])
    for row, shift in ((keep + 1, 0), (n - 1, 2)):
        cols[:, row, :] = O.to_arr([EDGE[(c + shift) % 5] for c in range(W)])
    if keep:
        cols[:, :keep, :] = prefix[:, :keep, :]
    public = [rnd.randrange(P) for _ in range(16)]
    return cols, public[:8], public[8:]


def _first_failing_step(O, cols, cd, ld, sd, draws, inputs, outputs):
    """the first step k < n - 1 of the un-extended table at which the oracle's evaluator reports non-vanishing transition constraints"""
    n = cols.shape[1]
    last = O.to_ints(cols[:, n - 1, :])
    g = O.root_of_unity(n)
    x, nxt = 1, O.to_ints(cols[:, 0, :])
    for k in range(n - 1):
        cur, nxt = nxt, O.to_ints(cols[:, k + 1, :])
        if not O.evaluate_at(n, cd, ld, sd, draws, last[1:3], last[0], inputs, outputs, 8 * k, x, cur, nxt)[3]:
            return k
        x = x * g % P
    return -1


def _check_arbitrary_rows(O, D, monkeypatch, cd, ld, sd, n, log_blowup, instance, prefix=None, keep=0, seed=None):
    W, B = 15 + cd + ld + sd, 1 << log_blowup
    cols, inputs, outputs = _arbitrary_columns(O, W, n, seed if seed is not None else 1000 * cd + 100 * ld + sd, prefix, keep)

    # ---- oracle ----
    op = O.Prover(cols, cd, ld, inputs, outputs, ext=B)
    for k in range(1, 6):
        op.step(k)
    assert op.get_u64("constraints_ok") == [0]
    draws = op.get("constraint_draws")
    t_ev = op.get("t_evaluations")
    off_trace = np.arange(8 * n) % 8 != 0
    assert t_ev[off_trace].any(axis=1).all(), "an off-trace transition evaluation of the oracle is zero: a kernel that writes zeros could pass"
    expected_bad = _first_failing_step(O, cols, cd, ld, sd, draws, inputs, outputs)
    assert expected_bad == (keep - 1 if keep else 0)       # the fixture: the arbitrary rows start failing where they begin

    # ---- library: default route, then boundary constraints by evaluation ----
    if instance:
        monkeypatch.setenv("DISTAFF_AIR", instance)
    log_n = n.bit_length() - 1
    for boundary in ("", "eval"):
        if boundary:
            monkeypatch.setenv("DISTAFF_BOUNDARY", boundary)
        else:
            monkeypatch.delenv("DISTAFF_BOUNDARY", raising=False)
        ctx = D.Context(log_n, W, cd, ld, log_blowup=log_blowup)
        ctx.upload(cols)
        assert ctx.commit_trace() == op.get_bytes("roots")[:32]
        with pytest.raises(D.DistaffError) as e:
            ctx.eval_constraints(inputs, outputs, draws)
        assert e.value.code == D.DST_ERR_AIR
        assert ctx.bad_step == expected_bad
        got_t = ctx.read_elements("ceval_t")
        assert (got_t == t_ev).all(), "ceval_t: first difference at step %d" % int(np.argmax((got_t != t_ev).any(axis=1)))
        if boundary:
            assert (ctx.read_elements("ceval_i") == op.get("i_evaluations")).all(), "ceval_i"
            assert (ctx.read_elements("ceval_f") == op.get("f_evaluations")).all(), "ceval_f"
        else:
            assert (ctx.read_elements("cpoly") == op.get("constraint_poly")).all(), "constraint poly"
            assert (ctx.read_elements("cevals") == op.get("constraint_evaluations")).all(), "constraint evaluations"
            assert ctx.read("cnodes").tobytes()[32:] == op.get_bytes("constraint_nodes")[32:], "constraint nodes"
        ctx.close()


# (ctx, loop, stack, n, log_blowup, forced instance).  n = 256 at blowup 32: two workgroups of AIR_THREADS = 128 lanes per coset,
# evaluation cosets 4 extension cosets apart; blowup 16: 2 apart; n = 16: one partial workgroup.
_BY_SHAPE = [(0, 0, 4), (1, 0, 4), (2, 1, 4),                                         # sd4
             (0, 0, 5), (1, 1, 7), (2, 1, 8),                                         # small
             (3, 0, 4), (2, 2, 8), (0, 0, 9), (5, 8, 12), (16, 0, 31), (16, 8, 32)]   # deep: by context, loop, stack depth; the widest
CASES = [s + (256, 5, "") for s in _BY_SHAPE]
CASES += [(2, 1, 4, 256, 5, i) for i in ("small", "deep", "generic")] + [(2, 1, 8, 256, 5, i) for i in ("small", "deep", "generic")]
CASES += [(16, 8, 32, 256, 5, i) for i in ("deep", "generic")]
CASES += [(2, 1, 8, 256, 4, ""), (16, 8, 32, 256, 4, ""), (0, 0, 4, 16, 5, "")]


def _case_id(c):
    return "c%d-l%d-s%d-n%d-b%d%s" % (c[0], c[1], c[2], c[3], 1 << c[4], "-" + c[5] if c[5] else "")


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_uniform_random_rows(oracle, monkeypatch, case):
    """every instance (sd4, small, deep by shape; small, deep, generic forced) and every boundary between them on uniform rows"""
    import distaff_amd as D
    cd, ld, sd, n, log_blowup, instance = case
    _check_arbitrary_rows(oracle, D, monkeypatch, cd, ld, sd, n, log_blowup, instance)


def _valid_trace_of_256_rows(O, family):
    """a valid 256-row trace of the instance family's shape: the Fibonacci trace (stack depth 4), a depth-8 program lengthened by `noop`s,
    and the depth-25 program with three context registers of tests/test_gpu_parity.py (DEEP_PROGRAMS[1]), which the VM pads to 256 rows"""
    if family == "sd4":
        t = O.fibonacci_trace(256)
    elif family == "small":
        t = O.Trace("begin dup.4 add mul swap.2 add drop drop block push.9 mul end " + "noop " * 130 + "end", [1, 2, 3, 4])
    else:
        from test_gpu_parity import DEEP_PROGRAMS
        t = O.Trace(DEEP_PROGRAMS[1][0], DEEP_PROGRAMS[1][1])
    assert t.length == 256, t.length
    return t


@pytest.mark.parametrize("keep", [128, 201])
@pytest.mark.parametrize("family", ["sd4", "small", "deep", "generic"])
def test_valid_prefix_then_random_rows(oracle, monkeypatch, family, keep):
    """Rows 0 .. k of a valid trace (k = 127: the last lane of the first workgroup, k = 200: inside the second), uniform rows behind
    them: every step from k on fails, in both workgroups of coset 0 and in every launch of the instance, and `bad_step` is their minimum k."""
    import distaff_amd as D
    t = _valid_trace_of_256_rows(oracle, "deep" if family == "generic" else family)
    assert {"sd4": t.stack_depth == 4 and t.ctx_depth <= 2, "small": 4 < t.stack_depth <= 8 and t.ctx_depth <= 2,
            "deep": t.stack_depth > 8, "generic": t.stack_depth > 8}[family]
    _check_arbitrary_rows(oracle, D, monkeypatch, t.ctx_depth, t.loop_depth, t.stack_depth, 256, 5, "generic" if family == "generic" else "",
                          prefix=t.columns, keep=keep, seed=keep)
