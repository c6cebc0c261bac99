"""The stack constraints as one flat sum over basis terms (air_stack_nested.h: st_output_basis, class sums formed once per point) on the
GPU, against the oracle.

Traces of 256 rows, the smallest size the launch records use: two workgroups of 128 lanes per coset, eight cosets.  Per case the THREE
evaluation arrays of `dst_eval_constraints` (both boundary combinations and the transition combination; DISTAFF_BOUNDARY=eval writes the
first two as vectors) are compared with the oracle's element for element on all 8n points -- integer arithmetic, no tolerance:

  * valid traces: the depth-4 Fibonacci trace by shape (depth-4 set) and forced through the small and deep sets, the depth-8 program
    (small set), the depth-25 program with three context registers (deep set);
  * tables whose ten op-bit registers cycle through {0, 1, 2, p - 1, p - 2, 2^64, 2^127} (tests/test_air_flag_edge_values_gpu.py), one
    per product set: the class sums are sums of products of the flag tables, and on such rows -- and on the seven cosets where the
    bits are arbitrary elements anyway -- no table sums to one;
  * the verdict on the trace rows (air_check_kernel walks the same section functions): a valid trace proves to the oracle's proof with no
    failing step, and the same trace with ONE stack item changed is rejected at the step the oracle's evaluator names.

The oracle's share of a case is computed once, shared and never written."""
import functools

import numpy as np
import pytest

from test_air_arbitrary_rows import _first_failing_step, _valid_trace_of_256_rows
from test_air_flag_edge_values_gpu import _columns as _edge_columns

pytestmark = pytest.mark.gpu

N = 256
P = 2**128 - 45 * 2**40 + 1
LOG_BLOWUP = 5
NUM_OUTPUTS = {"sd4": 1, "small": 2, "deep": 4}
VECTORS = (("ceval_i", "i_evaluations"), ("ceval_f", "f_evaluations"), ("ceval_t", "t_evaluations"))
# case -> (trace family, DISTAFF_AIR)
VALID = {"fibonacci": ("sd4", ""), "fibonacci-small": ("sd4", "small"), "fibonacci-deep": ("sd4", "deep"), "depth8": ("small", ""), "depth25": ("deep", "")}
EDGE_SHAPES = {"sd4": (2, 1, 4), "small": (2, 1, 8), "deep": (3, 2, 12)}


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _valid(family):
    import oracle as O
    t = _valid_trace_of_256_rows(O, family)
    op = O.Prover.from_trace(t, NUM_OUTPUTS[family], ext=1 << LOG_BLOWUP, grinding=8)
    for k in range(1, 10):
        op.step(k)
    assert op.get_u64("constraints_ok") == [1]
    return t, op.outputs, _frozen(op.get("constraint_draws")), {o: _frozen(op.get(o)) for _, o in VECTORS}, op.get_bytes("roots"), op.get_bytes("proof")


@functools.lru_cache(maxsize=None)
def _edge(aset):
    import oracle as O
    cd, ld, sd = EDGE_SHAPES[aset]
    cols, inputs, outputs = _edge_columns(O, 15 + cd + ld + sd, 9000 + sd)
    op = O.Prover(cols, cd, ld, inputs, outputs, ext=1 << LOG_BLOWUP)
    for k in range(1, 6):
        op.step(k)
    assert op.get_u64("constraints_ok") == [0]
    draws = _frozen(op.get("constraint_draws"))
    bad = _first_failing_step(O, cols, cd, ld, sd, draws, inputs, outputs)
    assert 0 <= bad < N - 1
    return _frozen(cols), inputs, outputs, draws, {o: _frozen(op.get(o)) for _, o in VECTORS}, op.get_bytes("roots"), bad


def _switches(monkeypatch, instance, boundary):
    for k, v in (("DISTAFF_AIR", instance), ("DISTAFF_BOUNDARY", boundary)):
        if v:
            monkeypatch.setenv(k, v)                  # the library reads its switches when a context is created
        else:
            monkeypatch.delenv(k, raising=False)


def _compare(ctx, want):
    for name, oname in VECTORS:
        got = ctx.read_elements(name)
        assert got.shape[0] == 8 * N and got.shape == want[oname].shape, name
        assert (got == want[oname]).all(), "%s: first difference at point %d" % (name, int(np.argmax((got != want[oname]).any(axis=1))))


@pytest.mark.parametrize("case", list(VALID))
def test_valid_traces(oracle, monkeypatch, case):
    import distaff_amd as D
    family, instance = VALID[case]
    t, outputs, draws, want, roots, _ = _valid(family)
    _switches(monkeypatch, instance, "eval")
    ctx = D.Context(N.bit_length() - 1, t.width, t.ctx_depth, t.loop_depth, log_blowup=LOG_BLOWUP, grinding=8)
    ctx.upload(t.columns)
    assert ctx.commit_trace() == roots[:32]
    assert ctx.eval_constraints(t.public_inputs, outputs, draws) == roots[32:]
    assert ctx.bad_step == -1
    _compare(ctx, want)
    ctx.close()


@pytest.mark.parametrize("aset", list(EDGE_SHAPES))
def test_edge_values_in_the_op_bit_registers(oracle, monkeypatch, aset):
    import distaff_amd as D
    cd, ld, sd = EDGE_SHAPES[aset]
    cols, inputs, outputs, draws, want, roots, bad = _edge(aset)
    _switches(monkeypatch, "", "eval")
    ctx = D.Context(N.bit_length() - 1, 15 + cd + ld + sd, cd, ld, log_blowup=LOG_BLOWUP)
    ctx.upload(cols)
    assert ctx.commit_trace() == roots[:32]
    with pytest.raises(D.DistaffError) as e:
        ctx.eval_constraints(inputs, outputs, draws)
    assert e.value.code == D.DST_ERR_AIR
    assert ctx.bad_step == bad
    _compare(ctx, want)                                # both sides have written every evaluation by then (tests/test_air_arbitrary_rows.py)
    ctx.close()


@pytest.mark.parametrize("family", ["sd4", "small", "deep"])
def test_trace_row_verdict(oracle, monkeypatch, family):
    """a valid trace, then the same trace with one stack item (slot 1, 2 or 3: flat outputs of every set) changed in one row"""
    import distaff_amd as D
    t, outputs, draws, _, _, proof = _valid(family)
    _switches(monkeypatch, "", "")
    ctx = D.Context(N.bit_length() - 1, t.width, t.ctx_depth, t.loop_depth, log_blowup=LOG_BLOWUP, grinding=8)
    ctx.upload(t.columns)
    assert ctx.prove(t.public_inputs, outputs) == proof and ctx.bad_step == -1
    stack0 = 15 + t.ctx_depth + t.loop_depth
    # the first (row, slot) near row 131 (second workgroup) whose change the oracle's evaluator rejects at the step that has the row as
    # its NEXT row: not every operation constrains every slot of its next row (READ2 leaves slots 0 and 1 free)
    for row, slot in [(131 + d, s) for d in (0, 1, 2, 3) for s in (1, 2, 3)]:
        cols = np.array(t.columns, copy=True)
        cols[stack0 + slot, row, :] = oracle.to_arr([(oracle.to_ints(cols[stack0 + slot, row:row + 1, :])[0] + 1) % P])[0]
        bad = _first_failing_step(oracle, cols, t.ctx_depth, t.loop_depth, t.stack_depth, draws, t.public_inputs, outputs)
        if bad == row - 1:
            break
    assert bad == row - 1, (row, slot, bad)            # the fixture
    ctx.upload(cols)
    with pytest.raises(D.DistaffError) as e:
        ctx.prove(t.public_inputs, outputs)
    assert e.value.code == D.DST_ERR_AIR and ctx.bad_step == bad
    ctx.close()
