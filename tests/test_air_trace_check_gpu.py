"""The check of the trace rows (air_check_kernel) beside the proof: `dst_prove` no longer takes the verdict on the trace from the
constraint evaluation -- whose lanes on coset 0 now return at once -- but from a chain of launches of its own, which DISTAFF_AIR_CHECK
places on the main stream behind the evaluation (`inline`) or on the low-priority side stream: from the end of the trace commitment on
(`trace`), from the first FRI layer on (`fri`), from the proof of work on (`pow`) or from the openings on (`open`).

Traces of 256 rows: two workgroups of 128 lanes on coset 0, the smallest shape with a block boundary.  Every case runs for the depth-4,
small and deep instance sets (by the shape of the trace) and the per-operation set (`DISTAFF_AIR=generic` on the deep trace; its check is
the deep chain, see kernels_air.hip k_air_check), and for each of the five placements.

A "broken row k" is row k of a valid trace with its op counter raised by one.  Every register of a row is constrained both as the
current and as the next row of a step, so the steps k - 1 and k fail; the expected `bad_step` is what the oracle's evaluator finds
first on the un-extended rows (test_air_arbitrary_rows._first_failing_step), and the fixture asserts that this is max(k - 1, 0).  Rows
0, 127, 128, 129 and n - 2: the failing steps 0, 126, 127 (last lane of the first workgroup), 128 (first lane of the second) and n - 3.

One section alone (test_one_section_alone): a raised op counter is rejected by the op-bit launch, the first of every chain, so the
other launches are asked one at a time.  Row k + 1 is changed in ONE register that step k reads only as a value of its NEXT row and only
in one section (air_kernel.h): a sponge register (air_sponge; the current row's sponge[0] also enters the flow section, the next row's
does not), the context register (air_flow, at steps of a flow operation: under HACC nothing constrains it), stack slot 1 (the stack sections: the launch of the operation's group forms the difference,
the partial values carry it through the later launches, the last launch judges it -- NOOP steps of the depth-8 trace pass four
hand-overs; slot 0 is left alone because PUSH feeds it to the sponge) and, for the deep trace, slots 8 and sd - 1 (air_stack_deep_slots).
Step k + 1, which reads the register as a current value, may fail in other sections too; step k is the minimum and only the one launch
can have reported it.  The expected step is again the oracle evaluator's.

Row n - 1 broken alone: step n - 2 has it as its next row and fails; the step from row n - 1 to row 0 is not checked.  The parent
library (the evaluation kernel's own verdict on coset 0), run on the same table through DISTAFF_HIP_LIB, answered DST_ERR_AIR at step
n - 2 = 254 for all three traces; that is what is asserted here."""
import functools

import numpy as np
import pytest

from test_air_arbitrary_rows import _first_failing_step, _valid_trace_of_256_rows

pytestmark = pytest.mark.gpu

N = 256
P = 2**128 - 45 * 2**40 + 1
SETS = {"sd4": ("sd4", ""), "small": ("small", ""), "deep": ("deep", ""), "generic": ("deep", "generic")}     # set -> (trace family, DISTAFF_AIR)
NUM_OUTPUTS = {"sd4": 1, "small": 2, "deep": 4}
GOLDEN_KEY = {"sd4": "fibonacci-default", "small": "depth8-default", "deep": "depth25-default", "generic": "depth25-generic-default"}
PLACES = ["inline", "trace", "fri", "pow", "open"]
BOTH = pytest.mark.parametrize("aset,place", [(s, p) for s in SETS for p in PLACES], ids=lambda v: v)


@functools.lru_cache(maxsize=None)
def _family(family):
    """the valid trace of a family, the oracle's proof of it and its transition evaluations: computed once, shared, never written"""
    import oracle as O
    t = _valid_trace_of_256_rows(O, family)
    op = O.Prover.from_trace(t, NUM_OUTPUTS[family], grinding=8)
    for k in range(1, 10):
        op.step(k)
    t_ev = op.get("t_evaluations")
    t_ev.setflags(write=False)
    return t, op.outputs, op.get_bytes("proof"), t_ev, op.get("constraint_draws")


def _context(D, monkeypatch, aset, place, t):
    family, force = SETS[aset]
    if force:
        monkeypatch.setenv("DISTAFF_AIR", force)
    else:
        monkeypatch.delenv("DISTAFF_AIR", raising=False)
    monkeypatch.delenv("DISTAFF_BOUNDARY", raising=False)
    monkeypatch.setenv("DISTAFF_AIR_CHECK", place)         # the library reads its switches when a context is created
    return D.Context(N.bit_length() - 1, t.width, t.ctx_depth, t.loop_depth, grinding=8)


def _broken(O, t, outputs, draws, rows):
    """-> (columns with the op counter of every row of `rows` raised by one, the first failing step by the oracle's evaluator)"""
    cols = np.array(t.columns, copy=True)
    for k in rows:
        cols[0, k, :] = O.to_arr([O.to_ints(cols[0, k:k + 1, :])[0] + 1])[0]
    bad = _first_failing_step(O, cols, t.ctx_depth, t.loop_depth, t.stack_depth, draws, t.public_inputs, outputs)
    return cols, bad


def _expect_air_error(D, ctx, t, outputs, cols, bad):
    ctx.upload(cols)
    with pytest.raises(D.DistaffError) as e:
        ctx.prove(t.public_inputs, outputs)
    assert e.value.code == D.DST_ERR_AIR and e.value.reason == "transition constraints were not satisfied"
    assert ctx.bad_step == bad


@BOTH
def test_valid_trace(oracle, monkeypatch, aset, place):
    """the proof equals the oracle's; the transition evaluations equal the oracle's everywhere, which on coset 0 means zero at every row
    but the last"""
    import distaff_amd as D
    t, outputs, proof, t_ev, _ = _family(SETS[aset][0])
    ctx = _context(D, monkeypatch, aset, place, t)
    ctx.upload(t.columns)
    assert ctx.prove(t.public_inputs, outputs) == proof
    assert ctx.bad_step == -1
    got = ctx.read_elements("ceval_t")                      # natural order over the 8n domain: index 8 k + q
    assert (got == t_ev).all(), "ceval_t: first difference at index %d" % int(np.argmax((got != t_ev).any(axis=1)))
    assert not got[0:8 * (N - 1):8].any(), "coset 0: a row before the last is not zero"
    assert (got[8 * (N - 1)] == t_ev[8 * (N - 1)]).all() and t_ev[8 * (N - 1)].any(), "coset 0, last row"
    ctx.close()


@BOTH
def test_broken_rows(oracle, monkeypatch, aset, place):
    """one broken row at 0, 127, 128, 129, n - 2; two broken rows together; row n - 1 alone"""
    import distaff_amd as D
    t, outputs, _, _, draws = _family(SETS[aset][0])
    ctx = _context(D, monkeypatch, aset, place, t)
    for rows, step in [((0,), 0), ((127,), 126), ((128,), 127), ((129,), 128), ((N - 2,), N - 3), ((200, 129), 128), ((128, 40), 39), ((N - 1,), N - 2)]:
        cols, bad = _broken(oracle, t, outputs, draws, rows)
        assert bad == step, (rows, bad)                     # the fixture
        _expect_air_error(D, ctx, t, outputs, cols, bad)
    ctx.close()


def _sections(t):
    """-> {section: registers that enter only that section as values of a step's next row}"""
    stack0 = 15 + t.ctx_depth + t.loop_depth
    regs = {"sponge": [2, 4], "flow": [15], "stack": [stack0 + 1, stack0 + t.stack_depth - 1 if t.stack_depth <= 8 else stack0 + 7]}
    if t.stack_depth > 8:
        regs["deep slots"] = [stack0 + 8, stack0 + t.stack_depth - 1]
    return regs


@BOTH
def test_one_section_alone(oracle, monkeypatch, aset, place):
    """steps in both workgroups and on both sides of their boundary, under different operations, fail in one section only"""
    import distaff_amd as D
    t, outputs, _, _, draws = _family(SETS[aset][0])
    assert t.ctx_depth >= 1
    ctx = _context(D, monkeypatch, aset, place, t)
    # the context stack is constrained by the flow operations only (under HACC, flow_ops.rs asks nothing of it): the flow section is asked
    # at four of the steps whose cf bits are not all zero, the other sections at or within two steps of 40, 125, 130 and 200 (never across the
    # boundary between the workgroups at 127 | 128)
    flow_steps = [k for k in range(N - 1) if t.columns[5:8, k, 0].any()]
    flow_steps = sorted({flow_steps[i * (len(flow_steps) - 1) // 3] for i in range(4)})
    assert len(flow_steps) >= 3
    for section, registers in _sections(t).items():
        for i, k in enumerate(flow_steps if section == "flow" else (40, 125, 130, 200)):
            # the first step at or next to k, and the first of the section's registers (starting with another one every time), whose
            # change the oracle's evaluator rejects at exactly that step.  Not every step constrains every register of its next row:
            # READ2 leaves slots 0 and 1 free, and an operation whose low bits are 10 has no flag at all under HACC (lo2[2] is made
            # with cf bit 1, trace_state.rs:301), so its step asks nothing of the stack.
            rotated = registers[i % len(registers):] + registers[:i % len(registers)]
            for k, reg in [(k + dk, reg) for dk in (0, 1, -1, 2, -2) for reg in rotated]:
                cols = np.array(t.columns, copy=True)
                cols[reg, k + 1, :] = oracle.to_arr([(oracle.to_ints(cols[reg, k + 1:k + 2, :])[0] + 1) % P])[0]
                bad = _first_failing_step(oracle, cols, t.ctx_depth, t.loop_depth, t.stack_depth, draws, t.public_inputs, outputs)
                if bad == k:
                    break
            assert bad == k, (section, registers, k, bad)        # the fixture
            _expect_air_error(D, ctx, t, outputs, cols, bad)
    ctx.close()


@BOTH
def test_context_reuse(oracle, monkeypatch, aset, place):
    """an upload after a proof overwrites the trace buffer the check chain of that proof read: bad -> good, then good -> bad -> good on one
    context, every good proof equal to the oracle's"""
    import distaff_amd as D
    t, outputs, proof, _, draws = _family(SETS[aset][0])
    cols, bad = _broken(oracle, t, outputs, draws, (128,))
    ctx = _context(D, monkeypatch, aset, place, t)
    _expect_air_error(D, ctx, t, outputs, cols, bad)
    for _ in range(2):
        ctx.upload(t.columns)
        assert ctx.prove(t.public_inputs, outputs) == proof and ctx.bad_step == -1
        _expect_air_error(D, ctx, t, outputs, cols, bad)
    ctx.upload(t.columns)
    assert ctx.prove(t.public_inputs, outputs) == proof and ctx.bad_step == -1
    ctx.close()


@BOTH
def test_one_check_launch_per_evaluation_launch(oracle, monkeypatch, aset, place):
    """kernel statistics of one proof: the air_kernel<...> entries are those of tests/golden/air_launches.json, and every one of them has an
    air_check<...> launch with the same template arguments.  The per-operation set has no check chain of its own: the deep set's answers."""
    import json
    import os
    import distaff_amd as D
    t, outputs, proof, _, _ = _family(SETS[aset][0])
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "air_launches.json")))
    ctx = _context(D, monkeypatch, aset, place, t)
    ctx.upload(t.columns)
    ctx.set_profiling(1)
    ctx.kernel_stats(reset=True)
    assert ctx.prove(t.public_inputs, outputs) == proof
    stats = ctx.kernel_stats()
    ctx.close()
    evals = {name: [st["launches"], st["bytes"]] for name, st in stats.items() if name.startswith("air_kernel<")}
    assert evals == golden[GOLDEN_KEY[aset]]
    checks = {name: st["launches"] for name, st in stats.items() if name.startswith("air_check")}
    twins = golden["depth25-default"] if aset == "generic" else evals
    assert checks == {name.replace("air_kernel<", "air_check<"): v[0] for name, v in twins.items()}
    assert all(st["ms"] >= 0 for st in stats.values())
