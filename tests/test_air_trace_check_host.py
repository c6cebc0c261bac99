"""The verdict of the check of the trace rows against the per-constraint evaluation, on the host: tests/emu/air_check_test.cpp calls
air_check_kernel row by row through the launch lists of the three product instance sets and compares its verdict with "some constraint is
non-zero", the constraints summed per index from the decoder sections and the per-operation statement of the stack constraints -- on
every step of valid traces, on valid traces with one register of one row replaced, and on rows of 0 / 1 op bits, of the edge values of
tests/emu/air_flags_test.cpp and of uniform values, up to the widest shape.  The periodic table and the valid traces come from the
oracle (a file the program reads); built like air_flags_test.cpp, with the emulated runtime linked for the launch layer's symbols."""
import os
import subprocess

import numpy as np

from test_air_arbitrary_rows import _valid_trace_of_256_rows


def test_check_verdict_equals_some_constraint_is_nonzero(oracle, tmp_path):
    emu = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    data = tmp_path / "rows.bin"
    with open(data, "wb") as fh:
        per = np.ascontiguousarray(oracle.periodic_tables(8), dtype=np.uint64)        # [128][23] elements: the cycle of 16 * 8 steps
        assert per.shape == (128, 23, 2)
        fh.write(per.tobytes())
        traces = [_valid_trace_of_256_rows(oracle, f) for f in ("sd4", "small", "deep")]
        fh.write(np.uint64(len(traces)).tobytes())
        for t in traces:
            cols = np.ascontiguousarray(t.columns, dtype=np.uint64)
            assert cols.shape == (t.width, 256, 2)
            fh.write(np.array([t.width, 256, t.ctx_depth, t.loop_depth, t.stack_depth], dtype=np.uint64).tobytes())
            fh.write(cols.tobytes())
    exe = tmp_path / "air_check_test"
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-pthread", "-I", emu, "-w", "-DFE_EMULATE_GFX950=1",
                           os.path.join(emu, "air_check_test.cpp"), os.path.join(emu, "emu_runtime.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(data)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert " 0 mismatches" in out, out
