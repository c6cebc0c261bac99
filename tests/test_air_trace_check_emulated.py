"""tests/test_air_trace_check_gpu.py as a whole on the emulated build (tests/emu/_build/libdistaff_emu.so, see tests/test_emulated_kernels.py):
the check chains of every instance set -- air_check_kernel itself, through the launch layer -- against the oracle's evaluator on valid
traces, broken rows and reused contexts, and dst_prove's control flow for every placement of the chain.  Launches are synchronous there,
so what this does NOT show is the ordering between the two streams: that is the GPU run's business."""
import importlib.util
import os

from test_emulated_kernels import _run, emulated_library  # noqa: F401  (the fixture builds the library)


def test_trace_check_on_the_emulated_build(emulated_library):  # noqa: F811
    workers = ["-n", "4"] if importlib.util.find_spec("xdist") is not None and (os.cpu_count() or 1) >= 8 else []
    r = _run(emulated_library, ["tests/test_air_trace_check_gpu.py"] + workers)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:]
    assert "100 passed" in out, out[-2000:]                               # 5 tests x 4 instance sets x 5 placements
