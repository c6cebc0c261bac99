"""tests/test_ctx_lifetime_gpu.py as a whole on the emulated build (tests/emu/_build/libdistaff_emu.so, see tests/test_emulated_kernels.py),
whose runtime counts what is live: the whole lives of every kind of context leave nothing behind, and a dst_ctx_create that fails at any one of
its acquisitions releases what it had made.  The second is checked here only -- no failure is provoked on a device."""
from test_emulated_kernels import _run, emulated_library  # noqa: F401  (the fixture builds the library)


def test_context_lifetimes_on_the_emulated_build(emulated_library):  # noqa: F811
    r = _run(emulated_library, ["tests/test_ctx_lifetime_gpu.py", "-s"])
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:]
    assert "12 passed" in out, out[-2000:]                                # 10 whole lives (6 kinds, 4 of them in two placements) + 2 worlds of the failing creation
    assert "skipped" not in out, out[-2000:]
