"""The decisions of the transform launch layer (distaff_amd/csrc/kernels_ntt.hip: ntt_plan_derive, ntt_select, ntt_run_pass), made observable
by dst_ntt_describe and pinned to what they were before the layer was rewritten.

tests/golden/ntt_launches.json holds, for every case of the matrix below, the lines dst_ntt_describe prints: one per kernel launch of the
transform, with the profiling name, the kernel family and instance, block, grid, dynamic LDS bytes, first-pass mode, pre-stage, tile shape,
tiles per workgroup, block order, the 1/n flag and the algorithmic bytes and multiply-adds.  The file was recorded from the launch layer as it
was BEFORE this description existed (an instrumented copy that logged these fields at every branch of its instance ladder instead of launching),
so a line that differs is a launch that changed.  `dit` and `has_scale` are recorded as the kernels see them: 0 where the pass does not read the
field.  The cases are not stored in the file; the test builds them and the file only answers, so a case cannot be dropped by editing the data."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ntt_launches.json")
SWITCHES = ("DISTAFF_NTT", "DISTAFF_NTT_SHAPE", "DISTAFF_NTT_WAVES", "DISTAFF_NTT_FIXED", "DISTAFF_NTT_DIF", "DISTAFF_NTT_ORDER", "DISTAFF_NTT_DEBUG")


def shapes(log_blowup):
    """(cosets, cols, inverse, lde, skip) of every transform the prover's callers launch"""
    B = 1 << log_blowup
    return [(1, 1, 1, 0, 0), (1, 4, 1, 0, 0), (1, 20, 1, 0, 0),                  # interpolation
            (B - 1, 4, 0, 1, 1), (B - 1, 20, 0, 1, 1), (B // 8, 20, 0, 1, 0),    # extension: all cosets but the trace's own; a rank's eighth
            (B, 1, 0, 0, 0),                                                     # the folded 8n-coefficient extension
            (8, 1, 1, 0, 0),                                                     # the eight evaluation cosets, inverted
            (1, 1, 1, 0, 0)]                                                     # a rank's local cosets


def matrix():
    """[(switches, log_n, log_blowup)]: the default plan at every size, then every switch value at the sizes where the suite sets it, then
    two values the plan ignores at their size"""
    cases = [({}, log_n, log_b) for log_n in range(4, 25) for log_b in (4, 5, 8)]
    forced = [({"DISTAFF_NTT": "pre"}, (10, 13, 16, 20, 22)),
              ({"DISTAFF_NTT": "3pass"}, (12, 13, 15, 20, 21, 22)),
              ({"DISTAFF_NTT": "reg"}, range(13, 25)),
              ({"DISTAFF_NTT": "lds"}, (13, 16, 19, 22)),
              ({"DISTAFF_NTT": "3pass", "DISTAFF_NTT_SHAPE": "5,4"}, (13,)),
              ({"DISTAFF_NTT_WAVES": "4"}, (13, 16, 20)), ({"DISTAFF_NTT_WAVES": "8"}, (13, 16, 20)),
              ({"DISTAFF_NTT_FIXED": "0"}, (16, 20, 21)),
              ({"DISTAFF_NTT_DIF": "0"}, (13, 16, 20, 21)), ({"DISTAFF_NTT_DIF": "1"}, (13, 16, 20, 21)), ({"DISTAFF_NTT_DIF": "2"}, (13, 16, 20, 21)),
              ({"DISTAFF_NTT_ORDER": "0"}, (16, 20)),
              ({"DISTAFF_NTT": "pre"}, (8,)), ({"DISTAFF_NTT": "3pass"}, (10,))]       # ignored at these sizes
    return cases + [(sw, log_n, 5) for sw, sizes in forced for log_n in sizes]


def case_key(switches, log_n, log_b, shape):
    return "%s|%d|%d|%s" % (",".join("%s=%s" % kv for kv in sorted(switches.items())), log_n, log_b, ",".join(map(str, shape)))


def describe_all(cases):
    """{case key: [lines]} from the library this process binds; the switches are read from the environment by every call"""
    import distaff_amd as D
    out = {}
    for switches, log_n, log_b in cases:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(switches)
        for shape in shapes(log_b):
            cosets, cols, inverse, lde, skip = shape
            out[case_key(switches, log_n, log_b, shape)] = D.ntt_describe(log_n, log_b, inverse, lde, cosets, cols, skip)
    for k in SWITCHES:
        os.environ.pop(k, None)
    return out


def golden():
    g = json.load(open(GOLDEN))
    return {key: [g["lines"][i] for i in idx] for key, idx in g["cases"].items()}


def compare(got, cases):
    want = golden()
    keys = [case_key(sw, log_n, log_b, shape) for sw, log_n, log_b in cases for shape in shapes(log_b)]
    missing = [k for k in keys if k not in want]
    assert not missing, "cases without a recorded answer: %s" % missing[:5]
    wrong = [(k, want[k], got[k]) for k in keys if got[k] != want[k]]
    assert not wrong, "%d of %d transforms launch differently, first: %s\nrecorded: %s\nnow:      %s" % ((len(wrong), len(keys)) + wrong[0])
    assert all(2 <= len(got[k]) <= 3 for k in keys)


WORKER = r'''
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_ntt_launch_plan as T
json.dump(T.describe_all(T.matrix()), open(sys.argv[1], "w"))
'''


def test_every_transform_launches_what_it_launched_before(tmp_path):
    """The whole matrix against the emulated build, in a subprocess (the library is chosen when the package is imported): every size 2^4 .. 2^24
    at blowup 16, 32 and 256 under the default switches, each DISTAFF_NTT_* value where the suite uses it, and two values that are ignored."""
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-C", emu_dir, "-j8"], stdout=subprocess.DEVNULL)
    script, result = tmp_path / "describe_worker.py", tmp_path / "described.json"
    script.write_text(WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    env = dict(os.environ, DISTAFF_HIP_LIB=os.path.join(emu_dir, "_build", "libdistaff_emu.so"), DISTAFF_HIP_RUNTIME="none")
    r = subprocess.run([sys.executable, str(script), str(result)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    compare(json.load(open(result)), matrix())


@pytest.mark.gpu
def test_gpu_build_derives_the_same_plan():
    """The test build for gfx950 describes 2^10 and 2^20 as the emulated build does: same plan, same instances.  No device memory is touched."""
    cases = [({}, log_n, log_b) for log_n in (10, 20) for log_b in (4, 5, 8)]
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    try:
        compare(describe_all(cases), cases)
    finally:
        os.environ.update(saved)
