"""The tile-major layout of the staging array between the two transform passes and of the four-step twiddle tables
(distaff_amd/csrc/kernels_ntt.hip, NttArgs::tile_major): two-pass plans whose tiles are four columns wide in both passes, and whose second
pass has no register pre-stage, keep element (k1, m2) at (((m2 >> 2) * n1) + k1) * 4 + (m2 & 3).  Neither array is visible from outside, so the layout is pinned through what it
carries: the coefficients (`polys`: inverse transform, DIF first pass, bit-reversed scatter inside a tile's block) and every register of
the extension (`lde`: coset DIT first pass, the block is the tile as it lies in LDS) against the oracle's transforms, element for
element -- at the smallest shapes where the indexing can go wrong, under every switch that selects another instance or another first
pass, and through the inverse transform of the eight evaluation cosets and the 8n-coefficient extension of a proof.

The library accepts extension factors 16 .. 256 and 16 registers or more: "the smallest blowup" is 16, and the register counts are
16 + 1, 16 + 3 and 16 + 5, so that the last chunk of four registers of the first pass's block order holds one, three and one register
behind a whole chunk.

The cases are marked `gpu`; test_tile_major_cases_on_the_emulated_build runs them (all but the 2^20 / 2^21 ones) on the host-emulated build, where
there is no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTT_SWITCHES = ("DISTAFF_NTT", "DISTAFF_NTT_DIF", "DISTAFF_NTT_WAVES", "DISTAFF_NTT_ORDER", "DISTAFF_NTT_FIXED", "DISTAFF_NTT_SHAPE", "DISTAFF_LDE_BATCH")
P_LO = 2**64 - 45 * 2**40 + 1                     # low limb of the modulus; its high limb is 2^64 - 1

_REFERENCE = {}


def _reference(O, log_n, W, log_blowup):
    """-> (columns [W, n, 2], the oracle's coefficients [W, n, 2], the oracle's extension [W, N, 2] in natural order); computed once per
    shape and shared by every case that runs on it"""
    key = (log_n, W)
    n = 1 << log_n
    if key not in _REFERENCE:
        rng = np.random.default_rng(500 + 64 * log_n + W)
        cols = rng.integers(0, 2**64, size=(W, n, 2), dtype=np.uint64, endpoint=False)
        over = (cols[..., 1] == np.uint64(2**64 - 1)) & (cols[..., 0] >= np.uint64(P_LO))
        cols[..., 0][over] -= np.uint64(P_LO)
        cols[:, 0] = np.array([0, 0], dtype=np.uint64)                       # 0 and p - 1 at the corners of the first and the last tile
        cols[:, n - 1] = np.array([P_LO - 1, 2**64 - 1], dtype=np.uint64)
        polys = np.stack([O.fft_interpolate(cols[c]) for c in range(W)])
        _REFERENCE[key] = {"cols": cols, "polys": polys, "lde": {}}
    ref = _REFERENCE[key]
    if log_blowup not in ref["lde"]:
        N = n << log_blowup
        padded = np.zeros((N, 2), dtype=np.uint64)
        out = []
        for c in range(W):
            padded[:n] = ref["polys"][c]
            out.append(O.fft_eval(padded))
        ref["lde"][log_blowup] = np.stack(out)
    for a in (ref["cols"], ref["polys"], ref["lde"][log_blowup]):
        a.setflags(write=False)
    return ref["cols"], ref["polys"], ref["lde"][log_blowup]


def _transforms_equal_the_oracle(O, monkeypatch, log_n, log_blowup, W, switches=None):
    import distaff_amd as D
    for k in NTT_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (switches or {}).items():
        monkeypatch.setenv(k, v)
    n, B = 1 << log_n, 1 << log_blowup
    cols, polys, lde = _reference(O, log_n, W, log_blowup)
    ctx = D.Context(log_n, W, 0, 0, log_blowup=log_blowup)
    try:
        ctx.upload(cols)
        ctx.commit_trace()
        got = ctx.read_elements("polys").reshape(W, n, 2)
        assert (got == polys).all(), ("polys", np.argwhere((got != polys).any(axis=2))[:4].tolist())
        for c in range(W):
            got = ctx.read_elements("lde", c)
            assert got.shape == (n * B, 2)
            assert (got == lde[c]).all(), ("lde register", c, np.argwhere((got != lde[c]).any(axis=1))[:4].ravel().tolist())
    finally:
        ctx.close()


# log n = 4: n1 = n2 = 4, one tile group, a tile is the whole array; 5 and 7: n1 = 2 n2; 6; 12 and 13: several tiles per workgroup and
# (13) n1 != n2 with 64-row runs 2 KiB apart
@pytest.mark.gpu
@pytest.mark.parametrize("W", [17, 19, 21])
@pytest.mark.parametrize("log_blowup", [4, 5])
@pytest.mark.parametrize("log_n", [4, 5, 6, 7, 12, 13])
def test_default_plan_equals_the_oracle(oracle, monkeypatch, log_n, log_blowup, W):
    _transforms_equal_the_oracle(oracle, monkeypatch, log_n, log_blowup, W)


# pre: a register pre-stage in front of both passes -- such a plan stays row-major, the pre-stage instances must still be right; pre_a: a
# pre-stage in the first pass alone, as 2^21 has by itself -- tile-major with the frequencies 2 k' + h inside a block of twice the LDS tile;
# row: the default plan on the row-major layout (what the instances that read the flag do for a plan such as DISTAFF_NTT=lds at 2^21);
# DISTAFF_NTT_DIF = 1: pre-scale + DIF as the first pass of the extension as well (the interpolation always has one), 0 / 2: the coset
# DIT with its whole table in LDS / with the last stage's pairs in global memory; waves 4 / 8: the 512-lane prefetching instances and the
# 1024-lane ones; 3pass: the three-pass plan keeps the row-major layout; order0 / lde batch: other block orders and coset counts per launch
SWITCHED = [("pre", 10, {"DISTAFF_NTT": "pre"}), ("pre", 13, {"DISTAFF_NTT": "pre"}),
            ("pre_a", 10, {"DISTAFF_NTT": "pre_a"}), ("pre_a", 13, {"DISTAFF_NTT": "pre_a"}),
            ("row", 12, {"DISTAFF_NTT": "row"}), ("row", 13, {"DISTAFF_NTT": "row"}),
            ("dif0", 12, {"DISTAFF_NTT_DIF": "0"}), ("dif1", 12, {"DISTAFF_NTT_DIF": "1"}), ("dif2", 12, {"DISTAFF_NTT_DIF": "2"}),
            ("waves4", 13, {"DISTAFF_NTT_WAVES": "4"}), ("waves8", 13, {"DISTAFF_NTT_WAVES": "8"}),
            ("3pass", 12, {"DISTAFF_NTT": "3pass"}), ("order0", 12, {"DISTAFF_NTT_ORDER": "0"}), ("batch", 12, {"DISTAFF_LDE_BATCH": "3,5"})]


@pytest.mark.gpu
@pytest.mark.parametrize("name,log_n,switches", SWITCHED, ids=["%s-%d" % (s[0], s[1]) for s in SWITCHED])
def test_switched_plans_equal_the_oracle(oracle, monkeypatch, name, log_n, switches):
    _transforms_equal_the_oracle(oracle, monkeypatch, log_n, 5, 19, switches)


@pytest.mark.gpu
def test_the_switches_select_what_the_cases_are_about(monkeypatch):
    """dst_ntt_describe under the switches of the cases above: pre-stages in both passes / in the first only, the three-pass plan (three
    launches, 16-column tiles), and four-column tiles in both passes of every other plan"""
    import distaff_amd as D

    def describe(log_n, switches):
        for k in NTT_SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in switches.items():
            monkeypatch.setenv(k, v)
        return list(D.ntt_describe(log_n, 5, 0, 1, 31, 19, 1))
    for name, log_n, switches in SWITCHED:
        lines = describe(log_n, switches)
        if name == "3pass":
            assert len(lines) == 3 and all("log_tile=4" in l for l in lines[:2]), lines
            continue
        assert len(lines) == 2 and all(" lds " in l and "log_tile=2" in l for l in lines), lines
        assert [("pre=1" in l) for l in lines] == [name in ("pre", "pre_a"), name == "pre"], lines
        if name.startswith("dif"):
            assert "dit=%s" % {"dif0": 1, "dif1": 0, "dif2": 2}[name] in lines[0], lines
        if name.startswith("waves"):
            assert all("block=%d" % {"waves4": 512, "waves8": 1024}[name] in l for l in lines), lines
    for log_n in (4, 5, 6, 7, 12, 13):
        lines = describe(log_n, {})
        assert len(lines) == 2 and all(" lds " in l and "log_tile=2" in l and "pre=0" in l for l in lines), lines


LDS_2_21 = [   # as the row-major parent printed them: a 2048 x 2 first pass in front of the second-pass instance compiled for 1024 x 4
    "ntt_pass_a lds a<1024,4,1,0,0,0> block=1024 grid=37696 lds=98304 dit=0 pre=0 log_len=11 log_tile=1 tiles_per_block=8 coset_fast=1 has_scale=0 bytes=20401094656 mads=159343706112",
    "ntt_pass_b lds b<1024,8,1,10,2,0> block=1024 grid=37696 lds=81920 dit=0 pre=0 log_len=10 log_tile=2 tiles_per_block=8 coset_fast=0 has_scale=0 bytes=39527120896 mads=94494523392",
    "ntt_pass_a lds a<1024,4,1,0,0,0> block=1024 grid=2560 lds=98304 dit=0 pre=0 log_len=11 log_tile=1 tiles_per_block=4 coset_fast=0 has_scale=0 bytes=1342177280 mads=4655677440",
    "ntt_pass_b lds b<1024,8,1,10,2,0> block=1024 grid=2560 lds=81920 dit=0 pre=0 log_len=10 log_tile=2 tiles_per_block=4 coset_fast=0 has_scale=1 bytes=1342177280 mads=3963617280"]


@pytest.mark.gpu
def test_lds_family_at_2_21_launches_what_it_launched_before(monkeypatch):
    """DISTAFF_NTT=lds at 2^21 puts a two-column first pass in front of the 1024 x 4 second-pass instance: a row-major plan served by an
    instance that tile-major plans use too.  The plan exists and its launches are the recorded ones (tests/golden/ntt_launches.json has
    the lds family at 13, 16, 19 and 22 only)."""
    import distaff_amd as D
    for k in NTT_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DISTAFF_NTT", "lds")
    assert list(D.ntt_describe(21, 5, 0, 1, 31, 19, 1)) + list(D.ntt_describe(21, 5, 1, 0, 1, 20, 0)) == LDS_2_21


@pytest.mark.gpu
def test_inverse_of_the_evaluation_cosets_and_the_8n_extension(oracle, monkeypatch):
    """2^10-step Fibonacci trace: the constraint polynomial (inverse transforms of the eight evaluation cosets, in place of their input)
    and its evaluations over the whole domain (8n coefficients folded per coset, then one forward transform per coset, in place) against
    the oracle's, with the oracle's draws"""
    import distaff_amd as D
    O = oracle
    for k in NTT_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    trace = O.fibonacci_trace(1 << 10)
    op = O.Prover.from_trace(trace, 1, ext=32, num_queries=50, grinding=8)
    for k in range(1, 6):
        op.step(k)
    ctx = D.Context(10, trace.width, trace.ctx_depth, trace.loop_depth, log_blowup=5, num_queries=50, grinding=8)
    try:
        ctx.upload(trace.columns)
        assert ctx.commit_trace() == op.get_bytes("roots")[:32]
        croot = ctx.eval_constraints(trace.public_inputs, op.outputs, op.get("constraint_draws"))
        assert (ctx.read_elements("ceval_t") == op.get("t_evaluations")).all(), "transition evaluations"
        assert (ctx.read_elements("cpoly") == op.get("constraint_poly")).all(), "constraint polynomial"
        assert (ctx.read_elements("cevals") == op.get("constraint_evaluations")).all(), "constraint evaluations"
        assert croot == op.get_bytes("roots")[32:64]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,switches", [(20, {}), (21, {}), (20, {"DISTAFF_NTT": "row"}), (21, {"DISTAFF_NTT": "lds"})], ids=["20", "21", "20-row", "21-lds"])
def test_shape_compiled_instances_at_2_20_and_2_21(oracle, monkeypatch, log_n, switches):
    """The instances compiled for 1024 x 4 tiles on both layouts: tile-major by default (2^20; at 2^21 the first pass is the pre-stage
    instance of that shape writing blocks with the frequencies 2 k' + h), row-major under DISTAFF_NTT=row and behind the 2048 x 2 first
    pass of DISTAFF_NTT=lds at 2^21.  A context at the smallest extension factor the library accepts
    (16): the coefficients of two registers give the trace at trace-domain points and the device's extension at 64 random positions of
    the extension domain, by the oracle's Horner evaluation."""
    import distaff_amd as D
    O = oracle
    for k in NTT_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    log_blowup, W = 4, 16
    n, B = 1 << log_n, 1 << log_blowup
    rng = np.random.default_rng(2000 + log_n)
    cols = rng.integers(0, 2**63, size=(W, n, 2), dtype=np.uint64)
    ctx = D.Context(log_n, W, 0, 0, log_blowup=log_blowup)
    try:
        ctx.upload(cols)
        ctx.commit_trace()
        polys = ctx.read_elements("polys").reshape(W, n, 2)
        registers = (3, W - 1)
        ldes = {c: ctx.read_elements("lde", c) for c in registers}
    finally:
        ctx.close()
    g_n, g_N = O.root_of_unity(n), O.root_of_unity(n * B)
    evaluate = getattr(O, "poly_eval_par", O.poly_eval)
    for c in registers:
        assert (ldes[c][::B] == cols[c]).all(), ("coset 0", c)
        for k in (0, n - 1, int(rng.integers(0, n))):
            assert evaluate(polys[c], O.exp(g_n, k)) == O.to_ints(cols[c, k:k + 1])[0], ("interpolation", c, k)
        for i in [1, n * B - 1] + [int(v) for v in rng.integers(0, n * B, size=62)]:
            assert evaluate(polys[c], O.exp(g_N, i)) == O.to_ints(ldes[c][i:i + 1])[0], ("extension", c, i)


def test_tile_major_cases_on_the_emulated_build():
    """every case above but the 2^20 / 2^21 ones on tests/emu/_build/libdistaff_emu.so (the library's own kernels, launched on the host)"""
    emu_dir = os.path.join(ROOT, "tests", "emu")
    emu_lib = os.path.join(emu_dir, "_build", "libdistaff_emu.so")
    subprocess.check_call(["make", "-C", emu_dir, "-j8"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, DISTAFF_HIP_LIB=emu_lib, DISTAFF_HIP_RUNTIME="none", DISTAFF_EMU_THREADS="2")
    import importlib.util
    workers = ["-n", "4"] if importlib.util.find_spec("xdist") is not None and (os.cpu_count() or 1) >= 8 else []
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", "-k", "not shape_compiled"] + workers + [os.path.abspath(__file__)],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:]
    assert "%d passed" % (36 + len(SWITCHED) + 3) in out, out[-2000:]
