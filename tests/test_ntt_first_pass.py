"""The first pass of the extension as it runs by default -- one-sided lazy butterflies in its coset DIT (fe.h: fe_addsub_lazy) and the trace
coefficients read from their copy in tile order (ctx.h: polys_tm, written by the interpolation's last pass beside `polys`) -- against the
same library under DISTAFF_NTT=row, the row-major reference path: no tile-order copy, the first pass reads `polys` in 64-byte row
segments.  Coefficients and every compared register of the extension must be equal byte for byte.

Shapes: n = 2^6, the smallest two-pass plan with four-column tiles in both passes (8 x 4 tiles, generic instance; the copy is one block per
tile pair); n = 2^12 (64 x 4, several tiles per workgroup); n = 2^20, the instance compiled for 1024 x 4 tiles.  The library accepts 16
registers or more and extension factors from 16: those are the figures at 2^20 (two of its registers are read back, 256 MiB each).
Inputs: uniform columns and columns that are p - 1 in every row, side by side in one trace.

One proof at 2^12 against the committed digest of the oracle's proof (tests/golden/proof_digests.json)."""
import json
import os

import numpy as np
import pytest

NTT_SWITCHES = ("DISTAFF_NTT", "DISTAFF_NTT_DIF", "DISTAFF_NTT_WAVES", "DISTAFF_NTT_ORDER", "DISTAFF_NTT_FIXED", "DISTAFF_NTT_SHAPE", "DISTAFF_LDE_BATCH")
P_LO = 2**64 - 45 * 2**40 + 1                     # low limb of the modulus; its high limb is 2^64 - 1


def _columns(log_n, W):
    """odd registers p - 1 in every row, even ones uniform below the modulus"""
    n = 1 << log_n
    rng = np.random.default_rng(7100 + log_n)
    cols = rng.integers(0, 2**64, size=(W, n, 2), dtype=np.uint64, endpoint=False)
    over = (cols[..., 1] == np.uint64(2**64 - 1)) & (cols[..., 0] >= np.uint64(P_LO))
    cols[..., 0][over] -= np.uint64(P_LO)
    cols[1::2] = np.array([P_LO - 1, 2**64 - 1], dtype=np.uint64)
    return cols


def _run(monkeypatch, log_n, W, log_blowup, cols, registers, switches):
    import distaff_amd as D
    for k in NTT_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    ctx = D.Context(log_n, W, 0, 0, log_blowup=log_blowup)
    try:
        ctx.upload(cols)
        ctx.commit_trace()
        return ctx.read("polys").copy(), [ctx.read("lde", c).copy() for c in registers]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,W,log_blowup,registers", [(6, 17, 4, range(17)), (12, 17, 5, range(17)), (20, 16, 4, (0, 15))], ids=["6", "12", "20"])
def test_extension_equals_the_row_major_reference_path(monkeypatch, log_n, W, log_blowup, registers):
    cols = _columns(log_n, W)
    polys, ldes = _run(monkeypatch, log_n, W, log_blowup, cols, registers, {})
    polys_row, ldes_row = _run(monkeypatch, log_n, W, log_blowup, cols, registers, {"DISTAFF_NTT": "row"})
    assert polys.size == W * (16 << log_n) and np.array_equal(polys, polys_row), "coefficients"
    for c, got, want in zip(registers, ldes, ldes_row):
        assert got.size == (16 << log_n) << log_blowup
        assert np.array_equal(got, want), ("register", c, np.flatnonzero(got != want)[:4].tolist())
        assert np.array_equal(got.view(np.uint64).reshape(-1, 2)[::1 << log_blowup], cols[c]), ("coset 0 is the trace", c)


@pytest.mark.gpu
def test_proof_at_2_12_matches_the_golden_digest(monkeypatch):
    import distaff_amd as D
    for k in NTT_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proof_digests.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["log_n"] == 12 and c["program"] == "fibonacci"]
    assert cases
    c = cases[0]
    cols, program_hash, result = D.fibonacci_trace(12)
    assert program_hash.hex() == c["program_hash"]
    ctx = D.Context(12, 20, 1, 0, log_blowup=c["extension_factor"].bit_length() - 1, num_queries=c["num_queries"], grinding=c["grinding_factor"])
    try:
        ctx.upload(cols)
        proof = ctx.prove([1, 0], [result])
    finally:
        ctx.close()
    assert len(proof) == c["proof_bytes"] and D.blake3(proof).hex() == c["proof_blake3"]
