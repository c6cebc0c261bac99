"""dst_verify on the proofs the GPU prover writes: single context, sharded, and through both builds of the library."""
import ctypes
import struct

import pytest

pytestmark = pytest.mark.gpu


def _fib(log_n):
    from test_gpu_parity import _fib as cached                     # the session's trace cache of the parity tests (2^20: 14 s of host time, once)
    return cached(log_n)


def _first_trace_value_offset(proof):
    """offset of the first opened trace value: root 32 | header 8 | trace_nodes | u64 rows | u64 row length | values ..."""
    o = 40
    k, = struct.unpack_from("<Q", proof, o); o += 8
    for _ in range(k):
        m, = struct.unpack_from("<Q", proof, o); o += 8 + 32 * m
    return o + 16


@pytest.mark.parametrize("log_n,log_blowup,queries", [(10, 5, 50), (16, 5, 50), (20, 5, 50), (24, 4, 100)], ids=["2^10", "2^16", "config3-2^20", "config5-2^24"])
def test_gpu_proofs_are_accepted_and_tamper_evident(oracle, log_n, log_blowup, queries):
    """dst_prove at 2^10, 2^16 and 2^20 steps (2^20 = BASELINE config 3) and at 2^24 steps with extension 16 / 100 queries (config 5, on one
    GPU as tests/test_gpu_parity.py::test_config5_full_size_on_one_gpu proves it: three-pass transforms, the longest Merkle paths, the most
    FRI layers): dst_verify accepts the proof, says what the oracle says for a wrong output, and rejects the proof after one opened trace
    value was changed (the row no longer hashes to its leaf)."""
    import distaff_amd as D
    cols, program_hash, result = _fib(log_n)
    ctx = D.Context(log_n, 20, 1, 0, log_blowup=log_blowup, num_queries=queries, grinding=20)
    ctx.upload(cols)
    del cols
    proof = ctx.prove([1, 0], [result], cap=1 << 24)
    ctx.close()
    assert D.verify(proof, program_hash, [1, 0], [result]) == (True, "")
    info = D.proof_info(proof)
    assert (info["log_trace_length"], info["extension_factor"], info["num_queries"], info["grinding_factor"], info["register_count"]) == (log_n, 1 << log_blowup, queries, 20, 20)
    assert oracle.verify(proof, program_hash, [1, 0], [result]) == (True, "")
    assert D.verify(proof, program_hash, [1, 0], [result + 1]) == oracle.verify(proof, program_hash, [1, 0], [result + 1])
    bad = bytearray(proof); bad[_first_trace_value_offset(proof)] ^= 1
    assert D.verify(bytes(bad), program_hash, [1, 0], [result]) == (False, "verification of trace Merkle proof failed")
    assert oracle.verify(bytes(bad), program_hash, [1, 0], [result]) == (False, "verification of trace Merkle proof failed")


@pytest.mark.parametrize("world", [2, 8])
def test_sharded_proof_is_accepted(world):
    """dst_prove_sharded_local with 2 and 8 thread-ranks at 2^12: dst_verify accepts rank 0's proof"""
    import distaff_amd as D
    cols, program_hash, result = _fib(12)
    ctxs = []
    for r in range(world):
        ctx = D.Context(12, 20, 1, 0, rank=r, world=world)
        ctx.upload(cols)
        ctxs.append(ctx)
    proof = D.prove_sharded_local(ctxs, [1, 0], [result])
    for ctx in ctxs:
        ctx.close()
    assert D.verify(proof, program_hash, [1, 0], [result]) == (True, "")
    assert D.verify(proof, program_hash, [1, 0], [result + 1])[0] is False


def test_both_libraries_verify():
    """the same call on libdistaff_hip.so and on libdistaff_hip_hooks.so"""
    import distaff_amd as D
    cols, program_hash, result = _fib(10)
    ctx = D.Context(10, 20, 1, 0)
    ctx.upload(cols)
    proof = ctx.prove([1, 0], [result])
    ctx.close()
    for path, hooks in ((D.PRODUCT_LIB, 0), (D.HOOKS_LIB, 1)):
        lib = ctypes.CDLL(path)
        assert lib.dst_test_hooks() == hooks
        assert D.verify(proof, program_hash, [1, 0], [result], lib=lib) == (True, "")
        assert D.verify(proof, program_hash, [1, 1], [result], lib=lib)[0] is False
        assert D.proof_info(proof, lib=lib)["log_trace_length"] == 10
