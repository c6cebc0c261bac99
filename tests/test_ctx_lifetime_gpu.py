"""What a context leaves behind.  A `dst_ctx` owns its device buffers, its page-locked block, its streams and its events through one registry
(distaff_amd/csrc/ctx.h dst_owned): everything it acquires goes through four helpers, and `dst_ctx_destroy` -- or a `dst_ctx_create` that
fails half way -- walks that registry once.

Whole lives: three cycles of create, use, close per kind of context.  On every build the proofs of the three cycles are byte-equal, are
accepted by `D.verify`, and the sharded proof equals the single-context one.  On the emulated build (tests/test_ctx_lifetime_emulated.py runs
this file there) the stand-in runtime keeps a ledger of what is live: after every cycle the four live counts are what they were before the
first one, and nothing was released that was not live (a second release, a pointer the runtime never handed out).

A creation that fails: on the emulated build only, the k-th acquisition is made to fail for k = 0, 1, 2, ... until `dst_ctx_create`
succeeds.  No failure is provoked on a device.

The smallest shape of the suite: the Fibonacci trace at 2^7 rows, 20 registers, grinding 8."""
import ctypes
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG_N = 7
CYCLES = 3
INPUTS = [1, 0]


@functools.lru_cache(maxsize=None)
def _trace():
    """the trace, what the verifier needs beside the proof, and the same trace with the op counter of row 64 raised by one"""
    import distaff_amd as D
    cols, program_hash, result = D.fibonacci_trace(LOG_N)
    broken = cols.copy()
    broken[0, 64, 0] += 1
    cols.setflags(write=False)
    broken.setflags(write=False)
    return cols, broken, program_hash, [result]


def _ledger():
    """the emulated runtime's two test functions through the loaded library's handle, or None on a real device"""
    import distaff_amd as D
    lib = D.load()
    try:
        return lib.emu_live_counts, lib.emu_fail_acquisition
    except AttributeError:
        return None


def _counts():
    out = (ctypes.c_long * 5)()
    _ledger()[0](out)
    return {"device": out[0], "pinned": out[1], "events": out[2], "streams": out[3], "bad releases": out[4]}


def _context(D, **kw):
    return D.Context(LOG_N, 20, 1, 0, grinding=8, **kw)


def _never_used(D):
    _context(D).close()
    return None


def _upload_prove(D):
    cols, _, _, outputs = _trace()
    ctx = _context(D)
    ctx.upload(cols)
    proof = ctx.prove(INPUTS, outputs)
    ctx.close()
    return proof


def _pinned_async(D):
    cols, _, _, outputs = _trace()
    ctx = _context(D)
    table, handle = ctx.pinned_trace(cols)
    ctx.upload_async(table)
    proof = ctx.prove(INPUTS, outputs)
    ctx.release_pinned(handle)
    ctx.close()
    return proof


def _profiling(D):
    cols, _, _, outputs = _trace()
    ctx = _context(D)
    ctx.upload(cols)
    ctx.set_profiling(1)
    proof = ctx.prove(INPUTS, outputs)
    stats = ctx.kernel_stats()
    assert stats and all(st["launches"] >= 1 for st in stats.values())
    ctx.close()
    return proof


def _broken_row(D):
    """the broken trace is refused at step 63 (row 64 is that step's next row); the same context then proves the valid one"""
    cols, broken, _, outputs = _trace()
    ctx = _context(D)
    ctx.upload(broken)
    with pytest.raises(D.DistaffError) as e:
        ctx.prove(INPUTS, outputs)
    assert e.value.code == D.DST_ERR_AIR and ctx.bad_step == 63
    ctx.upload(cols)
    proof = ctx.prove(INPUTS, outputs)
    ctx.close()
    return proof


def _thread_ranks(D):
    """two thread-ranks on the registers each of them owns: once with the communicators the library makes for itself
    (dst_prove_sharded_local), once over the handles of Comm.local(2), one Python thread per rank; the handles are closed inside the cycle"""
    cols, _, _, outputs = _trace()
    ctxs = [_context(D, rank=r, world=2) for r in range(2)]
    for ctx in ctxs:
        ctx.upload_owned(cols)
    proof = D.prove_sharded_local(ctxs, INPUTS, outputs)
    comms = D.Comm.local(2)
    proofs, errors = [None, None], []

    def run(r):
        try:
            proofs[r] = ctxs[r].prove_sharded(comms[r], INPUTS, outputs)
        except Exception as e:                                # noqa: BLE001 -- reported below, on the main thread
            errors.append((r, e))
    threads = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for cm in comms:
        cm.close()
    for ctx in ctxs:
        ctx.close()
    assert not errors, errors
    assert proofs[0] == proof and proofs[1] == proof
    return proof


KINDS = {"never-used": _never_used, "upload-prove": _upload_prove, "pinned-async": _pinned_async, "profiling": _profiling,
         "broken-row": _broken_row, "thread-ranks": _thread_ranks}
# every kind that goes through dst_prove in both placements of the check of the trace rows: on the side stream (the default) and inline
LIVES = [(kind, place) for kind in KINDS for place in (("default", "inline") if kind not in ("never-used", "thread-ranks") else ("default",))]


@pytest.mark.parametrize("kind,place", LIVES, ids=lambda v: v)
def test_whole_lives(monkeypatch, kind, place):
    import distaff_amd as D
    if place == "default":
        monkeypatch.delenv("DISTAFF_AIR_CHECK", raising=False)
    else:
        monkeypatch.setenv("DISTAFF_AIR_CHECK", place)       # the library reads its switches when a context is created
    _, _, program_hash, outputs = _trace()
    before = _counts() if _ledger() else None
    first = None
    for cycle in range(CYCLES):
        proof = KINDS[kind](D)
        if cycle == 0:
            first = proof
            if proof is not None:
                assert D.verify(proof, program_hash, INPUTS, outputs) == (True, "")
                if kind != "upload-prove":
                    assert proof == _upload_prove(D), "the proof differs from the one of a plain upload and dst_prove"
        assert proof == first, "cycle %d: the proof differs from the first cycle's" % cycle
        if before is not None:
            assert _counts() == before, "cycle %d" % cycle
            assert before["bad releases"] == 0


@pytest.mark.parametrize("world", [1, 2])
def test_a_creation_that_fails(world):
    """rank 0 of `world`: every acquisition of dst_ctx_create in turn is the one that fails"""
    import distaff_amd as D
    if not _ledger():
        pytest.skip("emulated build only: no failure is provoked on a device")
    lib = D.load()
    fail = _ledger()[1]
    from distaff_amd.lib import Params
    params = Params(log_trace_length=LOG_N, log_blowup=5, width=20, ctx_depth=1, loop_depth=0, num_queries=50, grinding_factor=8, device=0, rank=0, world=world)
    before = _counts()
    assert before["bad releases"] == 0
    failed = 0
    for k in range(1000):
        handle = ctypes.c_void_p()
        fail(ctypes.c_long(k))
        r = lib.dst_ctx_create(ctypes.byref(params), ctypes.byref(handle))
        fail(ctypes.c_long(-1))
        if r == D.DST_OK:
            break
        failed += 1
        assert r == D.DST_ERR_HIP, (k, r)
        assert handle.value is None, k
        assert lib.dst_last_error(None), k
        assert _counts() == before, k
    else:
        pytest.fail("dst_ctx_create still fails with the 1000th acquisition: a runaway loop")
    assert handle.value is not None
    lib.dst_ctx_destroy(handle)
    assert _counts() == before
    print("world %d: %d acquisitions of dst_ctx_create failed in turn" % (world, failed))
    assert failed >= 40, "the injected failure does not reach the library"
