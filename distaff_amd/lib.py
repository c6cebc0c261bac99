"""ctypes binding of libdistaff_hip.so (the product).  Nothing here falls back to a CPU implementation: if the shared
library is missing, or a call needs a GPU that is not there, an exception is raised.

Field elements cross the C-ABI as 16 little-endian bytes (the memory image of the reference's ``u128``); on the Python side
bulk data are numpy ``uint64`` arrays whose last axis has length 2 (low word, high word).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(_HERE, "libdistaff_hip.so")             # the product: what a host binds, what bench.py measures, what smoke() runs
HOOKS_LIB = os.path.join(_HERE, "libdistaff_hip_hooks.so")          # the same sources with -DDISTAFF_TEST_HOOKS (tests, bench.py's calibration kernels)
# DISTAFF_HIP_LIB names any other build (the tests' CPU emulation); DISTAFF_TEST_HOOKS=1 selects the test / bench build (tests/conftest.py)
LIB_PATH = os.environ.get("DISTAFF_HIP_LIB") or (HOOKS_LIB if os.environ.get("DISTAFF_TEST_HOOKS") == "1" else PRODUCT_LIB)


def use_test_hooks():
    """Bind the test / bench build (libdistaff_hip_hooks.so) instead of the product library -- before the first load(); child processes that
    import this package inherit the choice through DISTAFF_TEST_HOOKS=1 (bench.py removes the variable: it measures the product)."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("use_test_hooks() must be called before the library is loaded")
    os.environ["DISTAFF_TEST_HOOKS"] = "1"
    if not os.environ.get("DISTAFF_HIP_LIB"):
        LIB_PATH = HOOKS_LIB


def use_product():
    """Bind the product library whatever the environment said at import (an inherited DISTAFF_TEST_HOOKS=1) -- before the first load().
    An explicit DISTAFF_HIP_LIB still wins: it names a library, not a build flavour."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("use_product() must be called before the library is loaded")
    os.environ.pop("DISTAFF_TEST_HOOKS", None)
    if not os.environ.get("DISTAFF_HIP_LIB"):
        LIB_PATH = PRODUCT_LIB


def library_path():
    return LIB_PATH

DST_OK, DST_ERR_ARG, DST_ERR_HIP, DST_ERR_AIR, DST_ERR_STATE, DST_ERR_COMM = 0, -1, -2, -3, -4, -5

# ids of dst_read_buffer (distaff_amd/csrc/ctx.h)
BUF = {"polys": 0, "lde": 1, "trace_leaves": 2, "trace_nodes": 3, "ceval_i": 4, "ceval_f": 5, "ceval_t": 6, "cpoly": 7, "cevals": 8,
       "cnodes": 9, "comp_poly": 10, "comp_evals": 11, "fri_evals": 12, "fri_nodes": 13, "fri_leaves": 14}

EXPORTS = ["dst_ctx_create", "dst_ctx_destroy", "dst_last_error", "dst_phase_ms", "dst_trace_upload", "dst_trace_upload_contiguous", "dst_trace_upload_owned",
           "dst_commit_trace", "dst_eval_constraints", "dst_compose", "dst_fri_commit_layer", "dst_fri_fold", "dst_pow_grind",
           "dst_build_proof", "dst_prove", "dst_last_bad_step", "dst_prng_vector", "dst_query_positions", "dst_blake3", "dst_fibonacci_trace",
           "dst_read_buffer", "dst_bench_mulmod", "dst_bench_mad", "dst_bench_code", "dst_trace_upload_async", "dst_pinned_alloc", "dst_pinned_free", "dst_set_profiling", "dst_kernel_stats", "dst_field_op",
           "dst_shard_commit_trace", "dst_shard_eval_constraints", "dst_shard_combine", "dst_shard_fri_layer", "dst_shard_fri_fold",
           "dst_shard_export_size", "dst_shard_export", "dst_shard_import", "dst_shard_read", "dst_shard_fri_begin", "dst_shard_fri_end", "dst_shard_fri_roots", "dst_shard_open", "dst_shard_assemble", "dst_shard_info",
           "dst_comm_unique_id", "dst_comm_init", "dst_comm_init_local", "dst_comm_init_callbacks", "dst_comm_destroy", "dst_comm_last_error", "dst_comm_copy", "dst_prove_sharded", "dst_prove_sharded_local", "dst_shard_stage_ms",
           "dst_comm_describe", "dst_comm_trace", "dst_test_hooks", "dst_comm_set_timeout", "dst_comm_abort", "dst_shard_exchange_ms", "dst_bench_clock",
           "dst_verify", "dst_proof_info",
           "dst_rescue_digest_many", "dst_rtree_build", "dst_rtree_root", "dst_rtree_path", "dst_rtree_tapes", "dst_rtree_read_nodes", "dst_rtree_build_ms",
           "dst_rtree_destroy", "dst_rtree_last_error", "dst_rtree_update", "dst_rtree_update_ms", "dst_rtree_paths", "dst_rtree_tapes_many",
           "dst_stree_create", "dst_stree_set", "dst_stree_root", "dst_stree_paths", "dst_stree_tapes_many", "dst_stree_read_level", "dst_stree_info",
           "dst_stree_destroy", "dst_stree_last_error", "dst_rtree_apply", "dst_stree_apply", "dst_rescue_path_tapes",
           "dst_rescue_path_roots", "dst_rescue_verify_paths", "dst_rescue_verify_writes", "dst_rescue_refresh_paths", "dst_rescue_refresh_paths_w", "dst_rescue_refresh_last_gather_ms",
           "dst_stree_remove", "dst_stree_compact", "dst_stree_get",
           "dst_rescue_multiproof_size", "dst_rtree_multiproof", "dst_stree_multiproof", "dst_rescue_multiproof_root", "dst_rescue_verify_multiproof",
           "dst_rescue_multiproof_paths",
           "dst_rtree_save", "dst_rtree_load", "dst_rtree_audit", "dst_stree_save", "dst_stree_load", "dst_stree_audit",
           "dst_wtree_create", "dst_wtree_set", "dst_wtree_remove", "dst_wtree_compact", "dst_wtree_get", "dst_wtree_root", "dst_wtree_paths", "dst_wtree_apply",
           "dst_wtree_tapes_many", "dst_wtree_read_level", "dst_wtree_info", "dst_wtree_audit", "dst_wtree_destroy", "dst_wtree_last_error", "dst_wtree_test_set_node",
           "dst_rescue_path_roots_w", "dst_rescue_verify_paths_w", "dst_rescue_verify_writes_w", "dst_rescue_path_tapes_w",
           "dst_rescue_empty_nodes", "dst_rescue_multiproof_size_w", "dst_wtree_multiproof", "dst_rescue_multiproof_root_w", "dst_rescue_verify_multiproof_w",
           "dst_rescue_multiproof_paths_w", "dst_rescue_multiproof_last_levels", "dst_wtree_save", "dst_wtree_load"]


class DistaffError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libdistaff_hip error %d: %s" % (code, message))
        self.code = code
        self.reason = message


class Params(ctypes.Structure):
    _fields_ = [("log_trace_length", ctypes.c_uint32), ("log_blowup", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("ctx_depth", ctypes.c_uint32), ("loop_depth", ctypes.c_uint32), ("num_queries", ctypes.c_uint32),
                ("grinding_factor", ctypes.c_uint32), ("device", ctypes.c_int32), ("rank", ctypes.c_uint32), ("world", ctypes.c_uint32)]


class Public(ctypes.Structure):
    _fields_ = [("num_inputs", ctypes.c_uint32), ("num_outputs", ctypes.c_uint32),
                ("inputs", (ctypes.c_uint8 * 16) * 8), ("outputs", (ctypes.c_uint8 * 16) * 8)]


class CommInfo(ctypes.Structure):
    _fields_ = [("transport", ctypes.c_uint32), ("rank", ctypes.c_uint32), ("world", ctypes.c_uint32), ("device", ctypes.c_int32),
                ("rccl_ranks", ctypes.c_uint32), ("rccl_rank", ctypes.c_uint32), ("rccl_version", ctypes.c_uint32),
                ("peers_other_device", ctypes.c_uint32), ("peers_enabled", ctypes.c_uint32)]


class ProofInfo(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("log_trace_length", "extension_factor", "num_queries", "grinding_factor", "register_count", "ctx_depth", "loop_depth",
                                               "stack_depth", "op_count", "fri_layers", "remainder_length", "security_level", "security_level_proven")] + [("pow_nonce", ctypes.c_uint64)]


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so (soname libamdhip64.so.7) next to libtorch_hip.so;
    libdistaff_hip.so needs `libamdhip64.so.7`.  If the ROCm copy under /opt/rocm is loaded first, torch later brings its own copy
    in as a SECOND runtime, which then finds no devices; loaded the other way round, the dynamic linker resolves our NEEDED entry to
    torch's copy by soname and both share one runtime (and device pointers can be exchanged directly, which the sharded prover
    relies on).  So when torch is installed, its copy is loaded first, without importing torch.  Without torch nothing happens and
    the library binds to /opt/rocm as usual (that is the case for a Rust host binding the C-ABI)."""
    if os.environ.get("DISTAFF_HIP_RUNTIME", "torch") != "torch":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except OSError:
        pass


def _open(path):
    if not os.path.exists(path):
        raise ImportError("%s is missing: the HIP extension must be built (python -c 'import __graft_entry__ as g; g.build()'), there is no CPU fallback" % path)
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(path)
    lib.dst_last_error.restype = ctypes.c_char_p
    lib.dst_last_error.argtypes = [ctypes.c_void_p]
    if hasattr(lib, "dst_rescue_refresh_last_gather_ms"):              # a library named by DISTAFF_HIP_LIB may predate it
        lib.dst_rescue_refresh_last_gather_ms.restype = ctypes.c_double
        lib.dst_rescue_refresh_last_gather_ms.argtypes = []
    if hasattr(lib, "dst_last_bad_step"):                              # a library named by DISTAFF_HIP_LIB may predate it
        lib.dst_last_bad_step.restype = ctypes.c_int64
        lib.dst_last_bad_step.argtypes = [ctypes.c_void_p]
    return lib


def load():
    """Loads the shared library (raises if it has not been built: run ``python -c 'import __graft_entry__ as g; g.build()'``)."""
    global _lib
    if _lib is None:
        _lib = _open(LIB_PATH)
    return _lib


_hooks_lib = None


def load_hooks():
    """The test / bench build as a SECOND handle beside the product library (bench.py: the calibration kernels live only there)."""
    global _hooks_lib
    if _hooks_lib is None:
        bound = load()
        has = getattr(bound, "dst_test_hooks", None)
        _hooks_lib = bound if (has is not None and has() == 1) else _open(HOOKS_LIB)       # the bound library is itself a test build (tests, the CPU emulation)
    return _hooks_lib


def ntt_describe(log_n, log_blowup, inverse, lde, cosets, cols, skip=0, lib=None):
    """dst_ntt_describe (test build only): one line per kernel launch a transform of this size and shape would make under the DISTAFF_NTT_*
    switches as the environment has them now -- instance, block, grid, LDS bytes, what the launch layer decided.  Touches no device."""
    buf = ctypes.create_string_buffer(4096)
    r = (lib or load_hooks()).dst_ntt_describe(ctypes.c_uint32(log_n), ctypes.c_uint32(log_blowup), ctypes.c_int(int(inverse)), ctypes.c_int(int(lde)),
                                               ctypes.c_uint32(cosets), ctypes.c_uint32(cols), ctypes.c_uint32(skip), buf, ctypes.c_size_t(len(buf)))
    if r != DST_OK:
        raise DistaffError(r, "dst_ntt_describe(%d, %d) failed" % (log_n, log_blowup))
    return buf.value.decode().splitlines()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def int_to_bytes(v):
    return int(v).to_bytes(16, "little")


def ints_to_arr(values):
    out = np.empty((len(values), 2), dtype=np.uint64)
    for i, v in enumerate(values):
        out[i, 0] = int(v) & 0xFFFFFFFFFFFFFFFF
        out[i, 1] = int(v) >> 64
    return out


def arr_to_ints(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 2)
    return [int(lo) | (int(hi) << 64) for lo, hi in a]


def make_public(inputs, outputs):
    p = Public()
    p.num_inputs, p.num_outputs = len(inputs), len(outputs)
    for i, v in enumerate(inputs):
        p.inputs[i][:] = list(int_to_bytes(v))
    for i, v in enumerate(outputs):
        p.outputs[i][:] = list(int_to_bytes(v))
    return p


def prng_vector(seed, count):
    """field::prng_vector (src/math/field.rs:271) -- host side, StdRng(ChaCha20) + Uniform restatement inside the library."""
    out = np.zeros((count, 2), dtype=np.uint64)
    load().dst_prng_vector(bytes(seed), ctypes.c_uint32(count), _ptr(out))
    return out


def query_positions(seed, domain_size, blowup, num_queries):
    out = np.zeros(num_queries, dtype=np.uint64)
    k = load().dst_query_positions(bytes(seed), ctypes.c_uint64(domain_size), ctypes.c_uint32(blowup), ctypes.c_uint32(num_queries), _ptr(out))
    if k < 0:
        raise DistaffError(k, "could not generate enough query positions")
    return [int(x) for x in out[:k]]


def blake3(data):
    out = ctypes.create_string_buffer(32)
    load().dst_blake3(bytes(data), ctypes.c_size_t(len(data)), out)
    return out.raw


def verify(proof, program_hash, inputs, outputs, lib=None):
    """stark::verify (src/lib.rs:72) on the host through dst_verify: no context, no GPU.  -> (accepted, error): (True, "") for a valid proof,
    (False, the reference's error string) for a well-formed proof that does not verify.  Bytes that are not a StarkProof raise DistaffError
    (DST_ERR_ARG) with the reason."""
    proof, program_hash = bytes(proof), bytes(program_hash)
    if len(program_hash) != 32:
        raise DistaffError(DST_ERR_ARG, "program_hash must be 32 bytes")
    if len(inputs) > 8 or len(outputs) > 8:
        raise DistaffError(DST_ERR_ARG, "at most 8 public inputs and 8 outputs")
    pub = make_public(inputs, outputs)
    accepted = ctypes.c_int(0)
    err = ctypes.create_string_buffer(512)
    r = (lib or load()).dst_verify(program_hash, ctypes.byref(pub), proof, ctypes.c_size_t(len(proof)), ctypes.byref(accepted), err, ctypes.c_size_t(512))
    if r != DST_OK:
        raise DistaffError(r, err.value.decode())
    return accepted.value == 1, err.value.decode()


def proof_info(proof, lib=None):
    """dst_proof_info: what a proof says about itself, without verifying it (trace length, options, register counts, FRI layers, security level)."""
    proof = bytes(proof)
    info = ProofInfo()
    r = (lib or load()).dst_proof_info(proof, ctypes.c_size_t(len(proof)), ctypes.byref(info))
    if r != DST_OK:
        raise DistaffError(r, "not a StarkProof")
    return {f: int(getattr(info, f)) for f, _ in ProofInfo._fields_}


def fibonacci_trace(log_n):
    """Fibonacci example trace filling 2^log_n rows: returns (columns [20, n, 2] uint64, program_hash bytes, result int)."""
    n = 1 << log_n
    cols = np.zeros((20, n, 2), dtype=np.uint64)
    ph = ctypes.create_string_buffer(32)
    res = ctypes.create_string_buffer(16)
    r = load().dst_fibonacci_trace(ctypes.c_uint32(log_n), _ptr(cols), ph, res)
    if r != DST_OK:
        raise DistaffError(r, "dst_fibonacci_trace failed")
    return cols, ph.raw, int.from_bytes(res.raw, "little")


def _elements(values, per_item):
    """-> contiguous uint64 array [count, per_item, 2] from such an array or from a sequence of `per_item`-tuples of ints"""
    if isinstance(values, np.ndarray) and values.dtype == np.uint64:
        a = np.ascontiguousarray(values)
    else:
        rows = [tuple(v) for v in values]
        if any(len(r) != per_item for r in rows):
            raise DistaffError(DST_ERR_ARG, "every item must have %d elements" % per_item)
        a = ints_to_arr([x for r in rows for x in r])
    if a.size % (2 * per_item):
        raise DistaffError(DST_ERR_ARG, "expected [count, %d, 2] uint64 words" % per_item)
    return a.reshape(-1, per_item, 2)


def _rtree_error(lib, handle=None):
    lib.dst_rtree_last_error.restype = ctypes.c_char_p
    lib.dst_rtree_last_error.argtypes = [ctypes.c_void_p]
    return (lib.dst_rtree_last_error(handle) or b"").decode()


def _refresh_gather_ms(lib):
    """dst_rescue_refresh_last_gather_ms of a library however it was opened (the tests pass handles that did not come through _open)"""
    lib.dst_rescue_refresh_last_gather_ms.restype = ctypes.c_double
    lib.dst_rescue_refresh_last_gather_ms.argtypes = []
    return lib.dst_rescue_refresh_last_gather_ms()


def rescue_digest(values, device=0, lib=None):
    """utils::hasher::digest (src/utils/hasher.rs:12) of every 4-tuple of `values` (a sequence of 4-tuples of ints, or uint64 words
    [count, 4, 2]) through dst_rescue_digest_many -> uint64 words [count, 2, 2] (arr_to_ints turns them into ints).  device >= 0: on that GPU;
    device < 0: on the host, no GPU needed.  An element that is not below p raises DistaffError(DST_ERR_ARG)."""
    lib = lib or load()
    a = _elements(values, 4)
    out = np.zeros((a.shape[0], 2, 2), dtype=np.uint64)
    r = lib.dst_rescue_digest_many(ctypes.c_int(device), _ptr(a), ctypes.c_size_t(a.shape[0]), _ptr(out))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_digest_many failed")
    return out


def _wide_keys(indices):
    """16-byte little-endian keys from Python ints, or uint64 words [count, 2] (low half first) as they are -> (uint64 words [count, 2], pointer
    or None); an int outside 0 .. 2^128 - 1 cannot be a key"""
    if isinstance(indices, np.ndarray) and indices.dtype == np.uint64 and indices.ndim == 2 and indices.shape[1] == 2:
        idx = np.ascontiguousarray(indices)
        return idx, (_ptr(idx) if idx.shape[0] else None)
    vals = [int(i) for i in indices]
    if any(v < 0 or v >> 128 for v in vals):
        raise DistaffError(DST_ERR_ARG, "a key is an integer in 0 .. 2^128 - 1")
    idx = ints_to_arr(vals)
    return idx, (_ptr(idx) if len(vals) else None)


class _Keys:
    """the indices of a call without a tree: 8-byte words for the dst_rescue_* calls, 16-byte words for their _w forms (suffix)"""
    def __init__(self, indices, wide):
        self.arr, self.ptr = _wide_keys(indices) if wide else RescueTree._indices(indices)
        self.size = self.arr.shape[0]
        self.suffix = "_w" if wide else ""


def path_tapes(paths, indices, what=3, lib=None, _wide=False):
    """RescueTree.tapes_many over paths the caller holds (dst_rescue_path_tapes; host only, no tree): `paths` as paths() or apply() return them
    -- a list with one list of n pairs of ints per index -- or uint64 words [count, n, 2, 2] -> a list of (A, B)"""
    lib = lib or load()
    idx = _Keys(indices, _wide)
    ip, call = idx.ptr, getattr(lib, "dst_rescue_path_tapes" + idx.suffix)
    w, n_nodes = _path_words(paths, idx.size)
    nodes = ctypes.c_uint32(n_nodes)
    n = ctypes.c_size_t(0)
    r = call(_ptr(w) if idx.size else None, nodes, ip, ctypes.c_size_t(idx.size), ctypes.c_uint32(what), None, None, ctypes.c_size_t(0), ctypes.byref(n))
    if r == DST_OK:
        each = n.value
        a = np.zeros((max(idx.size * each, 1), 2), dtype=np.uint64)
        b = np.zeros((max(idx.size * each, 1), 2), dtype=np.uint64)
        r = call(_ptr(w) if idx.size else None, nodes, ip, ctypes.c_size_t(idx.size), ctypes.c_uint32(what), _ptr(a), _ptr(b), ctypes.c_size_t(each), ctypes.byref(n))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_path_tapes failed")
    va, vb = arr_to_ints(a[:idx.size * each]), arr_to_ints(b[:idx.size * each])
    return [(va[i * each:(i + 1) * each], vb[i * each:(i + 1) * each]) for i in range(idx.size)]


DST_PATH_OK, DST_PATH_BAD_LEAF, DST_PATH_BAD_ROOT, DST_PATH_BAD_NEXT_ROOT = 0, 1, 2, 3      # `why` of verify_paths / verify_writes


def _path_words(paths, count):
    """-> (uint64 words [count, n, 2, 2], n) from paths in either shape path_tapes accepts; no path at all counts as paths of 2 nodes"""
    if isinstance(paths, np.ndarray) and paths.dtype == np.uint64 and paths.ndim == 4:
        w = np.ascontiguousarray(paths)
    else:
        rows = [list(path) for path in paths]
        if len({len(r) for r in rows}) > 1:
            raise DistaffError(DST_ERR_ARG, "paths of one length")
        w = _elements([node for r in rows for node in r], 2).reshape(len(rows), -1, 2, 2) if rows else np.zeros((0, 2, 2, 2), dtype=np.uint64)
    if w.shape[0] != count:
        raise DistaffError(DST_ERR_ARG, "as many paths as indices")
    return w, w.shape[1]


def _nodes_for(values, count, what):
    """uint64 words [count, 2, 2] of `count` nodes (pairs of ints, or such words)"""
    a = _elements(values, 2)
    if a.shape[0] != count:
        raise DistaffError(DST_ERR_ARG, "as many %s as indices" % what)
    return a


def _pairs(words):
    v = arr_to_ints(words)
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


def path_roots(paths, indices, leaves=None, device=0, lib=None, stats=None, _wide=False):
    """compute_merkle_root (src/examples/merkle.rs:112-145) of every path with its index (dst_rescue_path_roots) -> a list of pairs of ints: what
    path i resolves to, or with `leaves` what it resolves to with leaves[i] as its first node.  `paths` as path_tapes takes them, what paths()
    and apply() return included.  device >= 0: one launch on that GPU for all paths; device < 0: on the host.  stats (a dict) receives device_ms."""
    lib = lib or load()
    idx = _Keys(indices, _wide)
    ip = idx.ptr
    w, n = _path_words(paths, idx.size)
    alt = _nodes_for(leaves, idx.size, "leaves") if leaves is not None else None
    out = np.zeros((max(idx.size, 1), 2, 2), dtype=np.uint64)
    ms = ctypes.c_double(0)
    r = getattr(lib, "dst_rescue_path_roots" + idx.suffix)(ctypes.c_int(device), _ptr(w) if idx.size else None, ctypes.c_uint32(n), ip, ctypes.c_size_t(idx.size),
                                  _ptr(alt) if alt is not None and idx.size else None, _ptr(out), ctypes.byref(ms))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_path_roots failed")
    if stats is not None:
        stats["device_ms"] = ms.value
    return _pairs(out[:idx.size])


def verify_paths(root, paths, indices, leaves=None, device=0, lib=None, stats=None, _wide=False):
    """membership / absence (dst_rescue_verify_paths) -> (first_bad, why): (-1, DST_PATH_OK) when every path resolves to `root` and, with
    `leaves`, has leaves[i] as its first node (the empty leaf of a sparse tree: the key is absent); else the lowest failing i and DST_PATH_BAD_LEAF
    or DST_PATH_BAD_ROOT.  A path that does not verify is a result, not an exception."""
    lib = lib or load()
    idx = _Keys(indices, _wide)
    ip = idx.ptr
    w, n = _path_words(paths, idx.size)
    want = _nodes_for(leaves, idx.size, "leaves") if leaves is not None else None
    r0 = _nodes_for([tuple(root)], 1, "roots")
    first, why, ms = ctypes.c_int64(-1), ctypes.c_uint32(0), ctypes.c_double(0)
    r = getattr(lib, "dst_rescue_verify_paths" + idx.suffix)(ctypes.c_int(device), _ptr(r0), _ptr(w) if idx.size else None, ctypes.c_uint32(n), ip,
                                    _ptr(want) if want is not None and idx.size else None, ctypes.c_size_t(idx.size), ctypes.byref(first), ctypes.byref(why), ctypes.byref(ms))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_verify_paths failed")
    if stats is not None:
        stats["device_ms"] = ms.value
    return first.value, why.value


def verify_writes(root_before, indices, paths, leaves, roots=None, device=0, lib=None, stats=None, _wide=False):
    """the checker of RescueTree.apply / SparseRescueTree.apply (dst_rescue_verify_writes) -> (first_bad, why, root_after): write i holds when
    paths[i] resolves to the root before it (root_before, then the root after write i - 1 as computed here) and, with `roots`, resolves to roots[i]
    with leaves[i] as its first node.  (-1, DST_PATH_OK, the root after the last write) when all hold.  Without `roots` a wrong new leaf shows one
    write later (DST_PATH_BAD_ROOT), in the last write only in root_after.  On a device all 2 * count chains run in one launch."""
    lib = lib or load()
    idx = _Keys(indices, _wide)
    ip = idx.ptr
    w, n = _path_words(paths, idx.size)
    new = _nodes_for(leaves, idx.size, "leaves")
    claimed = _nodes_for(roots, idx.size, "roots") if roots is not None else None
    r0 = _nodes_for([tuple(root_before)], 1, "roots")
    after = np.zeros((2, 2), dtype=np.uint64)
    first, why, ms = ctypes.c_int64(-1), ctypes.c_uint32(0), ctypes.c_double(0)
    r = getattr(lib, "dst_rescue_verify_writes" + idx.suffix)(ctypes.c_int(device), _ptr(r0), _ptr(w) if idx.size else None, ctypes.c_uint32(n), ip, _ptr(new) if idx.size else None,
                                     _ptr(claimed) if claimed is not None and idx.size else None, ctypes.c_size_t(idx.size), ctypes.byref(first), ctypes.byref(why), _ptr(after),
                                     ctypes.byref(ms))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_verify_writes failed")
    if stats is not None:
        stats["device_ms"] = ms.value
    return first.value, why.value, tuple(arr_to_ints(after))


def refresh_paths(root_before, indices, paths, leaves, held_indices, held_paths, roots=None, device=0, lib=None, stats=None, _wide=False):
    """the paths a client holds, carried across the ordered writes of an apply() without the tree (dst_rescue_refresh_paths) -> (first_bad, why,
    root_after, new_paths): the writes are checked as verify_writes checks them; when they hold, new_paths[j] is the path of held_indices[j] under
    root_after (a list of lists of pairs of ints), else new_paths is None.  `paths` and `held_paths` in either shape verify_writes accepts.  The held
    paths themselves are not checked: verify_paths(root_after, new_paths, held_indices) does that.  On a device: one launch for all 2 * count chains
    and one that gathers the paths; stats (a dict) receives device_ms, events around both, and gather_ms, the second launch's part of it."""
    lib = lib or load()
    idx, hidx = _Keys(indices, _wide), _Keys(held_indices, _wide)
    w, n = _path_words(paths, idx.size)
    hw, hn = _path_words(held_paths, hidx.size)
    if idx.size and hidx.size and hn != n:
        raise DistaffError(DST_ERR_ARG, "paths of one length")
    n = n if idx.size else hn
    new = _nodes_for(leaves, idx.size, "leaves")
    claimed = _nodes_for(roots, idx.size, "roots") if roots is not None else None
    r0 = _nodes_for([tuple(root_before)], 1, "roots")
    after = np.zeros((2, 2), dtype=np.uint64)
    out = np.zeros((max(hidx.size, 1), n, 2, 2), dtype=np.uint64)
    first, why, ms = ctypes.c_int64(-1), ctypes.c_uint32(0), ctypes.c_double(0)
    r = getattr(lib, "dst_rescue_refresh_paths" + idx.suffix)(ctypes.c_int(device), _ptr(r0), _ptr(w) if idx.size else None, ctypes.c_uint32(n), idx.ptr, _ptr(new) if idx.size else None,
                                     _ptr(claimed) if claimed is not None and idx.size else None, ctypes.c_size_t(idx.size), hidx.ptr, _ptr(hw) if hidx.size else None,
                                     ctypes.c_size_t(hidx.size), _ptr(out), ctypes.byref(first), ctypes.byref(why), _ptr(after), ctypes.byref(ms))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_refresh_paths failed")
    if stats is not None:
        stats["device_ms"], stats["gather_ms"] = ms.value, _refresh_gather_ms(lib)
    if first.value >= 0:
        return first.value, why.value, tuple(arr_to_ints(after)), None
    nodes = _pairs(out[:hidx.size])
    return first.value, why.value, tuple(arr_to_ints(after)), [nodes[j * n:(j + 1) * n] for j in range(hidx.size)]


def refresh_paths_wide(root_before, indices, paths, leaves, held_indices, held_paths, roots=None, device=0, lib=None, stats=None):
    """refresh_paths for the witnesses of WideSparseRescueTree.apply: paths of up to 128 nodes, indices of up to 127 bits (dst_rescue_refresh_paths_w)"""
    return refresh_paths(root_before, indices, paths, leaves, held_indices, held_paths, roots, device, lib, stats, _wide=True)


def path_tapes_wide(paths, indices, what=3, lib=None):
    """path_tapes for paths of up to 128 nodes and indices of up to 127 bits, Python ints (dst_rescue_path_tapes_w)"""
    return path_tapes(paths, indices, what, lib, _wide=True)


def path_roots_wide(paths, indices, leaves=None, device=0, lib=None, stats=None):
    """path_roots for paths of up to 128 nodes and indices of up to 127 bits, Python ints (dst_rescue_path_roots_w)"""
    return path_roots(paths, indices, leaves, device, lib, stats, _wide=True)


def verify_paths_wide(root, paths, indices, leaves=None, device=0, lib=None, stats=None):
    """verify_paths for paths of up to 128 nodes and indices of up to 127 bits, Python ints (dst_rescue_verify_paths_w)"""
    return verify_paths(root, paths, indices, leaves, device, lib, stats, _wide=True)


def verify_writes_wide(root_before, indices, paths, leaves, roots=None, device=0, lib=None, stats=None):
    """verify_writes for WideSparseRescueTree.apply: paths of up to 128 nodes, indices of up to 127 bits (dst_rescue_verify_writes_w)"""
    return verify_writes(root_before, indices, paths, leaves, roots, device, lib, stats, _wide=True)


def multiproof_size(n, indices, lib=None):
    """(M, digests) of the multiproof of the distinct leaf indices `indices` for paths of n nodes (dst_rescue_multiproof_size; host only, no
    hashing): how many sibling nodes it supplies and how many parents its check computes"""
    lib = lib or load()
    idx, ip = RescueTree._indices(indices)
    m, d = ctypes.c_size_t(0), ctypes.c_uint64(0)
    r = lib.dst_rescue_multiproof_size(ctypes.c_uint32(n), ip, ctypes.c_size_t(idx.size), ctypes.byref(m), ctypes.byref(d))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_multiproof_size failed")
    return m.value, d.value


def _multiproof_args(indices, leaves, nodes):
    idx, ip = RescueTree._indices(indices)
    a = _nodes_for(leaves, idx.size, "leaves")
    b = _elements(nodes, 2) if len(nodes) else np.zeros((0, 2, 2), dtype=np.uint64)
    return idx, ip, a, b


def _tree_multiproof(tree, call, indices, words):
    """(leaves, nodes) of a tree's multiproof through `call`: size query, then the gather"""
    idx, ip = RescueTree._indices(indices)
    m = ctypes.c_size_t(0)
    tree._check(call(tree._h, ip, ctypes.c_size_t(idx.size), None, None, ctypes.c_size_t(0), ctypes.byref(m)))
    leaves = np.zeros((idx.size, 2, 2), dtype=np.uint64)
    nodes = np.zeros((m.value, 2, 2), dtype=np.uint64)
    if idx.size:
        spare = np.zeros((1, 2, 2), dtype=np.uint64)                     # a set that needs no sibling still asks for the leaves
        tree._check(call(tree._h, ip, ctypes.c_size_t(idx.size), _ptr(leaves), _ptr(nodes) if m.value else _ptr(spare), ctypes.c_size_t(m.value), ctypes.byref(m)))
    return (leaves, nodes) if words else (_pairs(leaves), _pairs(nodes))


def multiproof_root(n, indices, leaves, nodes, device=0, lib=None, stats=None):
    """the root a multiproof resolves to (dst_rescue_multiproof_root) -> a pair of ints.  `leaves` in the order of `indices`, `nodes` as
    RescueTree.multiproof returns them (pairs of ints, or uint64 words [count, 2, 2]).  With other leaves over the same nodes: the root after
    those unordered writes.  Every shared ancestor is hashed once; stats (a dict) receives digests and device_ms."""
    lib = lib or load()
    idx, ip, a, b = _multiproof_args(indices, leaves, nodes)
    out = np.zeros((2, 2), dtype=np.uint64)
    d, ms = ctypes.c_uint64(0), ctypes.c_double(0)
    r = lib.dst_rescue_multiproof_root(ctypes.c_int(device), ctypes.c_uint32(n), ip, _ptr(a) if idx.size else None, ctypes.c_size_t(idx.size), _ptr(b) if b.shape[0] else None,
                                       ctypes.c_size_t(b.shape[0]), _ptr(out), ctypes.byref(d), ctypes.byref(ms))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_multiproof_root failed")
    if stats is not None:
        stats["digests"], stats["device_ms"] = d.value, ms.value
    return tuple(arr_to_ints(out))


def verify_multiproof(root, n, indices, leaves, nodes, device=0, lib=None, stats=None):
    """whether the multiproof resolves to `root` (dst_rescue_verify_multiproof) -> bool; one that does not is a result, not an exception"""
    lib = lib or load()
    idx, ip, a, b = _multiproof_args(indices, leaves, nodes)
    r0 = _nodes_for([tuple(root)], 1, "roots")
    ok, ms = ctypes.c_int(0), ctypes.c_double(0)
    r = lib.dst_rescue_verify_multiproof(ctypes.c_int(device), _ptr(r0), ctypes.c_uint32(n), ip, _ptr(a) if idx.size else None, ctypes.c_size_t(idx.size),
                                         _ptr(b) if b.shape[0] else None, ctypes.c_size_t(b.shape[0]), ctypes.byref(ok), ctypes.byref(ms))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_verify_multiproof failed")
    if stats is not None:
        stats["device_ms"] = ms.value
    return bool(ok.value)


def multiproof_paths(n, indices, leaves, nodes, device=0, lib=None, stats=None, words=False):
    """the full authentication paths a multiproof stands for (dst_rescue_multiproof_paths) -> (paths, root): paths in the shape
    RescueTree.paths returns (words=True: uint64 words [count, n, 2, 2]), in the order of `indices` -- what path_tapes, path_roots and
    verify_paths take -- and the root they resolve to"""
    lib = lib or load()
    idx, ip, a, b = _multiproof_args(indices, leaves, nodes)
    out = np.zeros((max(idx.size, 1), max(n, 1), 2, 2), dtype=np.uint64)
    root = np.zeros((2, 2), dtype=np.uint64)
    ms = ctypes.c_double(0)
    r = lib.dst_rescue_multiproof_paths(ctypes.c_int(device), ctypes.c_uint32(n), ip, _ptr(a) if idx.size else None, ctypes.c_size_t(idx.size), _ptr(b) if b.shape[0] else None,
                                        ctypes.c_size_t(b.shape[0]), _ptr(out), _ptr(root), ctypes.byref(ms))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_multiproof_paths failed")
    if stats is not None:
        stats["device_ms"] = ms.value
    if words:
        return out[:idx.size], tuple(arr_to_ints(root))
    v = arr_to_ints(out[:idx.size])
    return [[(v[2 * (i * n + k)], v[2 * (i * n + k) + 1]) for k in range(n)] for i in range(idx.size)], tuple(arr_to_ints(root))


def empty_nodes(n, empty_leaf=(0, 0), words=False, lib=None):
    """E_0 .. E_{n-1}, the value of an empty subtree of every level of a tree whose paths have n nodes and whose empty leaf is `empty_leaf`
    (dst_rescue_empty_nodes; host only, n - 1 digests) -> a list of n pairs of ints (words=True: uint64 words [n, 2, 2]): the table the compact
    checks take.  Compute it once per (empty leaf, depth) -- and compute it: the checks believe it."""
    lib = lib or load()
    e = _elements([tuple(empty_leaf)], 2)
    out = np.zeros((max(int(n), 1), 2, 2), dtype=np.uint64)
    r = lib.dst_rescue_empty_nodes(_ptr(e), ctypes.c_uint32(n), _ptr(out))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_empty_nodes failed")
    return out if words else _pairs(out)


def multiproof_size_wide(n, indices, lib=None):
    """multiproof_size for indices of up to 127 bits, Python ints, and 2 <= n <= 128 (dst_rescue_multiproof_size_w): the plain sizes (M, digests)"""
    lib = lib or load()
    idx, ip = _wide_keys(indices)
    m, d = ctypes.c_size_t(0), ctypes.c_uint64(0)
    r = lib.dst_rescue_multiproof_size_w(ctypes.c_uint32(n), ip, ctypes.c_size_t(idx.shape[0]), ctypes.byref(m), ctypes.byref(d))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_multiproof_size_w failed")
    return m.value, d.value


class _WideProof:
    """the arguments the three wide checks share: indices, leaves, nodes, and for the compact form the bits and the table"""
    def __init__(self, n, indices, leaves, nodes, absent_bits, empties):
        self.idx, self.ip = _wide_keys(indices)
        self.count = self.idx.shape[0]
        self.leaves = _nodes_for(leaves, self.count, "leaves")
        self.nodes = _elements(nodes, 2) if len(nodes) else np.zeros((0, 2, 2), dtype=np.uint64)
        self.bits = np.frombuffer(bytes(absent_bits), dtype=np.uint8) if absent_bits is not None else None
        self.table = None
        if empties is not None:
            self.table = _elements(empties, 2)
            if self.table.shape[0] != n:
                raise DistaffError(DST_ERR_ARG, "empties: one node per level, %d of them" % n)
        self.spare = np.zeros(1, dtype=np.uint8)                           # a proof without supplied nodes still has a (zero-length) bit string

    def args(self):
        """what stands between `n` and the outputs of each call"""
        bits = None if self.bits is None else (_ptr(self.bits) if self.bits.size else _ptr(self.spare))
        return (self.ip, _ptr(self.leaves) if self.count else None, ctypes.c_size_t(self.count), _ptr(self.nodes) if self.nodes.shape[0] else None,
                ctypes.c_size_t(self.nodes.shape[0]), bits, _ptr(self.table) if self.table is not None else None)


def _wide_stats(lib, stats, ms, digests=None):
    if stats is not None:
        stats["device_ms"], stats["levels"] = ms.value, lib.dst_rescue_multiproof_last_levels()
        if digests is not None:
            stats["digests"] = digests.value


def multiproof_root_wide(n, indices, leaves, nodes, absent_bits=None, empties=None, device=0, lib=None, stats=None):
    """multiproof_root over indices of up to 127 bits (dst_rescue_multiproof_root_w).  Plain: `nodes` are all M supplied nodes.  Compact:
    `absent_bits` (bytes, as WideSparseRescueTree.batch_proof returns them) says which supplied nodes are empty subtrees and not among `nodes`,
    and `empties` is the table of empty_nodes(n, empty_leaf); parents of two empty subtrees are not hashed.  stats receives digests (parents
    actually computed), levels (levels that had a job: the launches of a device call) and device_ms."""
    lib = lib or load()
    a = _WideProof(n, indices, leaves, nodes, absent_bits, empties)
    out = np.zeros((2, 2), dtype=np.uint64)
    d, ms = ctypes.c_uint64(0), ctypes.c_double(0)
    r = lib.dst_rescue_multiproof_root_w(ctypes.c_int(device), ctypes.c_uint32(n), *a.args(), _ptr(out), ctypes.byref(d), ctypes.byref(ms))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_multiproof_root_w failed")
    _wide_stats(lib, stats, ms, d)
    return tuple(arr_to_ints(out))


def verify_multiproof_wide(root, n, indices, leaves, nodes, absent_bits=None, empties=None, device=0, lib=None, stats=None):
    """whether the plain or compact multiproof resolves to `root` (dst_rescue_verify_multiproof_w) -> bool; stats receives levels and device_ms"""
    lib = lib or load()
    a = _WideProof(n, indices, leaves, nodes, absent_bits, empties)
    r0 = _nodes_for([tuple(root)], 1, "roots")
    ok, ms = ctypes.c_int(0), ctypes.c_double(0)
    r = lib.dst_rescue_verify_multiproof_w(ctypes.c_int(device), _ptr(r0), ctypes.c_uint32(n), *a.args(), ctypes.byref(ok), ctypes.byref(ms))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_verify_multiproof_w failed")
    _wide_stats(lib, stats, ms)
    return bool(ok.value)


def multiproof_paths_wide(n, indices, leaves, nodes, absent_bits=None, empties=None, device=0, lib=None, stats=None, words=False):
    """the full authentication paths a plain or compact multiproof stands for (dst_rescue_multiproof_paths_w) -> (paths, root), paths as
    WideSparseRescueTree.paths returns them (words=True: uint64 words [count, n, 2, 2]): what verify_paths_wide and path_tapes_wide take"""
    lib = lib or load()
    a = _WideProof(n, indices, leaves, nodes, absent_bits, empties)
    out = np.zeros((max(a.count, 1), max(n, 1), 2, 2), dtype=np.uint64)
    root = np.zeros((2, 2), dtype=np.uint64)
    ms = ctypes.c_double(0)
    r = lib.dst_rescue_multiproof_paths_w(ctypes.c_int(device), ctypes.c_uint32(n), *a.args(), _ptr(out), _ptr(root), ctypes.byref(ms))
    if r != DST_OK:
        raise DistaffError(r, _rtree_error(lib) or "dst_rescue_multiproof_paths_w failed")
    _wide_stats(lib, stats, ms)
    if words:
        return out[:a.count], tuple(arr_to_ints(root))
    v = arr_to_ints(out[:a.count])
    return [[(v[2 * (i * n + k)], v[2 * (i * n + k) + 1]) for k in range(n)] for i in range(a.count)], tuple(arr_to_ints(root))


def _tree_save(tree, call):
    """save() of either tree: the size query, then the bytes"""
    n = ctypes.c_size_t(0)
    tree._check(call(tree._h, None, ctypes.c_size_t(0), ctypes.byref(n)))
    out = np.zeros(n.value, dtype=np.uint8)
    tree._check(call(tree._h, _ptr(out), ctypes.c_size_t(n.value), ctypes.byref(n)))
    return out.tobytes()


def _tree_load(lib, call, error, blob, device, audit):
    """load() of either tree -> the handle; `error(lib)` = the text of the calling thread's last failed call without a tree"""
    a = np.frombuffer(blob, dtype=np.uint8)
    h = ctypes.c_void_p()
    r = call(ctypes.c_int(device), _ptr(a) if a.size else None, ctypes.c_size_t(a.size), ctypes.c_uint32(1 if audit else 0), ctypes.byref(h))
    if r != DST_OK:
        raise DistaffError(r, error(lib))
    return h


def _apply(tree, call, n, indices, leaves):
    """(paths, roots) of an ordered batch of writes: paths in the shape paths() returns, roots a list of pairs of ints"""
    idx, ip = getattr(tree, "_keys", RescueTree._indices)(indices)
    a = _elements(leaves, 2)
    count = idx.shape[0]
    if a.shape[0] != count:
        raise DistaffError(DST_ERR_ARG, "as many leaves as indices")
    paths = np.zeros((max(count, 1) * n, 2, 2), dtype=np.uint64)
    roots = np.zeros((max(count, 1), 2, 2), dtype=np.uint64)
    tree._check(call(tree._h, ip, _ptr(a) if count else None, ctypes.c_size_t(count), _ptr(paths), _ptr(roots)))
    v, r = arr_to_ints(paths[:count * n]), arr_to_ints(roots[:count])
    return ([[(v[2 * (i * n + k)], v[2 * (i * n + k) + 1]) for k in range(n)] for i in range(count)], [(r[2 * i], r[2 * i + 1]) for i in range(count)])


class RescueTree:
    """A Merkle tree of the kind the VM's smpath.n / pmpath.n authenticate (``dst_rtree``): nodes of two field elements, parent =
    hasher::digest(l0, l1, r0, r1).  `leaves`: a sequence of 2^k pairs of ints or uint64 words [2^k, 2, 2], 1 <= k <= 26.  device >= 0 builds
    it on that GPU and keeps it there; device < 0 builds it on the host."""

    def __init__(self, leaves, device=0, lib=None):
        self.lib = lib or load()
        a = _elements(leaves, 2)
        n = a.shape[0]
        if n < 2 or n & (n - 1):
            raise DistaffError(DST_ERR_ARG, "the number of leaves must be a power of two >= 2")
        self.log_leaves = n.bit_length() - 1
        h = ctypes.c_void_p()
        r = self.lib.dst_rtree_build(ctypes.c_int(device), _ptr(a), ctypes.c_uint32(self.log_leaves), ctypes.byref(h))
        if r != DST_OK:
            raise DistaffError(r, _rtree_error(self.lib))
        self._h = h

    def _check(self, r):
        if r != DST_OK:
            raise DistaffError(r, _rtree_error(self.lib, self._h))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.dst_rtree_destroy.restype = None
            self.lib.dst_rtree_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def root(self):
        """(r0, r1)"""
        out = np.zeros((2, 2), dtype=np.uint64)
        self._check(self.lib.dst_rtree_root(self._h, _ptr(out)))
        return tuple(arr_to_ints(out))

    @property
    def build_ms(self):
        """device milliseconds of the level kernels of the build (0 for a host tree)"""
        ms = ctypes.c_double(0)
        self._check(self.lib.dst_rtree_build_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def path(self, index):
        """authentication path of leaf `index`: [leaf, sibling, uncle, ...] as pairs of ints, log_leaves + 1 nodes"""
        out = np.zeros((self.log_leaves + 1, 2, 2), dtype=np.uint64)
        self._check(self.lib.dst_rtree_path(self._h, ctypes.c_uint64(index), _ptr(out)))
        v = arr_to_ints(out)
        return [(v[2 * k], v[2 * k + 1]) for k in range(self.log_leaves + 1)]

    def tapes(self, index, what=3):
        """secret tapes (A, B) as lists of ints for the program of src/examples/merkle.rs:46-56 with n = log_leaves + 1 and this index:
        ProgramInputs::new(&[], &a, &b).  what = 1: the leaf and the smpath inputs only, 2: the pmpath inputs only, 3: both."""
        n = ctypes.c_size_t(0)
        self._check(self.lib.dst_rtree_tapes(self._h, ctypes.c_uint64(index), ctypes.c_uint32(what), None, None, ctypes.c_size_t(0), ctypes.byref(n)))
        a = np.zeros((max(n.value, 1), 2), dtype=np.uint64)
        b = np.zeros((max(n.value, 1), 2), dtype=np.uint64)
        self._check(self.lib.dst_rtree_tapes(self._h, ctypes.c_uint64(index), ctypes.c_uint32(what), _ptr(a), _ptr(b), ctypes.c_size_t(n.value), ctypes.byref(n)))
        return arr_to_ints(a[:n.value]), arr_to_ints(b[:n.value])

    @staticmethod
    def _indices(indices):
        idx = np.ascontiguousarray(np.array([int(i) for i in indices], dtype=np.uint64))
        return idx, (_ptr(idx) if idx.size else None)

    def update(self, indices, leaves):
        """replaces the leaves at the distinct leaf indices `indices` (any order) by `leaves` (as many pairs of ints, or uint64 words
        [count, 2, 2]) and recomputes their ancestors: the tree then equals one built from the modified leaves (dst_rtree_update).  A repeated
        index, an index past the end or an element not below p raises DistaffError(DST_ERR_ARG) and leaves the tree as it was."""
        idx, ip = self._indices(indices)
        a = _elements(leaves, 2)
        if a.shape[0] != idx.size:
            raise DistaffError(DST_ERR_ARG, "as many leaves as indices")
        self._check(self.lib.dst_rtree_update(self._h, ip, _ptr(a) if idx.size else None, ctypes.c_size_t(idx.size)))

    def apply(self, indices, leaves):
        """the writes leaf indices[i] <- leaves[i] one after the other, indices may repeat (dst_rtree_apply) -> (paths, roots): paths[i] opens
        indices[i] in the tree as the earlier writes left it (its first node is the old leaf), roots[i] is the root after write i.  On a device
        tree all writes are hashed together, one launch per level."""
        return _apply(self, self.lib.dst_rtree_apply, self.log_leaves + 1, indices, leaves)

    @property
    def update_ms(self):
        """device milliseconds of the level launches of the last update or apply (0 for a host tree)"""
        ms = ctypes.c_double(0)
        self._check(self.lib.dst_rtree_update_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def paths(self, indices):
        """authentication paths of the leaves `indices` (repeats allowed) in one call (dst_rtree_paths): a list with one path(i) per index, i.e.
        count x (log_leaves + 1) x 2 elements"""
        idx, ip = self._indices(indices)
        n = self.log_leaves + 1
        out = np.zeros((max(idx.size, 1) * n, 2, 2), dtype=np.uint64)
        self._check(self.lib.dst_rtree_paths(self._h, ip, ctypes.c_size_t(idx.size), _ptr(out)))
        v = arr_to_ints(out[:idx.size * n])
        return [[(v[2 * (i * n + k)], v[2 * (i * n + k) + 1]) for k in range(n)] for i in range(idx.size)]

    def multiproof(self, indices, words=False):
        """the multiproof of the DISTINCT leaves `indices`, any order (dst_rtree_multiproof) -> (leaves, nodes): the leaves in the order of
        `indices` and the sibling nodes that cannot be recomputed from them, level by level from the leaf level up, ascending within a level
        -- lists of pairs of ints, or uint64 words [count, 2, 2] and [M, 2, 2] with words=True.  multiproof_root / verify_multiproof check it
        against a root, multiproof_paths expands it into paths(indices)."""
        return _tree_multiproof(self, self.lib.dst_rtree_multiproof, indices, words)

    def tapes_many(self, indices, what=3):
        """tapes(i, what) for every i of `indices` in one call (dst_rtree_tapes_many): a list of (A, B)"""
        idx, ip = self._indices(indices)
        n = ctypes.c_size_t(0)
        self._check(self.lib.dst_rtree_tapes_many(self._h, ip, ctypes.c_size_t(idx.size), ctypes.c_uint32(what), None, None, ctypes.c_size_t(0), ctypes.byref(n)))
        each = n.value
        a = np.zeros((max(idx.size * each, 1), 2), dtype=np.uint64)
        b = np.zeros((max(idx.size * each, 1), 2), dtype=np.uint64)
        self._check(self.lib.dst_rtree_tapes_many(self._h, ip, ctypes.c_size_t(idx.size), ctypes.c_uint32(what), _ptr(a), _ptr(b), ctypes.c_size_t(each), ctypes.byref(n)))
        va, vb = arr_to_ints(a[:idx.size * each]), arr_to_ints(b[:idx.size * each])
        return [(va[i * each:(i + 1) * each], vb[i * each:(i + 1) * each]) for i in range(idx.size)]

    def nodes(self, first, count):
        """`count` nodes of the node array from `first` as uint64 words [count, 2, 2]: index 1 = root, [2^log_leaves, 2^(log_leaves+1)) = the leaves"""
        out = np.zeros((count, 2, 2), dtype=np.uint64)
        self._check(self.lib.dst_rtree_read_nodes(self._h, ctypes.c_uint64(first), ctypes.c_uint64(count), _ptr(out)))
        return out

    def save(self):
        """the tree as bytes (dst_rtree_save): a 64-byte header and the nodes of heap positions 1 and up; include/distaff_hip.h has the layout.
        The same bytes whether the tree lives on the host or on a device."""
        return _tree_save(self, self.lib.dst_rtree_save)

    @classmethod
    def load(cls, blob, device=0, audit=False, lib=None):
        """the tree save() wrote, on `device` (dst_rtree_load), without hashing it again: build_ms is 0.  Malformed bytes raise
        DistaffError(DST_ERR_ARG).  Without `audit` the node values are believed -- the tree is only as good as its blob; with it, audit() runs
        first and a bad node raises DistaffError(DST_ERR_ARG) whose text names it."""
        t = cls.__new__(cls)
        t.lib = lib or load()
        t._h = _tree_load(t.lib, t.lib.dst_rtree_load, _rtree_error, blob, device, audit)
        t.log_leaves = int.from_bytes(bytes(blob[12:16]), "little")
        return t

    def audit(self):
        """None when every parent is the digest of its two children, else the lowest heap position in [1, 2^log_leaves) whose node is not
        (dst_rtree_audit).  One launch on a device tree; audit_ms then holds its device milliseconds.  The tree is unchanged."""
        bad, ms = ctypes.c_int64(0), ctypes.c_double(0)
        self._check(self.lib.dst_rtree_audit(self._h, ctypes.byref(bad), ctypes.byref(ms)))
        self.audit_ms = ms.value
        return None if bad.value < 0 else bad.value

class StreeInfo(ctypes.Structure):
    _fields_ = [("depth", ctypes.c_uint32), ("device", ctypes.c_int32), ("keys", ctypes.c_uint64), ("nodes", ctypes.c_uint64),
                ("last_digests", ctypes.c_uint64), ("last_device_ms", ctypes.c_double)]


class _SparseTree:
    """What SparseRescueTree (dst_stree_*, 8-byte keys) and WideSparseRescueTree (dst_wtree_*, 16-byte keys) share: every call the two handles
    have in common, stated once.  _PREFIX names the entry points, _keys packs the keys of a call, _prefixes / _as_key read keys back."""
    _PREFIX = None

    def _fn(self, name):
        return getattr(self.lib, self._PREFIX + name)

    @staticmethod
    def _keys(indices):
        return RescueTree._indices(indices)

    @staticmethod
    def _prefixes(m):
        return np.zeros(m, dtype=np.uint64)

    def __init__(self, depth, empty_leaf=(0, 0), device=0, lib=None):
        self.lib = lib or load()
        self.depth = int(depth)
        e = _elements([tuple(empty_leaf)], 2)
        h = ctypes.c_void_p()
        r = self._fn("create")(ctypes.c_int(device), ctypes.c_uint32(self.depth), _ptr(e), ctypes.byref(h))
        if r != DST_OK:
            raise DistaffError(r, self._error(None))
        self._h = h

    def _error(self, handle):
        self._fn("last_error").restype = ctypes.c_char_p
        self._fn("last_error").argtypes = [ctypes.c_void_p]
        return (self._fn("last_error")(handle) or b"").decode()

    def _check(self, r):
        if r != DST_OK:
            raise DistaffError(r, self._error(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy").restype = None
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set(self, indices, leaves):
        """inserts or replaces the leaves at the distinct keys `indices` (any order; `leaves`: as many pairs of ints, or uint64 words
        [count, 2, 2]) and hashes exactly their ancestors (dst_stree_set).  A repeated key, a key past 2^depth or an element not below p
        raises DistaffError(DST_ERR_ARG) and leaves the tree as it was."""
        idx, ip = self._keys(indices)
        a = _elements(leaves, 2)
        if a.shape[0] != idx.shape[0]:
            raise DistaffError(DST_ERR_ARG, "as many leaves as indices")
        self._check(self._fn("set")(self._h, ip, _ptr(a) if idx.shape[0] else None, ctypes.c_size_t(idx.shape[0])))

    def apply(self, indices, leaves):
        """RescueTree.apply on keys below 2^depth, stored or not (dst_stree_apply) -> (paths, roots); the old leaf of a key that is not stored is
        the empty leaf.  Afterwards the tree is set()'s of the distinct keys with the later value of each."""
        return _apply(self, self._fn("apply"), self.depth + 1, indices, leaves)

    def remove(self, indices):
        """deletes the stored keys among the distinct keys `indices` (any order) and every node left without a key below it
        (dst_stree_remove) -> how many were stored.  The tree then equals a fresh one set with the remaining keys; only the surviving
        ancestors of the removed keys are hashed.  A repeated key or a key past 2^depth raises DistaffError(DST_ERR_ARG)."""
        idx, ip = self._keys(indices)
        n = ctypes.c_uint64(0)
        self._check(self._fn("remove")(self._h, ip, ctypes.c_size_t(idx.shape[0]), ctypes.byref(n)))
        return n.value

    def compact(self):
        """deletes every stored key whose leaf is the empty leaf and every node left without a key below it (dst_stree_compact) -> how many
        keys.  The root and the remaining nodes do not change and nothing is hashed.  apply(keys, empty leaves) + compact() is a removal
        with a witness per key."""
        n = ctypes.c_uint64(0)
        self._check(self._fn("compact")(self._h, ctypes.byref(n)))
        return n.value

    def get_words(self, indices):
        """get() as (leaves: uint64 words [count, 2, 2], stored: uint8 [count])"""
        idx, ip = self._keys(indices)
        out = np.zeros((idx.shape[0], 2, 2), dtype=np.uint64)
        stored = np.zeros(idx.shape[0], dtype=np.uint8)
        self._check(self._fn("get")(self._h, ip, ctypes.c_size_t(idx.shape[0]), _ptr(out) if idx.shape[0] else None, _ptr(stored) if idx.shape[0] else None))
        return out, stored

    def get(self, indices):
        """the leaves at the keys `indices`, stored or not, repeats allowed, in one call (dst_stree_get) -> (leaves as pairs of ints, stored
        as a list of bool); a key that is not stored has the empty leaf"""
        w, stored = self.get_words(indices)
        v = arr_to_ints(w)
        return [(v[2 * i], v[2 * i + 1]) for i in range(w.shape[0])], [bool(b) for b in stored]

    @property
    def root(self):
        """(r0, r1)"""
        out = np.zeros((2, 2), dtype=np.uint64)
        self._check(self._fn("root")(self._h, _ptr(out)))
        return tuple(arr_to_ints(out))

    def paths_words(self, indices):
        """paths() as uint64 words [count, depth + 1, 2, 2]"""
        idx, ip = self._keys(indices)
        n = self.depth + 1
        out = np.zeros((idx.shape[0], n, 2, 2), dtype=np.uint64)
        self._check(self._fn("paths")(self._h, ip, ctypes.c_size_t(idx.shape[0]), _ptr(out) if idx.shape[0] else None))
        return out

    def paths(self, indices):
        """authentication paths [leaf, sibling, uncle, ...] of the keys `indices`, stored or not, repeats allowed, in one call
        (dst_stree_paths): a list of lists of depth + 1 pairs of ints.  A node that is not stored is the empty subtree of its level."""
        n = self.depth + 1
        w = self.paths_words(indices)
        v = arr_to_ints(w)
        return [[(v[2 * (i * n + k)], v[2 * (i * n + k) + 1]) for k in range(n)] for i in range(w.shape[0])]

    def path(self, index):
        return self.paths([index])[0]

    def tapes_many(self, indices, what=3):
        """RescueTree.tapes_many with n = depth + 1 (dst_stree_tapes_many): a list of (A, B)"""
        idx, ip = self._keys(indices)
        n = ctypes.c_size_t(0)
        self._check(self._fn("tapes_many")(self._h, ip, ctypes.c_size_t(idx.shape[0]), ctypes.c_uint32(what), None, None, ctypes.c_size_t(0), ctypes.byref(n)))
        each = n.value
        a = np.zeros((max(idx.shape[0] * each, 1), 2), dtype=np.uint64)
        b = np.zeros((max(idx.shape[0] * each, 1), 2), dtype=np.uint64)
        self._check(self._fn("tapes_many")(self._h, ip, ctypes.c_size_t(idx.shape[0]), ctypes.c_uint32(what), _ptr(a), _ptr(b), ctypes.c_size_t(each), ctypes.byref(n)))
        va, vb = arr_to_ints(a[:idx.shape[0] * each]), arr_to_ints(b[:idx.shape[0] * each])
        return [(va[i * each:(i + 1) * each], vb[i * each:(i + 1) * each]) for i in range(idx.shape[0])]

    def tapes(self, index, what=3):
        return self.tapes_many([index], what)[0]

    def level(self, l):
        """level l's sorted list (dst_stree_read_level): (prefixes uint64 [m], nodes uint64 words [m, 2, 2]); level depth = the leaves, 0 = the root"""
        m = ctypes.c_uint64(0)
        self._check(self._fn("read_level")(self._h, ctypes.c_uint32(l), ctypes.c_uint64(0), ctypes.c_uint64(0), None, None, ctypes.byref(m)))
        prefixes = self._prefixes(m.value)
        nodes = np.zeros((m.value, 2, 2), dtype=np.uint64)
        if m.value:
            self._check(self._fn("read_level")(self._h, ctypes.c_uint32(l), ctypes.c_uint64(0), ctypes.c_uint64(m.value), _ptr(prefixes), _ptr(nodes), ctypes.byref(m)))
        return prefixes, nodes

    def info(self):
        """dst_stree_info: depth, device, keys, nodes, last_digests, last_device_ms"""
        i = StreeInfo()
        self._check(self._fn("info")(self._h, ctypes.byref(i)))
        return {f: getattr(i, f) for f, _ in StreeInfo._fields_}

    def audit(self):
        """None when every stored parent is the digest of its two children (one that is not stored counts as the empty subtree of its
        level), else (level, prefix) of the bad parent nearest the root, the lowest prefix within its level (dst_stree_audit).  One launch on a
        device tree; audit_ms then holds its device milliseconds.  The tree is unchanged."""
        level, prefix, ms = ctypes.c_int32(0), self._prefixes(1), ctypes.c_double(0)
        self._check(self._fn("audit")(self._h, ctypes.byref(level), _ptr(prefix), ctypes.byref(ms)))
        self.audit_ms = ms.value
        return None if level.value < 0 else (level.value, self._as_key(prefix[0]))

    @staticmethod
    def _as_key(word):
        return int(word)


class SparseRescueTree(_SparseTree):
    """A sparse Rescue Merkle tree (``dst_stree``): the dense RescueTree over 2^depth leaves, 1 <= depth <= 63, in which every leaf that was
    never set holds `empty_leaf`; only the nodes above set leaves are stored.  Same roots, same paths (depth + 1 nodes), same tapes.
    device >= 0 keeps it on that GPU; device < 0 on the host."""
    _PREFIX = "dst_stree_"

    def multiproof(self, indices, words=False):
        """RescueTree.multiproof with n = depth + 1 for distinct keys, stored or not (dst_stree_multiproof) -> (leaves, nodes); a leaf or a
        sibling that is not stored is the empty subtree of its level, so absent keys are proven by the same call"""
        return _tree_multiproof(self, self.lib.dst_stree_multiproof, indices, words)

    def save(self):
        """the tree as bytes (dst_stree_save): a 64-byte header, the level lengths, every level's prefixes, every level's nodes, the leaf level
        first; include/distaff_hip.h has the layout.  The same bytes whether the tree lives on the host or on a device."""
        return _tree_save(self, self.lib.dst_stree_save)

    @classmethod
    def load(cls, blob, device=0, audit=False, lib=None):
        """the tree save() wrote, on `device` (dst_stree_load), without hashing it again: last_digests is 0.  Bytes that are malformed, or
        whose levels create + set could not have made, raise DistaffError(DST_ERR_ARG).  Without `audit` the node values are believed -- the
        tree is only as good as its blob; with it, audit() runs first and a bad node raises DistaffError(DST_ERR_ARG) whose text names it."""
        t = cls.__new__(cls)
        t.lib = lib or load()
        t._h = _tree_load(t.lib, t.lib.dst_stree_load, lambda l: t._error(None), blob, device, audit)
        t.depth = t.info()["depth"]
        return t


class WideSparseRescueTree(_SparseTree):
    """A sparse Rescue Merkle tree over keys of up to 127 bits (``dst_wtree``), 1 <= depth <= 127: the tree SparseRescueTree is, for keys that
    are hashes.  Keys are Python ints; level() returns its prefixes as uint64 words [m, 2] (low half first; arr_to_ints turns them into
    ints) and audit() names a prefix as an int.  The batch opening is batch_proof(), plain or compact; to_blob() / from_blob() save and restore."""
    _PREFIX = "dst_wtree_"

    @staticmethod
    def _keys(indices):
        return _wide_keys(indices)

    @staticmethod
    def _prefixes(m):
        return np.zeros((m, 2), dtype=np.uint64)

    @staticmethod
    def _as_key(word):
        return arr_to_ints(word)[0]

    def batch_proof(self, keys, compact=True, words=False):
        """the multiproof of the distinct keys `keys`, stored or not (dst_wtree_multiproof) -> (leaves, nodes, absent_bits).  compact=True:
        absent_bits is a bytes object with bit m set when supplied node m is not stored -- an empty subtree -- and `nodes` holds the stored ones
        alone; compact=False: the plain form, every supplied node, absent_bits None.  What multiproof_root_wide, verify_multiproof_wide and
        multiproof_paths_wide take.  The plain size query needs no look at the tree, so the buffers are made for M nodes and the tree is asked
        once: on a device tree two launches whatever len(keys) is, and only stored nodes come back."""
        idx, ip = self._keys(keys)
        count = idx.shape[0]
        call = self.lib.dst_wtree_multiproof
        s, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._check(call(self._h, ip, ctypes.c_size_t(count), None, None, ctypes.c_size_t(0), ctypes.byref(m), None, None))      # M: the plan alone
        leaves = np.zeros((count, 2, 2), dtype=np.uint64)
        nodes = np.zeros((max(m.value, 1), 2, 2), dtype=np.uint64)         # a set that needs no sibling still asks for the leaves
        bits = np.zeros((m.value + 7) // 8 + 1, dtype=np.uint8)
        if count:
            self._check(call(self._h, ip, ctypes.c_size_t(count), _ptr(leaves), _ptr(nodes), ctypes.c_size_t(m.value), ctypes.byref(s), _ptr(bits) if compact else None, ctypes.byref(m)))
        nodes, bits = nodes[:s.value], bits[:(m.value + 7) // 8]
        absent = bits.tobytes() if compact else None
        return (leaves, nodes, absent) if words else (_pairs(leaves), _pairs(nodes), absent)

    def to_blob(self):
        """the tree as bytes (dst_wtree_save): SparseRescueTree.save with blob kind 3 and 16-byte prefixes, 64 + 8 * (depth + 1) + 48 * nodes
        bytes; the same bytes whether the tree lives on the host or on a device"""
        return _tree_save(self, self.lib.dst_wtree_save)

    @classmethod
    def from_blob(cls, blob, device=0, audit=False, lib=None):
        """the tree to_blob() wrote, on `device` (dst_wtree_load), without hashing it again; SparseRescueTree.load's refusals, with all 128 bits
        of a prefix compared, and audit=True as there"""
        t = cls.__new__(cls)
        t.lib = lib or load()
        t._h = _tree_load(t.lib, t.lib.dst_wtree_load, lambda l: t._error(None), blob, device, audit)
        t.depth = t.info()["depth"]
        return t

    def test_set_node(self, level, index, node):
        """overwrites entry `index` of level `level`'s node list with the pair `node`, hashing nothing (dst_wtree_test_set_node; the test build
        of the library only): what an audit is then to find"""
        w = _elements([tuple(node)], 2)
        self._check(self.lib.dst_wtree_test_set_node(self._h, ctypes.c_uint32(level), ctypes.c_uint64(index), _ptr(w)))


class Comm:
    """One rank's communicator handle (``dst_comm``) for ``Context.prove_sharded``: RCCL over xGMI, the unique id created by
    ``Comm.unique_id()`` on rank 0 and handed to the other ranks by the host's own channel."""

    def __init__(self, handle):
        self.lib, self._h = load(), handle

    def describe(self):
        """dst_comm_describe: transport, rank / world, and what the transport says about itself -- for RCCL the number of ranks the live
        communicator connected (ncclCommCount), this rank's index and device; for the in-process transport the peer-access picture."""
        info = CommInfo()
        if self.lib.dst_comm_describe(self._h, ctypes.byref(info)) != DST_OK:
            raise DistaffError(DST_ERR_ARG, "dst_comm_describe failed")
        d = {f: int(getattr(info, f)) for f, _ in CommInfo._fields_}
        d["transport"] = ("rccl", "local", "callbacks")[d["transport"]]
        return d

    def set_timeout(self, seconds):
        """dst_comm_set_timeout: limit of every host wait behind a collective of this communicator (default 60 s; <= 0: none).  On expiry
        the rank aborts the communicator and prove_sharded raises DistaffError(DST_ERR_COMM)."""
        if self.lib.dst_comm_set_timeout(self._h, ctypes.c_double(seconds)) != DST_OK:
            raise DistaffError(DST_ERR_ARG, "dst_comm_set_timeout failed")

    def abort(self):
        """dst_comm_abort: gives the communicator up from the host's side; every later collective of this handle fails at once"""
        self.lib.dst_comm_abort(self._h)

    def last_error(self):
        self.lib.dst_comm_last_error.restype = ctypes.c_char_p
        self.lib.dst_comm_last_error.argtypes = [ctypes.c_void_p]
        return self.lib.dst_comm_last_error(self._h).decode()

    def trace(self, enable=-1):
        """dst_comm_trace: the collectives this rank has issued so far as [(kind, bytes per rank, stream index or None)]; enable = 1 starts a
        fresh record, 0 stops, -1 leaves recording as it is."""
        n = ctypes.c_size_t(0)
        self.lib.dst_comm_trace(self._h, ctypes.c_int(-1), None, ctypes.c_size_t(0), ctypes.byref(n))
        buf = ctypes.create_string_buffer(n.value + 1)
        if self.lib.dst_comm_trace(self._h, ctypes.c_int(enable), buf, ctypes.c_size_t(n.value + 1), ctypes.byref(n)) != DST_OK:
            raise DistaffError(DST_ERR_ARG, "dst_comm_trace failed")
        out = []
        for line in buf.value.decode().splitlines():
            k, b, st = line.split()
            out.append((k, int(b), None if st == "-" else int(st)))
        return out

    @staticmethod
    def unique_id():
        lib = load()
        buf = ctypes.create_string_buffer(128)
        if lib.dst_comm_unique_id(buf) != DST_OK:
            lib.dst_comm_last_error.restype = ctypes.c_char_p
            raise DistaffError(DST_ERR_HIP, lib.dst_comm_last_error(None).decode())
        return buf.raw

    @classmethod
    def rccl(cls, unique_id, rank, world, device):
        lib = load()
        h = ctypes.c_void_p()
        if lib.dst_comm_init(bytes(unique_id), ctypes.c_uint32(rank), ctypes.c_uint32(world), ctypes.c_int(device), ctypes.byref(h)) != DST_OK:
            lib.dst_comm_last_error.restype = ctypes.c_char_p
            raise DistaffError(DST_ERR_HIP, lib.dst_comm_last_error(None).decode())
        return cls(h)

    @classmethod
    def local(cls, world):
        """`world` handles whose ranks are threads of this process"""
        lib = load()
        arr = (ctypes.c_void_p * world)()
        if lib.dst_comm_init_local(ctypes.c_uint32(world), arr) != DST_OK:
            raise DistaffError(DST_ERR_ARG, "dst_comm_init_local failed")
        return [cls(ctypes.c_void_p(arr[r])) for r in range(world)]

    @classmethod
    def callbacks(cls, rank, world, fn):
        """The host's own transport: fn(kind, send_address, recv_address, bytes) -> 0 performs kind 0 = all-gather, 1 = all-to-all (device
        buffers), 2 = all-gather of host values."""
        lib = load()
        proto = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)

        def tramp(user, kind, send, recv, nbytes):
            try:
                return int(fn(kind, send, recv, nbytes))
            except Exception:                                         # noqa: BLE001 -- reported as a failed collective
                import traceback
                traceback.print_exc()
                return 1
        cb = proto(tramp)
        h = ctypes.c_void_p()
        if lib.dst_comm_init_callbacks(ctypes.c_uint32(rank), ctypes.c_uint32(world), cb, None, ctypes.byref(h)) != DST_OK:
            raise DistaffError(DST_ERR_ARG, "dst_comm_init_callbacks failed")
        c = cls(h)
        c._keep = cb                                                  # the trampoline must outlive the handle
        return c

    @classmethod
    def over_torch(cls, dist, group=None):
        """dst_prove_sharded's collectives carried by an initialised torch.distributed process group through the callback transport
        (dst_comm_init_callbacks): the host's own channel instead of the library's RCCL binding.  With a gloo group the device buffers
        are staged through host memory (dst_comm_copy), so the ranks may be processes that SHARE one GPU -- which RCCL refuses --
        or sit on hosts without RCCL; with an nccl group the exchange runs on device tensors.  The callbacks block until the
        exchange is complete, as the transport's contract asks."""
        import numpy as np
        import torch
        lib = load()
        lib.dst_comm_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        on_device = str(dist.get_backend(group)).lower() == "nccl"

        def copy(dst, src, nbytes):
            if lib.dst_comm_copy(ctypes.c_void_p(dst), ctypes.c_void_p(src), ctypes.c_size_t(nbytes)) != DST_OK:
                lib.dst_comm_last_error.restype = ctypes.c_char_p
                raise DistaffError(DST_ERR_HIP, lib.dst_comm_last_error(None).decode())

        def staged(src, nbytes):
            """`nbytes` at address `src` as a tensor the process group can send"""
            t = torch.empty(nbytes, dtype=torch.uint8, device="cuda" if on_device else "cpu")
            copy(t.data_ptr(), src, nbytes)
            return t

        def fn(kind, send, recv, nbytes):
            if nbytes == 0:
                return 0
            if kind == 1:                                             # all-to-all: chunk g of `send` goes to rank g
                mine = staged(send, nbytes * world)
                out = torch.empty_like(mine)
                if on_device:
                    dist.all_to_all_single(out, mine, group=group)
                    torch.cuda.synchronize()
                else:                                                 # gloo has no all-to-all on CPU tensors: gather and slice
                    every = [torch.empty_like(mine) for _ in range(world)]
                    dist.all_gather(every, mine, group=group)
                    out = torch.cat([e[rank * nbytes:(rank + 1) * nbytes] for e in every])
                copy(recv, out.data_ptr(), nbytes * world)
                return 0
            if kind == 2 and not on_device:                           # host values
                mine = torch.from_numpy(np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(send)).copy())
            else:
                mine = staged(send, nbytes)                           # (an in-place all-gather hands in send == recv + rank * nbytes: staged first)
            if on_device:
                out = torch.empty(nbytes * world, dtype=torch.uint8, device="cuda")
                dist.all_gather_into_tensor(out, mine, group=group)
                torch.cuda.synchronize()
            else:
                every = [torch.empty_like(mine) for _ in range(world)]
                dist.all_gather(every, mine, group=group)
                out = torch.cat(every)
            if kind == 2 and not on_device:
                ctypes.memmove(recv, out.data_ptr(), nbytes * world)
            else:
                copy(recv, out.data_ptr(), nbytes * world)
            return 0
        return cls.callbacks(rank, world, fn)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.dst_comm_destroy(self._h)
            self._h = None


class Calibration:
    """The calibration kernels of the test / bench build (dependent multiplication chains, multiply-add peak, straight-line-code probe) on
    `device`, through a small context of libdistaff_hip_hooks.so -- the product library does not contain them."""

    def __init__(self, device=0):
        self.ctx = Context(10, 20, 1, 0, device=device, lib=load_hooks())
        if not self.ctx.lib.dst_test_hooks():
            raise RuntimeError("the calibration kernels need the test / bench build (libdistaff_hip_hooks.so)")

    def bench_mad(self, lanes=1 << 21, iters=2048):
        return self.ctx.bench_mad(lanes, iters)

    def bench_mulmod(self, lanes=1 << 20, iters=256, portable=False):
        return self.ctx.bench_mulmod(lanes, iters, portable)

    def bench_code(self, code_kib):
        return self.ctx.bench_code(code_kib)

    def bench_clock(self, lanes=1 << 20, iters=1024):
        """dst_bench_clock: MHz of the shader clock under four fe_mul chains per lane on every SIMD (median over the wavefronts)"""
        mhz = ctypes.c_double(0)
        self.ctx._check(self.ctx.lib.dst_bench_clock(self.ctx._h, ctypes.c_uint64(lanes), ctypes.c_uint32(iters), ctypes.byref(mhz)))
        return mhz.value

    def close(self):
        self.ctx.close()


def prove_sharded_local(contexts, inputs, outputs, cap=1 << 22):
    """dst_prove_sharded_local: one proof over `len(contexts)` contexts (rank r of world, trace uploaded on each), one thread per
    context inside the library, in-process transport."""
    lib = load()
    world = len(contexts)
    arr = (ctypes.c_void_p * world)(*[c._h.value for c in contexts])
    pub = make_public(inputs, outputs)
    buf = ctypes.create_string_buffer(cap)
    ln = ctypes.c_size_t(0)
    r = lib.dst_prove_sharded_local(arr, ctypes.c_uint32(world), ctypes.byref(pub), buf, ctypes.c_size_t(cap), ctypes.byref(ln))
    if r != DST_OK:
        msgs = [lib.dst_last_error(c._h).decode() for c in contexts]
        raise DistaffError(r, "; ".join("rank %d: %s" % (i, m) for i, m in enumerate(msgs) if m))
    return buf.raw[:ln.value]


class Context:
    """One proving job on one GPU (``dst_ctx``): owns the device buffers; phases mirror stark::prove (prover.rs:17-168)."""

    def __init__(self, log_n, width, ctx_depth, loop_depth, log_blowup=5, num_queries=50, grinding=20, device=0, rank=0, world=1, lib=None):
        self.lib = lib or load()
        self.params = Params(log_n, log_blowup, width, ctx_depth, loop_depth, num_queries, grinding, device, rank, world)
        self.n, self.B, self.W = 1 << log_n, 1 << log_blowup, width
        self.N = self.n * self.B
        h = ctypes.c_void_p()
        r = self.lib.dst_ctx_create(ctypes.byref(self.params), ctypes.byref(h))
        if r != DST_OK:
            raise DistaffError(r, self.lib.dst_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.dst_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, r):
        if r != DST_OK:
            raise DistaffError(r, self.lib.dst_last_error(self._h).decode())

    def upload(self, columns):
        cols = np.ascontiguousarray(columns, dtype=np.uint64)
        assert cols.shape == (self.W, self.n, 2), cols.shape
        self._check(self.lib.dst_trace_upload_contiguous(self._h, _ptr(cols)))

    def pinned_trace(self, columns):
        """Copies the trace into page-locked host memory owned by the library and returns (pointer table, keep-alive handle) for
        upload_async: the host-resident TraceTable of the reference, placed where asynchronous DMA can read it."""
        cols = np.ascontiguousarray(columns, dtype=np.uint64)
        assert cols.shape == (self.W, self.n, 2), cols.shape
        p = ctypes.c_void_p()
        if self.lib.dst_pinned_alloc(ctypes.c_size_t(cols.nbytes), ctypes.byref(p)) != DST_OK:
            raise DistaffError(DST_ERR_HIP, "dst_pinned_alloc failed")
        ctypes.memmove(p, cols.ctypes.data, cols.nbytes)
        table = (ctypes.c_void_p * self.W)(*[p.value + i * self.n * 16 for i in range(self.W)])
        return table, p

    def release_pinned(self, handle):
        self.lib.dst_pinned_free(handle)

    def upload_owned(self, cols):
        """dst_trace_upload_owned: only the registers this rank interpolates (r = rank mod world) travel to the device; for prove_sharded"""
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        rank, world = self.params.rank, self.params.world
        ptrs = (ctypes.c_void_p * self.W)(*[cols[i].ctypes.data if i % world == rank else None for i in range(self.W)])
        self._check(self.lib.dst_trace_upload_owned(self._h, ptrs))

    def upload_async(self, table):
        """dst_trace_upload_async: returns at once, the next commit_trace() / prove() consumes the registers as they arrive"""
        self._check(self.lib.dst_trace_upload_async(self._h, table))

    def prove_sharded(self, comm, inputs, outputs, cap=1 << 22):
        """dst_prove_sharded: this rank's part of one proof over the communicator's ranks (every rank calls it, every rank gets the proof)"""
        pub = make_public(inputs, outputs)
        buf = ctypes.create_string_buffer(cap)
        ln = ctypes.c_size_t(0)
        self._check(self.lib.dst_prove_sharded(self._h, comm._h, ctypes.byref(pub), buf, ctypes.c_size_t(cap), ctypes.byref(ln)))
        return buf.raw[:ln.value]

    def shard_stage_ms(self):
        """host-side view of the last prove_sharded: ms inside the transport's calls, ms waiting for tree roots, tree exchanges"""
        v = (ctypes.c_double * 3)()
        self._check(self.lib.dst_shard_stage_ms(self._h, v))
        return {"transport_calls": v[0], "root_waits": v[1], "tree_exchanges": int(v[2])}

    def shard_exchange_ms(self):
        """dst_shard_exchange_ms: enqueue -> completion of the collectives of the last prove_sharded, per kind, from events on their streams"""
        v = (ctypes.c_double * 8)()
        self._check(self.lib.dst_shard_exchange_ms(self._h, v))
        return {"coefficients": v[0], "tree_all_to_all": v[1], "tree_all_gather": v[2], "constraint_evaluations": v[3], "fri_tail": v[4],
                "host_values": v[5], "collectives": int(v[6]), "timed_by_events": int(v[7])}

    def commit_trace(self):
        root = ctypes.create_string_buffer(32)
        self._check(self.lib.dst_commit_trace(self._h, root))
        return root.raw

    def eval_constraints(self, inputs, outputs, coeffs):
        c = np.ascontiguousarray(coeffs, dtype=np.uint64)
        assert c.shape == (344, 2)
        root = ctypes.create_string_buffer(32)
        bad = ctypes.c_int64(-1)
        pub = make_public(inputs, outputs)
        r = self.lib.dst_eval_constraints(self._h, ctypes.byref(pub), _ptr(c), root, ctypes.byref(bad))
        self.bad_step = bad.value
        self._check(r)
        return root.raw

    def compose(self, draws):
        d = np.ascontiguousarray(draws, dtype=np.uint64)
        assert d.shape == (516, 2)
        z1 = np.zeros((self.W, 2), dtype=np.uint64)
        z2 = np.zeros((self.W, 2), dtype=np.uint64)
        self._check(self.lib.dst_compose(self._h, _ptr(d), _ptr(z1), _ptr(z2)))
        return z1, z2

    def fri_commit_layer(self):
        root = ctypes.create_string_buffer(32)
        more = ctypes.c_int(0)
        self._check(self.lib.dst_fri_commit_layer(self._h, root, ctypes.byref(more)))
        return root.raw, bool(more.value)

    def fri_fold(self, special_x):
        self._check(self.lib.dst_fri_fold(self._h, int_to_bytes(special_x)))

    def pow_grind(self, seed, grinding):
        out = ctypes.create_string_buffer(32)
        nonce = ctypes.c_uint64(0)
        self._check(self.lib.dst_pow_grind(self._h, bytes(seed), ctypes.c_uint32(grinding), out, ctypes.byref(nonce)))
        return out.raw, nonce.value

    def build_proof(self, positions, pow_nonce):
        pos = np.asarray(positions, dtype=np.uint64)
        ln = ctypes.c_size_t(0)
        self._check(self.lib.dst_build_proof(self._h, _ptr(pos), ctypes.c_uint32(len(positions)), ctypes.c_uint64(pow_nonce), None, ctypes.c_size_t(0), ctypes.byref(ln)))
        buf = ctypes.create_string_buffer(ln.value)
        self._check(self.lib.dst_build_proof(self._h, _ptr(pos), ctypes.c_uint32(len(positions)), ctypes.c_uint64(pow_nonce), buf, ctypes.c_size_t(ln.value), ctypes.byref(ln)))
        return buf.raw[:ln.value]

    def prove(self, inputs, outputs, cap=1 << 22):
        """stark::prove on the uploaded trace; returns the serialised StarkProof."""
        pub = make_public(inputs, outputs)
        buf = ctypes.create_string_buffer(cap)
        ln = ctypes.c_size_t(0)
        r = self.lib.dst_prove(self._h, ctypes.byref(pub), buf, ctypes.c_size_t(cap), ctypes.byref(ln))
        if hasattr(self.lib, "dst_last_bad_step"):                     # a library named by DISTAFF_HIP_LIB may predate it
            self.bad_step = self.lib.dst_last_bad_step(self._h)
        self._check(r)
        return buf.raw[:ln.value]

    def phase_ms(self):
        ms = (ctypes.c_double * 9)()
        self._check(self.lib.dst_phase_ms(self._h, ms))
        return list(ms)

    def read(self, what, arg=0):
        ln = ctypes.c_size_t(0)
        self._check(self.lib.dst_read_buffer(self._h, ctypes.c_uint32(BUF[what]), ctypes.c_uint32(arg), None, ctypes.c_size_t(0), ctypes.byref(ln)))
        buf = np.zeros(ln.value, dtype=np.uint8)
        self._check(self.lib.dst_read_buffer(self._h, ctypes.c_uint32(BUF[what]), ctypes.c_uint32(arg), _ptr(buf), ctypes.c_size_t(ln.value), ctypes.byref(ln)))
        return buf

    def read_elements(self, what, arg=0):
        return self.read(what, arg).view(np.uint64).reshape(-1, 2)

    # ---- coset-sharded phases (world > 1): see distaff_amd/sharded.py ------------------------------------------------
    def shard_commit_trace(self):
        self._check(self.lib.dst_shard_commit_trace(self._h))

    def shard_eval_constraints(self, inputs, outputs, coeffs):
        c = np.ascontiguousarray(coeffs, dtype=np.uint64)
        bad = ctypes.c_int64(-1)
        pub = make_public(inputs, outputs)
        r = self.lib.dst_shard_eval_constraints(self._h, ctypes.byref(pub), _ptr(c), ctypes.byref(bad))
        if r == DST_ERR_AIR:
            return bad.value
        self._check(r)
        return -1

    def shard_combine(self):
        self._check(self.lib.dst_shard_combine(self._h))

    def shard_fri_layer(self):
        more = ctypes.c_int(0)
        self._check(self.lib.dst_shard_fri_layer(self._h, ctypes.byref(more)))
        return bool(more.value)

    def fri_fold_shard(self, special_x):
        self._check(self.lib.dst_shard_fri_fold(self._h, int_to_bytes(special_x)))

    def shard_export_size(self, what, arg=0):
        n = ctypes.c_size_t(0)
        self._check(self.lib.dst_shard_export_size(self._h, ctypes.c_uint32(what), ctypes.c_uint32(arg), ctypes.byref(n)))
        return n.value

    def shard_export(self, what, arg, dst_ptr, is_device):
        self._check(self.lib.dst_shard_export(self._h, ctypes.c_uint32(what), ctypes.c_uint32(arg), ctypes.c_void_p(dst_ptr), int(is_device)))

    def shard_import(self, what, arg, src_ptr, is_device):
        root = ctypes.create_string_buffer(32)
        self._check(self.lib.dst_shard_import(self._h, ctypes.c_uint32(what), ctypes.c_uint32(arg), ctypes.c_void_p(src_ptr), int(is_device), root))
        return root.raw

    def shard_read(self, buffer, arg, indices):
        idx = np.asarray(indices, dtype=np.uint64)
        item = self.W * 16 if buffer == 10 else (16 if buffer in (3, 6, 11) else 32)
        out = np.zeros(len(indices) * item, dtype=np.uint8)
        self._check(self.lib.dst_shard_read(self._h, ctypes.c_uint32(buffer), ctypes.c_uint32(arg), _ptr(idx), ctypes.c_uint32(len(indices)), _ptr(out)))
        return out.tobytes()

    def shard_fri_begin(self, send_ptr, is_device, cap):
        """-> (bytes written into the send buffer, another layer follows)"""
        n, more = ctypes.c_size_t(0), ctypes.c_int(0)
        self._check(self.lib.dst_shard_fri_begin(self._h, ctypes.c_void_p(send_ptr), ctypes.c_int(1 if is_device else 0), ctypes.c_size_t(cap),
                                                 ctypes.byref(n), ctypes.byref(more)))
        return n.value, bool(more.value)

    def shard_fri_end(self, gathered_ptr, is_device):
        root = ctypes.create_string_buffer(32)
        self._check(self.lib.dst_shard_fri_end(self._h, ctypes.c_void_p(gathered_ptr), ctypes.c_int(1 if is_device else 0), root))
        return root.raw

    def shard_fri_roots(self):
        """-> (roots of all FRI layers after the commit phase, first layer of the replicated tail)"""
        layers, rep = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(self.lib.dst_shard_fri_roots(self._h, None, ctypes.c_size_t(0), ctypes.byref(layers), ctypes.byref(rep)))
        buf = ctypes.create_string_buffer(32 * layers.value)
        self._check(self.lib.dst_shard_fri_roots(self._h, buf, ctypes.c_size_t(32 * layers.value), ctypes.byref(layers), ctypes.byref(rep)))
        return [buf.raw[32 * d:32 * d + 32] for d in range(layers.value)], rep.value

    def shard_open(self, positions):
        """-> (this rank's blob of openings, [blob length of every rank])"""
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        ln = ctypes.c_size_t(0)
        lens = np.zeros(self.params.world, dtype=np.uint64)
        self._check(self.lib.dst_shard_open(self._h, _ptr(pos), ctypes.c_uint32(len(pos)), None, ctypes.c_size_t(0), ctypes.byref(ln), _ptr(lens)))
        blob = np.zeros(max(ln.value, 1), dtype=np.uint8)
        self._check(self.lib.dst_shard_open(self._h, _ptr(pos), ctypes.c_uint32(len(pos)), _ptr(blob), ctypes.c_size_t(ln.value), ctypes.byref(ln), None))
        return blob[:ln.value], [int(v) for v in lens]

    def shard_assemble(self, positions, nonce, blobs, lens):
        """blobs: uint8 array holding the ranks' blobs back to back"""
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        bl = np.ascontiguousarray(blobs, dtype=np.uint8)
        ls = np.ascontiguousarray(lens, dtype=np.uint64)
        ln = ctypes.c_size_t(0)
        args = (self._h, _ptr(pos), ctypes.c_uint32(len(pos)), ctypes.c_uint64(nonce), _ptr(bl), _ptr(ls))
        self._check(self.lib.dst_shard_assemble(*args, None, ctypes.c_size_t(0), ctypes.byref(ln)))
        out = np.zeros(ln.value, dtype=np.uint8)
        self._check(self.lib.dst_shard_assemble(*args, _ptr(out), ctypes.c_size_t(ln.value), ctypes.byref(ln)))
        return out.tobytes()

    def shard_info(self):
        op = ctypes.c_uint64(0); layers = ctypes.c_uint32(0); sd = ctypes.c_uint32(0)
        self._check(self.lib.dst_shard_info(self._h, ctypes.byref(op), ctypes.byref(layers), ctypes.byref(sd)))
        return op.value, layers.value, sd.value

    def set_profiling(self, level=1):
        """0 / False: off, 1 / True: every kernel launch, 2: heavy kernels only (see include/distaff_hip.h)"""
        self._check(self.lib.dst_set_profiling(self._h, int(level)))

    def kernel_stats(self, reset=True):
        import json
        buf = ctypes.create_string_buffer(1 << 16)
        self._check(self.lib.dst_kernel_stats(self._h, buf, ctypes.c_size_t(1 << 16), int(reset)))
        return json.loads(buf.value.decode())

    def field_op(self, op, a, b):
        ops = {"add": 0, "sub": 1, "mul": 2, "mul_portable": 3, "inv": 4, "pow": 5, "dot40": 6, "mul_tw": 7, "shift64": 8, "addsub_sum": 9, "addsub_dif": 10,
               "mul_small": 11, "sqr": 12, "cube": 13}
        ops.update({"dot%d" % t: 256 + t for t in range(1, 65) if t != 40})        # dotT: the sum of dot40 over T terms
        a = np.ascontiguousarray(a, dtype=np.uint64); b = np.ascontiguousarray(b, dtype=np.uint64)
        out = np.zeros_like(a)
        self._check(self.lib.dst_field_op(self._h, ops[op], _ptr(a), _ptr(b), _ptr(out), ctypes.c_size_t(a.shape[0])))
        return out

    def bench_mad(self, lanes=1 << 21, iters=2048):
        """milliseconds for lanes * iters * 32 multiply-adds v_mad_u64_u32 (the integer-multiplier peak of the device)"""
        ms = ctypes.c_double(0)
        self._check(self.lib.dst_bench_mad(self._h, ctypes.c_uint64(lanes), ctypes.c_uint32(iters), ctypes.byref(ms)))
        return ms.value

    def bench_code(self, code_kib):
        """milliseconds for 2^23 lanes to run 16 or 176 KiB of straight-line multiply-adds once (box fingerprint, kernels_probe.hip)"""
        ms = ctypes.c_double(0)
        self._check(self.lib.dst_bench_code(self._h, ctypes.c_uint32(code_kib), ctypes.byref(ms)))
        return ms.value

    def bench_mulmod(self, lanes=1 << 20, iters=256, portable=False):
        ms = ctypes.c_double(0)
        self._check(self.lib.dst_bench_mulmod(self._h, ctypes.c_uint64(lanes), ctypes.c_uint32(iters | (0x80000000 if portable else 0)), ctypes.byref(ms)))
        return ms.value
