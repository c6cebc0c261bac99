"""dst_verify / dst_proof_info: the library's host-side verifier (distaff_amd/csrc/verify/) against the oracle's restatement of the reference
verifier.  No GPU: proofs come from the oracle's prover.  Every verdict below is taken from the PRODUCT library (libdistaff_hip.so, opened here by
path: the session itself binds the test build) through distaff_amd.verify; tests/test_verify_gpu.py runs the same call on both builds."""
import functools
import os
import random
import struct
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distaff_amd", "csrc")
HOST_SRC = os.path.join(ROOT, "tests", "verify_host", "verify_corpus.cpp")
WORKER = os.path.join(ROOT, "tests", "verify_host", "oracle_worker.py")
LOW_DEGREE = "verification of low-degree proof failed: "


@functools.lru_cache(maxsize=None)
def _fib_proof(log_n, ext=32, queries=50, grinding=20):
    import oracle as O
    t = O.fibonacci_trace(1 << log_n)
    p = O.Prover.from_trace(t, 1, ext=ext, num_queries=queries, grinding=grinding)
    return p.prove(), bytes(t.program_hash), tuple(t.public_inputs), tuple(p.outputs)


@functools.lru_cache(maxsize=None)
def _product():
    import ctypes
    import distaff_amd as D
    lib = ctypes.CDLL(D.PRODUCT_LIB)
    assert lib.dst_test_hooks() == 0
    return lib


def _verify(proof, program_hash, inputs, outputs):
    import distaff_amd as D
    return D.verify(proof, program_hash, inputs, outputs, lib=_product())


def _info(proof):
    import distaff_amd as D
    return D.proof_info(proof, lib=_product())


def _both(O, D, proof, program_hash, inputs, outputs):
    """(oracle verdict, product verdict); bytes the product calls malformed (DST_ERR_ARG: accepted = 0 and the reason in `err`) are (False, reason)"""
    want = O.verify(proof, program_hash, list(inputs), list(outputs))
    try:
        got = _verify(proof, program_hash, list(inputs), list(outputs))
    except D.DistaffError as e:
        assert e.code == D.DST_ERR_ARG
        got = (False, e.reason)
    return want, got


# ---- 1: accepts what the oracle proves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 32, 50, 20), (8, 32, 50, 20), (10, 32, 50, 20), (12, 32, 50, 20), (8, 16, 100, 0), (8, 64, 50, 20)],
                         ids=lambda s: "2^%d-ext%d-q%d-g%d" % s)
def test_accepts_oracle_proofs(oracle, shape):
    """Fibonacci traces of 2^7, 2^8, 2^10 and 2^12 steps at the default options, one at extension 16 / 100 queries / grinding 0, one at
    extension 64: the oracle's verifier and dst_verify both accept the oracle's proof."""
    import distaff_amd as D
    proof, ph, ins, outs = _fib_proof(*shape)
    want, got = _both(oracle, D, proof, ph, ins, outs)
    assert want == (True, "") and got == (True, "")


# ---- 2: the whole instruction set and every block kind -----------------------------------------------------------------------------------
def _isa():
    from test_gpu_parity import ISA_TRACE_NAMES, _isa_traces                    # the list the GPU parity tests use, unchanged
    return ISA_TRACE_NAMES, _isa_traces


@functools.lru_cache(maxsize=None)
def _isa_proof(name):
    import oracle as O
    trace, num_outputs = _isa()[1](O)[name]
    p = O.Prover.from_trace(trace, num_outputs, grinding=8)
    return p.prove(), bytes(trace.program_hash), tuple(trace.public_inputs), tuple(p.outputs), (trace.length, trace.width, trace.ctx_depth, trace.loop_depth)


@pytest.mark.parametrize("name", _isa()[0])
def test_accepts_the_whole_instruction_set(oracle, name):
    """The 21 traces of tests/test_gpu_parity.py (all 32 user operations, all 8 flow operations, context depth up to 2, loop depth up to 2, `if`
    and `while` programs), each proven by the oracle at its natural length: accepted -- which pins the host AIR at z for every operation --
    and rejected for a wrong output with the oracle's words."""
    import distaff_amd as D
    proof, ph, ins, outs, _ = _isa_proof(name)
    want, got = _both(oracle, D, proof, ph, ins, outs)
    assert want == (True, "") and got == (True, "")
    bad = list(outs); bad[0] = (bad[0] + 1) % oracle.P
    want, got = _both(oracle, D, proof, ph, ins, bad)
    assert want[0] is False and got == want


# ---- 3: rejects what the reference rejects, in its words -----------------------------------------------------------------------------------
def test_rejects_wrong_public_data_and_tampering(oracle):
    """/root/reference/src/tests/mod.rs:47-62 (wrong input, wrong output, wrong program hash) and the tamperings of the GPU parity tests (a flipped
    byte at offset 40 -- a length prefix: both sides say "proof truncated" --, in the middle, in an opened trace value): accepted == 0 and the
    oracle's error string."""
    import distaff_amd as D
    O = oracle
    proof, ph, ins, outs = _fib_proof(8)
    cases = [(proof, ph, (1, 1), outs), (proof, ph, ins, (outs[0] + 1,)), (proof, bytes(32), ins, outs), (proof, ph[16:] + ph[:16], ins, outs)]
    for off in (40, len(proof) // 2, len(proof) - 5, 3, 36):
        bad = bytearray(proof); bad[off] ^= 1
        cases.append((bytes(bad), ph, ins, outs))
    seen = set()
    for pr, h, i, o in cases:
        want, got = _both(O, D, pr, h, i, o)
        assert want[0] is False and got == want, (want, got)
        seen.add(want[1])
    assert LOW_DEGREE + "evaluations did not match column value at depth 0" in seen and "verification of trace Merkle proof failed" in seen
    assert "seed proof-of-work verification failed" in seen


# ---- 4: verdict parity under mutation ----------------------------------------------------------------------------------------------------
def proof_sections(b):
    """[(name, start, end)] over the bincode image of a StarkProof (proof.rs:11-37): every byte belongs to exactly one section"""
    o = 0
    out = []

    def u64():
        return struct.unpack_from("<Q", b, o)[0]

    def skip_hvv(o):
        k, = struct.unpack_from("<Q", b, o); o += 8
        for _ in range(k):
            m, = struct.unpack_from("<Q", b, o); o += 8 + 32 * m
        return o

    out.append(("root:trace", 0, 32)); o = 32
    out.append(("header", o, o + 8)); o += 8
    e = skip_hvv(o); out.append(("paths:trace", o, e)); o = e
    s = o; k = u64(); o += 8
    for _ in range(k):
        m, = struct.unpack_from("<Q", b, o); o += 8 + 16 * m
    out.append(("trace_rows", s, o))
    out.append(("root:constraint", o, o + 32)); o += 32
    s = o; k = u64(); o += 8 + 32 * k
    out.append(("constraint_values", s, o))
    e = skip_hvv(o) + 1; out.append(("paths:constraint", o, e)); o = e
    s = o
    for _ in range(2):
        k = u64(); o += 8 + 16 * k
    out.append(("deep_values", s, o))
    layers = u64(); out.append(("fri_count", o, o + 8)); o += 8
    for i in range(layers):
        s = o; o += 32
        k = u64(); o += 8 + 64 * k
        out.append(("fri%d:values" % i, s, o))
        e = skip_hvv(o) + 1; out.append(("fri%d:paths" % i, o, e)); o = e
    s = o; o += 32; k = u64(); o += 8 + 16 * k
    out.append(("remainder", s, o))
    out.append(("nonce", o, o + 8)); o += 8
    out.append(("options", o, o + 4)); o += 4
    assert o == len(b)
    return out


MUTANTS_PER_PROOF = 1500        # N: byte offsets per proof, one flipped bit each, shared out evenly over the sections
MUTATION_SEED = 20260116


def _mutants(proof, seed):
    """stratified by section: the same quota of offsets per section (all of a section that is smaller than its quota), so the 4 option bytes, the
    8 header bytes and the nonce are all hit; one bit per offset, both drawn by random.Random(seed)"""
    rnd = random.Random(seed)
    sections = proof_sections(proof)
    quota = MUTANTS_PER_PROOF // len(sections)
    out = []
    for name, s, e in sections:
        offsets = list(range(s, e)) if e - s <= quota else rnd.sample(range(s, e), quota)
        for off in offsets:
            bit = rnd.randrange(8)
            m = bytearray(proof); m[off] ^= 1 << bit
            out.append((name, off, bit, bytes(m)))
    return out


def _corpus(program_hash, inputs, outputs, items):
    b = bytes(program_hash) + struct.pack("<II", len(inputs), len(outputs)) + b"".join(int(v).to_bytes(16, "little") for v in list(inputs) + list(outputs))
    return b + struct.pack("<I", len(items)) + b"".join(struct.pack("<Q", len(it)) + it for it in items)


def _oracle_verdicts(path, count):
    """the oracle on every item of a corpus file, in a process of its own (tests/verify_host/oracle_worker.py): (ok, error) per item, or
    (False, None) where the oracle died on it (an assertion, an undefined shift, an allocation beyond the limit, the alarm)"""
    res = {}
    first = 0
    _oracle_verdicts.stderr = []                             # what the worker said when it died, for the failure message
    while first < count:
        r = subprocess.run([sys.executable, WORKER, path, str(first)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        for line in r.stdout.splitlines():
            i, ok, err = line.split("\t", 2)
            res[int(i)] = (ok == "1", err)
        done = max(res) + 1 if res else first
        if done < count and r.returncode == 0 and done == first:
            raise RuntimeError("oracle worker made no progress at item %d" % first)
        if done < count:
            res[done] = (False, None)                       # the worker died on this one
            _oracle_verdicts.stderr.append((done, r.returncode, r.stderr[-500:]))
            done += 1
        first = done
    return [res[i] for i in range(count)]


@pytest.mark.parametrize("log_n", [8, 10])
def test_verdict_parity_under_mutation(oracle, tmp_path, log_n):
    """One flipped bit at each of N = 1500 byte offsets of a 2^8 and of a 2^10 proof (seed 20260116 + log_n), stratified over the sections of the
    proof: options, roots, header, deep values, trace rows, every Merkle path group, every FRI layer, the remainder, the nonce.  For EVERY
    mutant dst_verify and the oracle agree on accept / reject, and on the error string when both parsed it; a mutant the product calls
    malformed (DST_ERR_ARG) is one the oracle fails on too (it rejects it, refuses to parse it, or dies on it).  A section shorter than its
    quota of N / (number of sections) offsets is taken whole, so the count is 1088 mutants at 2^8 and 1142 at 2^10.
    The 4 option bytes are also enumerated bit by bit in test_every_bit_of_the_option_bytes, with the one case where the two differ."""
    import distaff_amd as D
    proof, ph, ins, outs = _fib_proof(log_n)
    mutants = _mutants(proof, MUTATION_SEED + log_n)
    sections = {name for name, _, _, _ in mutants}
    assert {"options", "header", "nonce", "remainder", "deep_values", "trace_rows", "root:trace", "root:constraint", "paths:trace", "paths:constraint", "fri0:values", "fri0:paths"} <= sections
    path = str(tmp_path / "mutants.bin")
    open(path, "wb").write(_corpus(ph, ins, outs, [m[3] for m in mutants]))
    t0 = time.time()
    want = _oracle_verdicts(path, len(mutants))
    t1 = time.time()
    disagree, tally = [], {"accept": 0, "reject": 0, "malformed": 0, "oracle_died": 0, "strings_compared": 0}
    for (name, off, bit, m), (w_ok, w_err) in zip(mutants, want):
        try:
            g_ok, g_err = _verify(m, ph, list(ins), list(outs))
            kind = "accept" if g_ok else "reject"
        except D.DistaffError as e:
            assert e.code == D.DST_ERR_ARG
            g_ok, g_err, kind = False, None, "malformed"
        tally[kind] += 1
        tally["oracle_died"] += w_err is None
        oracle_parsed = w_err is not None and not w_err.startswith(("proof truncated", "trailing bytes", "unsupported hash", "std::", "vector", "cannot create"))
        tally["strings_compared"] += kind == "reject" and oracle_parsed
        if g_ok != w_ok or (kind == "reject" and oracle_parsed and g_err != w_err):
            disagree.append((name, off, bit, (w_ok, w_err), (kind, g_err)))
    print("2^%d: %d mutants, %s; oracle %.1f s, product %.1f s" % (log_n, len(mutants), tally, t1 - t0, time.time() - t1))
    assert not disagree, disagree[:10]
    assert tally["reject"] > 100 and tally["malformed"] > 10
    # the comparison compared something: the oracle ran (it may die on a few damaged headers, not on 5 % of the mutants), and hundreds of
    # rejections were matched string by string
    assert tally["oracle_died"] * 20 < len(mutants), _oracle_verdicts.stderr[:3]
    assert tally["strings_compared"] >= 300 and sum(1 for ok, err in want if err is not None) > 0.95 * len(mutants)


@pytest.mark.parametrize("log_n", [8, 10])
def test_every_bit_of_the_option_bytes(oracle, tmp_path, log_n):
    """All 32 one-bit mutants of the 4 option bytes (extension, queries, grinding, hash tag), whatever a seed would draw.  The same rule as in
    the mutation test holds for 30 of them.  The other two are pinned as the one place where product and oracle differ: bit 6 or 7 of the
    extension byte gives log2(extension) = 69 or 133, outside options.rs:35-46, which the product refuses as malformed with that rule's text;
    the oracle (oracle/prover.hpp:408), like the reference's release build, computes 1 << 69 as 1 << 5 -- an undefined shift -- and so
    verifies the proof as if the byte were intact.  The product is specified to refuse such a byte, so it cannot follow the oracle there."""
    import distaff_amd as D
    proof, ph, ins, outs = _fib_proof(log_n)
    base = len(proof) - 4
    mutants = []
    for byte in range(4):
        for bit in range(8):
            m = bytearray(proof); m[base + byte] ^= 1 << bit
            mutants.append((byte, bit, bytes(m)))
    path = str(tmp_path / "options.bin")
    open(path, "wb").write(_corpus(ph, ins, outs, [m[2] for m in mutants]))
    want = _oracle_verdicts(path, len(mutants))
    assert sum(err is None for _, err in want) <= 4, _oracle_verdicts.stderr[:3]      # a wild extension factor may cost the oracle its memory limit
    for (byte, bit, m), (w_ok, w_err) in zip(mutants, want):
        try:
            got = _verify(m, ph, list(ins), list(outs))
        except D.DistaffError as e:
            assert e.code == D.DST_ERR_ARG
            got = ("malformed", e.reason)
        if byte == 0 and bit in (6, 7):
            assert got == ("malformed", "extension_factor must be a power of 2 between 16 and 256") and (w_ok, w_err) == (True, ""), (byte, bit, got, w_ok, w_err)
        elif got[0] == "malformed":
            assert not w_ok, (byte, bit, got, w_ok, w_err)
        else:
            assert got[0] == w_ok and (w_err is None or got[1] == w_err), (byte, bit, got, w_ok, w_err)


def test_values_not_below_the_modulus_and_long_remainders_are_refused(oracle):
    """Field elements cross the C-ABI canonical (include/distaff_hip.h): a public value or a proof element >= p is DST_ERR_ARG, not arithmetic
    on a non-residue.  A remainder that is not the last layer of the proof's own FRI layers (here: twice as long) is refused before the
    quadratic remainder check sees it."""
    import distaff_amd as D
    proof, ph, ins, outs = _fib_proof(8)
    P = oracle.P
    for bad_ins, bad_outs in (([1, P], list(outs)), (list(ins), [P]), (list(ins), [(1 << 128) - 1])):
        with pytest.raises(D.DistaffError) as e:
            _verify(proof, ph, bad_ins, bad_outs)
        assert e.value.code == D.DST_ERR_ARG and e.value.reason == "public value not below the modulus"
    assert _verify(proof, ph, list(ins), [P - 1])[0] is False                                  # the largest residue is a value like any other
    sec = {name: (s, e) for name, s, e in proof_sections(proof)}
    for name, skip in (("deep_values", 8), ("trace_rows", 16), ("remainder", 40), ("fri0:values", 40)):
        for value in (P, (1 << 128) - 1):
            b = bytearray(proof); o = sec[name][0] + skip; b[o:o + 16] = value.to_bytes(16, "little")
            with pytest.raises(D.DistaffError) as e:
                _verify(bytes(b), ph, list(ins), list(outs))
            assert e.value.reason == "field element not below the modulus", name
    s, e_ = sec["remainder"]
    k, = struct.unpack_from("<Q", proof, s + 32)
    longer = proof[:s + 32] + struct.pack("<Q", 2 * k) + proof[s + 40:e_] + proof[s + 40:e_] + proof[e_:]
    assert proof_sections(longer)[-3][0] == "remainder"                                         # still a well-formed image
    with pytest.raises(D.DistaffError) as e:
        _verify(longer, ph, list(ins), list(outs))
    assert e.value.reason == "remainder length does not match the low-degree proof's layers"
    with pytest.raises(D.DistaffError):
        _info(longer)


# ---- 5: malformed input never crashes --------------------------------------------------------------------------------------------------------
def _malformed_corpus(proof):
    items = [b"", b"\x00", proof[:-1], proof + b"\x00"]
    items += [proof[:k] for k in range(0, len(proof), 997)] + [proof[:k] for k in range(0, 200)]
    for name, s, e in proof_sections(proof):                       # every length prefix that opens a section, patched to 2^63 and to 2^32
        if name in ("paths:trace", "trace_rows", "constraint_values", "paths:constraint", "deep_values", "fri_count", "fri0:paths"):
            for v in (1 << 63, 1 << 32, (1 << 64) - 1):
                items.append(proof[:s] + struct.pack("<Q", v) + proof[s + 8:])
    s = [x for x in proof_sections(proof) if x[0] == "fri0:values"][0][1] + 32
    items.append(proof[:s] + struct.pack("<Q", 1 << 63) + proof[s + 8:])
    s = [x for x in proof_sections(proof) if x[0] == "remainder"][0][1] + 32
    items.append(proof[:s] + struct.pack("<Q", 1 << 63) + proof[s + 8:])
    for off, val in ((32, 0), (32, 41), (32, 255), (33, 17), (34, 9), (35, 33), (len(proof) - 4, 3), (len(proof) - 4, 9), (len(proof) - 4, 69), (len(proof) - 3, 0),
                     (len(proof) - 3, 129), (len(proof) - 2, 33), (len(proof) - 1, 1)):
        b = bytearray(proof); b[off] = val
        items.append(bytes(b))
    return items


def _host_binary(tmp_path, sanitize):
    exe = str(tmp_path / ("verify_corpus_san" if sanitize else "verify_corpus"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-w"] + flags + ["-I", CSRC, "-o", exe, HOST_SRC])
    return exe


def test_malformed_input_never_crashes(oracle, tmp_path):
    """The empty buffer, every prefix length below 200 and every 997th above, length prefixes patched to 2^32, 2^63 and 2^64 - 1, header and
    option bytes outside their ranges: DST_ERR_ARG or a clean reject from the library, and the same corpus (plus a sample of the mutants of the
    parity test) through a host-only build of the verifier with -fsanitize=address,undefined: exit status 0, nothing on stderr."""
    import distaff_amd as D
    proof, ph, ins, outs = _fib_proof(7)
    items = _malformed_corpus(proof)
    kinds = {"malformed": 0, "reject": 0}
    for it in items:
        try:
            ok, err = _verify(it, ph, list(ins), list(outs))
            assert not ok and err
            kinds["reject"] += 1
            assert _info(it)["extension_factor"] >= 16                            # what parses for one call parses for the other
        except D.DistaffError as e:
            assert e.code == D.DST_ERR_ARG
            kinds["malformed"] += 1
            with pytest.raises(D.DistaffError):
                _info(it)
    assert kinds["malformed"] > 200
    assert _verify(proof, ph, list(ins), list(outs)) == (True, "")                     # the process is alive and well
    items += [m[3] for m in _mutants(proof, 5)[::4]] + [proof]
    path = str(tmp_path / "corpus.bin")
    open(path, "wb").write(_corpus(ph, ins, outs, items))
    r = subprocess.run([_host_binary(tmp_path, True), path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(items) and lines[-1] == "A" and lines[0].startswith("M ")
    for it, line in zip(items, lines):                              # the sanitized build and the library give the same verdicts
        try:
            ok, err = _verify(it, ph, list(ins), list(outs))
            assert line == ("A" if ok else "R " + err)
        except D.DistaffError:
            assert line.startswith("M ")


# ---- 6: no device ---------------------------------------------------------------------------------------------------------------------------
NO_DEVICE_WORKER = r"""
import sys
sys.path.insert(0, %r)
import distaff_amd as D
D.use_product()
proof = open(sys.argv[1], "rb").read()
ph = bytes.fromhex(sys.argv[2])
ok, err = D.verify(proof, ph, [1, 0], [int(sys.argv[3])])
info = D.proof_info(proof)
assert ok and err == "", err
assert info["log_trace_length"] == 8 and info["extension_factor"] == 32
bad = bytearray(proof); bad[3] ^= 1
assert D.verify(bytes(bad), ph, [1, 0], [int(sys.argv[3])]) == (False, "verification of trace Merkle proof failed")
print("ok")
"""


def test_verify_needs_no_device(oracle, tmp_path):
    """dst_verify and dst_proof_info of the PRODUCT library in a process that sees no GPU (HIP_VISIBLE_DEVICES and ROCR_VISIBLE_DEVICES empty)"""
    proof, ph, ins, outs = _fib_proof(8)
    (tmp_path / "p.bin").write_bytes(proof)
    script = tmp_path / "w.py"
    script.write_text(NO_DEVICE_WORKER % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    env.pop("DISTAFF_TEST_HOOKS", None)
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "p.bin"), ph.hex(), str(outs[0])], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_verifier_links_without_the_hip_runtime(oracle, tmp_path):
    """the host-only verifier binary, plain g++, nothing but the C++ runtime on the link line: that it links shows verify/host_verify.h pulls in no
    hip* call; it accepts a proof and is not bound to libamdhip64"""
    exe = _host_binary(tmp_path, False)
    needed = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True).stdout
    assert "amdhip" not in needed and "hsa" not in needed
    proof, ph, ins, outs = _fib_proof(8)
    path = str(tmp_path / "one.bin")
    open(path, "wb").write(_corpus(ph, ins, outs, [proof, proof[:100]]))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, text=True, check=True)
    assert r.stdout.splitlines()[0] == "A" and r.stdout.splitlines()[1].startswith("M ")


# ---- 7: dst_proof_info -----------------------------------------------------------------------------------------------------------------------
def test_proof_info_reports_the_parameters(oracle):
    import distaff_amd as D
    for shape, level in (((8, 32, 50, 20), (2 * 50 + 20, 2 * 25)), ((8, 16, 100, 0), (100, 50)), ((8, 64, 50, 20), (3 * 50 + 20, 75))):
        proof = _fib_proof(*shape)[0]
        info = _info(proof)
        log_n, ext, queries, grinding = shape
        assert (info["log_trace_length"], info["extension_factor"], info["num_queries"], info["grinding_factor"]) == shape
        assert (info["register_count"], info["ctx_depth"], info["loop_depth"], info["stack_depth"]) == (20, 1, 0, 4)
        assert info["fri_layers"] == len([s for s in proof_sections(proof) if s[0].endswith(":values")]) and info["remainder_length"] in (64, 128, 256)
        assert (info["security_level"], info["security_level_proven"]) == level                 # options.rs:68-79
        assert info["op_count"] >= 16 and info["pow_nonce"] == struct.unpack_from("<Q", proof, len(proof) - 12)[0]
    proof, _, _, _, (length, width, ctx, lp) = _isa_proof("nested_loops")
    info = _info(proof)
    assert (1 << info["log_trace_length"], info["register_count"], info["ctx_depth"], info["loop_depth"]) == (length, width, ctx, lp)
    with pytest.raises(D.DistaffError):
        _info(proof[:-1])


# ---- 8: the C example and the command-line tool ----------------------------------------------------------------------------------------------
def test_example_verify_proof_c(oracle, tmp_path):
    """examples/verify_proof.c: C99, the header and the product library only; accepts an oracle proof (exit 0), rejects a tampered one and a wrong
    output with the reference's words (exit 1)"""
    import distaff_amd as D
    exe = str(tmp_path / "verify_proof")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "examples", "verify_proof.c"),
                           "-L", os.path.dirname(D.PRODUCT_LIB), "-ldistaff_hip", "-Wl,-rpath," + os.path.dirname(D.PRODUCT_LIB)])
    proof, ph, ins, outs = _fib_proof(8)
    good, bad = tmp_path / "good.bin", tmp_path / "bad.bin"
    good.write_bytes(proof)
    t = bytearray(proof); t[len(proof) // 2] ^= 1
    bad.write_bytes(bytes(t))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    args = [ph.hex(), "--inputs", "1", "0", "--outputs", str(outs[0])]
    r = subprocess.run([exe, str(good)] + args, stdout=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip().startswith("accepted")
    r = subprocess.run([exe, str(bad)] + args, stdout=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 1 and oracle.verify(bytes(t), ph, list(ins), list(outs))[1] in r.stdout
    r = subprocess.run([exe, str(good), ph.hex(), "--inputs", "1", "0", "--outputs", str(outs[0] + 1)], stdout=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 1 and LOW_DEGREE in r.stdout


def test_tool_verify_proof_py(oracle, tmp_path):
    proof, ph, ins, outs = _fib_proof(8)
    (tmp_path / "p.bin").write_bytes(proof)
    tool = os.path.join(ROOT, "tools", "verify_proof.py")
    env = dict(os.environ); env.pop("DISTAFF_TEST_HOOKS", None)
    r = subprocess.run([sys.executable, tool, str(tmp_path / "p.bin"), "--program-hash", ph.hex(), "--inputs", "1", "0", "--outputs", str(outs[0])],
                       stdout=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 0 and "accepted" in r.stdout
    r = subprocess.run([sys.executable, tool, str(tmp_path / "p.bin"), "--program-hash", ph.hex(), "--inputs", "1", "1", "--outputs", str(outs[0])],
                       stdout=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 1 and LOW_DEGREE in r.stdout
