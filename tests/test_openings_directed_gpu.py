"""Step 9 of the prover at DIRECTED query positions, single context and sharded, against the oracle.

Every other test opens the ~50 positions the proof's own seed draws; uniform draws almost never hold siblings, two positions of one
constraint leaf, positions of one FRI row, a covered subtree or a lone position (tests/openings_sets.py builds such sets by formula).
Here one proof per shape is made once; opening is read-only, so many position sets are then opened on the same context and on the same
oracle prover (`Prover.step(8, positions=...)`, `verify(..., positions=...)`): the library's bytes must be the oracle's, and the oracle's
verifier must accept them at those positions.

Shapes: A = Fibonacci, 2^7 rows, blowup 32 (N = 4096: FRI layers 4096, 1024, remainder 256); B = Fibonacci, 2^10 rows, blowup 16
(N = 16384: 16384, 4096, 1024, remainder 256); C = the shortest trace the VM produces, 32 rows, blowup 16 (N = 512: one layer of 512 and
a remainder of 128 -- a proof without any layer would need a 16-row trace, which no program fills).

tests/test_openings_directed_emulated.py runs a part of this file on the CPU build of the library's sources."""
import ctypes

import numpy as np
import pytest

from openings_sets import FAMILIES, off_trace, opened_bytes, position_sets

pytestmark = pytest.mark.gpu

GRINDING = 8
SHAPES = {"A": (7, 5), "B": (10, 4), "C": (5, 4)}                     # log2(rows), log2(blowup)
STAGE_BYTES = 8 << 20                                                 # the context's staging buffer for gathers (api.hip)


class Proved:
    """One shape: the oracle prover through step 9 at the drawn positions, and a context that has proved the same trace."""

    def __init__(self, O, D, shape):
        log_n, log_b = SHAPES[shape]
        self.O, self.D, self.shape, self.log_n, self.log_b = O, D, shape, log_n, log_b
        self.trace = t = O.fibonacci_trace(1 << log_n) if log_n >= 7 else O.Trace("begin add end", [1, 2])
        assert t.length == 1 << log_n
        self.B, self.n, self.N, self.W = 1 << log_b, t.length, t.length << log_b, t.width
        self.op = O.Prover.from_trace(t, 1, ext=self.B, grinding=GRINDING)
        for k in range(1, 10):
            self.op.step(k)
        self.outputs = self.op.outputs
        self.drawn, self.drawn_proof, self.nonce = self.op.get_u64("positions"), self.op.get_bytes("proof"), self.op.get_u64("pow_nonce")[0]
        self.layer_sizes = [self.N >> (2 * d) for d in range(self.op.get_u64("fri_layers")[0])]
        self.ctx = D.Context(log_n, t.width, t.ctx_depth, t.loop_depth, log_blowup=log_b, grinding=GRINDING)
        self.ctx.upload(t.columns)
        assert self.ctx.prove(t.public_inputs, self.outputs) == self.drawn_proof
        self.sets = {label: (family, pos) for family, label, pos in position_sets(self.N, self.B)}
        self._oracle, self._single = {}, {}

    def oracle_proof(self, label):
        """the oracle's proof at a set: computed once, shared by the tests that need it"""
        if label not in self._oracle:
            self.op.step(8, positions=self.sets[label][1]); self.op.step(9)
            assert self.op.get_u64("positions") == self.sets[label][1] and self.op.get_u64("pow_nonce")[0] == self.nonce
            self._oracle[label] = self.op.get_bytes("proof")
        return self._oracle[label]

    def single_proof(self, label):
        if label not in self._single:
            self._single[label] = self.ctx.build_proof(self.sets[label][1], self.nonce)
        return self._single[label]

    def verify(self, proof, positions):
        return self.O.verify(proof, self.trace.program_hash, self.trace.public_inputs, self.outputs, positions=positions)

    def still_usable(self):
        """after a refusal: the drawn openings come out as before"""
        assert self.ctx.build_proof(self.drawn, self.nonce) == self.drawn_proof

    def need_bytes(self, positions):
        """what the batched gather of a whole proof stages: 8 bytes of address and 16 bytes of data per 16-byte piece"""
        from distaff_amd import sharded
        pieces = opened_bytes(positions, self.N, self.W, self.layer_sizes, sharded.plan_batch, sharded.augmented_positions, sharded.constraint_positions) // 16
        return 24 * pieces

    def labels(self, family):
        return [label for label, (f, pos) in self.sets.items() if f == family and self.need_bytes(pos) <= STAGE_BYTES]


@pytest.fixture(scope="module")
def proved(oracle):
    import distaff_amd as D
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Proved(oracle, D, shape)
        return made[shape]
    yield get
    for p in made.values():
        p.ctx.close()


def test_position_sets_hold_what_they_are_meant_to():
    """siblings, shared constraint leaves, FRI rows shared in layer 0 / 1 / 2 only, covered subtrees, unsorted input: by construction"""
    for shape, (log_n, log_b) in SHAPES.items():
        N, B = 1 << (log_n + log_b), 1 << log_b
        sets = {label: (family, pos) for family, label, pos in position_sets(N, B)}
        assert {f for f, _ in sets.values()} == set(FAMILIES)
        for family in FAMILIES:
            assert any(off_trace(pos, B) for f, pos in sets.values() if f == family), (shape, family)
        assert sorted(sets["all"][1]) == list(range(N)) and len(sets["off-trace"][1]) == N - N // B
        for label in ("pair-middle", "riap-last"):
            a, b = sets[label][1]
            assert a ^ b == 1
        a, b = sets["neighbours-middle"][1]
        assert b == a + 1 and a ^ b != 1
        R = N // 4
        assert len({p % R for p in sets["row-high-shuffled"][1]}) == 1 and sets["row-high-shuffled"][1] != sorted(sets["row-high-shuffled"][1])
        a, b = sets["layer1"][1]
        assert a % R != b % R and a % (R // 4) == b % (R // 4)
        a, b = sets["layer2"][1]
        assert a % (R // 4) != b % (R // 4) and a % (R // 16) == b % (R // 16)
        assert sets["mixed-descending"][1] == sorted(sets["mixed-descending"][1], reverse=True)
        assert len({p % B for p in sets["whole-coset1"][1]}) == 1 and len(sets["whole-coset1"][1]) == N // B
        assert sets["draw128"][1] != sorted(sets["draw128"][1])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_single_context_openings(proved, shape, family):
    """dst_build_proof at every set of the family: the oracle's bytes, and a proof the oracle's verifier accepts at those positions (on the
    trace domain as well: the prover's transition divisor vanishes there, nothing the verifier divides by does)"""
    p = proved(shape)
    labels = p.labels(family)
    assert labels and ("all" in labels) == (family == "everything" and shape != "B")      # all N of shape B: test_openings_beyond_the_staging_buffer
    verified = 0
    for label in labels:
        positions = p.sets[label][1]
        proof = p.single_proof(label)
        assert proof == p.oracle_proof(label), (shape, label)
        assert p.verify(proof, positions) == (True, ""), (shape, label)
        verified += off_trace(positions, p.B)
    assert verified >= 1, (shape, family)                              # every family has a member clear of the trace domain
    p.still_usable()


def test_verifier_at_given_positions_is_not_vacuous(proved):
    """a proof opened at S is rejected at another S' -- by position, by order, by count -- and a damaged opening is rejected at S"""
    p = proved("A")
    S = p.sets["draw7"][1]
    proof = p.single_proof("draw7")
    assert p.verify(proof, S) == (True, "")
    assert p.verify(proof, [S[1], S[0]] + S[2:]) == (False, "verification of trace Merkle proof failed")
    assert p.verify(proof, S[:-1] + [S[-1] ^ 1]) == (False, "verification of trace Merkle proof failed")
    assert p.verify(proof, S[:-1])[0] is False
    assert p.verify(proof, p.sets["mixed-descending"][1])[0] is False
    ok, why = p.verify(proof, None)                                    # the drawn positions are not S
    assert not ok and why
    assert p.verify(p.drawn_proof, None) == (True, "") and p.verify(p.drawn_proof, p.drawn) == (True, "")
    assert p.verify(p.drawn_proof, S)[0] is False
    row = np.ascontiguousarray(p.op.get("registers")[:, S[2], :]).tobytes()      # one bit of an opened row, one bit of the remainder
    at = proof.find(row)
    assert at > 0
    for offset, why in ((at + 16 * 3, "verification of trace Merkle proof failed"), (len(proof) - 12 - 16 * 100, "verification of low-degree proof failed")):
        damaged = bytearray(proof)
        damaged[offset] ^= 1
        ok, text = p.verify(bytes(damaged), S)
        assert not ok and text.startswith(why), text


def _open_on_every_rank(ctxs, positions):
    blobs, lens = [], None
    for ctx in ctxs:
        blob, ls = ctx.shard_open(positions)                           # two calls: the size query with every rank's length, then the blob
        assert lens is None or ls == lens
        lens = ls
        assert len(blob) == lens[ctx.params.rank]
        blobs.append(blob)
    return blobs, lens


@pytest.mark.parametrize("world,shape,replicate_log,gather", [(2, "A", None, False), (8, "A", 9, False), (4, "B", 9, True), (8, "B", 9, False)])
def test_sharded_openings(proved, monkeypatch, world, shape, replicate_log, gather):
    """dst_shard_open on every rank and dst_shard_assemble on every rank after ONE dst_prove_sharded_local: the single-context bytes for every
    set.  Owners of three kinds serve the items: the rank of a coset (rank-local heaps, rows, elements), the k-range owner of a subtree,
    rank 0 for what is replicated (top heaps, the FRI tail)."""
    p = proved(shape)
    D, t = p.D, p.trace
    if replicate_log is None:
        monkeypatch.delenv("DISTAFF_FRI_REPLICATE_LOG", raising=False)
    else:
        monkeypatch.setenv("DISTAFF_FRI_REPLICATE_LOG", str(replicate_log))
    if gather:
        monkeypatch.setenv("DISTAFF_SHARD_TREE_GATHER", "1")
    else:
        monkeypatch.delenv("DISTAFF_SHARD_TREE_GATHER", raising=False)
    ctxs = []
    for r in range(world):
        ctx = D.Context(p.log_n, t.width, t.ctx_depth, t.loop_depth, rank=r, world=world, log_blowup=p.log_b, grinding=GRINDING)
        ctx.upload(t.columns)
        ctxs.append(ctx)
    try:
        from distaff_amd import sharded
        assert D.prove_sharded_local(ctxs, t.public_inputs, p.outputs) == p.drawn_proof
        ran = set()
        for family in FAMILIES:
            for label in p.labels(family):
                if label == "all":
                    continue                                           # left to the single context
                positions = p.sets[label][1]
                blobs, lens = _open_on_every_rank(ctxs, positions)
                assert sum(lens) == opened_bytes(positions, p.N, p.W, p.layer_sizes, sharded.plan_batch, sharded.augmented_positions, sharded.constraint_positions), label
                packed = np.concatenate(blobs) if sum(lens) else np.zeros(1, dtype=np.uint8)
                want = p.single_proof(label)
                assert want == p.oracle_proof(label), label
                for ctx in ctxs:
                    assert ctx.shard_assemble(positions, p.nonce, packed, lens) == want, (label, ctx.params.rank)
                if label.startswith("whole-coset"):                    # every row from one owner: the rows of the extension sit in that rank's blob alone
                    owner = (positions[0] % p.B) // (p.B // world)
                    regs = p.op.get("registers")
                    for q in positions[:: max(1, len(positions) // 64)]:
                        row = np.ascontiguousarray(regs[:, q, :]).tobytes()
                        assert [row in blob.tobytes() for blob in blobs] == [g == owner for g in range(world)], (label, q)
                    others = [lens[g] for g in range(world) if g != owner]
                    assert lens[owner] >= len(positions) * p.W * 16 and sum(others) == sum(lens) - lens[owner]
                ran.add(family)
        assert ran == set(FAMILIES)
        # the drawn openings still come out
        blobs, lens = _open_on_every_rank(ctxs, p.drawn)
        assert ctxs[-1].shard_assemble(p.drawn, p.nonce, np.concatenate(blobs), lens) == p.drawn_proof
    finally:
        for ctx in ctxs:
            ctx.close()


def test_python_planned_openings(proved, monkeypatch):
    """The Python statement of the opening plan (ShardedProver(python_openings=True), two thread-ranks) at directed positions: the proof's
    draw is replaced by a set, everything else in distaff_amd/sharded.py runs as it is"""
    from distaff_amd import sharded
    p = proved("A")
    t = p.trace
    monkeypatch.delenv("DISTAFF_FRI_REPLICATE_LOG", raising=False)
    for label in ("half+1", "riap-middle", "leaf-middle-between", "mixed-descending", "whole-coset17", "draw7"):
        positions = p.sets[label][1]
        monkeypatch.setattr(sharded.L, "query_positions", lambda seed, N, B, count, positions=positions: list(positions))
        proofs = sharded.prove_local(t.columns, p.log_n, t.width, t.ctx_depth, t.loop_depth, t.public_inputs, p.outputs, 2, python_openings=True,
                                     log_blowup=p.log_b, grinding=GRINDING)
        assert all(proof == p.oracle_proof(label) for proof in proofs), label


def _raw_build_proof(p, positions, fill=0xA5, cap=1 << 16):
    """dst_build_proof with a caller's buffer: -> (code, the buffer afterwards)"""
    pos = np.asarray(positions, dtype=np.uint64)
    out = np.full(cap, fill, dtype=np.uint8)
    ln = ctypes.c_size_t(0)
    code = p.ctx.lib.dst_build_proof(p.ctx._h, pos.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(pos)), ctypes.c_uint64(p.nonce),
                                     out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap), ctypes.byref(ln))
    return code, out


@pytest.mark.parametrize("shape", ["A", "C"])
def test_refused_positions_leave_the_context_usable(proved, shape):
    p = proved(shape)
    D = p.D
    long_set = list(p.sets["draw128"][1])
    repeat = long_set[:100] + [long_set[3]] + long_set[100:]
    for bad, text in (([p.N], "out of range"), ([1 << 63], "out of range"), ([5, p.N, 9], "out of range"), (long_set[:50] + [(1 << 64) - 1], "out of range"),
                      (repeat, "repeating indexes")):
        with pytest.raises(D.DistaffError) as e:
            p.ctx.build_proof(bad, p.nonce)
        assert e.value.code == D.DST_ERR_ARG and text in str(e.value), bad[:4]
        code, out = _raw_build_proof(p, bad)
        assert code == D.DST_ERR_ARG and (out == 0xA5).all()
        p.still_usable()


def test_no_position_at_all(proved):
    """the oracle builds a proof of empty batch openings from an empty list of positions: so does the library, byte for byte"""
    p = proved("A")
    p.op.step(8, positions=[]); p.op.step(9)
    want = p.op.get_bytes("proof")
    assert p.op.get_u64("positions") == []
    code, out = _raw_build_proof(p, np.zeros(1, dtype=np.uint64)[:0], cap=len(want) + 64)
    assert code == 0 and out[:len(want)].tobytes() == want and (out[len(want):] == 0xA5).all()
    p.still_usable()


def test_openings_beyond_the_staging_buffer(proved):
    """All N positions of shape B need more than the 8 MiB the context stages gathers in (8 bytes of address + 16 bytes of data per piece):
    dst_build_proof refuses and writes nothing, and so does dst_shard_open on a rank whose share is that large (the one rank of a
    one-rank world)"""
    p = proved("B")
    D = p.D
    positions = p.sets["all"][1]
    assert len(positions) == p.N and p.need_bytes(positions) > STAGE_BYTES
    assert p.need_bytes(p.sets["krows4"][1]) < STAGE_BYTES
    with pytest.raises(D.DistaffError) as e:
        p.ctx.build_proof(positions, p.nonce)
    assert e.value.code == D.DST_ERR_ARG and "staging buffer too small" in str(e.value)
    code, out = _raw_build_proof(p, positions, cap=16 << 20)
    assert code == D.DST_ERR_ARG and (out == 0xA5).all()
    p.still_usable()
    # dst_shard_open: the size query answers (nothing is gathered), the blob is refused
    pos = np.asarray(positions, dtype=np.uint64)
    lens, ln = np.zeros(1, dtype=np.uint64), ctypes.c_size_t(0)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    assert p.ctx.lib.dst_shard_open(p.ctx._h, ptr(pos), ctypes.c_uint32(len(pos)), None, ctypes.c_size_t(0), ctypes.byref(ln), ptr(lens)) == 0
    assert ln.value == int(lens[0]) == p.need_bytes(positions) // 24 * 16
    blob = np.full(ln.value, 0xA5, dtype=np.uint8)
    assert p.ctx.lib.dst_shard_open(p.ctx._h, ptr(pos), ctypes.c_uint32(len(pos)), ptr(blob), ctypes.c_size_t(ln.value), ctypes.byref(ln), None) == D.DST_ERR_ARG
    assert (blob == 0xA5).all()
    p.still_usable()
