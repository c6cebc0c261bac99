"""The one-sided lazy butterflies of the first pass's coset DIT (fe.h: fe_add_lazy / fe_addsub_lazy; ntt_lds.h: the LAZY switch of
lds_dit_round / lds_dit_tail), on the host-emulated dataflow -- no GPU.

In a DIT butterfly every sum and difference is u +- r with r fresh out of fe_mul_tw, i.e. canonical; u may then be ANY 128-bit value:
u + r < 2^128 + p, one wrap (drop 2^128, add C = 2^128 - p) brings the sum below 2^128 again, and fe_sub is right as it is.  The results
are congruent, not canonical; they may feed fe_mul_tw / fe_mul_wide, which take any 128-bit operand.

The reference is Python integers.  A result is four 32-bit limbs, so "below 2^128" is what the congruence asserts: a lost carry out of the
wrap would leave the limbs 2^128 short of the sum, i.e. off by C modulo p."""
import os
import random
import subprocess

P = 2**128 - 45 * 2**40 + 1
C = 2**128 - P
M128 = 2**128
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")

ALL_ONES_LIMBS = [(2**32 - 1) << (32 * i) for i in range(4)] + [M128 - 1 - ((2**32 - 1) << (32 * i)) for i in range(4)] + [(2**64 - 1) << 64, 2**64 - 1, (2**96 - 1) << 32]
U_DIRECTED = [0, 1, P - 1, P, P + 1, M128 - 1, M128 - C] + ALL_ONES_LIMBS
R_DIRECTED = [0, 1, C, P - 1, P - 2]
W_DIRECTED = [1, P - 1, 2**64, C]


def _operands():
    rnd = random.Random(20260131)
    triples = [(u, r, w) for u in U_DIRECTED for r in R_DIRECTED for w in W_DIRECTED]
    for _ in range(4000):
        kind = rnd.randrange(4)
        u = rnd.randrange(M128) if kind else P + rnd.randrange(C)                        # every fourth u in [p, 2^128)
        r = rnd.randrange(P) if kind != 1 else (P - u % P + rnd.randrange(-3, C)) % P      # every fourth sum within C of a multiple of p
        triples.append((u, r, rnd.randrange(P)))
    return triples


def test_lazy_additions_against_python_integers(tmp_path):
    exe = tmp_path / "fe_lazy_test"
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-w", "-DFE_EMULATE_GFX950=1", os.path.join(EMU, "fe_lazy_test.cpp"), "-o", str(exe)])
    triples = _operands()
    assert all(r < P and w < P and u < M128 for u, r, w in triples)
    text = "".join("%x %x %x\n" % t for t in triples)
    out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, timeout=300, check=True).stdout.decode().split("\n")
    rows = [[int(x, 16) for x in line.split()] for line in out if line]
    assert len(rows) == len(triples)
    wraps = noncanonical = 0
    for (u, r, w), (add, s, d, s_tw, s_wide, d_tw, d_wide) in zip(triples, rows):
        what = (hex(u), hex(r), hex(w))
        assert add == s, what                                          # fe_add_lazy and the sum of fe_addsub_lazy are one function
        assert s < M128 and s % P == (u + r) % P, ("sum",) + what
        assert s == (u + r if u + r < M128 else u + r - M128 + C), ("sum: one wrap",) + what
        assert d < M128 and d % P == (u - r) % P, ("difference",) + what
        assert s_tw == s_wide == (u + r) % P * w % P, ("product of the sum",) + what
        assert d_tw == d_wide == (u - r) % P * w % P, ("product of the difference",) + what
        wraps += u + r >= M128
        noncanonical += s >= P
    assert wraps > 1000 and noncanonical > 500, (wraps, noncanonical)         # the operands reach both sides of the wrap and leave non-canonical sums


def test_first_pass_tile_with_lazy_rounds_equals_the_canonical_rounds(tmp_path):
    """tests/emu/ntt_lazy_test.cpp: 64 x 4 and 32 x 4 tiles through the coset DIT with the switch on and off, every coset of blowup 8, four
    inputs; equal byte for byte after the read-out multiplication, and equal to the transform summed term by term."""
    exe = tmp_path / "ntt_lazy_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-I", EMU, "-w", "-DFE_EMULATE_GFX950=1", "-x", "c++", os.path.join(EMU, "ntt_lazy_test.cpp"),
                           os.path.join(EMU, "emu_runtime.cpp"), "-o", str(exe), "-ldl"])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0 and " mismatches 0 " in text, text[-2000:]
    words = text.split()
    assert int(words[1]) == 2 * 4 * 8 and int(words[3]) == 4 * 8 * 4 * (64 + 32), text
    assert int(words[-1]) > 0, "no element of a lazy tile was a non-canonical value: the inputs do not tell the two forms apart"
