"""The op flags and the op-bit constraints of the constraint kernel on arbitrary field elements.

`air_op_flags` forms one product per flag table and the other entries by subtraction (x * (1 - b) = x - x * b), and `air_op_bits` takes
the bit products of constraints 10 - 12 from the flags; both identities hold for every field element, and the kernel runs on seven
cosets where the op bits are not 0 / 1.  tests/emu/air_flags_test.cpp compares every flag and all fifteen op-bit constraints with the
products written out as the reference states them, computed with integer arithmetic that shares no carry path with the kernel's: every
combination of {0, 1, 2, p - 1, p - 2, 2^64, 2^127} in the registers that a product pairs, and 20 000 uniform rows.  Host build of the
kernel header against the stand-in HIP header of tests/emu (built like air_merge_test.cpp)."""
import os
import subprocess


def test_flags_and_op_bit_constraints_equal_their_written_out_products(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    emu = os.path.join(root, "tests", "emu")
    exe = tmp_path / "air_flags_test"
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-pthread", "-I", emu, "-w", "-DFE_EMULATE_GFX950=1", os.path.join(emu, "air_flags_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and b" 0 mismatches" in out.stdout, out.stdout.decode()[-2000:]
    rows = int(out.stdout.split()[0])
    assert rows >= 7**7 + 7**5 + 10**4, out.stdout.decode()[-200:]
