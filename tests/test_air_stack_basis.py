"""The flat statement of the low-degree stack operations against the nested one, on the host.

The constraint kernels evaluate the stack slots >= 1 as ONE sum of products over the distinct basis terms of the launch's operations,
with coefficients that are adds / subtracts of class sums formed once per point (air_stack_nested.h: st_basis_table, st_class_sums,
st_output_basis).  tests/emu/air_basis_test.cpp compares that statement with `st_output` -- exactly, both are canonical field elements --
for every output (slots 0 - 7 and the two auxiliary constraints), every GROUPS value of the three product launch lists and all low-degree
operations together, compile-time depths 0 and 4, plain and deep slices of 8, 9 and 12 items, with the outputs the kernels take in flat
form and with ALL outputs in flat form; on 20 000 uniform rows whose table entries are drawn independently of each other, and on every
combination of {0, 1, 2, p - 1, p - 2, 2^64, 2^127} in the table entries that a class sum multiplies.  Host build of the kernel header
against the stand-in HIP header of tests/emu (built like air_merge_test.cpp); the program has its own main."""
import os
import subprocess


def test_flat_statement_equals_the_nested_one(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    emu = os.path.join(root, "tests", "emu")
    exe = tmp_path / "air_basis_test"
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-pthread", "-I", emu, "-w", "-DFE_EMULATE_GFX950=1", os.path.join(emu, "air_basis_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and b" 0 mismatches" in out.stdout, out.stdout.decode()[-2000:]
    # ten GROUPS values (the four with operations 0x00 .. 0x0F touch all ten outputs, the others the eight slots), 8 shapes each, 20 000
    # uniform rows for the kernels' selection of flat outputs alone
    assert int(out.stdout.split()[0]) >= (4 * 10 + 6 * 8) * 8 * 20000, out.stdout.decode()[-200:]
