"""Verify a serialised StarkProof on the host through the library's binding (dst_verify): no GPU needed.

    python tools/verify_proof.py proof.bin --program-hash <64 hex digits> --inputs 1 0 --outputs <value> ...

Pairs with `bench.py --dump-outputs`, which writes the proof it timed.  Prints "accepted" and what the proof says about itself (exit 0), or
the reference's error string / why the bytes are not a StarkProof (exit 1)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("proof")
    ap.add_argument("--program-hash", required=True, help="32 bytes as hex")
    ap.add_argument("--inputs", nargs="*", default=[], type=int)
    ap.add_argument("--outputs", nargs="*", default=[], type=int)
    a = ap.parse_args()
    import distaff_amd as D
    proof = open(a.proof, "rb").read()
    try:
        ok, err = D.verify(proof, bytes.fromhex(a.program_hash), a.inputs, a.outputs)
    except D.DistaffError as e:
        print("not a StarkProof: %s" % e)
        return 1
    if not ok:
        print("rejected: %s" % err)
        return 1
    print("accepted: %s" % D.proof_info(proof))
    return 0


if __name__ == "__main__":
    sys.exit(main())
