"""TEST INFRASTRUCTURE: runs the oracle's verifier over a corpus of (possibly damaged) proofs in a process of its own.

The oracle restates the reference, and the reference trusts a proof's own header (options.rs:14 "TODO: validate field values on
de-serialization"): a damaged depth or extension byte can send it into an assertion, an undefined shift, or an allocation of many
gigabytes.  So the mutation-parity test of tests/test_verify_host.py calls it here, under an address-space limit and an alarm per
item; the parent treats the death of this process as "the oracle fails on that item" and restarts it behind that item.

usage: oracle_worker.py corpus.bin first_index     (corpus format: tests/verify_host/verify_corpus.cpp)
prints one line per item, flushed: "<index>\t<1|0>\t<error string>"
"""
import os
import resource
import signal
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def read_corpus(path):
    b = open(path, "rb").read()
    ph = b[:32]
    nin, nout = struct.unpack_from("<II", b, 32)
    o = 40
    vals = [int.from_bytes(b[o + 16 * i:o + 16 * i + 16], "little") for i in range(nin + nout)]
    o += 16 * (nin + nout)
    count, = struct.unpack_from("<I", b, o)
    o += 4
    items = []
    for _ in range(count):
        n, = struct.unpack_from("<Q", b, o)
        items.append(b[o + 8:o + 8 + n])
        o += 8 + n
    return ph, vals[:nin], vals[nin:], items


def main():
    path, first = sys.argv[1], int(sys.argv[2])
    import oracle as O
    O.lib()
    resource.setrlimit(resource.RLIMIT_AS, (6 << 30, 6 << 30))
    ph, ins, outs, items = read_corpus(path)
    for i in range(first, len(items)):
        signal.alarm(20)                                  # default action: the process dies, the parent books the item as a failure
        ok, err = O.verify(items[i], ph, ins, outs)
        signal.alarm(0)
        sys.stdout.write("%d\t%d\t%s\n" % (i, 1 if ok else 0, err.replace("\n", " ")))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
