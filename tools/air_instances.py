#!/usr/bin/env python3
"""Time of the constraint evaluation of a 2^20-step Fibonacci proof under every instance set of the constraint kernel: by shape (the
depth-4 set) and forced through the small, deep and per-operation sets (DISTAFF_AIR, read when a context is created).  The per-operation
set exists in the test build only, so the test build is measured unless DISTAFF_HIP_LIB names another library:

    DISTAFF_TEST_HOOKS=1 python tools/air_instances.py [log_n]

One context per set, six proofs, the constraint phase (ms) of the last five; one JSON line.  profiles/air_layer.md compares two trees with it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import distaff_amd as D

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
cols, _, result = D.fibonacci_trace(log_n)
out = {}
for inst in ("", "small", "deep", "generic"):
    if inst:
        os.environ["DISTAFF_AIR"] = inst
    else:
        os.environ.pop("DISTAFF_AIR", None)
    ctx = D.Context(log_n, 20, 1, 0)
    ctx.upload(cols)
    ms = []
    for _ in range(6):
        ctx.prove([1, 0], [result])
        ms.append(round(ctx.phase_ms()[2], 4))
    out[inst or "sd4"] = ms[1:]
    ctx.close()
print(json.dumps(out))
