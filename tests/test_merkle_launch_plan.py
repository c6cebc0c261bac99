"""Which kernel builds which level of a BLAKE3 Merkle tree (distaff_amd/csrc/host/merkle_plan.h, walked by k_merkle in kernels_hash.hip), pinned
to what the launch code did before the plan existed.

tests/golden/merkle_launches.json holds two records of the code as it was BEFORE: five loops in kernels_hash.hip that each chose between
merkle_level_kernel, merkle_level2_kernel, merkle_subtree_kernel and merkle_top_kernel.

  * "launches": per tree shape, the lines an instrumented copy of those loops printed instead of launching -- profiling name, profiling bytes,
    grid.x, block.x, the kernel's count argument, the offset it reads at in the node array ("leaves": the leaf array) and the lowest offset it
    writes.  tests/merkle_plan/merkle_plan_check.cpp prints the same lines from merkle_plan.h; a line that differs is a launch that changed.
  * "kernel_stats": launches and profiling bytes of every kernel of kernels_hash.hip in a 2^7-step Fibonacci proof, as dst_kernel_stats
    reported them from the emulated build of that code: what the callers (api.hip, shard.hip, host/steps_impl.h) ask the plan for.

The cases are not stored by the file; the tests build them and the file only answers, so a case cannot be dropped by editing the data."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "merkle_launches.json")
SWITCH_SETS = ({}, {"DISTAFF_MERKLE_LEVEL2_LOG": "3"}, {"DISTAFF_MERKLE_LEVELS": "1"})       # what the suite sets
HASH_KERNELS = ("trace_leaves_kernel", "merkle_level_kernel", "merkle_level2_kernel", "merkle_subtree_kernel", "merkle_top_kernel", "constraint_level1_kernel",
                "fri_leaves0_kernel", "fri_leaves_kernel", "fri_leaves_cm_kernel", "interleave_boundary_kernel", "digests_from_records_kernel")


def plan_cases():
    """[(a, in_place, stop_log, level2_log, levels_only)]: trees over 2^a children, a = 1 .. 34, from a leaf array and from a filled level of the
    node array; to the root (stop_log -1) and to every level of 2^s nodes with 2 * 2^s <= 2^a; under each switch set"""
    out = []
    for level2_log, levels_only in ((-1, 0), (3, 0), (-1, 1)):
        for a in range(1, 35):
            for in_place in (0, 1):
                out += [(a, in_place, stop_log, level2_log, levels_only) for stop_log in range(-1, a)]
    return out


def described(exe, cases):
    """{case: [lines]} from a program that answers cases on standard input with '# case' and the launch lines"""
    r = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % c for c in cases).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out, cur = {}, None
    for ln in r.stdout.decode().splitlines():
        if ln.startswith("# "):
            cur = out.setdefault(ln[2:], [])
        else:
            cur.append(ln)
    return out


def test_every_tree_launches_what_it_launched_before(tmp_path):
    """merkle_plan.h alone, compiled by g++ with the address and undefined-behaviour sanitizers and run as a program: 3774 trees, line for line."""
    exe = str(tmp_path / "merkle_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "distaff_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_plan", "merkle_plan_check.cpp")])
    cases = plan_cases()
    got = described(exe, cases)
    g = json.load(open(GOLDEN))
    keys = ["%d %d %d %d %d" % c for c in cases]
    assert len(set(keys)) == len(keys) == 3774
    missing = [k for k in keys if k not in g["launches"]]
    assert not missing, "cases without a recorded answer: %s" % missing[:5]
    want = {k: [g["lines"][int(i)] for i in g["launches"][k].split()] for k in keys}
    wrong = [(k, want[k], got.get(k)) for k in keys if got.get(k) != want[k]]
    assert not wrong, "%d of %d trees are built differently, first (a, in_place, stop_log, level2_log, levels_only) = %s\nrecorded: %s\nnow:      %s" % ((len(wrong), len(keys)) + wrong[0])
    assert all(got[k] for k in keys)


def switch_key(switches):
    return ",".join("%s=%s" % kv for kv in sorted(switches.items())) or "default"


def hash_kernel_stats(switches):
    """{'single' | 'world2' | 'world8': {kernel of kernels_hash.hip: [launches, bytes]}} of a 2^7-step Fibonacci proof with every launch profiled;
    the sharded proofs report the sum over their ranks.  Binds the library the process has chosen."""
    import distaff_amd as D
    import oracle as O
    saved = {k: os.environ.pop(k, None) for sw in SWITCH_SETS for k in sw}
    os.environ.update(switches)
    try:
        t = O.fibonacci_trace(1 << 7)
        op = O.Prover.from_trace(t, 1, grinding=8)
        expected = op.prove()
        out = {}
        for world in (1, 2, 8):
            ctxs = []
            for r in range(world):
                ctx = D.Context(7, t.width, t.ctx_depth, t.loop_depth, rank=r, world=world, grinding=8)
                ctx.upload(t.columns)
                ctx.set_profiling(1)
                ctxs.append(ctx)
            proof = ctxs[0].prove(t.public_inputs, op.outputs) if world == 1 else D.prove_sharded_local(ctxs, t.public_inputs, op.outputs)
            assert proof == expected
            total = {}
            for ctx in ctxs:
                for name, st in ctx.kernel_stats().items():
                    if name in HASH_KERNELS:
                        acc = total.setdefault(name, [0, 0.0])
                        acc[0] += st["launches"]; acc[1] += st["bytes"]
                ctx.close()
            out["single" if world == 1 else "world%d" % world] = total
        return out
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def check_kernel_stats(switches):
    want = json.load(open(GOLDEN))["kernel_stats"][switch_key(switches)]
    got = hash_kernel_stats(switches)
    for way in ("single", "world2", "world8"):
        assert {k: list(v) for k, v in got[way].items()} == want[way], "%s, %s" % (switch_key(switches), way)


def check_two_cosets_per_rank():
    """Blowup 16 on 8 ranks at 2^7 steps: two cosets per rank, the narrowest tiles of the transposing kernels (2 columns x 128 k), a trace tree
    with one rank-local level and a constraint tree with none -- dst_prove_sharded_local returns the oracle's proof."""
    import distaff_amd as D
    import oracle as O
    t = O.fibonacci_trace(1 << 7)
    op = O.Prover.from_trace(t, 1, ext=16, num_queries=100, grinding=8)
    expected = op.prove()
    ctxs = []
    for r in range(8):
        ctx = D.Context(7, t.width, t.ctx_depth, t.loop_depth, log_blowup=4, num_queries=100, grinding=8, rank=r, world=8)
        ctx.upload(t.columns)
        ctxs.append(ctx)
    try:
        assert D.prove_sharded_local(ctxs, t.public_inputs, op.outputs) == expected
    finally:
        for ctx in ctxs:
            ctx.close()


WORKER = r'''
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_merkle_launch_plan as T
T.check_two_cosets_per_rank()
json.dump({T.switch_key(sw): T.hash_kernel_stats(sw) for sw in T.SWITCH_SETS}, open(sys.argv[1], "w"))
'''


def test_callers_ask_for_the_trees_they_asked_for_before(tmp_path):
    """The emulated build, in a subprocess (the library is chosen when the package is imported): one context, two ranks and eight ranks under the
    three switch sets -- launches and bytes of every hashing kernel as recorded.  The same process first proves the two-cosets-per-rank shape."""
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-C", emu_dir, "-j8"], stdout=subprocess.DEVNULL)
    script, result = tmp_path / "stats_worker.py", tmp_path / "stats.json"
    script.write_text(WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    env = dict(os.environ, DISTAFF_HIP_LIB=os.path.join(emu_dir, "_build", "libdistaff_emu.so"), DISTAFF_HIP_RUNTIME="none")
    r = subprocess.run([sys.executable, str(script), str(result)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    got, want = json.load(open(result)), json.load(open(GOLDEN))["kernel_stats"]
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("switches", SWITCH_SETS, ids=switch_key)
def test_callers_ask_for_the_same_trees_on_the_device(switches):
    check_kernel_stats(switches)


@pytest.mark.gpu
def test_two_cosets_per_rank_at_128_steps():
    check_two_cosets_per_rank()
