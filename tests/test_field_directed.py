"""fe.h on the device, operation by operation, on inputs DIRECTED at the rare branches of its reductions.

On gfx950 the primitives of fe.h are single VALU instructions in inline assembly whose carries and borrows are lane masks in SGPR pairs;
the host and the emulated build run the same dataflow on plain integers and cannot see those instructions.  Uniform operands do not reach
the branches where the masks matter: the second fold leaving bit 128 set, a value in [p, 2^128) that only the trial subtraction catches,
an add-carry cancelled by the subtract-borrow -- each has a probability of 2^-35 .. 2^-82 per uniform product.  Here every such branch
is a CLASS of at least 256 operand pairs, built by choosing the result r and one factor a and solving the other one, b = r / a.

Classes of a product T are named from the stage values that fe.h's comments define (C = 2^128 - p, K = 45 * 2^8):

    hi, lo = divmod(T, 2^128);  v = lo + hi * C;  vh, vl = divmod(v, 2^128);  y = vl + vh * C
    "y4"         y >= 2^128
    "ge_cancel"  p <= y < 2^128 and vl + ((vh * K) << 32) >= 2^128      (the carry of the add chain is cancelled by the borrow)
    "ge_plain"   p <= y < 2^128 without that carry
    "lt"         y < p
    "lt_cancel"  y < p with that carry: only the cancellation (c & ~d) keeps bit 128 clear, and nothing else catches a slip, because the
                 trial subtraction of p borrows.  It needs vh > C: no product of two 128-bit values has it (vh <= C - 1), a sum of many
                 products (fe_acc, vh < 2^54) and the single fold of fe_mul_tw (H < 2^65 in the place of vh) do.

and for the multiplication by a table entry, T = (x mod 2^64) * w + (x >> 64) * (w * 2^64 mod p), the same with its single fold
(H, L = divmod(T, 2^128), y = L + H * C) and T6 = H >> 64.

Unreachable classes.  In the single fold of fe_mul_tw the add chain computes L + ((H * K) << 32) = y + H, so with T6 = 1 (H >= 2^64 > C)
a value y >= p always comes with the carry: "T6=1/ge_plain" does not exist, the other nine combinations of T6 and the classes do.
fe_shift64 reduces w * 2^64 < 2^192 and fe_mul_small x * k < 2^160: hi < 2^64, so v < 2^128 + 2^110, and when
vh = 1 then vl < 2^110: neither y >= 2^128 nor vl + (K << 32) >= 2^128 can happen.  Their classes are "ge_plain" and "lt" only.
fe_mul_small(x, 0) and (x, 1) reduce a value below 2^128 that is canonical already: "lt" only; "ge_plain" comes from k >= 2.

The reference is Python integers, never another function of fe.h.  Equality of all four limbs is exact, which also proves that every
output is canonical.  Every set runs in two lane layouts: class by class in contiguous blocks (whole wavefronts take one branch), and
shuffled by a fixed permutation with a common-case pair after every directed one (neighbouring lanes disagree on every mask)."""
import functools
import random

import pytest

P = 2**128 - 45 * 2**40 + 1
C = 2**128 - P
K = 11520
M128 = 2**128
M64 = 2**64
FLOOR = 256                       # members of every class: every lane position of four wavefronts
KINDS = ("y4", "ge_cancel", "ge_plain", "lt")
EDGE = [e % P for e in (0, 1, 2, P - 1, P - 2, (P + 1) // 2, 2**64, 2**64 - 1, 2**127, 2**96, P - 2**40, C, C + 1, 2**128 - 2**88, 2**32 - 1, 2**96 - 1)]
EXACT = [1, P - 1, C - 1, C, C + 1, 2**128 - P - 1, 2**64]
DELTAS = [1, 2**32 - 1, 2**32, C - 1, C, C + 1, 2**64, 2**96]
SMALL_K = [0, 1, 2, 2**32 - 1, 11520]
DOT_TERMS = [1, 2, 39, 40, 63, 64]
SINGLE_LIMB = [(2**32 - 1) << (32 * i) for i in range(4)]
Y4_RANGE, GE_RANGE, ANY_RANGE, TOP_RANGE = (C, 2**80), (0, C), (0, P), (P - 2**44, P)


# ---- stage values and class names -----------------------------------------------------------------------------------------------------
def _kind(carry, y):
    return "y4" if y >= M128 else ("ge_cancel" if carry else "ge_plain") if y >= P else "lt_cancel" if carry else "lt"


def stages(T):
    """-> (vh, class name, y) of the two folds of a product or a sum of products T"""
    hi, lo = divmod(T, M128)
    vh, vl = divmod(lo + hi * C, M128)
    y = vl + vh * C
    return vh, _kind(vl + ((vh * K) << 32) >= M128, y), y


def classify(T):
    return stages(T)[1]


def tw_sum(x, w):
    return (x % M64) * w + (x >> 64) * (w * M64 % P)


def stages_tw(x, w):
    """-> (T6, class name, y) of the single fold of a multiplication by the table entry of w"""
    H, L = divmod(tw_sum(x, w), M128)
    y = L + H * C
    return H >> 64, _kind(L + ((H * K) << 32) >= M128, y), y


def classify_tw(x, w):
    t6, kind, _ = stages_tw(x, w)
    return "T6=%d/%s" % (t6, kind)


def cube_product(x, _=None):
    return (x % P) * (x % P) % P * x          # what the second multiplication of fe_cube reduces


Q_ODD = (P - 1) >> 40                          # p - 1 = 2^40 * (2^88 - 45)
NON_RESIDUE = next(z for z in range(2, 100) if pow(z, (P - 1) // 2, P) == P - 1)
THIRD = pow(3, -1, P - 1)                      # 3 does not divide p - 1: cubing is a bijection


def sqrt_mod(r):
    """a square root of r modulo p (Tonelli-Shanks over the 2^40 two-part of p - 1), or None"""
    if r == 0:
        return 0
    if pow(r, (P - 1) // 2, P) != 1:
        return None
    m, c, t, x = 40, pow(NON_RESIDUE, Q_ODD, P), pow(r, Q_ODD, P), pow(r, (Q_ODD + 1) // 2, P)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % P, i + 1
        b = pow(c, 1 << (m - i - 1), P)
        m, c = i, b * b % P
        t, x = t * c % P, x * b % P
    return x


TW_KINDS = tuple("T6=%d/%s" % (t6, k) for t6 in (0, 1) for k in KINDS + ("lt_cancel",) if (t6, k) != (1, "ge_plain"))


# ---- the reference: Python integers ---------------------------------------------------------------------------------------------------
REFERENCE = {
    "add": lambda x, y: (x + y) % P,
    "sub": lambda x, y: (x - y) % P,
    "addsub_sum": lambda x, y: (x + y) % P,
    "addsub_dif": lambda x, y: (x - y) % P,
    "mul": lambda x, y: (x % P) * (y % P) % P,
    "mul_portable": lambda x, y: x * y % P,
    "mul_tw": lambda x, y: (x % P) * y % P,
    "sqr": lambda x, y: (x % P) * (x % P) % P,
    "cube": lambda x, y: (x % P) ** 3 % P,
    "shift64": lambda x, y: x * 2**64 % P,
    "mul_small": lambda x, y: x * (y % 2**32) % P,
}
ELEMENTWISE = sorted(REFERENCE)


def _fill(want, draw, kind, limit=400000):
    """draws pairs until every class of `want` has FLOOR members -> {class: [(x, y), ...]} (a class may stay short: the count test says so)"""
    out = {k: [] for k in want}
    for _ in range(limit):
        if all(len(v) >= FLOOR for v in out.values()):
            break
        pair = draw()
        if pair is None:
            continue
        k = kind(*pair)
        if k in out and len(out[k]) < FLOOR:
            out[k].append(pair)
    return out


@functools.lru_cache(maxsize=None)
def directed_cases():
    """-> {operation: {class name: ([(x, y), ...], predicate(x, y))}}: the operand pairs of every class and the test that says a pair is
    a member, from a fixed seed.  Built once per process."""
    rnd = random.Random(20250128)
    cases = {op: {} for op in ELEMENTWISE}

    def put(ops, name, pairs, pred):
        for op in ops:
            assert name not in cases[op]
            cases[op][name] = (list(pairs), pred)

    def put_kinds(ops, prefix, filled, kind):
        for k, pairs in filled.items():
            put(ops, prefix + k, pairs, lambda x, y, k=k: kind(x, y) == k)

    def target(ranges):
        return rnd.randrange(*rnd.choice(ranges))

    def rep(pairs):
        pairs = list(pairs)
        return pairs * -(-FLOOR // len(pairs))

    # -- general multiplication, canonical operands: mul and mul_portable
    def draw_mul():
        a = rnd.randrange(1, P)
        return a, target((Y4_RANGE, GE_RANGE, GE_RANGE, GE_RANGE, ANY_RANGE)) * pow(a, -1, P) % P
    prod = lambda x, y: classify(x * y)
    both = ("mul", "mul_portable")
    put_kinds(both, "", _fill(KINDS, draw_mul, prod), prod)
    exact = []
    for r in EXACT:
        for _ in range(40):
            a = rnd.randrange(1, P)
            exact.append((a, r * pow(a, -1, P) % P))
    put(both, "exact", exact, lambda x, y: x * y % P in EXACT)
    small = []
    for _ in range(FLOOR):
        bits = rnd.randrange(0, 129)
        small.append((rnd.randrange(2**bits), rnd.randrange(2**(128 - bits))))
    put(both, "vh0", small, lambda x, y: x < P and y < P and stages(x * y)[0] == 0)
    vh_top = stages((P - 1) ** 2)[0]
    put(both, "vh_max", [(P - 1 - i, P - 1 - j) for i in range(16) for j in range(16)], lambda x, y: stages(x * y)[0] == vh_top)
    single = [(a, b) for a in SINGLE_LIMB for b in SINGLE_LIMB]
    put(both, "single_limb", rep(single), lambda x, y: x in SINGLE_LIMB and y in SINGLE_LIMB)

    # -- general multiplication, non-canonical operands (fe_mul_wide takes ANY 128-bit values): mul only
    def draw_noncanon_x():
        a = P + rnd.randrange(1, C)
        return a, target((Y4_RANGE, GE_RANGE, GE_RANGE, GE_RANGE)) * pow(a - P, -1, P) % P
    directed = KINDS[:3]
    put_kinds(["mul"], "noncanon_x/", _fill(directed, draw_noncanon_x, prod), lambda x, y: x >= P > y and prod(x, y))
    put_kinds(["mul"], "noncanon_y/", {k: [(y, x) for x, y in v] for k, v in _fill(directed, draw_noncanon_x, prod).items()},
              lambda x, y: y >= P > x and prod(x, y))
    special = [(a, rnd.randrange(M128)) for a in (P, P + 1, M128 - 1) for _ in range(86)]
    put(["mul"], "noncanon_x/special", special, lambda x, y: x in (P, P + 1, M128 - 1))
    top_wide = stages((M128 - 1) ** 2)[0]
    put(["mul"], "noncanon_both/vh_max", [(M128 - 1 - i, M128 - 1 - j) for i in range(16) for j in range(16)], lambda x, y: min(x, y) >= P and stages(x * y)[0] == top_wide)
    put(["mul"], "noncanon_both/uniform", [(P + rnd.randrange(C), P + rnd.randrange(C)) for _ in range(FLOOR)], lambda x, y: min(x, y) >= P)
    put(["mul", "sqr", "cube"], "all_ones", [(M128 - 1, M128 - 1)] * FLOOR, lambda x, y: x == y == M128 - 1)

    # -- squares and cubes: the root of the chosen result
    def draw_sqr():
        x = sqrt_mod(target((Y4_RANGE, GE_RANGE, GE_RANGE, GE_RANGE, GE_RANGE, ANY_RANGE)))
        return None if x is None else (rnd.choice((x, P - x)), 0)
    sq = lambda x, y: classify(x * x)
    put_kinds(["sqr"], "", _fill(KINDS, draw_sqr, sq), sq)
    roots = [(x, 0) for r in EXACT for s in [sqrt_mod(r)] if s is not None for x in (s, P - s)]
    put(["sqr"], "exact", rep(roots), lambda x, y: x * x % P in EXACT)
    put(["sqr"], "vh0", [(rnd.randrange(M64), 0) for _ in range(FLOOR)], lambda x, y: stages(x * x)[0] == 0)
    put(["sqr"], "vh_max", [(P - 1 - i, 0) for i in range(FLOOR)], lambda x, y: stages(x * x)[0] == vh_top)

    def draw_cube():
        return pow(target((Y4_RANGE, GE_RANGE, GE_RANGE, GE_RANGE, ANY_RANGE)), THIRD, P), 0
    cu = lambda x, y: classify(cube_product(x))
    put_kinds(["cube"], "", _fill(KINDS, draw_cube, cu), cu)
    put(["cube"], "exact", rep((pow(r, THIRD, P), 0) for r in EXACT), lambda x, y: x**3 % P in EXACT)
    put(["cube"], "vh0", [(rnd.randrange(2**42), 0) for _ in range(FLOOR)], lambda x, y: stages(cube_product(x))[0] == 0)
    put(["sqr", "cube"], "single_limb", rep((a, 0) for a in SINGLE_LIMB), lambda x, y: x in SINGLE_LIMB)

    # -- multiplication by a table entry: x any 128-bit value, w canonical
    def draw_tw():
        how = rnd.randrange(5)
        if how == 4:                                                         # H < C - r, so that no carry comes with p <= y < 2^128
            x = rnd.randrange(1, 2**40)
            return x, rnd.randrange(C // 2) * pow(x, -1, P) % P
        if how == 0:                                                         # both halves of x at the top: T reaches 2^192 for half of the w
            x = ((M64 - 1 - rnd.randrange(2**60)) << 64) | (M64 - 1 - rnd.randrange(2**60))
        elif how == 1:
            return M128 - 1 - rnd.randrange(2**60), P - 1 - rnd.randrange(2**40)
        else:
            x = rnd.randrange(1, M128)
        if x % P == 0:
            return None
        return x, target((Y4_RANGE, GE_RANGE, GE_RANGE, GE_RANGE, ANY_RANGE, (C, 2**100), TOP_RANGE)) * pow(x % P, -1, P) % P
    tw_kinds = [k for k in TW_KINDS]
    put_kinds(["mul_tw"], "", _fill(tw_kinds, draw_tw, classify_tw), classify_tw)

    def draw_tw_noncanon():
        if rnd.randrange(4) == 0:                                            # x = p + d and a small w: y = p + d * w, the carry comes with (d + 1) * w > C
            return P + rnd.randrange(1, 2**20), rnd.randrange(1, 2**24)
        x = P + rnd.randrange(1, C)
        return x, target((Y4_RANGE, GE_RANGE, GE_RANGE, TOP_RANGE)) * pow(x - P, -1, P) % P
    tw_kind = lambda x, w: stages_tw(x, w)[1]
    put_kinds(["mul_tw"], "noncanon_x/", _fill(directed + ("lt_cancel",), draw_tw_noncanon, tw_kind), lambda x, w: x >= P and tw_kind(x, w))
    put(["mul_tw"], "noncanon_x/special", [(a, rnd.randrange(P)) for a in (P, P + 1, M128 - 1) for _ in range(86)], lambda x, w: x in (P, P + 1, M128 - 1) and w < P)
    exact = []
    for r in EXACT:
        for _ in range(40):
            x = rnd.randrange(1, M128)
            exact.append((x, r * pow(x % P, -1, P) % P))
    put(["mul_tw"], "exact", exact, lambda x, w: x * w % P in EXACT and w < P)
    put(["mul_tw"], "h0", [(rnd.randrange(M64), rnd.randrange(M64)) for _ in range(FLOOR)], lambda x, w: tw_sum(x, w) < M128)
    h_top = tw_sum(M128 - 1, P - 1) >> 128
    put(["mul_tw"], "h_max", [(M128 - 1 - i, P - 1 - j) for i in range(16) for j in range(16)], lambda x, w: h_top - (tw_sum(x, w) >> 128) < 2**20)
    # bit 192 set over T5 == 0 (the merge chain and the top window's counter at their wrap-around): x = 2^128 - 1 - (small) and
    # w = h * 2^64 + (2^64 - 1 - h) give w + w * 2^64 = 2^128 - 1 + h (C - 1) (mod p), so T = 2^192 + (about h * C * 2^64)
    def draw_t5_wrap():
        h = rnd.randrange(2**20, 2**49)
        return M128 - 1 - (rnd.randrange(4) << 64) - rnd.randrange(4), (h << 64) + M64 - 1 - h
    t5_wrap = lambda x, w: (tw_sum(x, w) >> 160) == 2**32
    put(["mul_tw"], "T6=1/T5=0", _fill(["T6=1/T5=0"], draw_t5_wrap, lambda x, w: t5_wrap(x, w) and "T6=1/T5=0")["T6=1/T5=0"], lambda x, w: w < P and t5_wrap(x, w))
    put(["mul_tw"], "single_limb", rep(single), lambda x, w: x in SINGLE_LIMB and w in SINGLE_LIMB)
    put(["mul_tw"], "all_ones", [(M128 - 1, P - 1)] * FLOOR, lambda x, w: x == M128 - 1 and w == P - 1)       # the largest canonical table entry

    # -- sums and differences
    def some(n, draw):
        return [draw() for _ in range(n)]
    adds = ("add", "sub", "addsub_sum", "addsub_dif")

    def below():
        s = rnd.randrange(P)
        x = rnd.randrange(s + 1)
        return x, s - x

    def at(s):                                                               # canonical x, y with x + y == s >= p
        x = rnd.randrange(s - (P - 1), P)
        return x, s - x
    put(adds, "sum<p", some(FLOOR, below), lambda x, y: x + y < P)
    put(adds, "sum==p", some(FLOOR, lambda: at(P)), lambda x, y: x + y == P)
    put(adds, "p<sum<2^128", some(FLOOR, lambda: at(P + rnd.randrange(1, C))), lambda x, y: P < x + y < M128)
    put(adds, "sum>=2^128", some(FLOOR, lambda: at(rnd.randrange(M128, 2 * P - 1))), lambda x, y: x + y >= M128)
    put(adds, "x==y", [(x, x) for x in EDGE] + some(FLOOR, lambda: (rnd.randrange(P),) * 2), lambda x, y: x == y)
    deltas = [d for d in DELTAS for _ in range(16)] + [rnd.randrange(1, 2**46) for _ in range(128)]
    minus = [(y - d, y) for d in deltas for y in [rnd.randrange(d, P)]]
    in_deltas = lambda d: d in DELTAS or 0 < d < 2**46
    put(adds, "dif==-delta", minus, lambda x, y: in_deltas(y - x))
    put(adds, "dif==+delta", [(y, x) for x, y in minus], lambda x, y: in_deltas(x - y))
    for op in both + ("mul_tw",) + adds:
        put([op], "edge_pairs", [(x, y) for x in EDGE for y in EDGE], lambda x, y: x in EDGE and y in EDGE)

    # -- w * 2^64 and x * k (k < 2^32) through the portable reduction; see the module docstring for the classes that do not exist
    inv64 = pow(M64, -1, P)
    put_kinds(["shift64"], "", _fill(("ge_plain", "lt"), lambda: (target((GE_RANGE, ANY_RANGE)) * inv64 % P, 0), lambda w, _: classify(w * M64)), lambda w, _: classify(w * M64))
    put(["shift64"], "edge", rep((e, 0) for e in EDGE), lambda w, _: w in EDGE)

    def draw_small():
        k = rnd.choice(SMALL_K[2:])
        return target((GE_RANGE, ANY_RANGE)) * pow(k, -1, P) % P, k
    sm = lambda x, k: classify(x * k)
    put_kinds(["mul_small"], "", _fill(("ge_plain", "lt"), draw_small, sm), lambda x, k: k in SMALL_K and sm(x, k))
    put(["mul_small"], "edge", rep((e, k) for e in EDGE for k in SMALL_K), lambda x, k: x in EDGE and k in SMALL_K)
    for k in SMALL_K:
        put(["mul_small"], "k=%d" % k, [(rnd.randrange(P), k) for _ in range(FLOOR)], lambda x, kk, k=k: kk == k)
    return cases


COMMON = {                                  # the common case of every operation: what uniform data gives
    "mul_tw": lambda rnd: (rnd.randrange(M128), rnd.randrange(P)),
    "mul_small": lambda rnd: (rnd.randrange(P), rnd.randrange(2**32)),
}


@functools.lru_cache(maxsize=None)
def laid_out(op, layout):
    """-> ([(x, y)], [class name per lane]): every class of `op` in contiguous blocks, or shuffled by a fixed permutation with a
    common-case pair after every directed one"""
    pairs, names = [], []
    for name, (members, _) in directed_cases()[op].items():
        pairs += members
        names += [name] * len(members)
    if layout == "blocks":
        return pairs, names
    rnd = random.Random("mixed " + op)
    order = list(range(len(pairs)))
    rnd.shuffle(order)
    common = COMMON.get(op, lambda rnd: (rnd.randrange(P), rnd.randrange(P)))
    mixed, mixed_names = [], []
    for i in order:
        mixed += [pairs[i], common(rnd)]
        mixed_names += [names[i], "common"]
    return mixed, mixed_names


# ---- sums of products with one reduction ----------------------------------------------------------------------------------------------
DOT_DIRECTED = KINDS[:3]


def dot_wide_classes(terms):
    return ("y4", "ge_cancel") + (("lt_cancel",) if terms >= 39 else ())


@functools.lru_cache(maxsize=None)
def dot_case(terms, layout):
    """-> (a, b, [class per lane]) for out[i] = sum_{j<terms} a[(i+j) % n] * b[(i+7j) % n] + a[i].  Lanes [0, n - 7 (terms - 1)) read b
    without wrapping, so from the top lane down each one owns the pair a[i], b[i]: the result is chosen and b[i] solved (b[i] canonical),
    drawn again until the integer sum of the lane is in the class wanted there.

    Two regions.  In the WIDE one every operand is any 128-bit value (every fourth a and every sixteenth b of the uniform lanes
    non-canonical: p, p + 1, 2^128 - 1 among them); a sum of many such products has vh >= C, so a value in [p, 2^128) always comes with the
    cancelled carry there: its classes are "y4", "ge_cancel", "lt" and, from 39 terms on, "lt_cancel" (one or two products seldom or never
    reach vh > C).  "ge_plain" needs vh < C - r, that is a sum below 2^256: in the
    NARROW region behind it (and in the wrapping tail those lanes read) a < 2^128 / 2^ceil(log2 terms) while b stays any 128-bit value."""
    rnd = random.Random("dot %d %s" % (terms, layout))
    wide = [k for k in dot_wide_classes(terms) + ("lt",) for _ in range(FLOOR)]
    narrow = [k for k in ("ge_plain", "lt") for _ in range(FLOOR)]
    if layout == "mixed":
        wide += ["lt"] * FLOOR
        rnd.shuffle(wide)
        rnd.shuffle(narrow)
    lanes = wide + ["lt"] * 64 + narrow                       # 64 uniform lanes: no directed lane of the wide region reads a narrow a
    wide = lanes[:-len(narrow)]
    n = len(lanes) + 7 * (terms - 1)
    a_narrow = 2**(128 - (terms - 1).bit_length())
    noncanon = [P, P + 1, M128 - 1]

    def any128(one_in):
        return rnd.choice(noncanon + [P + rnd.randrange(C)]) if rnd.randrange(one_in) == 0 else rnd.randrange(M128)
    a = [any128(4) for _ in wide] + [rnd.randrange(a_narrow) for _ in range(n - len(wide))]
    b = [any128(16) for _ in range(n)]
    for i in reversed(range(len(lanes))):
        if lanes[i] == "lt":
            continue
        rest = sum(a[i + j] * b[i + 7 * j] for j in range(1, terms))
        for _ in range(400):
            a[i] = rnd.randrange(1, M128 if i < len(wide) else a_narrow)
            if a[i] % P == 0:
                continue
            r = rnd.randrange(*{"y4": Y4_RANGE, "ge_cancel": GE_RANGE, "lt_cancel": TOP_RANGE, "ge_plain": (0, 2**rnd.randrange(1, 46))}[lanes[i]])
            b[i] = (r - rest - a[i]) * pow(a[i] % P, -1, P) % P
            if classify(rest + a[i] * b[i] + a[i]) == lanes[i]:
                break
    return a, b, lanes + ["tail"] * (n - len(lanes))


def dot_sums(terms, a, b):
    """the integer value every lane reduces"""
    n = len(a)
    return [sum(a[(i + j) % n] * b[(i + 7 * j) % n] for j in range(terms)) + a[i] for i in range(n)]


# ---- the classes hold what they say (no GPU) --------------------------------------------------------------------------------------------
REQUIRED = {
    "mul": list(KINDS) + ["exact", "vh0", "vh_max", "single_limb", "all_ones", "edge_pairs", "noncanon_x/special", "noncanon_both/vh_max", "noncanon_both/uniform"]
           + ["noncanon_%s/%s" % (s, k) for s in "xy" for k in DOT_DIRECTED],
    "mul_portable": list(KINDS) + ["exact", "vh0", "vh_max", "single_limb", "edge_pairs"],
    "sqr": list(KINDS) + ["exact", "vh0", "vh_max", "single_limb", "all_ones"],
    "cube": list(KINDS) + ["exact", "vh0", "single_limb", "all_ones"],
    "mul_tw": list(TW_KINDS) + ["noncanon_x/" + k for k in DOT_DIRECTED + ("lt_cancel",)]
              + ["noncanon_x/special", "exact", "h0", "h_max", "T6=1/T5=0", "single_limb", "all_ones", "edge_pairs"],
    "shift64": ["ge_plain", "lt", "edge"],
    "mul_small": ["ge_plain", "lt", "edge"] + ["k=%d" % k for k in SMALL_K],
}
for _op in ("add", "sub", "addsub_sum", "addsub_dif"):
    REQUIRED[_op] = ["sum<p", "sum==p", "p<sum<2^128", "sum>=2^128", "x==y", "dif==-delta", "dif==+delta", "edge_pairs"]


def test_every_class_has_its_members():
    """Every class of every operation exists, has at least 256 members, and every member passes the class's own test on the stage values.
    The stage values themselves are consistent: y = T (mod p) and y < 2p, which is what the last conditional subtraction relies on."""
    cases = directed_cases()
    short = []
    for op in ELEMENTWISE:
        assert sorted(cases[op]) == sorted(REQUIRED[op]), op
        for name, (members, pred) in cases[op].items():
            if len(members) < FLOOR:
                short.append((op, name, len(members)))
            wrong = [m for m in members if not pred(*m)]
            assert not wrong, (op, name, len(wrong), wrong[:2])
            if op not in ("mul", "mul_tw", "sqr", "cube"):
                assert all(x < P and y < P for x, y in members), (op, name)
        for x, y in laid_out(op, "mixed")[0][:2000]:
            if op == "mul_tw":
                yy, T = stages_tw(x, y)[2], tw_sum(x, y)
                assert y < P and T < 2**193
            elif op in ("mul", "mul_portable", "sqr", "cube"):
                T = {"mul": x * y, "mul_portable": x * y, "sqr": x * x, "cube": cube_product(x)}[op]
                yy = stages(T)[2]
            else:
                continue
            assert yy % P == T % P and yy < 2 * P, (op, x, y)
    assert not short, short
    # the exact results, each of them
    for op, result in (("mul", lambda x, y: x * y % P), ("mul_tw", lambda x, y: x * y % P), ("sqr", lambda x, y: x * x % P), ("cube", lambda x, y: x**3 % P)):
        hit = {result(x, y) for x, y in cases[op]["exact"][0]}
        assert hit == set(EXACT) if op != "sqr" else hit and hit <= set(EXACT), (op, hit)
    assert {y - x for x, y in cases["add"]["dif==-delta"][0]} >= set(DELTAS)


@pytest.mark.parametrize("terms", DOT_TERMS)
def test_every_directed_sum_is_in_its_class(terms):
    """the sums of products: at least 256 lanes of each of "y4", "ge_cancel", "ge_plain" and (from 39 terms on) "lt_cancel" in both layouts, by the stage values of the
    integer sum each lane reduces; the overflow limb of every sum stays below the documented 2^7"""
    for layout in ("blocks", "mixed"):
        a, b, lanes = dot_case(terms, layout)
        sums = dot_sums(terms, a, b)
        assert all(s >> 256 < 2**7 for s in sums)
        assert any(v >= P for v in a) and any(v >= P for v in b)
        for kind in dot_wide_classes(terms) + ("ge_plain",):
            members = [i for i, k in enumerate(lanes) if k == kind]
            assert len(members) >= FLOOR, (terms, layout, kind, len(members))
            wrong = [i for i in members if classify(sums[i]) != kind]
            assert not wrong, (terms, layout, kind, len(wrong))
        if layout == "mixed":
            directed = [k not in ("lt", "tail") for k in lanes]
            assert sum(x != y for x, y in zip(directed, directed[1:])) > FLOOR        # neighbouring lanes disagree


# ---- on the device ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import distaff_amd as D
    c = D.Context(6, 17, 0, 0, log_blowup=4)
    yield c
    c.close()


CHUNK = 16384                                # 3 * count elements of the context's scratch per call


def _device(ctx, op, xs, ys):
    import distaff_amd as D
    out = []
    for k in range(0, len(xs), CHUNK):
        out += D.arr_to_ints(ctx.field_op(op, D.ints_to_arr(xs[k:k + CHUNK]), D.ints_to_arr(ys[k:k + CHUNK])))
    return out


def _compare(got, want, names, what):
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    classes = sorted({names[i] for i in bad})
    assert not bad, "%s: %d of %d lanes differ, classes %s; first: lane %d (%s) got %#x want %#x" % (
        what, len(bad), len(want), classes, bad[0], names[bad[0]], got[bad[0]], want[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["blocks", "mixed"])
@pytest.mark.parametrize("op", ELEMENTWISE)
def test_directed_operands(ctx, op, layout):
    """one fe.h function per operation on every class of its directed operands, exact against Python integers"""
    pairs, names = laid_out(op, layout)
    xs, ys = [x for x, _ in pairs], [y for _, y in pairs]
    want = [REFERENCE[op](x, y) for x, y in pairs]
    _compare(_device(ctx, op, xs, ys), want, names, "%s, %s" % (op, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["blocks", "mixed"])
@pytest.mark.parametrize("terms", DOT_TERMS)
def test_directed_sums_of_products(ctx, terms, layout):
    """fe_acc over 1 .. 64 terms of any 128-bit operands whose totals are directed at the classes of the nine-limb reduction"""
    import distaff_amd as D
    a, b, lanes = dot_case(terms, layout)
    want = [s % P for s in dot_sums(terms, [v % P for v in a], [v % P for v in b])]
    got = D.arr_to_ints(ctx.field_op("dot%d" % terms, D.ints_to_arr(a), D.ints_to_arr(b)))
    _compare(got, want, lanes, "dot%d, %s" % (terms, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("terms", DOT_TERMS)
def test_sums_of_maximal_products(ctx, terms):
    """fe_acc with every window's counter at its maximum: all operands p - 1, all operands 2^128 - 1 (at 64 terms the documented limit
    of fe_acc: the overflow limb is 63), and operands whose upper two limbs are all ones over uniform lower ones -- the top window of
    the sum then sits just below 2^64 and the counters' chain carries into the overflow limb in some lanes and not in others"""
    import distaff_amd as D
    assert (64 * (M128 - 1) ** 2 + M128 - 1) >> 256 == 63
    rnd = random.Random("top %d" % terms)
    upper = (M64 - 1) << 64
    for name, a, b in (("p - 1", [P - 1] * FLOOR, [P - 1] * FLOOR), ("2^128 - 1", [M128 - 1] * FLOOR, [M128 - 1] * FLOOR),
                       ("upper limbs", [upper | rnd.randrange(M64) for _ in range(2 * FLOOR)], [upper | rnd.randrange(M64) for _ in range(2 * FLOOR)])):
        want = [s % P for s in dot_sums(terms, [v % P for v in a], [v % P for v in b])]
        got = D.arr_to_ints(ctx.field_op("dot%d" % terms, D.ints_to_arr(a), D.ints_to_arr(b)))
        _compare(got, want, [name] * len(a), "dot%d" % terms)


@pytest.mark.gpu
def test_unknown_operation_is_refused(ctx):
    """an operation number outside 0 .. 13 and 256 + (1 .. 64) is an argument error, not a vector of zeros"""
    import ctypes
    import distaff_amd as D
    one, out = D.ints_to_arr([1]), D.ints_to_arr([7])
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for op in (14, 255, 256, 256 + 65, -1):
        assert ctx.lib.dst_field_op(ctx._h, op, ptr(one), ptr(one), ptr(out), ctypes.c_size_t(1)) == D.DST_ERR_ARG
    assert D.arr_to_ints(out) == [7]
