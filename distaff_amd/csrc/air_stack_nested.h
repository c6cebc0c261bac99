// The user-stack constraints as nested sums: the statement that the product instances of the constraint kernel evaluate (air_kernel.h,
// section air_stack_nested).  What is here has no kernel arguments and no memory access -- two stack rows, the small flag tables and a
// selection of operations in, one constraint value out -- so the suite's air_merge_test.cpp checks its three tables (st_has, st_desc,
// st_term) against each other on the host.  The per-operation statement of the same constraints is air_stack_perop.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "fe.h"

__device__ __forceinline__ fe bnot(const fe& v) { return fe_sub(fe_one(), v); }
__device__ __forceinline__ fe is_bin(const fe& v) { return fe_sub(fe_sqr(v), v); }

template <int I, int N, class F>
__device__ __forceinline__ void static_for_air(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for_air<I + 1, N>(f); }
}

// ---- low-degree stack operations as nested sums -------------------------------------------------------------------------------
// The flag of low-degree operation `op` is lo2[op & 3] * mid[(op >> 2) & 3] * top[op >> 4] (trace_state.rs:281-350), and every
// stack constraint is sum_op flag(op) * term(op, slot) (constraints/stack/mod.rs:117-195).  Written as
//     sum_c top[c] * ( sum_b mid[b] * ( sum_a lo2[a] * term(a + 4b + 16c, slot) ) )
// the 32 flags are never formed and every level is a sum of products with one reduction (fe_acc): ~13k instructions per point
// instead of ~21k for flag products + per-term multiply-adds.  st_term states, per operation and slot, exactly what the
// per-operation statement (air_stack_perop.h) passes to agg(): slots 0..7 are the stack constraints, ST_AUX0 and ST_AUX1 the two
// auxiliary constraints.
struct StackRows { fe o[12], nw[8]; int sl; };            // o[8..11] and sl only matter to the deep instance (slice longer than 8)
#define ST_AUX0 8
#define ST_AUX1 9

// stack slots 0..7 (the slice always has max(depth, 8) = 8 items for depth <= 8), ST_AUX0, ST_AUX1
template <int OP, int I> constexpr bool st_has() {
    constexpr bool slot = I < 8, aux0 = I == ST_AUX0, aux1 = I == ST_AUX1;
    switch (OP) {
        case 0x00: case 0x01: case 0x05: case 0x06: case 0x07: return slot || aux0;       // ASSERT, ASSERTEQ, CHOOSE, CHOOSE2, CSWAP2
        case 0x02: case 0x0E: return slot || aux0;                                       // EQ, NOT
        case 0x03: case 0x04: case 0x08: case 0x09: case 0x0C: case 0x0D: return slot;   // DROP, DROP4, ADD, MUL, INV, NEG
        case 0x0A: case 0x0B: return slot || aux0 || aux1;                               // AND, OR
        case 0x10: return I >= 1 && slot;                                                // READ
        case 0x11: return I >= 2 && slot;                                                // READ2
        case 0x12: case 0x13: case 0x14: case 0x15: return slot;                         // DUP, DUP2, DUP4, PAD2
        case 0x18: return slot && I != 1;                                                // SWAP: both constraints in slot 0 (manipulation.rs:63-64)
        case 0x19: case 0x1A: case 0x1B: case 0x1C: case 0x1D: return slot;              // SWAP2, SWAP4, ROLL4, ROLL8, BINACC
        default: return false;
    }
}

template <int OP, int I>
__device__ __forceinline__ fe st_term(const StackRows& s) {
    const fe* o = s.o; const fe* nw = s.nw;
    constexpr int i = I < 8 ? I : 0;
    // the shift helpers of constraints/stack/mod.rs on a slice of s.sl >= 8 items (8 unless the stack is deeper): a left shift by
    // num zero-fills the last num slots
    auto L = [&](int num) {
        if (i + num < 8) return fe_sub(o[i + num < 8 ? i + num : 0], nw[i]);
        return i + num < s.sl ? fe_sub(o[i + num < 12 ? i + num : 0], nw[i]) : nw[i];
    };
    auto R = [&](int num) { return fe_sub(o[i - num < 0 ? 0 : i - num], nw[i]); };   // right shift by num (callers: i >= num)
    auto C = [&]() { return fe_sub(o[i], nw[i]); };                       // copy
    auto sel = [&](const fe& c, const fe& x, const fe& y) { return fe_add(y, fe_mul(c, fe_sub(x, y))); };   // c*x + (1-c)*y with one multiplication
    if constexpr (OP == 0x00) { if constexpr (I == ST_AUX0) return bnot(o[0]); else return L(1); }   // the ASSERT flag carries hd[0] (trace_state.rs:346): st_output puts it into the coefficient
    else if constexpr (OP == 0x01) { if constexpr (I == ST_AUX0) return fe_sub(o[0], o[1]); else return L(2); }
    else if constexpr (OP == 0x02) {
        const fe diff = fe_sub(o[1], o[2]);
        if constexpr (I == ST_AUX0) return fe_mul(nw[0], diff);
        else if constexpr (I == 0) return fe_sub(nw[0], bnot(fe_mul(diff, o[0])));
        else return L(2);
    }
    else if constexpr (OP == 0x03) return L(1);
    else if constexpr (OP == 0x04) return L(4);
    else if constexpr (OP == 0x05) {
        if constexpr (I == ST_AUX0) return is_bin(o[2]);
        else if constexpr (I == 0) return fe_sub(nw[0], sel(o[2], o[0], o[1]));
        else return L(2);
    }
    else if constexpr (OP == 0x06) {
        if constexpr (I == ST_AUX0) return is_bin(o[4]);
        else if constexpr (I == 0) return fe_sub(nw[0], sel(o[4], o[0], o[2]));
        else if constexpr (I == 1) return fe_sub(nw[1], sel(o[4], o[1], o[3]));
        else return L(4);
    }
    else if constexpr (OP == 0x07) {
        if constexpr (I == ST_AUX0) return is_bin(o[4]);
        else if constexpr (I == 0) return fe_sub(nw[0], sel(o[4], o[2], o[0]));
        else if constexpr (I == 1) return fe_sub(nw[1], sel(o[4], o[3], o[1]));
        else if constexpr (I == 2) return fe_sub(nw[2], sel(o[4], o[0], o[2]));
        else if constexpr (I == 3) return fe_sub(nw[3], sel(o[4], o[1], o[3]));
        else return L(2);
    }
    else if constexpr (OP == 0x08) { if constexpr (I == 0) return fe_sub(nw[0], fe_add(o[0], o[1])); else return L(1); }
    else if constexpr (OP == 0x09) { if constexpr (I == 0) return fe_sub(nw[0], fe_mul(o[0], o[1])); else return L(1); }
    else if constexpr (OP == 0x0A) {
        if constexpr (I == ST_AUX0) return is_bin(o[0]);
        else if constexpr (I == ST_AUX1) return is_bin(o[1]);
        else if constexpr (I == 0) return fe_sub(nw[0], fe_mul(o[0], o[1]));
        else return L(1);
    }
    else if constexpr (OP == 0x0B) {
        if constexpr (I == ST_AUX0) return is_bin(o[0]);
        else if constexpr (I == ST_AUX1) return is_bin(o[1]);
        else if constexpr (I == 0) return fe_sub(nw[0], fe_sub(fe_add(o[0], o[1]), fe_mul(o[0], o[1])));     // 1 - (1-x)(1-y) = x + y - xy (shares xy with MUL / AND)
        else return L(1);
    }
    else if constexpr (OP == 0x0C) { if constexpr (I == 0) return fe_sub(fe_one(), fe_mul(nw[0], o[0])); else return C(); }
    else if constexpr (OP == 0x0D) { if constexpr (I == 0) return fe_add(nw[0], o[0]); else return C(); }
    else if constexpr (OP == 0x0E) {
        if constexpr (I == ST_AUX0) return is_bin(o[0]);
        else if constexpr (I == 0) return fe_sub(nw[0], bnot(o[0]));
        else return C();
    }
    else if constexpr (OP == 0x10) return R(1);
    else if constexpr (OP == 0x11) return R(2);
    else if constexpr (OP == 0x12) { if constexpr (I == 0) return fe_sub(nw[0], o[0]); else return R(1); }
    else if constexpr (OP == 0x13) { if constexpr (I < 2) return fe_sub(nw[i], o[i]); else return R(2); }
    else if constexpr (OP == 0x14) { if constexpr (I < 4) return fe_sub(nw[i], o[i]); else return R(4); }
    else if constexpr (OP == 0x15) { if constexpr (I < 2) return nw[i]; else return R(2); }
    else if constexpr (OP == 0x18) { if constexpr (I == 0) return fe_add(fe_sub(nw[0], o[1]), fe_sub(nw[1], o[0])); else return C(); }
    else if constexpr (OP == 0x19) { if constexpr (I < 4) return fe_sub(nw[i], o[i ^ 2]); else return C(); }
    else if constexpr (OP == 0x1A) return fe_sub(nw[i], o[i ^ 4]);
    else if constexpr (OP == 0x1B) { if constexpr (I < 4) return fe_sub(nw[i], o[(i + 3) & 3]); else return C(); }
    else if constexpr (OP == 0x1C) return fe_sub(nw[i], o[(i + 7) & 7]);
    else if constexpr (OP == 0x1D) {
        if constexpr (I == 0) return is_bin(nw[0]);
        else if constexpr (I == 1) return nw[1];
        else if constexpr (I == 2) return fe_sub(nw[2], fe_double(o[2]));
        else if constexpr (I == 3) return fe_sub(nw[3], fe_add(o[3], fe_mul(nw[0], o[2])));
        else return C();
    }
    else return fe_zero();
}

// ---- which operations a launch evaluates ---------------------------------------------------------------------------------------------
// The stack constraints are linear in the operation flags, so a launch may evaluate any subset of the operations for all slots and hand
// the partial values on through memory (AirArgs::ev); the launch that holds the last subset emits the constraints.  Cutting by operation
// group rather than by slot keeps what a launch has to derive first small: the low-degree groups of one `c` need lo2, mid and one top
// entry, the high-degree / flow operations the four hd flags -- and no straight-line kernel grows past the 64 KiB instruction cache of a
// CU pair (tools/codeobj_info.py, gated by build()).
//   bits 0..3: low-degree operations 4b .. 4b+3 (c = 0), bits 4..7: 16 + 4b .. (c = 1), then PUSH, CMP, RESCR, BEGIN / NOOP ("keep"),
//   and the slots >= 8 of the deep instance.
#define AG_LOW(c, b) (1u << ((c) * 4 + (b)))
#define AG_LOW0 0x00Fu
#define AG_LOW1 0x0F0u
#define AG_PUSH 0x100u
#define AG_CMP 0x200u
#define AG_RESCR 0x400u
#define AG_KEEP 0x800u
#define AG_HIGH 0xF00u
#define AG_DEEP 0x1000u
#define AG_STACK_ALL 0x1FFFu

// What term(op, slot) is, for the terms that are plain differences of stack items: kind 1: o[j] - nw[I], 2: nw[I] - o[j], 3: nw[I],
// 4: -nw[I], 5: anything else (st_term computes it), 0: the operation does not constrain the slot.  SDK = compile-time stack depth (0:
// known at run time only): items o[j], j >= SDK, are zeros then (trace_state.rs:58-60 pads the slice), which turns differences into +-nw[I]
// and removes the selector of CHOOSE2 / CSWAP2 (item 4).  DEEP: the slice may be longer than 8, left shifts past item 7 stay with st_term.
struct StDesc { int kind, j; };
template <int SDK, bool DEEP>
constexpr StDesc st_desc(int op, int I) {
    const bool o4_zero = SDK != 0 && SDK <= 4;
    if (I >= 8) {                                                      // auxiliary constraints: computed; j >= 100 names values that several operations share
        if ((op == 0x0A || op == 0x0B)) return StDesc{5, I == ST_AUX0 ? 100 : 101};         // is_bin(o[0]) / is_bin(o[1])
        if ((op == 0x06 || op == 0x07) && o4_zero) return StDesc{0, 0};                     // is_bin(o[4]) of a zero
        return StDesc{5, -1};
    }
    const int i = I;
    auto diff = [&](int j) { return (SDK != 0 && j >= SDK) ? StDesc{4, 0} : StDesc{1, j}; };
    auto rdiff = [&](int j) { return (SDK != 0 && j >= SDK) ? StDesc{3, 0} : StDesc{2, j}; };
    auto L = [&](int num) { return i + num < 8 ? diff(i + num) : (DEEP ? StDesc{5, -1} : StDesc{3, 0}); };
    auto R = [&](int num) { return diff(i - num < 0 ? 0 : i - num); };
    switch (op) {
        case 0x00: return L(1);
        case 0x01: return L(2);
        case 0x02: return i == 0 ? StDesc{5, -1} : L(2);
        case 0x03: return L(1);
        case 0x04: return L(4);
        case 0x05: return i == 0 ? StDesc{5, -1} : L(2);
        case 0x06: return i < 2 ? (o4_zero ? rdiff(i + 2) : StDesc{5, -1}) : L(4);          // selector o[4] = 0: the second operand
        case 0x07: return i < 4 ? (o4_zero ? rdiff(i) : StDesc{5, -1}) : L(2);
        case 0x08: case 0x0B: return i == 0 ? StDesc{5, -1} : L(1);
        case 0x09: case 0x0A: return i == 0 ? StDesc{5, 102} : L(1);                         // MUL and AND: nw[0] - o[0] * o[1]
        case 0x0C: case 0x0D: case 0x0E: return i == 0 ? StDesc{5, -1} : diff(i);
        case 0x10: return R(1);
        case 0x11: return R(2);
        case 0x12: return i == 0 ? rdiff(0) : R(1);
        case 0x13: return i < 2 ? rdiff(i) : R(2);
        case 0x14: return i < 4 ? rdiff(i) : R(4);
        case 0x15: return i < 2 ? StDesc{3, 0} : R(2);
        case 0x18: return i == 0 ? StDesc{5, -1} : diff(i);
        case 0x19: return i < 4 ? rdiff(i ^ 2) : diff(i);
        case 0x1A: return rdiff(i ^ 4);
        case 0x1B: return i < 4 ? rdiff((i + 3) & 3) : diff(i);
        case 0x1C: return rdiff((i + 7) & 7);
        case 0x1D: return i == 1 ? StDesc{3, 0} : (i < 4 ? StDesc{5, -1} : diff(i));
        default: return StDesc{0, 0};
    }
}
// operations of one group (4 consecutive opcodes) whose terms for slot I coincide up to sign share ONE product: entry e of the merge
// holds the basis term (kind / j of its first member) and the sign of every member's coefficient relative to it
struct StMerge { int n; int kind[4], j[4], lead[4]; int sgn[4][4]; };
template <int BASE, int I, int SDK, bool DEEP>
constexpr StMerge st_merge() {
    StMerge m{};
    for (int a = 0; a < 4; a++) {
        const StDesc d = st_desc<SDK, DEEP>(BASE + a, I);
        // has the operation a term here at all?  (st_has is the authority: st_desc only classifies)
        bool has = false;
        switch (a) { case 0: has = st_has<BASE, I>(); break; case 1: has = st_has<BASE + 1, I>(); break; case 2: has = st_has<BASE + 2, I>(); break; default: has = st_has<BASE + 3, I>(); }
        if (!has || d.kind == 0) continue;
        const int cls = d.kind == 5 ? 5 : (d.kind <= 2 ? 1 : 3);           // 1: differences with o[j], 3: +-nw[I], 5: computed
        const int sign = (d.kind == 2 || d.kind == 4) ? -1 : 1;
        int e = -1;
        for (int k = 0; k < m.n; k++) {
            const int kc = m.kind[k] == 5 ? 5 : (m.kind[k] <= 2 ? 1 : 3);
            if (kc != cls) continue;
            if (cls == 3 || (cls == 1 && m.j[k] == d.j) || (cls == 5 && d.j >= 100 && m.j[k] == d.j)) e = k;
        }
        if (e < 0) { e = m.n++; m.kind[e] = d.kind; m.j[e] = d.j; m.lead[e] = a; m.sgn[e][a] = 1; }
        else { const int lead_sign = (m.kind[e] == 2 || m.kind[e] == 4) ? -1 : 1; m.sgn[e][a] = sign * lead_sign; }
    }
    return m;
}

// The operations selected by the high-degree bits and the flow flags join the outermost sum of a slot (one more product each,
// no separate multiplication and modular addition): PUSH (input.rs:6), CMP (comparison.rs:64-105), RESCR (hash.rs:9-35; its six
// differences are computed once by the caller), BEGIN / NOOP (stack untouched).
struct StackHigh { fe push, cmp, rescr, keep; fe resc[6]; };       // the four flags and the RESCR differences

template <int I, uint32_t GROUPS, int SDK>
__device__ __forceinline__ void st_high_degree(fe_acc& outer, const StackRows& s, const StackHigh& h) {
    if constexpr (I < 8) {
        const fe* o = s.o; const fe* nw = s.nw;
        if constexpr (I >= 1 && (GROUPS & AG_PUSH) != 0) fe_acc_mac(outer, h.push, fe_sub(o[I - 1 < 0 ? 0 : I - 1], nw[I]));
        if constexpr ((GROUPS & AG_CMP) != 0) {
            const fe x_bit = nw[1], y_bit = nw[2], not_set = nw[3];
            fe v;
            if constexpr (I == 0) v = is_bin(x_bit);
            else if constexpr (I == 1) v = is_bin(y_bit);
            // x (1 - y) = x - x y and y (1 - x) = y - x y: slots 2 and 3 share x y where the depth is a constant.  With a run-time depth
            // the shared product stays live between the two slots and costs the PUSH / CMP / BEGIN / NOOP launch a resident wave (131
            // against 123 registers, profiles/air_flags.md), so those instances multiply by the complements
            else if constexpr (I == 2) v = fe_sub(nw[4], fe_add(o[4], fe_mul(SDK ? fe_sub(x_bit, fe_mul(x_bit, y_bit)) : fe_mul(x_bit, bnot(y_bit)), not_set)));
            else if constexpr (I == 3) v = fe_sub(nw[5], fe_add(o[5], fe_mul(SDK ? fe_sub(y_bit, fe_mul(x_bit, y_bit)) : fe_mul(y_bit, bnot(x_bit)), not_set)));
            else if constexpr (I == 4) v = fe_sub(nw[6], fe_add(o[6], fe_mul(y_bit, o[0])));
            else if constexpr (I == 5) v = fe_sub(nw[7], fe_add(o[7], fe_mul(x_bit, o[0])));
            else if constexpr (I == 6) v = fe_sub(not_set, fe_mul(bnot(o[5]), bnot(o[4])));
            else v = fe_sub(fe_double(nw[0]), o[0]);
            fe_acc_mac(outer, h.cmp, v);
        }
        if constexpr ((GROUPS & (AG_RESCR | AG_KEEP)) != 0) {
            const fe keep = fe_sub(o[I < 8 ? I : 0], nw[I < 8 ? I : 0]);
            if constexpr ((GROUPS & AG_RESCR) != 0) { if constexpr (I < 6) fe_acc_mac(outer, h.rescr, h.resc[I < 6 ? I : 0]); else fe_acc_mac(outer, h.rescr, keep); }
            if constexpr ((GROUPS & AG_KEEP) != 0) fe_acc_mac(outer, h.keep, keep);
        }
    }
}

// does the launch's selection contribute anything to output I?  (the auxiliary constraints only hear from low-degree operations of c = 0)
template <int I, uint32_t GROUPS> constexpr bool st_touches() {
    if (I >= 8) return (GROUPS & AG_LOW0) != 0;
    return (GROUPS & (AG_LOW0 | AG_LOW1 | AG_HIGH)) != 0;
}

// output I (slot 0..7, ST_AUX0, ST_AUX1) of the selected operations:
//     sum_c top[c] * ( sum_b mid[b] * ( sum_e coefficient_e * basis term_e ) )  +  high-degree / flow flags * their terms
// every level one sum of products with a single reduction (fe_acc); coefficient_e = +-lo2[a] summed over the merged members
// (lo0h = lo2[0] * hd[0] stands for lo2[0] in group 0: the ASSERT flag carries hd[0], trace_state.rs:346)
template <int I, uint32_t GROUPS, int SDK, bool DEEP>
__device__ __forceinline__ fe st_output(const StackRows& s, const fe* lo2, const fe& lo0h, const fe* mid, const fe* top, const StackHigh& h) {
    fe_acc outer; fe_acc_zero(outer);
    static_for_air<0, 2>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
        if constexpr (((GROUPS >> (4 * c)) & 0xFu) != 0) {
            fe_acc middle; fe_acc_zero(middle);
            static_for_air<0, 4>([&](auto b_) {
                constexpr int b = decltype(b_)::value;
                constexpr int base = 4 * b + 16 * c;
                if constexpr ((GROUPS & AG_LOW(c, b)) != 0) {
                    static constexpr StMerge M = st_merge<base, I, SDK, DEEP>();
                    if constexpr (M.n > 0) {
                        fe_acc inner; fe_acc_zero(inner);
                        static_for_air<0, M.n>([&](auto e_) {
                            constexpr int e = decltype(e_)::value;
                            // coefficient: the leader's, plus / minus the other members'
                            fe cf = (base == 0 && M.lead[e] == 0) ? lo0h : lo2[M.lead[e]];
                            static_for_air<0, 4>([&](auto a_) {
                                constexpr int a = decltype(a_)::value;
                                if constexpr (a != M.lead[e] && M.sgn[e][a] != 0) {
                                    const fe other = (base == 0 && a == 0) ? lo0h : lo2[a];
                                    cf = M.sgn[e][a] > 0 ? fe_add(cf, other) : fe_sub(cf, other);
                                }
                            });
                            constexpr int ii = I < 8 ? I : 0;
                            fe term;
                            if constexpr (M.kind[e] == 1) term = fe_sub(s.o[M.j[e]], s.nw[ii]);
                            else if constexpr (M.kind[e] == 2) term = fe_sub(s.nw[ii], s.o[M.j[e]]);
                            else if constexpr (M.kind[e] == 3) term = s.nw[ii];
                            else if constexpr (M.kind[e] == 4) term = fe_neg(s.nw[ii]);
                            else term = st_term<base + M.lead[e], I>(s);
                            fe_acc_mac(inner, cf, term);
                        });
                        fe_acc_mac(middle, mid[b], fe_acc_reduce(inner));
                    }
                }
            });
            fe_acc_mac(outer, top[c], fe_acc_reduce(middle));
        }
    });
    if constexpr ((GROUPS & AG_HIGH) != 0) st_high_degree<I, GROUPS, SDK>(outer, s, h);
    return fe_acc_reduce(outer);
}

// ---- the same outputs as ONE flat sum over the distinct basis terms of the launch -------------------------------------------------------
// st_output pays the `mid` and `top` levels again for every output, although mid[b], top[c] and the sums of lo2 entries do not depend on
// the slot, and merges terms only inside a group of four opcodes.  For slots >= 1 almost every term is one of a handful of plain
// differences that recur across groups ("shift left by one" is the term of ASSERT, DROP, ADD, MUL, AND and OR; "copy" that of INV, NEG,
// NOT and, with its sign flipped, of CSWAP2 on the low slots).  By the distributive law alone
//     output = sum_T K_T * T                    over the DISTINCT basis terms T of the output among ALL selected groups,
//     K_T    = sum of +- flag(op) = +- top[c] * mid[b] * lo2[a]   over the operations whose term is +-T
// and every K_T is an add / subtract of a few CLASS SUMS: sums of flags over sets of operations that always appear together, formed
// once per point (st_class_sums) and shared by the slots.  Nothing about the table entries is assumed (not sum_b mid[b] = 1, and not
// sum_a lo2[a] = 1, which is false: lo2[2] carries the reference's cf_op_bits[1] quirk), so the statement holds on the cosets where the
// op bits are not 0 / 1.  st_has and st_desc stay the authority; the merge rule is st_merge's (equal up to sign; computed terms only
// through the shared values j >= 100).  FLAT is the mask of outputs (bit I) that take this form; the others keep st_output.
#define ST_NB 32
struct StBasis { int n; int kind[ST_NB], j[ST_NB], lead[ST_NB]; uint32_t pos[ST_NB], neg[ST_NB]; };   // per basis: leader's kind / j / opcode, operations that contribute with + and with -
struct StBasisTable {
    StBasis b[10];                 // per output (slots 0..7, ST_AUX0, ST_AUX1); n = 0 where the output is not flat
    int nclass; uint32_t cls[32];  // the class sums: disjoint sets of operations (masks by opcode)
};

template <int I, int... OP> constexpr uint32_t st_has_mask_of(std::integer_sequence<int, OP...>) { return ((st_has<OP, I>() ? (1u << OP) : 0u) | ...); }
template <int I> constexpr uint32_t st_has_mask() { return st_has_mask_of<I>(std::make_integer_sequence<int, 32>{}); }
// the opcodes of the low-degree groups a launch selects
constexpr uint32_t st_group_ops(uint32_t groups) {
    uint32_t ops = 0;
    for (int g = 0; g < 8; g++) if ((groups >> g) & 1u) ops |= 0xFu << (4 * g);
    return ops;
}

template <int SDK, bool DEEP>
constexpr StBasis st_basis(uint32_t ops, int I) {
    StBasis m{};
    for (int op = 0; op < 32; op++) {
        if (!((ops >> op) & 1u)) continue;
        const StDesc d = st_desc<SDK, DEEP>(op, I);
        if (d.kind == 0) continue;
        const int cls = d.kind == 5 ? 5 : (d.kind <= 2 ? 1 : 3);           // as st_merge: differences with o[j], +-nw[I], computed
        const int sign = (d.kind == 2 || d.kind == 4) ? -1 : 1;
        int e = -1;
        for (int k = 0; k < m.n; k++) {
            const int kc = m.kind[k] == 5 ? 5 : (m.kind[k] <= 2 ? 1 : 3);
            if (kc != cls) continue;
            if (cls == 3 || (cls == 1 && m.j[k] == d.j) || (cls == 5 && d.j >= 100 && m.j[k] == d.j)) e = k;
        }
        if (e < 0) { e = m.n++; m.kind[e] = d.kind; m.j[e] = d.j; m.lead[e] = op; m.pos[e] = 1u << op; }
        else {
            const int lead_sign = (m.kind[e] == 2 || m.kind[e] == 4) ? -1 : 1;
            if (sign * lead_sign > 0) m.pos[e] |= 1u << op; else m.neg[e] |= 1u << op;
        }
    }
    return m;
}

template <uint32_t GROUPS, int SDK, bool DEEP, uint32_t FLAT>
constexpr StBasisTable st_basis_table() {
    StBasisTable t{};
    const uint32_t has[10] = {st_has_mask<0>(), st_has_mask<1>(), st_has_mask<2>(), st_has_mask<3>(), st_has_mask<4>(), st_has_mask<5>(), st_has_mask<6>(),
                              st_has_mask<7>(), st_has_mask<ST_AUX0>(), st_has_mask<ST_AUX1>()};
    const uint32_t ops = st_group_ops(GROUPS & (AG_LOW0 | AG_LOW1));
    int sig[32][10] = {};          // where an operation sits: +-(basis + 1) per flat output
    for (int I = 0; I < 10; I++) {
        if (!((FLAT >> I) & 1u)) continue;
        t.b[I] = st_basis<SDK, DEEP>(ops & has[I], I);
        for (int e = 0; e < t.b[I].n; e++)
            for (int op = 0; op < 32; op++) {
                if ((t.b[I].pos[e] >> op) & 1u) sig[op][I] = e + 1;
                if ((t.b[I].neg[e] >> op) & 1u) sig[op][I] = -(e + 1);
            }
    }
    // operations that sit in the same basis with the same sign in EVERY flat output form one class
    int first[32] = {};
    for (int op = 0; op < 32; op++) {
        bool used = false;
        for (int I = 0; I < 10; I++) used = used || sig[op][I] != 0;
        if (!used) continue;
        int k = -1;
        for (int c = 0; c < t.nclass && k < 0; c++) {
            bool same = true;
            for (int I = 0; I < 10; I++) same = same && sig[op][I] == sig[first[c]][I];
            if (same) k = c;
        }
        if (k < 0) { k = t.nclass++; first[k] = op; }
        t.cls[k] |= 1u << op;
    }
    return t;
}
template <uint32_t GROUPS, int SDK, bool DEEP, uint32_t FLAT> struct StBasisOf { static constexpr StBasisTable T = st_basis_table<GROUPS, SDK, DEEP, FLAT>(); };
template <uint32_t GROUPS, int SDK, bool DEEP, uint32_t FLAT> constexpr int st_class_count() { return StBasisOf<GROUPS, SDK, DEEP, FLAT>::T.nclass; }

// Which outputs of a launch take the flat form: slots >= 1 whose computed terms (each needs the full flag of its own operation, two
// multiplications) are few.  Slot 0 and the auxiliary constraints are computed terms throughout: there the nested levels of st_output,
// which never form a flag, are the cheaper statement.
template <uint32_t GROUPS, int SDK, bool DEEP>
constexpr uint32_t st_flat_default() {
    constexpr StBasisTable all = st_basis_table<GROUPS, SDK, DEEP, 0x0FEu>();
    uint32_t flat = 0;
    for (int I = 1; I < 8; I++) {
        int computed = 0, members = 0;
        for (int e = 0; e < all.b[I].n; e++) {
            if (all.b[I].kind[e] == 5) computed++;
            for (int op = 0; op < 32; op++) members += (int)(((all.b[I].pos[e] | all.b[I].neg[e]) >> op) & 1u);
        }
        if (all.b[I].n > 0 && computed <= 2 && members > all.b[I].n) flat |= 1u << I;
    }
    return flat;
}

template <int N> struct StClassSums { fe k[N > 0 ? N : 1]; };

// sum of the lo2 entries of the operations `ops` (a 4-bit mask) of group `base` (lo0h stands for lo2[0] in group 0, see st_output)
template <int BASE, uint32_t OPS>
__device__ __forceinline__ fe st_lo_sum(const fe* lo2, const fe& lo0h) {
    fe v = fe_zero(); bool any = false;
    static_for_air<0, 4>([&](auto a_) {
        constexpr int a = decltype(a_)::value;
        if constexpr (((OPS >> a) & 1u) != 0) {
            const fe x = (BASE == 0 && a == 0) ? lo0h : lo2[a];
            v = any ? fe_add(v, x) : x; any = true;
        }
    });
    return v;
}
// sum over the operations of one class of top[c] * mid[b] * lo2[a], as sum over the groups of mt[4c + b] * (sum of the group's lo2
// entries) with mt[4c + b] = mid[b] * top[c]: one multiplication for a class inside one group, else one sum of products
template <uint32_t OPS>
__device__ __forceinline__ fe st_class_sum(const fe* lo2, const fe& lo0h, const fe* mt) {
    constexpr int ng = ((OPS & 0xFu) != 0) + ((OPS & 0xF0u) != 0) + ((OPS & 0xF00u) != 0) + ((OPS & 0xF000u) != 0) + ((OPS & 0xF0000u) != 0) + ((OPS & 0xF00000u) != 0) +
                       ((OPS & 0xF000000u) != 0) + ((OPS & 0xF0000000u) != 0);
    fe_acc sum; fe_acc_zero(sum);
    fe only = fe_zero();
    static_for_air<0, 8>([&](auto g_) {
        constexpr int g = decltype(g_)::value;
        constexpr uint32_t grp = (OPS >> (4 * g)) & 0xFu;
        if constexpr (grp != 0) {
            const fe lo = st_lo_sum<4 * g, grp>(lo2, lo0h);
            if constexpr (ng == 1) only = fe_mul(mt[g], lo); else fe_acc_mac(sum, mt[g], lo);
        }
    });
    if constexpr (ng == 1) return only; else return fe_acc_reduce(sum);
}
template <uint32_t GROUPS, int SDK, bool DEEP, uint32_t FLAT>
__device__ __forceinline__ void st_class_sums(StClassSums<st_class_count<GROUPS, SDK, DEEP, FLAT>()>& cs, const fe* lo2, const fe& lo0h, const fe* mid, const fe* top) {
    using B = StBasisOf<GROUPS, SDK, DEEP, FLAT>;
    fe mt[8];                       // only the groups some class has operations in
    static_for_air<0, 8>([&](auto g_) {
        constexpr int g = decltype(g_)::value;
        constexpr bool used = [] { for (int k = 0; k < B::T.nclass; k++) if ((B::T.cls[k] >> (4 * g)) & 0xFu) return true; return false; }();
        if constexpr (used) mt[g] = fe_mul(mid[g & 3], top[g >> 2]);
    });
    static_for_air<0, B::T.nclass>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        cs.k[k] = st_class_sum<B::T.cls[k]>(lo2, lo0h, mt);
    });
}

// output I of the selected operations: flat where FLAT says so -- per basis term one coefficient (adds / subtracts of class sums) and
// one product, ONE reduction, the high-degree / flow products in the same accumulator -- and st_output elsewhere
template <int I, uint32_t GROUPS, int SDK, bool DEEP, uint32_t FLAT>
__device__ __forceinline__ fe st_output_basis(const StackRows& s, const StClassSums<st_class_count<GROUPS, SDK, DEEP, FLAT>()>& cs, const fe* lo2, const fe& lo0h, const fe* mid,
                                              const fe* top, const StackHigh& h) {
    if constexpr (((FLAT >> I) & 1u) == 0) return st_output<I, GROUPS, SDK, DEEP>(s, lo2, lo0h, mid, top, h);
    else {
        using B = StBasisOf<GROUPS, SDK, DEEP, FLAT>;
        fe_acc outer; fe_acc_zero(outer);
        static_for_air<0, B::T.b[I].n>([&](auto e_) {
            constexpr int e = decltype(e_)::value;
            constexpr uint32_t pos = B::T.b[I].pos[e], neg = B::T.b[I].neg[e];
            // the leader's class comes first (it is in pos), so the coefficient starts from a plain copy
            fe cf = fe_zero(); bool any = false;
            static_for_air<0, B::T.nclass>([&](auto k_) {
                constexpr int k = decltype(k_)::value;
                if constexpr ((B::T.cls[k] & pos) != 0) { cf = any ? fe_add(cf, cs.k[k]) : cs.k[k]; any = true; }
            });
            static_for_air<0, B::T.nclass>([&](auto k_) {
                constexpr int k = decltype(k_)::value;
                if constexpr ((B::T.cls[k] & neg) != 0) cf = fe_sub(cf, cs.k[k]);
            });
            constexpr int ii = I < 8 ? I : 0;
            constexpr int kind = B::T.b[I].kind[e], j = B::T.b[I].j[e] < 0 ? 0 : (B::T.b[I].j[e] < 12 ? B::T.b[I].j[e] : 0);
            fe term;
            if constexpr (kind == 1) term = fe_sub(s.o[j], s.nw[ii]);
            else if constexpr (kind == 2) term = fe_sub(s.nw[ii], s.o[j]);
            else if constexpr (kind == 3) term = s.nw[ii];
            else if constexpr (kind == 4) term = fe_neg(s.nw[ii]);
            else term = st_term<B::T.b[I].lead[e], I>(s);
            fe_acc_mac(outer, cf, term);
        });
        if constexpr ((GROUPS & AG_HIGH) != 0) st_high_degree<I, GROUPS, SDK>(outer, s, h);
        return fe_acc_reduce(outer);
    }
}
