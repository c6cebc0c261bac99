// Host form of the AIR at one out-of-domain point: what the verifier needs of the constraint system (dst_verify, include/distaff_hip.h).
//
// The device form (air_kernel.h) evaluates the constraints on domain points with the periodic columns as device tables.  At the DEEP point z
// nothing is a table: the round constants and the cycle masks are the degree-15 polynomials through their 16 values, evaluated at
// z^(n/16) (/root/reference/src/stark/constraints/utils.rs:87-113, decoder/mod.rs:155-170,219-223, stack/mod.rs:98-110), and the state is
// the pair of DeepValues rows.  Written plainly over host_vm.h's u128 field, for any shape the wire format can carry: context depth 0..16,
// loop depth 0..8, user stack 1..32, all 32 user and 8 flow operations.
//
// Follows (all under /root/reference/src/stark/):
//   trace/trace_state.rs        from_vec :73, op_code :165, set_op_flags :281-350
//   constraints/utils.rs        is_binary :15, binary_not :20, are_equal :25, enforce_stack_copy :35, enforce_right_shift :44,
//                               enforce_left_shift :53, agg_constraint :73
//   constraints/decoder/        mod.rs :31-47 (degrees), :155 (evaluate_at); op_bits.rs :10-79; sponge.rs :10-43; flow_ops.rs :10-165
//   constraints/stack/          mod.rs :58, :98, :117-195; input, arithmetic, manipulation, comparison, conditional, hash .rs
//   constraints/evaluator.rs    from_proof :81, evaluate_transition_at :167, evaluate_boundaries :181-326, combine_transition_constraints :335,
//                               group_transition_constraints :385
//   utils/coefficients.rs       ConstraintCoefficients :62-77,108-185
// The reference's quirks Q1-Q6 are part of the statement a proof was made for and are kept: ld_op_flags[2] is built
// from cf_op_bits[1]; SWAP aggregates both of its constraints into slot 0; the PUSH / ASSERT flag adjustments take bit 0 of the other bank
// and happen after the BEGIN / NOOP flags were formed; the transition coefficients are consumed in degree-group order.
#pragma once
#include <stddef.h>
#include "../host_vm.h"

namespace dsth {
namespace hair {

static const size_t MAX_CTX = 16, MAX_LOOP = 8, MAX_STACK = 32, MAX_PUBLIC = 8;                  // lib.rs:80,81,138,136
static const size_t NUM_STATIC_DECODER = 15 + 4 + 1, NUM_AUX_STACK = 2;                           // decoder/mod.rs:53, stack/mod.rs:39
static const size_t NUM_BOUNDARY = 1 + 4 + 10 + MAX_CTX + MAX_LOOP + MAX_PUBLIC;                   // 47
static const size_t NUM_TRANSITION = NUM_STATIC_DECODER + MAX_CTX + MAX_LOOP + MAX_STACK + NUM_AUX_STACK;   // 78
static const size_t NUM_DRAWS = 2 * (NUM_TRANSITION + 2 * NUM_BOUNDARY);                           // 344
static const size_t MAX_CONSTRAINT_DEGREE = 8;                                                    // stark/mod.rs:25

enum : uint8_t { F_HACC = 0, F_BEGIN = 1, F_TEND = 2, F_FEND = 3, F_LOOP = 4, F_WRAP = 5, F_BREAK = 6, F_VOID = 7 };
enum : uint8_t {                                                                                    // processor/opcodes.rs
    OP_ASSERT = 0x60, OP_ASSERTEQ = 0x61, OP_EQ = 0x62, OP_DROP = 0x63, OP_DROP4 = 0x64, OP_CHOOSE = 0x65, OP_CHOOSE2 = 0x66, OP_CSWAP2 = 0x67,
    OP_ADD = 0x68, OP_MUL = 0x69, OP_AND = 0x6A, OP_OR = 0x6B, OP_INV = 0x6C, OP_NEG = 0x6D, OP_NOT = 0x6E,
    OP_READ = 0x70, OP_READ2 = 0x71, OP_DUP = 0x72, OP_DUP2 = 0x73, OP_DUP4 = 0x74, OP_PAD2 = 0x75,
    OP_SWAP = 0x78, OP_SWAP2 = 0x79, OP_SWAP4 = 0x7A, OP_ROLL4 = 0x7B, OP_ROLL8 = 0x7C, OP_BINACC = 0x7D,
    OP_PUSH = 0x1F, OP_CMP = 0x3F, OP_RESCR = 0x5F, OP_BEGIN = 0x00, OP_NOOP = 0x7F,
};
inline size_t ld_index(uint8_t op) { return op & 0x1F; }                                           // opcodes.rs:90
inline size_t hd_index(uint8_t op) { return (op >> 5) & 3; }                                       // opcodes.rs:101

inline u128 hf_inv(u128 x) { return x == 0 ? 0 : hf_pow(x, FIELD_P - 2); }                          // field.rs:83: inv(0) = 0
inline u128 hf_div(u128 a, u128 b) { return hf_mul(a, hf_inv(b)); }
inline u128 hf_root_of_unity(uint32_t log_order) {                                                  // field.rs:228, log_order <= 40
    const u128 g = (((u128)0x120532E7B364080Aull) << 64) | 0x86B8723E1920F4AAull;
    return hf_pow(g, (u128)1 << (40 - log_order));
}
inline u128 is_binary(u128 v) { return hf_sub(hf_mul(v, v), v); }
inline u128 binary_not(u128 v) { return hf_sub(1, v); }
inline u128 are_equal(u128 a, u128 b) { return hf_sub(a, b); }
inline void agg(u128* r, size_t i, u128 flag, u128 value) { r[i] = hf_add(r[i], hf_mul(flag, value)); }
inline void stack_copy(u128* r, size_t len, const u128* o, const u128* n, size_t from, u128 f) {
    for (size_t i = from; i < len; i++) agg(r, i, f, are_equal(o[i], n[i]));
}
inline void right_shift(u128* r, size_t len, const u128* o, const u128* n, size_t num, u128 f) {
    for (size_t i = num; i < len; i++) agg(r, i, f, are_equal(o[i - num], n[i]));
}
inline void left_shift(u128* r, size_t len, const u128* o, const u128* n, size_t from, size_t num, u128 f) {
    size_t start = from - num, rem = len - num;
    for (size_t i = start; i < rem; i++) agg(r, i, f, are_equal(o[i + num], n[i]));
    for (size_t i = rem; i < len; i++) agg(r, i, f, n[i]);
}
inline u128 poly_eval(const u128* p, size_t n, u128 x) {                                            // polynom.rs:9
    u128 y = 0, pw = 1;
    for (size_t i = 0; i < n; i++) { y = hf_add(y, hf_mul(p[i], pw)); pw = hf_mul(pw, x); }
    return y;
}

// ---- one trace row (trace_state.rs:21-41): stacks padded with zeros to their minimum depths (lib.rs:87-89) ---------------------------
struct Row {
    u128 op_counter, sponge[4], cf[3], ld[5], hd[2];
    u128 ctx[MAX_CTX], loop[MAX_LOOP], user[MAX_STACK];
    size_t ctx_n, loop_n, user_n;                                // padded lengths: max(depth, 1), max(depth, 1), max(depth, 8)
    u128 cf_flags[8], ld_flags[32], hd_flags[4], begin_flag, noop_flag;

    Row(size_t ctx_depth, size_t loop_depth, size_t stack_depth, const u128* s) {                 // from_vec :73
        memset((void*)this, 0, sizeof(*this));
        ctx_n = ctx_depth < 1 ? 1 : ctx_depth; loop_n = loop_depth < 1 ? 1 : loop_depth; user_n = stack_depth < 8 ? 8 : stack_depth;
        op_counter = s[0];
        for (int i = 0; i < 4; i++) sponge[i] = s[1 + i];
        for (int i = 0; i < 3; i++) cf[i] = s[5 + i];
        for (int i = 0; i < 5; i++) ld[i] = s[8 + i];
        for (int i = 0; i < 2; i++) hd[i] = s[13 + i];
        size_t c = 15;
        for (size_t i = 0; i < ctx_depth; i++) ctx[i] = s[c + i];
        c += ctx_depth;
        for (size_t i = 0; i < loop_depth; i++) loop[i] = s[c + i];
        c += loop_depth;
        for (size_t i = 0; i < stack_depth; i++) user[i] = s[c + i];
        set_op_flags();
    }
    u128 op_code() const {                                                                          // :165
        u128 r = ld[0];
        for (int i = 1; i < 5; i++) r = hf_add(r, hf_mul(ld[i], (u128)1 << i));
        r = hf_add(r, hf_mul(hd[0], 32));
        return hf_add(r, hf_mul(hd[1], 64));
    }
    void set_op_flags() {                                                                           // :281-350
        u128 not0 = binary_not(cf[0]), not1 = binary_not(cf[1]);
        cf_flags[0] = hf_mul(not0, not1); cf_flags[1] = hf_mul(cf[0], not1);
        cf_flags[2] = hf_mul(not0, cf[1]); cf_flags[3] = hf_mul(cf[0], cf[1]);
        for (int i = 0; i < 4; i++) cf_flags[4 + i] = cf_flags[i];
        u128 not2 = binary_not(cf[2]);
        for (int i = 0; i < 4; i++) cf_flags[i] = hf_mul(cf_flags[i], not2);
        for (int i = 4; i < 8; i++) cf_flags[i] = hf_mul(cf_flags[i], cf[2]);

        not0 = binary_not(ld[0]); not1 = binary_not(ld[1]);
        ld_flags[0] = hf_mul(not0, not1); ld_flags[1] = hf_mul(ld[0], not1);
        ld_flags[2] = hf_mul(not0, cf[1]);                       // Q1: the reference multiplies by cf_op_bits[1] here (:301)
        ld_flags[3] = hf_mul(ld[0], ld[1]);
        for (int width = 4, bit = 2; bit < 5; width *= 2, bit++) {
            for (int i = 0; i < width; i++) ld_flags[width + i] = ld_flags[i];
            u128 nb = binary_not(ld[bit]);
            for (int i = 0; i < width; i++) ld_flags[i] = hf_mul(ld_flags[i], nb);
            for (int i = width; i < 2 * width; i++) ld_flags[i] = hf_mul(ld_flags[i], ld[bit]);
        }
        not0 = binary_not(hd[0]); not1 = binary_not(hd[1]);
        hd_flags[0] = hf_mul(not0, not1); hd_flags[1] = hf_mul(hd[0], not1);
        hd_flags[2] = hf_mul(not0, hd[1]); hd_flags[3] = hf_mul(hd[0], hd[1]);

        begin_flag = hf_mul(ld_flags[ld_index(OP_BEGIN)], hd_flags[hd_index(OP_BEGIN)]);
        noop_flag = hf_mul(ld_flags[ld_index(OP_NOOP)], hd_flags[hd_index(OP_NOOP)]);
        hd_flags[0] = hf_mul(hd_flags[0], ld[0]);                // PUSH adjustment (:343), after the composite flags
        ld_flags[0] = hf_mul(ld_flags[0], hd[0]);                // ASSERT adjustment (:346)
    }
};

// ---- periodic columns as polynomials (constraints/utils.rs:87: interpolation over the 16-point cycle) ----------------------------------
static const uint8_t CYCLE_MASKS[3][16] = {                      // decoder/mod.rs:219
    {0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},
    {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0},
    {0, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1},
};
// value at x of the polynomial of degree < 16 that takes v[i] at g16^i: c_k = 1/16 sum_i v_i g16^(-ik), then Horner's sum
struct Cycle16 {
    u128 inv_pow[16], inv16;
    Cycle16() {
        u128 g = hf_root_of_unity(4), gi = hf_inv(g);
        inv_pow[0] = 1;
        for (int i = 1; i < 16; i++) inv_pow[i] = hf_mul(inv_pow[i - 1], gi);
        inv16 = hf_inv(16);
    }
    u128 eval(const u128 v[16], u128 x) const {
        u128 c[16];
        for (int k = 0; k < 16; k++) {
            u128 acc = 0;
            for (int i = 0; i < 16; i++) acc = hf_add(acc, hf_mul(v[i], inv_pow[(i * k) & 15]));
            c[k] = hf_mul(acc, inv16);
        }
        return poly_eval(c, 16, x);
    }
};
struct Periodic { u128 sponge_ark[8], hasher_ark[12], masks[3]; };
inline Periodic periodic_at(u128 x, uint64_t trace_length) {                                        // decoder/mod.rs:155, stack/mod.rs:98
    Cycle16 cy;
    u128 xc = hf_pow(x, (u128)(trace_length / 16));
    Periodic p;
    u128 v[16];
    for (int r = 0; r < 8; r++) { for (int i = 0; i < 16; i++) v[i] = limbs(SPONGE_ARK[r][i]); p.sponge_ark[r] = cy.eval(v, xc); }
    for (int r = 0; r < 12; r++) { for (int i = 0; i < 16; i++) v[i] = limbs(HASHER_ARK[r][i]); p.hasher_ark[r] = cy.eval(v, xc); }
    for (int r = 0; r < 3; r++) { for (int i = 0; i < 16; i++) v[i] = CYCLE_MASKS[r][i]; p.masks[r] = cy.eval(v, xc); }
    return p;
}
template <int W>
inline void matmul(u128* s, const uint32_t (*m)[4]) {
    u128 r[W];
    for (int i = 0; i < W; i++) { u128 acc = 0; for (int j = 0; j < W; j++) acc = hf_add(acc, hf_mul(limbs(m[i * W + j]), s[j])); r[i] = acc; }
    for (int i = 0; i < W; i++) s[i] = r[i];
}
template <int W> inline void sbox(u128* s) { for (int i = 0; i < W; i++) s[i] = hf_mul(hf_sqr(s[i]), s[i]); }

// ---- decoder (op_bits.rs:10, sponge.rs:10, flow_ops.rs:10-165); result has 20 + ctx_n + loop_n slots -----------------------------------
inline void decoder_at(const Row& cur, const Row& nxt, const Periodic& pc, u128* result) {
    size_t i = 0;
    u128 cf_bit_sum = 0, ld_bit_prod = 1, hd_bit_prod = 1;
    for (int k = 0; k < 3; k++) { result[i++] = is_binary(cur.cf[k]); cf_bit_sum = hf_add(cf_bit_sum, cur.cf[k]); }
    for (int k = 0; k < 5; k++) { result[i++] = is_binary(cur.ld[k]); ld_bit_prod = hf_mul(ld_bit_prod, cur.ld[k]); }
    for (int k = 0; k < 2; k++) { result[i++] = is_binary(cur.hd[k]); hd_bit_prod = hf_mul(hd_bit_prod, cur.hd[k]); }
    u128 is_hacc = cur.cf_flags[F_HACC];
    u128 hacc_transition = hf_mul(hf_add(cur.op_counter, 1), is_hacc);
    u128 rest_transition = hf_mul(cur.op_counter, binary_not(is_hacc));
    result[i++] = are_equal(hf_add(hacc_transition, rest_transition), nxt.op_counter);
    result[i++] = hf_mul(cur.op_counter, hf_mul(binary_not(ld_bit_prod), binary_not(hd_bit_prod)));
    result[i++] = hf_mul(cf_bit_sum, binary_not(hf_mul(ld_bit_prod, hd_bit_prod)));
    result[i++] = hf_mul(cur.cf_flags[F_VOID], binary_not(nxt.cf_flags[F_VOID]));
    result[i] = 0;                                               // alignment of flow operations and of PUSH within the 16-step cycle
    agg(result, i, cur.cf_flags[F_BEGIN], pc.masks[1]); agg(result, i, cur.cf_flags[F_LOOP], pc.masks[1]);
    agg(result, i, cur.cf_flags[F_WRAP], pc.masks[1]);  agg(result, i, cur.cf_flags[F_BREAK], pc.masks[1]);
    agg(result, i, cur.cf_flags[F_TEND], pc.masks[0]);  agg(result, i, cur.cf_flags[F_FEND], pc.masks[0]);
    agg(result, i, cur.hd_flags[hd_index(OP_PUSH)], pc.masks[2]);

    u128* r = result + 15;                                       // sponge x4, loop image, context stack, loop stack
    const size_t cl = cur.ctx_n, ll = cur.loop_n;
    u128* rc = r + 5;
    u128* rl = r + 5 + cl;
    for (size_t k = 0; k < 5 + cl + ll; k++) r[k] = 0;
    u128 f;
    {                                                            // HACC (sponge.rs:10): one Rescue round met in the middle
        f = cur.cf_flags[F_HACC];
        u128 op_value = hf_mul(nxt.user[0], cur.hd_flags[hd_index(OP_PUSH)]);
        u128 os[4], ns[4];
        for (int k = 0; k < 4; k++) os[k] = hf_add(cur.sponge[k], pc.sponge_ark[k]);
        sbox<4>(os); matmul<4>(os, SPONGE_MDS);
        os[0] = hf_add(os[0], cur.op_code());
        os[1] = hf_add(os[1], op_value);
        for (int k = 0; k < 4; k++) ns[k] = nxt.sponge[k];
        matmul<4>(ns, SPONGE_INV_MDS); sbox<4>(ns);
        for (int k = 0; k < 4; k++) ns[k] = hf_sub(ns[k], pc.sponge_ark[4 + k]);
        for (int k = 0; k < 4; k++) agg(r, k, f, are_equal(os[k], ns[k]));
    }
    f = cur.cf_flags[F_BEGIN];
    for (int k = 0; k < 4; k++) agg(r, k, f, nxt.sponge[k]);
    agg(rc, 0, f, are_equal(cur.sponge[0], nxt.ctx[0]));
    right_shift(rc, cl, cur.ctx, nxt.ctx, 1, f);
    stack_copy(rl, ll, cur.loop, nxt.loop, 0, f);
    f = cur.cf_flags[F_TEND];
    agg(r, 0, f, are_equal(cur.ctx[0], nxt.sponge[0]));
    agg(r, 1, f, are_equal(cur.sponge[0], nxt.sponge[1]));
    agg(r, 3, f, nxt.sponge[3]);
    left_shift(rc, cl, cur.ctx, nxt.ctx, 1, 1, f);
    stack_copy(rl, ll, cur.loop, nxt.loop, 0, f);
    f = cur.cf_flags[F_FEND];
    agg(r, 0, f, are_equal(cur.ctx[0], nxt.sponge[0]));
    agg(r, 2, f, are_equal(cur.sponge[0], nxt.sponge[2]));
    agg(r, 3, f, nxt.sponge[3]);
    left_shift(rc, cl, cur.ctx, nxt.ctx, 1, 1, f);
    stack_copy(rl, ll, cur.loop, nxt.loop, 0, f);
    f = cur.cf_flags[F_LOOP];
    for (int k = 0; k < 4; k++) agg(r, k, f, nxt.sponge[k]);
    agg(rc, 0, f, are_equal(cur.sponge[0], nxt.ctx[0]));
    right_shift(rc, cl, cur.ctx, nxt.ctx, 1, f);
    right_shift(rl, ll, cur.loop, nxt.loop, 1, f);
    f = cur.cf_flags[F_WRAP];
    for (int k = 0; k < 4; k++) agg(r, k, f, nxt.sponge[k]);
    agg(r, 4, f, are_equal(cur.sponge[0], cur.loop[0]));
    stack_copy(rc, cl, cur.ctx, nxt.ctx, 0, f);
    stack_copy(rl, ll, cur.loop, nxt.loop, 0, f);
    f = cur.cf_flags[F_BREAK];
    for (int k = 0; k < 4; k++) agg(r, k, f, are_equal(cur.sponge[k], nxt.sponge[k]));
    agg(r, 4, f, are_equal(cur.sponge[0], cur.loop[0]));
    stack_copy(rc, cl, cur.ctx, nxt.ctx, 0, f);
    left_shift(rl, ll, cur.loop, nxt.loop, 1, 1, f);
    f = cur.cf_flags[F_VOID];
    for (int k = 0; k < 4; k++) agg(r, k, f, are_equal(cur.sponge[k], nxt.sponge[k]));
    stack_copy(rc, cl, cur.ctx, nxt.ctx, 0, f);
    stack_copy(rl, ll, cur.loop, nxt.loop, 0, f);
}

// ---- user stack (stack/mod.rs:117-195); aux has 2 slots, e has user_n slots --------------------------------------------------------------
inline void stack_at(const Row& cur, const Row& nxt, const Periodic& pc, u128* aux, u128* e) {
    const u128* o = cur.user;
    const u128* n = nxt.user;
    const size_t L = cur.user_n;
    const u128* ld = cur.ld_flags;
    const u128* hd = cur.hd_flags;
    aux[0] = aux[1] = 0;
    for (size_t i = 0; i < L; i++) e[i] = 0;
    u128 f;
    // assertions (comparison.rs:24-38)
    f = ld[ld_index(OP_ASSERT)];   left_shift(e, L, o, n, 1, 1, f); agg(aux, 0, f, are_equal(1, o[0]));
    f = ld[ld_index(OP_ASSERTEQ)]; left_shift(e, L, o, n, 2, 2, f); agg(aux, 0, f, are_equal(o[0], o[1]));
    // input (input.rs:6-22)
    right_shift(e, L, o, n, 1, ld[ld_index(OP_READ)]);
    right_shift(e, L, o, n, 2, ld[ld_index(OP_READ2)]);
    // manipulation (manipulation.rs:12-117)
    f = ld[ld_index(OP_DUP)];  agg(e, 0, f, are_equal(n[0], o[0])); right_shift(e, L, o, n, 1, f);
    f = ld[ld_index(OP_DUP2)]; agg(e, 0, f, are_equal(n[0], o[0])); agg(e, 1, f, are_equal(n[1], o[1])); right_shift(e, L, o, n, 2, f);
    f = ld[ld_index(OP_DUP4)]; for (int i = 0; i < 4; i++) agg(e, i, f, are_equal(n[i], o[i])); right_shift(e, L, o, n, 4, f);
    f = ld[ld_index(OP_PAD2)]; agg(e, 0, f, n[0]); agg(e, 1, f, n[1]); right_shift(e, L, o, n, 2, f);
    left_shift(e, L, o, n, 1, 1, ld[ld_index(OP_DROP)]);
    left_shift(e, L, o, n, 4, 4, ld[ld_index(OP_DROP4)]);
    f = ld[ld_index(OP_SWAP)];                                   // Q2: both constraints go to slot 0 (manipulation.rs:63-64)
    agg(e, 0, f, are_equal(n[0], o[1])); agg(e, 0, f, are_equal(n[1], o[0])); stack_copy(e, L, o, n, 2, f);
    f = ld[ld_index(OP_SWAP2)];
    agg(e, 0, f, are_equal(n[0], o[2])); agg(e, 1, f, are_equal(n[1], o[3])); agg(e, 2, f, are_equal(n[2], o[0])); agg(e, 3, f, are_equal(n[3], o[1]));
    stack_copy(e, L, o, n, 4, f);
    f = ld[ld_index(OP_SWAP4)];
    for (int i = 0; i < 4; i++) agg(e, i, f, are_equal(n[i], o[4 + i]));
    for (int i = 0; i < 4; i++) agg(e, 4 + i, f, are_equal(n[4 + i], o[i]));
    stack_copy(e, L, o, n, 8, f);
    f = ld[ld_index(OP_ROLL4)];
    agg(e, 0, f, are_equal(n[0], o[3])); for (int i = 1; i < 4; i++) agg(e, i, f, are_equal(n[i], o[i - 1]));
    stack_copy(e, L, o, n, 4, f);
    f = ld[ld_index(OP_ROLL8)];
    agg(e, 0, f, are_equal(n[0], o[7])); for (int i = 1; i < 8; i++) agg(e, i, f, are_equal(n[i], o[i - 1]));
    stack_copy(e, L, o, n, 8, f);
    // arithmetic and boolean (arithmetic.rs:12-118)
    f = ld[ld_index(OP_ADD)]; agg(e, 0, f, are_equal(n[0], hf_add(o[0], o[1]))); left_shift(e, L, o, n, 2, 1, f);
    f = ld[ld_index(OP_MUL)]; agg(e, 0, f, are_equal(n[0], hf_mul(o[0], o[1]))); left_shift(e, L, o, n, 2, 1, f);
    f = ld[ld_index(OP_INV)]; agg(e, 0, f, are_equal(1, hf_mul(n[0], o[0]))); stack_copy(e, L, o, n, 1, f);
    f = ld[ld_index(OP_NEG)]; agg(e, 0, f, hf_add(n[0], o[0])); stack_copy(e, L, o, n, 1, f);
    f = ld[ld_index(OP_NOT)]; agg(e, 0, f, are_equal(n[0], binary_not(o[0]))); stack_copy(e, L, o, n, 1, f); agg(aux, 0, f, is_binary(o[0]));
    f = ld[ld_index(OP_AND)]; agg(e, 0, f, are_equal(n[0], hf_mul(o[0], o[1]))); left_shift(e, L, o, n, 2, 1, f);
    agg(aux, 0, f, is_binary(o[0])); agg(aux, 1, f, is_binary(o[1]));
    f = ld[ld_index(OP_OR)]; agg(e, 0, f, are_equal(n[0], binary_not(hf_mul(binary_not(o[0]), binary_not(o[1]))))); left_shift(e, L, o, n, 2, 1, f);
    agg(aux, 0, f, is_binary(o[0])); agg(aux, 1, f, is_binary(o[1]));
    {                                                            // comparison.rs:45
        f = ld[ld_index(OP_EQ)];
        u128 diff = hf_sub(o[1], o[2]);
        agg(e, 0, f, are_equal(n[0], binary_not(hf_mul(diff, o[0]))));
        left_shift(e, L, o, n, 3, 2, f);
        agg(aux, 0, f, hf_mul(n[0], diff));
    }
    {                                                            // comparison.rs:110
        f = ld[ld_index(OP_BINACC)];
        u128 bit = n[0], pw = o[2];
        agg(e, 0, f, is_binary(bit)); agg(e, 1, f, n[1]);
        agg(e, 2, f, are_equal(n[2], hf_mul(pw, 2)));
        agg(e, 3, f, are_equal(n[3], hf_add(o[3], hf_mul(bit, pw))));
        stack_copy(e, L, o, n, 4, f);
    }
    {                                                            // conditional.rs:12-82
        f = ld[ld_index(OP_CHOOSE)];
        u128 c = o[2], nc = binary_not(c);
        agg(e, 0, f, are_equal(n[0], hf_add(hf_mul(c, o[0]), hf_mul(nc, o[1]))));
        left_shift(e, L, o, n, 3, 2, f);
        agg(aux, 0, f, is_binary(c));
    }
    {
        f = ld[ld_index(OP_CHOOSE2)];
        u128 c = o[4], nc = binary_not(c);
        agg(e, 0, f, are_equal(n[0], hf_add(hf_mul(c, o[0]), hf_mul(nc, o[2]))));
        agg(e, 1, f, are_equal(n[1], hf_add(hf_mul(c, o[1]), hf_mul(nc, o[3]))));
        left_shift(e, L, o, n, 6, 4, f);
        agg(aux, 0, f, is_binary(c));
    }
    {
        f = ld[ld_index(OP_CSWAP2)];
        u128 c = o[4], nc = binary_not(c);
        agg(e, 0, f, are_equal(n[0], hf_add(hf_mul(c, o[2]), hf_mul(nc, o[0]))));
        agg(e, 1, f, are_equal(n[1], hf_add(hf_mul(c, o[3]), hf_mul(nc, o[1]))));
        agg(e, 2, f, are_equal(n[2], hf_add(hf_mul(c, o[0]), hf_mul(nc, o[2]))));
        agg(e, 3, f, are_equal(n[3], hf_add(hf_mul(c, o[1]), hf_mul(nc, o[3]))));
        left_shift(e, L, o, n, 6, 2, f);
        agg(aux, 0, f, is_binary(c));
    }
    // high-degree operations
    right_shift(e, L, o, n, 1, hd[hd_index(OP_PUSH)]);                                             // input.rs:6
    {                                                            // comparison.rs:64
        f = hd[hd_index(OP_CMP)];
        u128 x_bit = n[1], y_bit = n[2], not_set = n[3];
        agg(e, 0, f, is_binary(x_bit)); agg(e, 1, f, is_binary(y_bit));
        u128 bit_gt = hf_mul(x_bit, binary_not(y_bit)), bit_lt = hf_mul(y_bit, binary_not(x_bit));
        agg(e, 2, f, are_equal(n[4], hf_add(o[4], hf_mul(bit_gt, not_set))));
        agg(e, 3, f, are_equal(n[5], hf_add(o[5], hf_mul(bit_lt, not_set))));
        u128 pw = o[0];
        u128 x_acc = hf_add(o[7], hf_mul(x_bit, pw)), y_acc = hf_add(o[6], hf_mul(y_bit, pw));
        agg(e, 4, f, are_equal(n[6], y_acc)); agg(e, 5, f, are_equal(n[7], x_acc));
        agg(e, 6, f, are_equal(not_set, hf_mul(binary_not(o[5]), binary_not(o[4]))));
        agg(e, 7, f, are_equal(hf_mul(n[0], 2), pw));
        stack_copy(e, L, o, n, 8, f);
    }
    {                                                            // hash.rs:9: one Rescue round of the 6-wide hasher met in the middle
        f = hd[hd_index(OP_RESCR)];
        u128 os[6], ns[6];
        for (int i = 0; i < 6; i++) os[i] = hf_add(o[i], pc.hasher_ark[i]);
        sbox<6>(os); matmul<6>(os, HASHER_MDS);
        for (int i = 0; i < 6; i++) ns[i] = n[i];
        matmul<6>(ns, HASHER_INV_MDS); sbox<6>(ns);
        for (int i = 0; i < 6; i++) ns[i] = hf_sub(ns[i], pc.hasher_ark[6 + i]);
        for (int i = 0; i < 6; i++) agg(e, i, f, are_equal(ns[i], os[i]));
        stack_copy(e, L, o, n, 6, f);
    }
    // composite operations
    stack_copy(e, L, o, n, 0, cur.begin_flag);
    stack_copy(e, L, o, n, 0, cur.noop_flag);
}

// ---- evaluator (evaluator.rs:81 from_proof) ---------------------------------------------------------------------------------------------
struct Shape { size_t ctx_depth, loop_depth, stack_depth; uint64_t trace_length; };
struct Public { u128 program_hash[2]; u128 op_count; const u128* inputs; size_t num_inputs; const u128* outputs; size_t num_outputs; };

// combine_transition_constraints (:335) of the evaluations at x, with the draws of utils/coefficients.rs:140 and the degree groups of :385
inline u128 transition_at(const Shape& sh, const u128 draws[NUM_DRAWS], const Row& cur, const Row& nxt, u128 x) {
    const size_t cl = cur.ctx_n, ll = cur.loop_n;
    const size_t ndec = NUM_STATIC_DECODER + cl + ll, count = ndec + NUM_AUX_STACK + sh.stack_depth;
    u128 ev[NUM_STATIC_DECODER + MAX_CTX + MAX_LOOP + NUM_AUX_STACK + MAX_STACK];
    uint8_t degree[NUM_STATIC_DECODER + MAX_CTX + MAX_LOOP + NUM_AUX_STACK + MAX_STACK];
    static const uint8_t dec_deg[NUM_STATIC_DECODER] = {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 8, 8, 6, 4, 6, 7, 6, 6, 4};   // decoder/mod.rs:31-47
    for (size_t i = 0; i < NUM_STATIC_DECODER; i++) degree[i] = dec_deg[i];
    for (size_t i = NUM_STATIC_DECODER; i < ndec; i++) degree[i] = 4;
    for (size_t i = ndec; i < count; i++) degree[i] = 7;                                            // stack/mod.rs:58
    Periodic pc = periodic_at(x, sh.trace_length);
    decoder_at(cur, nxt, pc, ev);
    u128 se[MAX_STACK];
    stack_at(cur, nxt, pc, ev + ndec, se);
    for (size_t i = 0; i < sh.stack_depth; i++) ev[ndec + NUM_AUX_STACK + i] = se[i];               // only stack_depth of the max(stack_depth, 8) slots count
    // the coefficient pairs of this shape, out of the maximal layout (coefficients.rs:140-185)
    u128 cc[2 * (NUM_STATIC_DECODER + MAX_CTX + MAX_LOOP + NUM_AUX_STACK + MAX_STACK)];
    const u128* c = draws + 4 * NUM_BOUNDARY;
    size_t k = 0, s = 0;
    for (size_t i = 0; i < 2 * NUM_STATIC_DECODER; i++) cc[k++] = c[s + i];
    s += 2 * NUM_STATIC_DECODER;
    for (size_t i = 0; i < 2 * cl; i++) cc[k++] = c[s + i];
    s += 2 * MAX_CTX;
    for (size_t i = 0; i < 2 * ll; i++) cc[k++] = c[s + i];
    s += 2 * MAX_LOOP;
    for (size_t i = 0; i < 2 * NUM_AUX_STACK; i++) cc[k++] = c[s + i];
    s += 2 * NUM_AUX_STACK;
    for (size_t i = 0; i < 2 * cur.user_n; i++) cc[k++] = c[s + i];
    const uint64_t n = sh.trace_length, target = (MAX_CONSTRAINT_DEGREE - 1) * n + (n - 1);         // evaluator.rs:426
    u128 result = 0;
    size_t i = 0;                                                // Q6: coefficients are taken in the order the groups are walked, not by constraint index
    for (unsigned d = 0; d <= MAX_CONSTRAINT_DEGREE; d++) {
        u128 result_adj = 0;
        bool any = false;
        for (size_t idx = 0; idx < count; idx++) {
            if (degree[idx] != d) continue;
            any = true;
            result = hf_add(result, hf_mul(ev[idx], cc[i * 2]));
            result_adj = hf_add(result_adj, hf_mul(ev[idx], cc[i * 2 + 1]));
            i++;
        }
        if (any) result = hf_add(result, hf_mul(result_adj, hf_pow(x, (u128)(target - (n - 1) * d))));
    }
    return result;
}

// evaluate_boundaries (:181-326): the combinations for the first and for the last step
inline void boundaries_at(const Shape& sh, const u128 draws[NUM_DRAWS], const Public& pub, const Row& cur, u128 x, u128& i_out, u128& f_out) {
    const uint64_t n = sh.trace_length;
    u128 xp = hf_pow(x, (u128)((MAX_CONSTRAINT_DEGREE - 1) * n + 1 - (n - 1)));                     // evaluator.rs:417
    for (int pass = 0; pass < 2; pass++) {
        const u128* c = draws + (size_t)pass * 2 * NUM_BOUNDARY;  // op_counter 2 | sponge 8 | op bits 20 | ctx 32 | loop 16 | user 16  (coefficients.rs:108)
        const u128 *c_sponge = c + 2, *c_bits = c + 10, *c_ctx = c + 30, *c_loop = c + 62, *c_user = c + 78;
        u128 res = 0, adj = 0;
        auto term = [&](u128 val, u128 c0, u128 c1) { res = hf_add(res, hf_mul(val, c0)); adj = hf_add(adj, hf_mul(val, c1)); };
        u128 bit = pass == 0 ? 0 : 1;                            // all op bits 0 (BEGIN) at the first step, all 1 (VOID / NOOP) at the last
        term(pass == 0 ? cur.op_counter : hf_sub(cur.op_counter, pub.op_count), c[0], c[1]);
        if (pass == 0) { for (int i = 0; i < 4; i++) term(cur.sponge[i], c_sponge[i * 2], c_sponge[i * 2 + 1]); }
        else { for (int i = 0; i < 2; i++) term(hf_sub(cur.sponge[i], pub.program_hash[i]), c_sponge[i * 2], c_sponge[i * 2 + 1]); }
        size_t k = 0;
        for (int i = 0; i < 3; i++, k += 2) term(hf_sub(cur.cf[i], bit), c_bits[k], c_bits[k + 1]);
        for (int i = 0; i < 5; i++, k += 2) term(hf_sub(cur.ld[i], bit), c_bits[k], c_bits[k + 1]);
        for (int i = 0; i < 2; i++, k += 2) term(hf_sub(cur.hd[i], bit), c_bits[k], c_bits[k + 1]);
        for (size_t i = 0; i < cur.ctx_n; i++) term(cur.ctx[i], c_ctx[i * 2], c_ctx[i * 2 + 1]);
        for (size_t i = 0; i < cur.loop_n; i++) term(cur.loop[i], c_loop[i * 2], c_loop[i * 2 + 1]);
        const u128* io = pass == 0 ? pub.inputs : pub.outputs;
        const size_t nio = pass == 0 ? pub.num_inputs : pub.num_outputs;
        for (size_t i = 0; i < nio; i++) term(hf_sub(cur.user[i], io[i]), c_user[i * 2], c_user[i * 2 + 1]);
        (pass == 0 ? i_out : f_out) = hf_add(res, hf_mul(adj, xp));
    }
}

}  // namespace hair
}  // namespace dsth
