// AIR constraint evaluation over the degree-8 sub-domain of the LDE domain, one lane per evaluation point.
//
// Replaces the loop at /root/reference/src/stark/prover.rs:53-64: for every i in (0..N).step_by(B/8) it fills `current` =
// row i and `next` = row (i+B) mod N (trace_state.rs:251-277), derives the op flags (trace_state.rs:281-350), evaluates
// the boundary combinations (constraints/evaluator.rs:181-326) and the 20 + ctx + loop decoder constraints
// (constraints/decoder/{mod,op_bits,sponge,flow_ops}.rs) and 2 + stack_depth stack constraints (constraints/stack/*.rs),
// and folds them into one value per point with the random coefficients in degree-group order
// (evaluator.rs:335-358,385-406).  Instead of materialising the per-constraint vector the kernel accumulates
// sum cc[2i]*D and, per degree group, sum cc[2i+1]*D on the fly; x^p factors are table look-ups w_N^(i*p mod N)
// instead of field::exp.  The reference's quirks are reproduced on purpose: ld flag 2 uses
// cf bit 1, SWAP aggregates both constraints into slot 0, PUSH/ASSERT flag adjustments.
//
// The header in reading order: arguments; what a launch evaluates (AS_*, AG_*, AF_*, air_stack); the two rows and the flags of a point;
// one function per constraint section; the kernel, which calls them in turn; the check of the trace rows (air_check_kernel), which calls them
// with an accumulator that only asks for zero; launch_air and the two walks of an instance set's launch list.  The two statements of the user-stack
// constraints have their own headers: air_stack_nested.h (product) and air_stack_perop.h (test build).
//
// Data access: with the coset-major LDE a point is (coset jl, index k); rows i and i+B are (jl,k) and (jl,k+1 mod n),
// so a wavefront reads 64 consecutive elements of each register -- unit stride, no halo.
#pragma once
#include "ctx.h"
#include "air_stack_nested.h"        // bnot, is_bin, static_for_air; StackRows .. st_output; the AG_* operation groups

#ifndef AIR_THREADS
#define AIR_THREADS 128
#endif
#ifndef AIR_WAVES_PER_SIMD
#define AIR_WAVES_PER_SIMD 2      // -DAIR_WAVES_PER_SIMD=3 builds a three-wave form for comparison (tools/ab_variant.sh passes flags through)
#endif
// Waves per SIMD the compiler must make room for: two = at most 256 registers per lane.  Since the evaluation is cut by operation group
// the nested-sum launches need 117 - 193 registers and no scratch (two to four waves per SIMD are resident, profiles/air_layer.md, profiles/air_flags.md); only the per-operation
// instance (tests) reaches the cap.  History: round 2's 172 KB stack launch ran three times slower on one lease and on the driver's box
// (12.7 - 13.4 against 4.3 - 4.6 ms); it had no scratch, so the size of its straight-line code is the suspect -- no
// launch is larger than the 64 KiB instruction cache any more.  Workgroup barriers between the sections (256 lanes per workgroup, the
// wavefronts of a workgroup sharing instruction-cache lines) were measured in round 3 and dropped: profiles/README.md, round 3, and
// profiles/r3_leases.md.

// Rescue matrices (utils/sponge.rs:72-83, utils/hasher.rs:97-113), uploaded once per context to device memory
struct AirConsts { fe sponge_mds[16], sponge_inv_mds[16], hasher_mds[36], hasher_inv_mds[36]; };

struct AirArgs {
    const fe* lde;               // [W][Bc][n]
    fe* out;                     // [3][Q][n]  (i, f, t), Q = local constraint cosets
    const fe* coef;              // 344 raw draws: [0,94) first-step boundary, [94,188) last-step boundary
    const fe* tc;                // [2][NC] transition coefficients by constraint index: plain then degree-adjusted
    const fe* periodic;          // [128][AIR_PERIODIC_STRIDE]: 8 sponge ark, 12 hasher ark, 3 masks, cubes of hasher ark 0..5
    const AirConsts* consts;
    fe* partial;                 // [7][Q][n] partial sums between launches
    fe* ev[10];                  // [Q][n] each: partial values of the stack constraints between launches (slots 0..7, two auxiliary)
    const fe* tw_lo; const fe* tw_hi; uint32_t lo_bits;
    unsigned long long* bad_step;
    size_t n, col_stride;        // col_stride = Bc * n
    uint32_t log_n, log_N, log_b, W, ctx_depth, loop_depth, stack_depth;
    uint32_t cl, ll, sl;         // lengths of the ctx / loop / user stack slices: max(depth, 1), max(depth, 1), max(depth, 8) (trace_state.rs:58-60)
    uint32_t coset_step;         // B / 8: local lde coset of evaluation coset q is q * coset_step (within the local range)
    uint32_t q0;                 // global index of the first local evaluation coset
    uint32_t num_inputs, num_outputs;
    fe inputs[8], outputs[8], program_hash[2], op_count;
};



__device__ __forceinline__ fe dpow(const AirArgs& a, uint64_t e) {
    uint32_t l = (uint32_t)e & ((1u << a.lo_bits) - 1u), h = (uint32_t)(e >> a.lo_bits);
    fe v = a.tw_lo[l];
    return h ? fe_mul(v, a.tw_hi[h]) : v;
}

// MDS matrix times state: every row is a sum of Wd products with one reduction (fe_acc)
template <int Wd>
__device__ __forceinline__ void matmul(fe* s, const fe* m) {
    fe r[Wd];
#pragma unroll
    for (int i = 0; i < Wd; i++) {
        fe_acc A; fe_acc_zero(A);
#pragma unroll
        for (int j = 0; j < Wd; j++) fe_acc_mac(A, m[i * Wd + j], s[j]);
        r[i] = fe_acc_reduce(A);
    }
#pragma unroll
    for (int i = 0; i < Wd; i++) s[i] = r[i];
}

// ---- what a launch evaluates ---------------------------------------------------------------------------------------------------------
// air_kernel<CL, LL, SD, SLCAP, SECT, GROUPS, FLAGS>:
//   CL, LL   compile-time capacities of the context / loop stack slices (>= a.cl, a.ll)
//   SD       compile-time user stack depth, or 0 when the depth is only known at run time (then SLCAP bounds the slice length); only
//            the first `stack_depth` stack constraints are emitted (stack/mod.rs:194), so with SD known the unused slots vanish
//   SLCAP    with SD, names the formulation of the stack constraints (air_stack below)
//   SECT     the constraint sections of the launch, a mask of AS_*
//   GROUPS   the stack OPERATIONS of a nested-sum launch, a mask of AG_* (air_stack_nested.h); the per-operation instance selects
//            its stack sections with SECT instead
//   FLAGS    a mask of AF_*: the launch's place in the chain of partial sums
// The combination is linear in the constraints, so a launch that is not FIRST starts from the partial sums (res, adj[6]) left by the
// previous launch and one that is not LAST stores them; the stack constraints themselves are linear in the operation flags, so their
// partial values travel the same way (AF_EV_IN / AF_EV_OUT) and are emitted by the launch that completes them.  Splitting the evaluation
// this way keeps the live state of each launch within the register budget and its code within the instruction cache.
#define AS_BOUNDARY 1           // the two boundary combinations (tests: DISTAFF_BOUNDARY=eval; normally written in coefficient form)
#define AS_OP_BITS 2            // decoder: op bits
#define AS_SPONGE 4             // decoder: sponge
#define AS_STACK_MOVE 8         // per-operation stack: low-degree operations that move items
#define AS_STACK_HIGH 16        // per-operation stack: PUSH, CMP, BEGIN / NOOP
#define AS_STACK_ARITH 32       // per-operation stack: low-degree arithmetic / selection operations
#define AS_STACK_RESCR 64       // per-operation stack: RESCR
#define AS_FLOW 128             // decoder: loop image, context / loop stacks
#define AS_STACK_ANY (AS_STACK_MOVE | AS_STACK_HIGH | AS_STACK_ARITH | AS_STACK_RESCR)     // 120: any per-operation stack section
#define AS_STACK_AUX (AS_STACK_MOVE | AS_STACK_ARITH)                                      // 40: the sections that touch the auxiliary constraints
// FIRST / LAST in the chain of partial sums (res, adj[6]); EV_IN: partial stack values come in; EV_OUT: they go out (else this launch
// emits the stack constraints)
#define AF_FIRST 1
#define AF_LAST 2
#define AF_EV_IN 4
#define AF_EV_OUT 8

// Which formulation of the stack constraints an instance is, and what follows from it.
//   depth-4 nested     (SD 4):             slots 0..3 as nested sums, items 4.. of the slice are known zeros
//   run-time nested    (SD 0, SLCAP 8):    any depth <= 8: all eight slots as nested sums, `stack_depth` of them emitted
//   deep               (SD 0, SLCAP 12):   any depth: slots 0..7 as nested sums from twelve register-resident items of the current row,
//                                          slots 8.. from memory as seven flag sums times shifted differences (air_stack_deep_slots)
//   per-operation      (anything else; instantiated with SD 0, SLCAP 32): air_stack_perop.h, every slot in registers
struct AirStack {
    bool nested, deep;          // nested: slots 0..7 are nested sums (all but per-operation); deep: slots 8.. exist
    int sl;                     // SL: compile-time length of the stack slice held in registers
    int slots;                  // nested-sum stack constraints (slots 0 .. slots-1, then ST_AUX0, ST_AUX1)
    int partials;               // partial-value arrays (AirArgs::ev) that travel between the stack launches: slots + 2
};
constexpr AirStack air_stack(int sd, int slcap) {
    if (sd == 4) return AirStack{true, false, 8, 4, 6};
    if (sd == 0 && slcap == 8) return AirStack{true, false, 8, 8, 10};
    if (sd == 0 && slcap == 12) return AirStack{true, true, 12, 8, 10};
    return AirStack{false, false, sd ? (sd > 8 ? sd : 8) : slcap, 0, 0};
}

// degree-group slots: 2->0 3->1 4->2 6->3 7->4 8->5
// ACC_MASK: the degree-group sums (bit = slot) that are fe_acc accumulators too; an accumulator is 21 registers, so launches that
// emit into many groups keep the rarely used ones as plain field elements
template <uint32_t ACC_MASK>
struct Acc {
    fe_acc res_acc;        // sum over all constraints of value * coefficient: one reduction at the end of the launch (fe_acc)
    fe_acc adj_acc[6];     // only the entries selected by ACC_MASK are ever touched (the others are eliminated)
    fe res, adj[6];
    bool nonzero;
    const fe* tc; uint32_t nc;
    __device__ __forceinline__ void emit(uint32_t cidx, int slot, const fe& d) {
        nonzero |= !fe_is_zero(d);
        fe_acc_mac(res_acc, d, tc[cidx]);
        if ((ACC_MASK >> slot) & 1u) fe_acc_mac(adj_acc[slot], d, tc[nc + cidx]);
        else adj[slot] = fe_add(adj[slot], fe_mul(d, tc[nc + cidx]));
    }
};
// nested-sum instances: every group a launch without op bits emits into; with op bits (five groups) only degree 2, which takes ten of
// its fifteen constraints.  Per-operation instance: none.
constexpr uint32_t air_acc_mask(const AirStack& st, int sect) { return !st.nested ? 0u : ((sect & AS_OP_BITS) ? 0x01u : 0x3Fu); }

// ---- one evaluation point: its two rows and its flags ----------------------------------------------------------------------------------
// where rows i and i + B of the extension are: register c of the current / next row is cur(c) / nxt(c)
struct AirColumns {
    const fe* cur_p; const fe* nxt_p; size_t cs;
    __device__ __forceinline__ fe cur(size_t c) const { return cur_p[c * cs]; }
    __device__ __forceinline__ fe nxt(size_t c) const { return nxt_p[c * cs]; }
};

// the two rows in registers: decoder registers, and the context / loop slices padded with zeros to their capacities (the stack slices
// o[SL] / nw[SL] are arrays of the kernel: the closures of the per-operation statement capture them and nothing else of the rows)
template <int CL, int LL>
struct AirRows {
    fe c_opc, n_opc, c_sp[4], n_sp[4], cf[3], n_cf[3], ld[5], hd[2];
    fe c_ctx[CL], n_ctx[CL], c_lp[LL], n_lp[LL];
};

template <int SL, int CL, int LL>
__device__ __forceinline__ void air_load_rows(AirRows<CL, LL>& r, fe* o, fe* nw, const AirArgs& a, const AirColumns p, int sd) {
    r.c_opc = p.cur(0); r.n_opc = p.nxt(0);
#pragma unroll
    for (int i = 0; i < 4; i++) { r.c_sp[i] = p.cur(1 + i); r.n_sp[i] = p.nxt(1 + i); }
#pragma unroll
    for (int i = 0; i < 3; i++) { r.cf[i] = p.cur(5 + i); r.n_cf[i] = p.nxt(5 + i); }
#pragma unroll
    for (int i = 0; i < 5; i++) r.ld[i] = p.cur(8 + i);
#pragma unroll
    for (int i = 0; i < 2; i++) r.hd[i] = p.cur(13 + i);
    uint32_t col = 15;
#pragma unroll
    for (int i = 0; i < CL; i++) { bool on = (uint32_t)i < a.ctx_depth; r.c_ctx[i] = on ? p.cur(col + i) : fe_zero(); r.n_ctx[i] = on ? p.nxt(col + i) : fe_zero(); }
    col += a.ctx_depth;
#pragma unroll
    for (int i = 0; i < LL; i++) { bool on = (uint32_t)i < a.loop_depth; r.c_lp[i] = on ? p.cur(col + i) : fe_zero(); r.n_lp[i] = on ? p.nxt(col + i) : fe_zero(); }
    col += a.loop_depth;
#pragma unroll
    for (int i = 0; i < SL; i++) { bool on = i < sd; o[i] = on ? p.cur(col + i) : fe_zero(); nw[i] = on ? p.nxt(col + i) : fe_zero(); }
}

// op flags (trace_state.rs:281-350).  The low-degree op flags are products of three small tables and are formed where they are used:
// ldf(idx) = lo2[idx & 3] * mid[(idx >> 2) & 3] * top[idx >> 4]
struct AirFlags {
    fe cff[8], hdf[4], begin_flag, noop_flag, n_void, assert_flag;      // hdf[0] is the PUSH flag
    fe lo2[4], mid[4], top[2];
    fe ld_all;                                                          // ldf(31) = ld[0] * ld[1] * ld[2] * ld[3] * ld[4]: NOOP's low-degree part, and the op bits' ld product
    __device__ __forceinline__ fe ldf(int idx) const { return fe_mul(fe_mul(lo2[idx & 3], mid[(idx >> 2) & 3]), top[idx >> 4]); }
};

// The four products of two values with two bits and their complements, x * y for x in {1 - a, a}, y in {1 - b, b}, from ONE
// multiplication: with na = 1 - a, nb = 1 - b and t[0] = na * nb,
//     a * nb = nb - t[0],   na * b = na - t[0],   a * b = a - a * nb
// (x * (1 - b) = x - x * b holds for every field element, so also on the cosets where the bits are not 0 / 1).  A subtraction is 10
// instructions against the 71 of a multiplication.
__device__ __forceinline__ void air_bit_pairs(fe* t, const fe& a, const fe& na, const fe& nb) {
    t[0] = fe_mul(na, nb); t[1] = fe_sub(nb, t[0]); t[2] = fe_sub(na, t[0]); t[3] = fe_sub(a, t[1]);
}

template <class ROWS>
__device__ __forceinline__ void air_op_flags(AirFlags& f, const ROWS& r) {
    const fe* cf = r.cf; const fe* ld = r.ld; const fe* hd = r.hd;
    {
        fe n0 = bnot(cf[0]), n1 = bnot(cf[1]), n2 = bnot(cf[2]);
        fe t[4];
        air_bit_pairs(t, cf[0], n0, n1);
#pragma unroll
        for (int i = 0; i < 4; i++) { f.cff[i] = fe_mul(t[i], n2); f.cff[4 + i] = fe_sub(t[i], f.cff[i]); }       // t * cf[2] = t - t * (1 - cf[2])
        f.n_void = fe_mul(fe_mul(r.n_cf[0], r.n_cf[1]), r.n_cf[2]);      // next.cf_op_flags()[VOID]
        fe l0 = bnot(ld[0]), l1 = bnot(ld[1]), l2 = bnot(ld[2]), l3 = bnot(ld[3]);
        f.lo2[0] = fe_mul(l0, l1); f.lo2[1] = fe_sub(l1, f.lo2[0]);
        f.lo2[2] = fe_mul(l0, cf[1]);                                  // sic: cf_op_bits[1] (trace_state.rs:301): no complement of another entry
        f.lo2[3] = fe_sub(ld[0], f.lo2[1]);
        air_bit_pairs(f.mid, ld[2], l2, l3);
        f.top[0] = bnot(ld[4]); f.top[1] = ld[4];
        fe h0 = bnot(hd[0]), h1 = bnot(hd[1]);
        air_bit_pairs(f.hdf, hd[0], h0, h1);
    }
    {
        fe ld0 = f.ldf(0);
        f.ld_all = f.ldf(31);
        f.begin_flag = fe_mul(ld0, f.hdf[0]);                          // trace_state.rs:329
        f.noop_flag = fe_mul(f.ld_all, f.hdf[3]);                      // trace_state.rs:335
        f.hdf[0] = fe_mul(f.hdf[0], ld[0]);                            // PUSH (trace_state.rs:343)
        f.assert_flag = fe_mul(ld0, hd[0]);                            // ASSERT (trace_state.rs:346)
    }
}

#include "air_stack_perop.h"

// ---- the sections ----------------------------------------------------------------------------------------------------------------------
// boundary constraints (evaluator.rs:181-326): writes the two boundary combinations of the point
template <int CL, int LL, class ROWS>
__device__ __forceinline__ void air_boundary(const AirArgs& a, const ROWS& r, const fe* o, int cl, int ll, uint64_t gi, uint64_t n64, uint64_t nmask, uint32_t ql, size_t k) {
    const fe xp = dpow(a, (gi * (6 * n64 + 2)) & nmask);            // b_degree_adj = 7n + 1 - (n - 1)
    const fe one = fe_one();
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        const fe* cc = a.coef + pass * 94;
        // two sums of ~25 products each, reduced once (fe_acc)
        fe_acc R, A; fe_acc_zero(R); fe_acc_zero(A);
        auto term = [&](const fe& v, uint32_t idx) { fe_acc_mac(R, v, cc[idx]); fe_acc_mac(A, v, cc[idx + 1]); };
        term(pass ? fe_sub(r.c_opc, a.op_count) : r.c_opc, 0);
        if (pass == 0) { for (int i = 0; i < 4; i++) term(r.c_sp[i], 2 + 2 * i); }
        else { for (int i = 0; i < 2; i++) term(fe_sub(r.c_sp[i], a.program_hash[i]), 2 + 2 * i); }
        for (int i = 0; i < 3; i++) term(pass ? fe_sub(r.cf[i], one) : r.cf[i], 10 + 2 * i);
        for (int i = 0; i < 5; i++) term(pass ? fe_sub(r.ld[i], one) : r.ld[i], 16 + 2 * i);
        for (int i = 0; i < 2; i++) term(pass ? fe_sub(r.hd[i], one) : r.hd[i], 26 + 2 * i);
        for (int i = 0; i < CL; i++) if (i < cl) term(r.c_ctx[i], 30 + 2 * i);
        for (int i = 0; i < LL; i++) if (i < ll) term(r.c_lp[i], 62 + 2 * i);
        const uint32_t nio = pass ? a.num_outputs : a.num_inputs;
#pragma unroll
        for (int i = 0; i < 8; i++) if ((uint32_t)i < nio) term(fe_sub(o[i], pass ? a.outputs[i] : a.inputs[i]), 78 + 2 * i);
        const fe adj = fe_acc_reduce(A);
        fe_acc_mac(R, adj, xp);
        a.out[((size_t)pass * gridDim.y + ql) * a.n + k] = fe_acc_reduce(R);
    }
}

// decoder: op bits (decoder/op_bits.rs:10-79): constraints 0..14
template <class ACC, class ROWS>
__device__ __forceinline__ void air_op_bits(ACC& acc, const ROWS& r, const AirFlags& f, const fe* per) {
    const fe* cf = r.cf; const fe* ld = r.ld; const fe* hd = r.hd;
    fe cf_sum = fe_add(fe_add(cf[0], cf[1]), cf[2]);
    // the products of all ld bits and of both hd bits are what the flags already hold: ldf(31), hdf[3] (the PUSH adjustment only touches
    // hdf[0]), and their product is the NOOP flag
    const fe ld_prod = f.ld_all, hd_prod = f.hdf[3], all_prod = f.noop_flag;
#pragma unroll
    for (int i = 0; i < 3; i++) acc.emit(i, 0, is_bin(cf[i]));
#pragma unroll
    for (int i = 0; i < 5; i++) acc.emit(3 + i, 0, is_bin(ld[i]));
#pragma unroll
    for (int i = 0; i < 2; i++) acc.emit(8 + i, 0, is_bin(hd[i]));
    const fe is_hacc = f.cff[0];
    // (opc + 1) * hacc + opc * (1 - hacc) - next opc  (op_bits.rs:38-42)  =  opc + hacc - next opc
    acc.emit(10, 1, fe_sub(fe_add(r.c_opc, is_hacc), r.n_opc));
    // opc * (1 - L)(1 - H) and cf_sum * (1 - L H) share L H:  (1 - L)(1 - H) = (1 - L) - H + L H
    acc.emit(11, 5, fe_mul(r.c_opc, fe_add(fe_sub(bnot(ld_prod), hd_prod), all_prod)));
    acc.emit(12, 5, fe_mul(cf_sum, bnot(all_prod)));
    acc.emit(13, 3, fe_mul(f.cff[7], bnot(f.n_void)));
    fe prefix = fe_add(fe_add(f.cff[1], f.cff[4]), fe_add(f.cff[5], f.cff[6]));  // BEGIN, LOOP, WRAP, BREAK
    fe v = fe_mul(prefix, per[21]);
    v = fe_add(v, fe_mul(fe_add(f.cff[2], f.cff[3]), per[20]));                  // TEND, FEND
    v = fe_add(v, fe_mul(f.hdf[0], per[22]));                                    // PUSH
    acc.emit(14, 2, v);
}

// decoder: sponge (decoder/sponge.rs): constraints 15..18.  Of the context and stack slices it reads one item each, the top of the
// current context stack and of the next user stack (nw[0]).  OWN_CTX (the run-time-depth instances): it reads the context item from
// the column itself -- with both items taken from the loaded slices, their two guarded loads at the head of the kernel cost the launch
// a resident wave; with a compile-time depth the slices' values give the code this section had inside the kernel (profiles/air_layer.md).
template <bool OWN_CTX, class ACC, class ROWS>
__device__ __forceinline__ void air_sponge(ACC& acc, const AirArgs& a, const AirColumns p, const ROWS& r, const fe* nw, const AirFlags& f, const fe* per) {
    const AirConsts* consts = a.consts;
    fe ctx0;
    if constexpr (OWN_CTX) ctx0 = 0u < a.ctx_depth ? p.cur(15u) : fe_zero();
    else ctx0 = r.c_ctx[0];
    fe sp[4];
    const fe f_begin = f.cff[1], f_tend = f.cff[2], f_fend = f.cff[3], f_loop = f.cff[4], f_wrap = f.cff[5], f_break = f.cff[6], f_void = f.cff[7];
    {
        // every sponge constraint is a sum of four flag * value products, reduced once (fe_acc):
        //   HACC (sponge.rs:10-43) | cleared by BEGIN, LOOP, WRAP | copied by BREAK, VOID | TEND / FEND merge hashes
        fe os[4], ns[4];
#pragma unroll
        for (int i = 0; i < 4; i++) os[i] = fe_cube(fe_add(r.c_sp[i], per[i]));
        matmul<4>(os, consts->sponge_mds);
        // op_code = ld0 + 2 ld1 + 4 ld2 + 8 ld3 + 16 ld4 + 32 hd0 + 64 hd1 (sponge.rs:27-33) as a doubling chain: six doublings and six
        // additions (144 instructions) instead of five multiplications by small constants
        fe op_code = r.hd[1];
        op_code = fe_add(fe_double(op_code), r.hd[0]);
        op_code = fe_add(fe_double(op_code), r.ld[4]);
        op_code = fe_add(fe_double(op_code), r.ld[3]);
        op_code = fe_add(fe_double(op_code), r.ld[2]);
        op_code = fe_add(fe_double(op_code), r.ld[1]);
        op_code = fe_add(fe_double(op_code), r.ld[0]);
        os[0] = fe_add(os[0], op_code);
        os[1] = fe_add(os[1], fe_mul(nw[0], f.hdf[0]));           // op_value = next.user_stack[0] * push_flag
#pragma unroll
        for (int i = 0; i < 4; i++) ns[i] = r.n_sp[i];
        matmul<4>(ns, consts->sponge_inv_mds);
#pragma unroll
        for (int i = 0; i < 4; i++) ns[i] = fe_sub(fe_cube(ns[i]), per[4 + i]);
        const fe clr = fe_add(fe_add(f_begin, f_loop), f_wrap);
        const fe cpy = fe_add(f_break, f_void);
        const fe tf = fe_add(f_tend, f_fend);
        const fe xf[4] = {tf, f_tend, f_fend, tf};
        const fe xv[4] = {fe_sub(ctx0, r.n_sp[0]), fe_sub(r.c_sp[0], r.n_sp[1]), fe_sub(r.c_sp[0], r.n_sp[2]), r.n_sp[3]};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            fe_acc A; fe_acc_zero(A);
            fe_acc_mac(A, f.cff[0], fe_sub(os[i], ns[i]));
            fe_acc_mac(A, clr, r.n_sp[i]);
            fe_acc_mac(A, cpy, fe_sub(r.c_sp[i], r.n_sp[i]));
            fe_acc_mac(A, xf[i], xv[i]);
            sp[i] = fe_acc_reduce(A);
        }
    }
    acc.emit(15, 3, sp[0]); acc.emit(16, 4, sp[1]); acc.emit(17, 3, sp[2]); acc.emit(18, 3, sp[3]);
}

// Context-stack constraint of slot i (flow_ops.rs): BEGIN / LOOP push sponge[0], TEND / FEND pop (the last slot takes a zero),
// WRAP / BREAK / VOID copy.  ctx_cur(j): item j of the current row's context slice, ni: item i of the next row's.
template <class CUR>
__device__ __forceinline__ fe air_ctx_constraint(int i, int cl, const fe& push, const fe& pop, const fe& ccpy, const fe& sp0, CUR&& ctx_cur, const fe& ni) {
    fe_acc A; fe_acc_zero(A);
    fe_acc_mac(A, push, fe_sub(i == 0 ? sp0 : ctx_cur(i - 1), ni));
    fe_acc_mac(A, pop, i + 1 < cl ? fe_sub(ctx_cur(i + 1), ni) : ni);
    fe_acc_mac(A, ccpy, fe_sub(ctx_cur(i), ni));
    return fe_acc_reduce(A);
}

// decoder: loop image, context and loop stacks (decoder/flow_ops.rs): constraints 19 .. 19 + cl + ll
template <int CL, int LL, class ACC, class ROWS>
__device__ __forceinline__ void air_flow(ACC& acc, const AirArgs& a, const AirColumns p, const ROWS& r, const AirFlags& f, int cl, int ll) {
    const fe f_begin = f.cff[1], f_tend = f.cff[2], f_fend = f.cff[3], f_loop = f.cff[4], f_wrap = f.cff[5], f_break = f.cff[6], f_void = f.cff[7];
    // loop image (WRAP, BREAK)
    acc.emit(19, 2, fe_mul(fe_add(f_wrap, f_break), fe_sub(r.c_sp[0], r.c_lp[0])));
    // context stack: BEGIN/LOOP push sponge[0]; TEND/FEND pop; WRAP/BREAK/VOID copy
    // loop stack: BEGIN/TEND/FEND/WRAP/VOID copy; LOOP shifts right (slot 0 unconstrained); BREAK pops
    const fe push = fe_add(f_begin, f_loop), pop = fe_add(f_tend, f_fend), ccpy = fe_add(fe_add(f_wrap, f_break), f_void);
    const fe lcpy = fe_add(fe_add(fe_add(f_begin, f_tend), fe_add(f_fend, f_wrap)), f_void);
    if constexpr (CL <= 2 && LL <= 1) {
        // small shapes: the slices are register arrays with constant indices
        auto ctx_cur = [&](int j) { return r.c_ctx[j < 0 ? 0 : (j < CL ? j : 0)]; };
#pragma unroll
        for (int i = 0; i < CL; i++) {
            if (i >= cl) break;
            const fe v = air_ctx_constraint(i, cl, push, pop, ccpy, r.c_sp[0], ctx_cur, r.n_ctx[i]);
            acc.emit(20 + i, 2, v);
        }
#pragma unroll
        for (int i = 0; i < LL; i++) {
            if (i >= ll) break;
            fe v = fe_mul(lcpy, fe_sub(r.c_lp[i], r.n_lp[i]));
            if (i >= 1) v = fe_add(v, fe_mul(f_loop, fe_sub(r.c_lp[i - 1 < 0 ? 0 : i - 1], r.n_lp[i])));
            v = fe_add(v, fe_mul(f_break, i + 1 < ll ? fe_sub(r.c_lp[i + 1 < LL ? i + 1 : 0], r.n_lp[i]) : r.n_lp[i]));
            acc.emit(20 + cl + i, 2, v);
        }
    } else {
        // any depth (up to 16 + 8 registers, known at run time): the rows are read from memory inside run-time loops -- register arrays
        // with run-time indices would live in scratch.  A slice of depth 0 is one zero (trace_state.rs:58-59).
        auto ctx_cur = [&](int i) { return (uint32_t)i < a.ctx_depth ? p.cur(15 + i) : fe_zero(); };
        auto ctx_nxt = [&](int i) { return (uint32_t)i < a.ctx_depth ? p.nxt(15 + i) : fe_zero(); };
        const uint32_t lcol = 15 + a.ctx_depth;
        auto lp_cur = [&](int i) { return (uint32_t)i < a.loop_depth ? p.cur(lcol + i) : fe_zero(); };
        auto lp_nxt = [&](int i) { return (uint32_t)i < a.loop_depth ? p.nxt(lcol + i) : fe_zero(); };
#pragma unroll 1
        for (int i = 0; i < cl; i++) {
            const fe ni = ctx_nxt(i);
            acc.emit(20 + i, 2, air_ctx_constraint(i, cl, push, pop, ccpy, r.c_sp[0], ctx_cur, ni));
        }
        // the same loop-stack constraint as above, its three products in one sum (fe_acc)
#pragma unroll 1
        for (int i = 0; i < ll; i++) {
            const fe ni = lp_nxt(i);
            fe_acc A; fe_acc_zero(A);
            fe_acc_mac(A, lcpy, fe_sub(lp_cur(i), ni));
            if (i >= 1) fe_acc_mac(A, f_loop, fe_sub(lp_cur(i - 1), ni));
            fe_acc_mac(A, f_break, i + 1 < ll ? fe_sub(lp_cur(i + 1), ni) : ni);
            acc.emit(20 + cl + i, 2, fe_acc_reduce(A));
        }
    }
}

// Which outputs of a nested-sum launch are evaluated as a flat sum over basis terms (st_output_basis) instead of nested sums
// (st_output): a mask by output.  The static instruction counts and the registers decide per instance (profiles/air_stack_basis.md).
template <int SD, bool DEEP, uint32_t GROUPS>
constexpr uint32_t air_stack_flat() {
    return st_flat_default<GROUPS, SD, DEEP>();
}

// The six RESCR differences of the nested-sum statement (hash.rs:9-35), computed once per point.  Items at and above a known depth are
// zeros: their round-constant cubes come from the periodic table's values alone, and the inverse-matrix rows are shorter.
template <int SD, int NS>
__device__ __forceinline__ void air_rescr_differences(fe* resc, const fe* o, const fe* nw, const fe* per, const AirConsts* consts) {
    constexpr int NZ = (SD != 0 && SD < 6) ? SD : 6;         // items that can be non-zero
    fe os[6], ns[6];
#pragma unroll
    for (int i = 0; i < 6; i++) os[i] = i < NZ ? fe_cube(fe_add(o[i], per[8 + i])) : per[23 + i];      // an absent item is zero: the constant's cube, from the table
    matmul<6>(os, consts->hasher_mds);
    constexpr int NR = NS < 6 ? NS : 6;                      // differences that are used
#pragma unroll
    for (int i = 0; i < NR; i++) {
        fe_acc A; fe_acc_zero(A);
#pragma unroll
        for (int j = 0; j < NZ; j++) fe_acc_mac(A, consts->hasher_inv_mds[i * 6 + j], nw[j]);
        ns[i] = fe_acc_reduce(A);
    }
#pragma unroll
    for (int i = 0; i < NR; i++) resc[i] = fe_sub(fe_sub(fe_cube(ns[i]), per[14 + i]), os[i]);
}

// stack constraints (constraints/stack/mod.rs:117-195) of slots 0..NS-1, ST_AUX0, ST_AUX1 as nested sums: low-degree operations over the
// merged terms of each group (st_output), high-degree / flow operations inside the outermost sum.  The launch adds the operations of
// GROUPS to the partial values that come in (EV_IN) and hands them on (EV_OUT) or emits the constraints.
template <int SD, bool DEEP, int NS, int SL, uint32_t GROUPS, bool EV_IN, bool EV_OUT, class ACC, class ROWS>
__device__ __forceinline__ void air_stack_nested(ACC& acc, const AirArgs& a, const ROWS& r, const fe* o, const fe* nw, const AirFlags& f, const fe* per, int cl, int ll, int sl, int sd, size_t pidx) {
    StackRows rows;
#pragma unroll
    for (int i = 0; i < 8; i++) { rows.o[i] = o[i]; rows.nw[i] = nw[i]; }
#pragma unroll
    for (int i = 8; i < 12; i++) rows.o[i] = DEEP ? o[i < SL ? i : 0] : fe_zero();
    rows.sl = DEEP ? sl : 8;
    const fe lo0h = fe_mul(f.lo2[0], r.hd[0]);                   // ASSERT = LDF(0) * hd[0] (trace_state.rs:346)
    StackHigh high;
    high.push = f.hdf[0]; high.cmp = f.hdf[1]; high.rescr = f.hdf[2]; high.keep = fe_add(f.begin_flag, f.noop_flag);
    if constexpr ((GROUPS & AG_RESCR) != 0) air_rescr_differences<SD, NS>(high.resc, o, nw, per, a.consts);
    constexpr uint32_t FLAT = air_stack_flat<SD, DEEP, GROUPS>();       // the outputs that are one flat sum over the launch's basis terms
    StClassSums<st_class_count<GROUPS, SD, DEEP, FLAT>()> classes;
    const uint32_t sbase = 20 + cl + ll;
    auto output = [&](auto k_) {
        constexpr int kk = decltype(k_)::value;
        constexpr int I = kk < NS ? kk : (kk == NS ? ST_AUX0 : ST_AUX1);
        constexpr bool touched = st_touches<I, GROUPS>();
        // a launch that neither completes the constraints nor contributes to this one leaves the partial value where it is
        if constexpr (touched || !EV_OUT) {
            if (I >= 8 || I < sd) {
                fe v = fe_zero();
                if constexpr (touched) v = st_output_basis<I, GROUPS, SD, DEEP, FLAT>(rows, classes, f.lo2, lo0h, f.mid, f.top, high);
                fe* slot = a.ev[I] + pidx;
                if constexpr (EV_IN) v = touched ? fe_add(v, *slot) : *slot;
                if constexpr (EV_OUT) *slot = v;
                else acc.emit(I >= 8 ? sbase + (I - 8) : sbase + 2 + I, 4, v);
            }
        } else if constexpr (!EV_IN) {
            a.ev[I][pidx] = fe_zero();                           // the first stack launch defines every partial value
        }
    };
    // The nested outputs first: they are the last readers of lo2, mid and top, so the class sums, formed once for all flat outputs, replace the
    // tables in the registers instead of joining them.  (The order of the outputs is free: the emitted sums are exact and the partial
    // values have an array each.)
    static_for_air<0, NS + 2>([&](auto k_) {
        constexpr int kk = decltype(k_)::value;
        if constexpr (((FLAT >> (kk < NS ? kk : (kk == NS ? ST_AUX0 : ST_AUX1))) & 1u) == 0) output(k_);
    });
    st_class_sums<GROUPS, SD, DEEP, FLAT>(classes, f.lo2, lo0h, f.mid, f.top);
    static_for_air<0, NS + 2>([&](auto k_) {
        constexpr int kk = decltype(k_)::value;
        if constexpr (((FLAT >> (kk < NS ? kk : (kk == NS ? ST_AUX0 : ST_AUX1))) & 1u) != 0) output(k_);
    });
}

// Slots 8 .. sd-1 of a deep stack.  No operation computes anything there: a slot is copied, or takes the item 1, 2 or 4
// places to its left or right (left shifts zero-fill the end of the slice), constraints/stack/mod.rs:117-195 with the
// shift helpers :199-262.  So the constraint is a sum of seven products, flag sum * (shifted old item - new item), and
// the seven flag sums are formed once per point from the three small tables (never the 32 flags):
//   left by 1: ASSERT DROP ADD MUL AND OR | by 2: ASSERTEQ EQ CHOOSE CSWAP2 | by 4: DROP4 CHOOSE2
//   right by 1: READ DUP PUSH | by 2: READ2 DUP2 PAD2 | by 4: DUP4
//   copy: INV NEG NOT SWAP SWAP2 SWAP4 ROLL4 ROLL8 BINACC CMP RESCR BEGIN NOOP
template <class ACC>
__device__ __forceinline__ void air_stack_deep_slots(ACC& acc, const AirArgs& a, const AirColumns p, const AirFlags& f, int cl, int ll, int sl, int sd) {
    const fe* lo2 = f.lo2; const fe* mid = f.mid; const fe* top = f.top;
    const uint32_t sbase = 20 + cl + ll;
    const fe lo_all = fe_add(fe_add(lo2[0], lo2[1]), fe_add(lo2[2], lo2[3]));
    fe fl1, fl2, fl4, fr1, fr2, fr4, fcp;
    { fe_acc A; fe_acc_zero(A); fe_acc_mac(A, mid[0], lo2[3]); fe_acc_mac(A, mid[2], lo_all); fl1 = fe_add(fe_mul(top[0], fe_acc_reduce(A)), f.assert_flag); }
    { fe_acc A; fe_acc_zero(A); fe_acc_mac(A, mid[0], fe_add(lo2[1], lo2[2])); fe_acc_mac(A, mid[1], fe_add(lo2[1], lo2[3])); fl2 = fe_mul(top[0], fe_acc_reduce(A)); }
    fl4 = fe_mul(top[0], fe_mul(mid[1], fe_add(lo2[0], lo2[2])));
    fr1 = fe_add(fe_mul(top[1], fe_mul(mid[0], fe_add(lo2[0], lo2[2]))), f.hdf[0]);
    { fe_acc A; fe_acc_zero(A); fe_acc_mac(A, mid[0], fe_add(lo2[1], lo2[3])); fe_acc_mac(A, mid[1], lo2[1]); fr2 = fe_mul(top[1], fe_acc_reduce(A)); }
    fr4 = fe_mul(top[1], fe_mul(mid[1], lo2[0]));
    {
        fe_acc A; fe_acc_zero(A); fe_acc_mac(A, mid[2], lo_all); fe_acc_mac(A, mid[3], fe_add(lo2[0], lo2[1]));
        fe_acc B; fe_acc_zero(B); fe_acc_mac(B, top[1], fe_acc_reduce(A)); fe_acc_mac(B, top[0], fe_mul(mid[3], fe_add(fe_add(lo2[0], lo2[1]), lo2[2])));
        fcp = fe_add(fe_add(fe_acc_reduce(B), fe_add(f.hdf[1], f.hdf[2])), fe_add(f.begin_flag, f.noop_flag));
    }
    const uint32_t scol = 15 + a.ctx_depth + a.loop_depth;
#pragma unroll 1
    for (int i = 8; i < sd; i++) {
        const fe ni = p.nxt(scol + i);
        auto item = [&](int j) { return p.cur(scol + j); };              // j in [4, sd) here
        auto left = [&](int num) { return i + num < sl ? fe_sub(item(i + num), ni) : ni; };
        fe_acc A; fe_acc_zero(A);
        fe_acc_mac(A, fcp, fe_sub(item(i), ni));
        fe_acc_mac(A, fr1, fe_sub(item(i - 1), ni)); fe_acc_mac(A, fr2, fe_sub(item(i - 2), ni)); fe_acc_mac(A, fr4, fe_sub(item(i - 4), ni));
        fe_acc_mac(A, fl1, left(1)); fe_acc_mac(A, fl2, left(2)); fe_acc_mac(A, fl4, left(4));
        acc.emit(sbase + 2 + i, 4, fe_acc_reduce(A));
    }
}

// combination (evaluator.rs:139-162, 335-358) by the last launch of a chain: the transition value of the point from the completed sums
__device__ __forceinline__ void air_combine(const fe& res, const fe* adj, const AirArgs& a, size_t k, uint32_t ql, uint32_t qg, uint64_t gi, uint64_t n64, uint64_t nmask) {
    const bool on_trace = (qg == 0);
    fe t;
    if (on_trace && k + 1 != a.n) {
        t = fe_zero();
    } else {
        // x^p with p = 8n - 1 - (n - 1) * degree for degrees 2, 3, 4, 6, 7, 8: res + sum_g adj[g] * x^p_g as ONE sum of products
        const uint32_t degs[6] = {2, 3, 4, 6, 7, 8};
        fe_acc T; fe_acc_zero(T);
        fe_acc_add(T, res);
#pragma unroll
        for (int g = 0; g < 6; g++) {
            uint64_t p = 8 * n64 - 1 - (n64 - 1) * degs[g];
            fe_acc_mac(T, adj[g], dpow(a, (gi * p) & nmask));
        }
        t = fe_acc_reduce(T);
    }
    a.out[((size_t)2 * gridDim.y + ql) * a.n + k] = t;
}

// ---- the kernel: one lane per evaluation point ----------------------------------------------------------------------------------------
template <int CL, int LL, int SD, int SLCAP, int SECT, uint32_t GROUPS, int FLAGS>
__global__ void __launch_bounds__(AIR_THREADS, AIR_WAVES_PER_SIMD) air_kernel(AirArgs a) {
    constexpr AirStack ST = air_stack(SD, SLCAP);
    constexpr bool FIRST = (FLAGS & AF_FIRST) != 0, LAST = (FLAGS & AF_LAST) != 0, EV_IN = (FLAGS & AF_EV_IN) != 0, EV_OUT = (FLAGS & AF_EV_OUT) != 0;
    static_assert(ST.nested ? (SECT & AS_STACK_ANY) == 0 : (GROUPS == 0 && !EV_IN && !EV_OUT),
                  "nested-sum instances select stack operations with GROUPS, the per-operation instance with SECT");
    const int cl = (int)a.cl, ll = (int)a.ll;
    const int sl = SD ? ST.sl : (int)a.sl;
    const int sd = SD ? SD : (int)a.stack_depth;
    const size_t k = (size_t)blockIdx.x * AIR_THREADS + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t ql = blockIdx.y;                       // local evaluation coset
    const uint32_t qg = a.q0 + ql;
    const uint32_t jl = ql * a.coset_step;                // local lde coset
    const size_t kn = (k + 1 == a.n) ? 0 : k + 1;
    const AirColumns cols{a.lde + (size_t)jl * a.n + k, a.lde + (size_t)jl * a.n + kn, a.col_stride};
    const uint64_t nmask = ((uint64_t)1 << a.log_N) - 1;
    const uint64_t gi = ((uint64_t)k << a.log_b) + (uint64_t)qg * a.coset_step;     // index into the LDE domain, x = w_N^gi
    const uint32_t step = (uint32_t)(((uint64_t)k << 3) + qg);                      // index into the 8n evaluation domain
    const uint64_t n64 = a.n;

    AirRows<CL, LL> rows;
    fe o[ST.sl], nw[ST.sl];             // the stack slices
    air_load_rows<ST.sl>(rows, o, nw, a, cols, sd);
    if constexpr ((SECT & AS_BOUNDARY) != 0) air_boundary<CL, LL>(a, rows, o, cl, ll, gi, n64, nmask, ql, k);
    if constexpr (SECT == AS_BOUNDARY) return;              // a boundary-only launch neither reads nor writes the partial sums
    // Coset 0 is the trace itself: the transition value of its rows is zero by definition except at the last one (air_combine), and
    // whether their constraints vanish is air_check_kernel's question (below), not this kernel's.  Nothing reads the partial sums or
    // partial stack values of these points.
    if (qg == 0 && k + 1 != a.n) {
        if constexpr (LAST) a.out[((size_t)2 * gridDim.y + ql) * a.n + k] = fe_zero();
        return;
    }
    AirFlags flags;
    air_op_flags(flags, rows);
    const fe* per = a.periodic + (size_t)(step & 127u) * AIR_PERIODIC_STRIDE;

    constexpr uint32_t ACC_MASK = air_acc_mask(ST, SECT);
    Acc<ACC_MASK> acc;
#pragma unroll
    for (int i = 0; i < 6; i++) if ((ACC_MASK >> i) & 1u) fe_acc_zero(acc.adj_acc[i]);
    fe_acc_zero(acc.res_acc); acc.res = fe_zero(); acc.nonzero = false; acc.tc = a.tc; acc.nc = 20 + cl + ll + 2 + sd;
#pragma unroll
    for (int i = 0; i < 6; i++) acc.adj[i] = fe_zero();
    const size_t pstride = (size_t)gridDim.y * a.n, pidx = (size_t)ql * a.n + k;

    if constexpr ((SECT & AS_OP_BITS) != 0) air_op_bits(acc, rows, flags, per);
    if constexpr ((SECT & AS_SPONGE) != 0) air_sponge<SD == 0>(acc, a, cols, rows, nw, flags, per);
    if constexpr ((SECT & AS_FLOW) != 0) air_flow<CL, LL>(acc, a, cols, rows, flags, cl, ll);
    if constexpr (ST.nested && (GROUPS & AG_STACK_ALL & ~AG_DEEP) != 0) air_stack_nested<SD, ST.deep, ST.slots, ST.sl, GROUPS, EV_IN, EV_OUT>(acc, a, rows, o, nw, flags, per, cl, ll, sl, sd, pidx);
    if constexpr (!ST.nested && (SECT & AS_STACK_ANY) != 0) air_stack_per_operation<ST.sl, SECT>(acc, o, nw, sl, sd, 20 + cl + ll, flags, per, a.consts);
    if constexpr (ST.deep && (GROUPS & AG_DEEP) != 0) air_stack_deep_slots(acc, a, cols, flags, cl, ll, sl, sd);

    // ---- hand-over of the partial sums, combination ----
    // degree-group sums the launch moves: op bits {2,3,4,6,8}, sponge {6,7}, loop image / context / loop stacks {4}, stack {7}
    constexpr bool EMITS_STACK = (SECT & AS_STACK_ANY) != 0 || (GROUPS & AG_DEEP) != 0 || ((GROUPS & AG_STACK_ALL) != 0 && !EV_OUT);
    constexpr uint32_t USED = ((SECT & AS_OP_BITS) ? 0x2Fu : 0u) | ((SECT & AS_SPONGE) ? 0x18u : 0u) | ((SECT & AS_FLOW) ? 0x04u : 0u) | (EMITS_STACK ? 0x10u : 0u);
    // hand-over: the partial sums of the previous launches join at the end (they are not live during the evaluation); a launch only
    // moves the degree-group sums its sections emit into.  (Stated here and not in a function of its own: there the index arithmetic
    // of the partial sums compiled to other instructions, profiles/air_layer.md.)
    acc.res = fe_acc_reduce(acc.res_acc);
#pragma unroll
    for (int i = 0; i < 6; i++) if (((ACC_MASK & USED) >> i) & 1u) acc.adj[i] = fe_add(acc.adj[i], fe_acc_reduce(acc.adj_acc[i]));
    if constexpr (!FIRST) {
        acc.res = fe_add(acc.res, a.partial[pidx]);
#pragma unroll
        for (int i = 0; i < 6; i++) if (LAST || ((USED >> i) & 1u)) acc.adj[i] = fe_add(acc.adj[i], a.partial[(size_t)(i + 1) * pstride + pidx]);
    }
    if constexpr (!LAST) {
        a.partial[pidx] = acc.res;
#pragma unroll
        for (int i = 0; i < 6; i++) if (FIRST || ((USED >> i) & 1u)) a.partial[(size_t)(i + 1) * pstride + pidx] = acc.adj[i];
        return;
    }
    air_combine(acc.res, acc.adj, a, k, ql, qg, gi, n64, nmask);
}

// ---- the check of the trace rows (evaluator.rs:152-158): one lane per row of the trace ----------------------------------------------------
// On the trace itself every transition constraint must vanish between rows k and k + 1, k < n - 1; the first k where one does not is
// the failing step.  The verdict depends on the trace alone -- no coefficient enters it -- so it is a chain of launches of its own that
// may run beside anything that leaves the trace alone: the same sections, called with an accumulator that only asks whether a value
// is zero.  The stack launches hand their partial values on exactly like air_kernel's (AF_EV_IN / AF_EV_OUT), through arrays of the
// chain's own (AirArgs::ev, n elements each), and the launch that completes a constraint judges it.  Of AirArgs the chain reads lde,
// periodic, consts, ev, bad_step and the shape; AF_FIRST / AF_LAST name the instance and nothing else.
struct AirCheckAcc {
    bool nonzero;
    __device__ __forceinline__ void emit(uint32_t, int, const fe& d) { nonzero |= !fe_is_zero(d); }
};

template <int CL, int LL, int SD, int SLCAP, int SECT, uint32_t GROUPS, int FLAGS>
__global__ void __launch_bounds__(AIR_THREADS, AIR_WAVES_PER_SIMD) air_check_kernel(AirArgs a) {
    constexpr AirStack ST = air_stack(SD, SLCAP);
    constexpr bool EV_IN = (FLAGS & AF_EV_IN) != 0, EV_OUT = (FLAGS & AF_EV_OUT) != 0;
    static_assert(ST.nested ? (SECT & AS_STACK_ANY) == 0 : (GROUPS == 0 && !EV_IN && !EV_OUT),
                  "nested-sum instances select stack operations with GROUPS, the per-operation instance with SECT");
    static_assert((SECT & AS_BOUNDARY) == 0, "the boundary combinations are no part of the check");
    const int cl = (int)a.cl, ll = (int)a.ll;
    const int sl = SD ? ST.sl : (int)a.sl;
    const int sd = SD ? SD : (int)a.stack_depth;
    const size_t k = (size_t)blockIdx.x * AIR_THREADS + threadIdx.x;
    if (k + 1 >= a.n) return;                               // the step from the last row to the first is no step of the program
    const AirColumns cols{a.lde + k, a.lde + k + 1, a.col_stride};                  // coset 0 of the extension: rows k and k + 1 of the trace

    AirRows<CL, LL> rows;
    fe o[ST.sl], nw[ST.sl];
    air_load_rows<ST.sl>(rows, o, nw, a, cols, sd);
    AirFlags flags;
    air_op_flags(flags, rows);
    const fe* per = a.periodic + (size_t)(((uint32_t)k << 3) & 127u) * AIR_PERIODIC_STRIDE;     // step 8 k of the 8n evaluation domain

    AirCheckAcc acc; acc.nonzero = false;
    if constexpr ((SECT & AS_OP_BITS) != 0) air_op_bits(acc, rows, flags, per);
    if constexpr ((SECT & AS_SPONGE) != 0) air_sponge<SD == 0>(acc, a, cols, rows, nw, flags, per);
    if constexpr ((SECT & AS_FLOW) != 0) air_flow<CL, LL>(acc, a, cols, rows, flags, cl, ll);
    if constexpr (ST.nested && (GROUPS & AG_STACK_ALL & ~AG_DEEP) != 0) air_stack_nested<SD, ST.deep, ST.slots, ST.sl, GROUPS, EV_IN, EV_OUT>(acc, a, rows, o, nw, flags, per, cl, ll, sl, sd, k);
    if constexpr (!ST.nested && (SECT & AS_STACK_ANY) != 0) air_stack_per_operation<ST.sl, SECT>(acc, o, nw, sl, sd, 20 + cl + ll, flags, per, a.consts);
    if constexpr (ST.deep && (GROUPS & AG_DEEP) != 0) air_stack_deep_slots(acc, a, cols, flags, cl, ll, sl, sd);
    if (acc.nonzero) atomicMin(a.bad_step, (unsigned long long)k);
}

template <int CL, int LL, int SD, int SLCAP, int SECT, uint32_t GROUPS, int FLAGS>
static void launch_air_check(dst_ctx* c, const AirArgs& a, hipStream_t stream) {
    dim3 g((unsigned)((c->n + AIR_THREADS - 1) / AIR_THREADS), 1);
    static char name[64];
    if (!name[0]) snprintf(name, sizeof(name), "air_check<%d,%d,%d,%d,%d,%u,%d>", CL, LL, SD, SLCAP, SECT, (unsigned)GROUPS, FLAGS);
    // algorithmic bytes: the W registers of a row, the stack partial values that come in and go out
    constexpr int NS = air_stack(SD, SLCAP).partials;
    const double units = c->W + ((FLAGS & AF_EV_IN) ? NS : 0) + ((FLAGS & AF_EV_OUT) ? NS : 0);
    { KScope ks_(c, name, 16.0 * c->n * units, true, 0.0, stream); hipLaunchKernelGGL((air_check_kernel<CL, LL, SD, SLCAP, SECT, GROUPS, FLAGS>), g, dim3(AIR_THREADS), 0, stream, a); }
}

template <int CL, int LL, int SD, int SLCAP, int SECT, uint32_t GROUPS, int FLAGS>
static void launch_air(dst_ctx* c, const AirArgs& a, uint32_t Q) {
    dim3 g((unsigned)((c->n + AIR_THREADS - 1) / AIR_THREADS), Q);
    static char name[64];          // one name per instantiation, matching the template arguments rocprofv3 prints
    if (!name[0]) snprintf(name, sizeof(name), "air_kernel<%d,%d,%d,%d,%d,%u,%d>", CL, LL, SD, SLCAP, SECT, (unsigned)GROUPS, FLAGS);
    // algorithmic bytes: the W registers of a row, the partial sums that come in and go out, the stack partial values, the result
    constexpr int NS = air_stack(SD, SLCAP).partials;
    const double units = c->W + ((FLAGS & AF_FIRST) ? 0 : 7) + ((FLAGS & AF_LAST) ? 1 : 7) + ((SECT & AS_BOUNDARY) ? 2 : 0) + ((FLAGS & AF_EV_IN) ? NS : 0) + ((FLAGS & AF_EV_OUT) ? NS : 0);
    { KScope ks_(c, name, 16.0 * c->n * Q * units, true); hipLaunchKernelGGL((air_kernel<CL, LL, SD, SLCAP, SECT, GROUPS, FLAGS>), g, dim3(AIR_THREADS), 0, c->stream, a); }
}
// the boundary combinations by evaluation (tests: DISTAFF_BOUNDARY=eval; normally written in coefficient form, api.hip
// dst_internal_boundary_polys): the first launch of every instance set in the test build
template <int CL, int LL, int SD, int SLCAP>
static void launch_air_boundary(dst_ctx* c, const AirArgs& a, uint32_t Q) {
#if DST_TEST_HOOKS
    if (dst_internal_boundary_by_evaluation(c)) launch_air<CL, LL, SD, SLCAP, AS_BOUNDARY, 0, 0>(c, a, Q);
#endif
}
// The launches of an instance set are stated once (air_chain_* in the set's unit) and walked twice: by AirEvalChain, which launches
// air_kernel over the Q local evaluation cosets, and by AirCheckChain, which launches air_check_kernel over the trace rows.
struct AirEvalChain {
    dst_ctx* c; const AirArgs& a; uint32_t Q;
    template <int CL, int LL, int SD, int SLCAP, int SECT, uint32_t GROUPS, int FLAGS> void run() const { launch_air<CL, LL, SD, SLCAP, SECT, GROUPS, FLAGS>(c, a, Q); }
    template <int CL, int LL, int SD, int SLCAP> void boundary() const { launch_air_boundary<CL, LL, SD, SLCAP>(c, a, Q); }
};
struct AirCheckChain {
    dst_ctx* c; const AirArgs& a; hipStream_t stream;
    template <int CL, int LL, int SD, int SLCAP, int SECT, uint32_t GROUPS, int FLAGS> void run() const { launch_air_check<CL, LL, SD, SLCAP, SECT, GROUPS, FLAGS>(c, a, stream); }
    template <int CL, int LL, int SD, int SLCAP> void boundary() const {}
};
// instances live in their own translation units (compile time): Fibonacci shape, small stacks, fully generic
void air_launch_sd4(dst_ctx* c, const AirArgs& a, uint32_t Q);      // cl <= 2, ll <= 1, stack_depth == 4
void air_launch_small(dst_ctx* c, const AirArgs& a, uint32_t Q);    // cl <= 2, ll <= 1, stack_depth <= 8
void air_launch_deep(dst_ctx* c, const AirArgs& a, uint32_t Q);     // anything the VM can produce, nested sums + flag sums for slots >= 8
void air_launch_generic(dst_ctx* c, const AirArgs& a, uint32_t Q);  // anything the VM can produce, per-operation formulation (DISTAFF_AIR=generic)
// the check chains of the same sets (a.ev: the chain's own arrays), queued on `stream`
void air_check_sd4(dst_ctx* c, const AirArgs& a, hipStream_t stream);
void air_check_small(dst_ctx* c, const AirArgs& a, hipStream_t stream);
void air_check_deep(dst_ctx* c, const AirArgs& a, hipStream_t stream);      // also behind the per-operation set (kernels_air.hip k_air_check)
