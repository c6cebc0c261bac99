// Launcher of the AIR constraint kernel (air_kernel.h) and, in the test build, its per-operation instance (air_stack_perop.h).
#include "air_kernel.h"
#include "rescue_constants.h"

#if DST_TEST_HOOKS            // the per-operation formulation: an independent statement of the constraints for the tests (DISTAFF_AIR=generic)
void air_launch_generic(dst_ctx* c, const AirArgs& a, uint32_t Q) {
    // any shape the VM can produce (up to 16 context, 8 loop and 32 stack registers, known at run time), per-operation formulation,
    // cut into the same section launches as the specialised instances
    launch_air<16, 8, 0, 32, AS_OP_BITS, 0, AF_FIRST>(c, a, Q);            // op bits
    launch_air_boundary<16, 8, 0, 32>(c, a, Q);                            // boundary combinations by evaluation
    launch_air<16, 8, 0, 32, AS_SPONGE | AS_FLOW, 0, 0>(c, a, Q);          // sponge, loop image, context / loop stacks
    launch_air<16, 8, 0, 32, AS_STACK_MOVE, 0, 0>(c, a, Q);                // stack: low-degree ops that move items
    launch_air<16, 8, 0, 32, AS_STACK_ARITH, 0, 0>(c, a, Q);               // stack: low-degree arithmetic / selection ops
    launch_air<16, 8, 0, 32, AS_STACK_HIGH, 0, 0>(c, a, Q);                // stack: PUSH, CMP, BEGIN / NOOP
    launch_air<16, 8, 0, 32, AS_STACK_RESCR, 0, AF_LAST>(c, a, Q);         // stack: RESCR + combination
}
#endif

// Which instance set evaluates a trace of the shape (cl, ll, sd): the most special one that fits, unless DISTAFF_AIR=small|deep|generic
// forces a more general one (tests run the same trace through all of them).  The per-operation set exists in the test build only: the
// product library answers `generic` with the deep set.
enum AirInstanceSet { AIR_SET_SD4, AIR_SET_SMALL, AIR_SET_DEEP, AIR_SET_GENERIC };
static AirInstanceSet air_instance_set(uint32_t cl, uint32_t ll, uint32_t sd, const char* force) {
    const bool small_shape = cl <= 2 && ll <= 1 && sd <= 8;
    const auto forced = [&](const char* name) { return force && !strcmp(force, name); };
    if (forced("generic")) return DST_TEST_HOOKS ? AIR_SET_GENERIC : AIR_SET_DEEP;
    if (forced("deep") || !small_shape) return AIR_SET_DEEP;
    return sd == 4 && !forced("small") ? AIR_SET_SD4 : AIR_SET_SMALL;
}

int k_constraint_check(dst_ctx* c, int64_t* bad_step) {
    const unsigned long long res = c->air_flag_host;
    if (res != ~0ull) { if (bad_step) *bad_step = (int64_t)res; return DST_ERR_AIR; }
    if (bad_step) *bad_step = -1;
    return DST_OK;
}
// what the evaluation and the check of the trace rows both read: the extension, the tables, the shape of the trace
static int air_shape_args(dst_ctx* c, AirArgs& a) {
    if (!c->air_consts) {
        AirConsts h;
        memcpy(h.sponge_mds, SPONGE_MDS, sizeof(h.sponge_mds)); memcpy(h.sponge_inv_mds, SPONGE_INV_MDS, sizeof(h.sponge_inv_mds));
        memcpy(h.hasher_mds, HASHER_MDS, sizeof(h.hasher_mds)); memcpy(h.hasher_inv_mds, HASHER_INV_MDS, sizeof(h.hasher_inv_mds));
        { const int r = ctx_dev_bytes(c, &c->air_consts, sizeof(AirConsts)); if (r) return r; }
        HIP_TRY(c, hipMemcpy(c->air_consts, &h, sizeof(AirConsts), hipMemcpyHostToDevice));
    }
    a.lde = c->lde; a.periodic = c->periodic; a.consts = (const AirConsts*)c->air_consts;
    a.tw_lo = c->tw_lo; a.tw_hi = c->tw_hi; a.lo_bits = c->tw_lo_bits;
    a.bad_step = (unsigned long long*)c->d_u64;
    a.n = c->n; a.col_stride = c->Bc * c->n;
    a.log_n = c->log_n; a.log_N = c->log_N; a.log_b = c->log_b; a.W = (uint32_t)c->W;
    a.ctx_depth = c->prm.ctx_depth; a.loop_depth = c->prm.loop_depth; a.stack_depth = (uint32_t)c->stack_depth;
    a.coset_step = (uint32_t)(c->B / 8);
    a.q0 = (uint32_t)(c->j0 / (c->B / 8));
    const uint32_t cd = c->prm.ctx_depth, lp = c->prm.loop_depth, sd = (uint32_t)c->stack_depth;
    a.cl = cd > 1 ? cd : 1; a.ll = lp > 1 ? lp : 1; a.sl = sd > 8 ? sd : 8;
    return DST_OK;
}

int k_eval_constraints(dst_ctx* c, const fe* coeffs_dev, const fe* tc_dev, int64_t* bad_step, bool defer_check, bool check_here) {
    AirArgs a{};
    { const int r = air_shape_args(c, a); if (r) return r; }
    a.out = c->ceval; a.coef = coeffs_dev; a.tc = tc_dev; a.partial = c->cwork;
    // partial values of the stack constraints between launches: buffers that are idle during the evaluation -- the staging buffer of the
    // transforms (>= 4 registers x Bc cosets = (B / 2) of these arrays for B >= 16) and the two polynomials written after this phase
    {
        const size_t per = (size_t)(c->Bc / (c->B / 8)) * c->n;
        if (8 * per > c->Bc * c->tmp_regs * c->n) { c->err = "constraint evaluation: staging buffer too small for the stack partial values"; return DST_ERR_STATE; }
        for (int i = 0; i < 8; i++) a.ev[i] = c->tmp + (size_t)i * per;
        a.ev[8] = c->cpoly; a.ev[9] = c->comp_poly;
    }
    uint32_t Q = (uint32_t)(c->Bc / (c->B / 8));
    a.num_inputs = c->pub.num_inputs; a.num_outputs = c->pub.num_outputs;
    memcpy(a.inputs, c->pub.inputs, sizeof(a.inputs)); memcpy(a.outputs, c->pub.outputs, sizeof(a.outputs));
    memcpy(a.program_hash, c->program_hash, sizeof(a.program_hash));
    a.op_count = c->op_counter;
    switch (air_instance_set(a.cl, a.ll, a.stack_depth, c->sw("DISTAFF_AIR"))) {
        case AIR_SET_SD4: air_launch_sd4(c, a, Q); break;
        case AIR_SET_SMALL: air_launch_small(c, a, Q); break;
        case AIR_SET_GENERIC:                   // the product library has no per-operation set: the deep set answers
#if DST_TEST_HOOKS
            air_launch_generic(c, a, Q); break;
#endif
        case AIR_SET_DEEP: air_launch_deep(c, a, Q); break;
    }
    // The evaluation gives no verdict on the trace: the check of the trace rows does (evaluator.rs:152-158 panics at the failing step).
    // Here it follows the evaluation on the same stream, unless the caller queues it elsewhere (dst_prove: k_air_check_side).  With
    // defer_check the host does not wait -- the caller looks at the flag (k_constraint_check) at its next synchronisation, after work
    // that does not depend on it.
    if (!check_here) return DST_OK;
    { const int r = k_air_check(c, c->stream); if (r) return r; }
    if (defer_check && c->h_stage) return DST_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->air_flag_host = *reinterpret_cast<unsigned long long*>(c->h_stage + HS_AIR_FLAG);
    return k_constraint_check(c, bad_step);
}

// partial-value arrays (n elements each) the check chain of this context's instance set hands on between its stack launches
size_t k_air_check_partials(const dst_ctx* c) {
    const uint32_t cd = c->prm.ctx_depth, lp = c->prm.loop_depth;
    const bool sd4 = air_instance_set(cd > 1 ? cd : 1, lp > 1 ? lp : 1, (uint32_t)c->stack_depth, c->sw("DISTAFF_AIR")) == AIR_SET_SD4;
    return (size_t)(sd4 ? air_stack(4, 8).partials : air_stack(0, 12).partials);       // 6; the small and the deep set: 10
}

// The check of the trace rows on `stream`: the failing-step word reset, the chain of the instance set over coset 0 of the extension -- the
// trace; a sharded context that does not own it has nothing to check, as before -- and the word read back into page-locked memory.
int k_air_check(dst_ctx* c, hipStream_t stream) {
    AirArgs a{};
    { const int r = air_shape_args(c, a); if (r) return r; }
    HIP_TRY(c, hipMemsetAsync(c->d_u64, 0xFF, 8, stream));              // ~0 = no failing step yet
    if (a.q0 == 0) {
        // the chain's own partial-value arrays, packed: the set's stack slots, then the two auxiliary constraints (k_air_check_partials)
        const size_t slots = k_air_check_partials(c) - 2;
        for (size_t i = 0; i < slots; i++) a.ev[i] = c->check_partials + i * c->n;
        a.ev[ST_AUX0] = c->check_partials + slots * c->n; a.ev[ST_AUX1] = c->check_partials + (slots + 1) * c->n;
        switch (air_instance_set(a.cl, a.ll, a.stack_depth, c->sw("DISTAFF_AIR"))) {
            case AIR_SET_SD4: air_check_sd4(c, a, stream); break;
            case AIR_SET_SMALL: air_check_small(c, a, stream); break;
            // the per-operation set has no check chain of its own (its stack launches hold all 32 slots in registers: without the
            // exceptions its evaluation has, they do not pass the build's kernel gate): the deep set, which covers every shape, answers
            case AIR_SET_GENERIC:
            case AIR_SET_DEEP: air_check_deep(c, a, stream); break;
        }
    }
    HIP_TRY(c, hipMemcpyAsync(c->h_stage + HS_AIR_FLAG, c->d_u64, 8, hipMemcpyDeviceToHost, stream));
    return DST_OK;
}

// The same beside the main stream: on a stream of the lowest priority, behind everything the main stream holds at this moment.  Nothing
// later on the main stream waits for it; the caller drains it (k_air_check_drain) before it reports, and so does whoever writes or frees the
// trace buffer.
int k_air_check_side(dst_ctx* c) {
    if (!c->check_stream) { const int r = ctx_stream(c, &c->check_stream, hipStreamNonBlocking, /*lowest=*/true); if (r) return r; }
    if (!c->check_ev) { const int r = ctx_event(c, &c->check_ev, hipEventDisableTiming); if (r) return r; }
    HIP_TRY(c, hipEventRecord(c->check_ev, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->check_stream, c->check_ev, 0));
    c->check_pending = true;                                           // from the first thing queued on: a failure below leaves work on the stream
    return k_air_check(c, c->check_stream);
}
int k_air_check_drain(dst_ctx* c) {
    if (!c->check_pending) return DST_OK;
    c->check_pending = false;
    HIP_TRY(c, hipStreamSynchronize(c->check_stream));
    c->air_flag_host = *reinterpret_cast<unsigned long long*>(c->h_stage + HS_AIR_FLAG);
    return DST_OK;
}
