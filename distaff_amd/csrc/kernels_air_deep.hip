// AIR kernel instances for any trace shape the VM can produce (up to 16 context, 8 loop and 32 stack registers, known at run time)
// in the deep formulation (air_kernel.h air_stack): the first eight stack slots as nested sums like the depth <= 8 instances
// (air_stack_nested.h, from twelve register-resident items of the current row), deeper slots from memory as flag sums times shifted
// differences (air_kernel.h air_stack_deep_slots, AG_DEEP).  The per-operation formulation (air_stack_perop.h, launched by
// kernels_air.hip) stays as an independent statement of the same constraints (DISTAFF_AIR=generic).
#include "air_kernel.h"
// the launches of the set, stated once: walked by the evaluation (air_kernel) and by the check of the trace rows (air_check_kernel)
template <class CHAIN>
static void air_chain_deep(const CHAIN& ch) {
    ch.template boundary<16, 8, 0, 12>();                                                     // boundary combinations by evaluation (test build only)
    ch.template run<16, 8, 0, 12, AS_OP_BITS, 0, AF_FIRST>();                                     // op bits (starts the partial sums)
    ch.template run<16, 8, 0, 12, AS_SPONGE, 0, 0>();                                             // sponge
    ch.template run<16, 8, 0, 12, AS_FLOW, 0, 0>();                                               // loop image, context / loop stacks
    ch.template run<16, 8, 0, 12, 0, AG_DEEP, 0>();                                               // stack slots 8..: flag sums x shifted differences
    ch.template run<16, 8, 0, 12, 0, AG_RESCR, AF_EV_OUT>();                                      // stack slots 0..7: RESCR
    ch.template run<16, 8, 0, 12, 0, AG_PUSH | AG_CMP | AG_KEEP, AF_EV_IN | AF_EV_OUT>();         // PUSH, CMP, BEGIN / NOOP
    ch.template run<16, 8, 0, 12, 0, AG_LOW(0, 0) | AG_LOW(0, 2), AF_EV_IN | AF_EV_OUT>();        // operations 0x00 .. 0x03, 0x08 .. 0x0B
    ch.template run<16, 8, 0, 12, 0, AG_LOW(0, 1) | AG_LOW(0, 3), AF_EV_IN | AF_EV_OUT>();        // operations 0x04 .. 0x07, 0x0C .. 0x0F
    ch.template run<16, 8, 0, 12, 0, AG_LOW(1, 2) | AG_LOW(1, 3), AF_EV_IN | AF_EV_OUT>();        // operations 0x18 .. 0x1F
    ch.template run<16, 8, 0, 12, 0, AG_LOW(1, 0) | AG_LOW(1, 1), AF_EV_IN | AF_LAST>();          // operations 0x10 .. 0x17; emits slots 0..7; combination
}
void air_launch_deep(dst_ctx* c, const AirArgs& a, uint32_t Q) { air_chain_deep(AirEvalChain{c, a, Q}); }
void air_check_deep(dst_ctx* c, const AirArgs& a, hipStream_t stream) { air_chain_deep(AirCheckChain{c, a, stream}); }
