// AIR kernel instances for traces with <= 2 context registers, <= 1 loop register and a user stack of depth <= 8 (depth known
// at run time): the run-time-depth nested-sum formulation (air_kernel.h air_stack, air_stack_nested.h); cut into launches by constraint
// section (AS_*) and, for the stack, by operation group (AG_*): every launch without scratch and inside the 64 KiB instruction cache of
// a CU pair.
#include "air_kernel.h"
// the launches of the set, stated once: walked by the evaluation (air_kernel) and by the check of the trace rows (air_check_kernel)
template <class CHAIN>
static void air_chain_small(const CHAIN& ch) {
    ch.template boundary<2, 1, 0, 8>();                                                      // boundary combinations by evaluation (test build only)
    ch.template run<2, 1, 0, 8, AS_OP_BITS | AS_FLOW, 0, AF_FIRST>();                            // op bits, loop image, context / loop stacks (starts the partial sums)
    ch.template run<2, 1, 0, 8, AS_SPONGE, 0, 0>();                                              // sponge
    ch.template run<2, 1, 0, 8, 0, AG_RESCR, AF_EV_OUT>();                                       // stack: RESCR
    ch.template run<2, 1, 0, 8, 0, AG_PUSH | AG_CMP | AG_KEEP, AF_EV_IN | AF_EV_OUT>();          // stack: PUSH, CMP, BEGIN / NOOP
    ch.template run<2, 1, 0, 8, 0, AG_LOW(0, 0) | AG_LOW(0, 2), AF_EV_IN | AF_EV_OUT>();         // stack: operations 0x00 .. 0x03, 0x08 .. 0x0B
    ch.template run<2, 1, 0, 8, 0, AG_LOW(0, 1) | AG_LOW(0, 3), AF_EV_IN | AF_EV_OUT>();         // stack: operations 0x04 .. 0x07, 0x0C .. 0x0F
    ch.template run<2, 1, 0, 8, 0, AG_LOW(1, 2) | AG_LOW(1, 3), AF_EV_IN | AF_EV_OUT>();         // stack: operations 0x18 .. 0x1F
    ch.template run<2, 1, 0, 8, 0, AG_LOW(1, 0) | AG_LOW(1, 1), AF_EV_IN | AF_LAST>();           // stack: operations 0x10 .. 0x17; emits the stack constraints; combination
}
void air_launch_small(dst_ctx* c, const AirArgs& a, uint32_t Q) { air_chain_small(AirEvalChain{c, a, Q}); }
void air_check_small(dst_ctx* c, const AirArgs& a, hipStream_t stream) { air_chain_small(AirCheckChain{c, a, stream}); }
